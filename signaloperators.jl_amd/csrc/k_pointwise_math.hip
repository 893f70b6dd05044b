// K1's math instantiation: the pointwise steps whose programs contain expression-program operations (traced
// `elementwise` closures, kmath.h) when hipRTC does not serve them (SIGOPS_RTC=0, no hipRTC, a failed compile).  A
// translation unit of its own, compiled with -ffp-contract=off (build.py) like the hipRTC kernels: the leaf evaluators it
// inlines (kleaf.h: `t*omega + phi` of a generator) then round every operation as the hipRTC kernel and the host do, and
// the two paths give the same values bit for bit.
#include "kpointwise.h"

namespace so {

void launch_pointwise_math(const DPiece* d_pieces, int npieces, int64_t nblocks, const DOp* d_ops, const DLeaf* d_leaves,
                           OutView out, hipStream_t st) {
    if (nblocks <= 0) return;
    hipLaunchKernelGGL((k_pointwise<kPointwiseE, true, false, false, true>), dim3((unsigned)nblocks), dim3(kBlock), 0, st,
                       d_pieces, npieces, d_ops, d_leaves, out);
}

}  // namespace so
