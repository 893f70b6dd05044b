// k_randn_fill: the fill form of counter-based white noise (krand.h; `Signal(randn, rng=DeviceRNG(...))`, reference
// src/functions.jl:98-114).  A pointwise step that is exactly a noise leaf over frame ranges -- optionally times a
// constant, replicated to the channels of `ToChannels` -- is the commonest one: noise at the bottom of a pipeline is
// always materialised for the filter or resampler above it.  The interpreter's math instantiation evaluates one frame
// per lane and run and throws the other half of every Box-Muller pair away; here a lane owns a PAIR: one Philox block,
// one log, one sqrt, one sincospi, two frames, one 16-byte store per channel (two 8-byte stores where the
// pair does not lie on a 16-byte boundary of the result: a window that starts on an odd frame).  No loads, no LDS.
// Compiled with -ffp-contract=off (build.py) like k_pointwise_math.hip and the hipRTC kernels, and calling the same
// randn_pair: the forms give the same values bit for bit.
#include "kcommon.h"

namespace so {

__global__ __launch_bounds__(kBlock) void k_randn_fill(const DPiece* __restrict__ pieces, int npieces,
                                                       const DLeaf* __restrict__ leaves, OutView out) {
    const int64_t bid = blockIdx.x;
    int lo = 0, hi = npieces - 1;
    while (lo < hi) {  // wave-uniform binary search: piece owning this workgroup
        const int mid = (lo + hi + 1) >> 1;
        if (pieces[mid].block0 <= bid) lo = mid;
        else hi = mid - 1;
    }
    const DPiece P = pieces[lo];
    const DLeaf& L = leaves[fill_noise_leaf(P)];
    const int64_t df = L.df;
    const uint64_t seed = randn_seed(L), stream = randn_stream(L);
    // pairs of the piece: absolute frames [a + df, b + df) -> pair indices [(a + df) >> 1, (b - 1 + df) >> 1]
    const int64_t p = ((P.a + df) >> 1) + (bid - P.block0) * kBlock + threadIdx.x;
    if (p > ((P.b - 1 + df) >> 1)) return;
    double z0, z1;
    randn_pair(seed, stream, (uint64_t)p, z0, z1);
    if (fill_flags(P) & kFillRoundNoise) {
        z0 = (double)(float)z0;
        z1 = (double)(float)z1;
    }
    if (fill_scale_leaf(P) >= 0) {
        const double g = leaves[fill_scale_leaf(P)].v0;
        z0 = z0 * g;
        z1 = z1 * g;
    }
    if (fill_flags(P) & kFillRoundProduct) {
        z0 = (double)(float)z0;
        z1 = (double)(float)z1;
    }
    // the piece's frames of this pair (a range that starts or ends on an odd absolute frame keeps one half)
    const int64_t n0 = 2 * p - df;
    const bool ok0 = n0 >= P.a && n0 < P.b, ok1 = n0 + 1 >= P.a && n0 + 1 < P.b;
    for (int c = P.c0; c < P.c1; ++c) {
        const int64_t off = (int64_t)c * out.cstride + n0 * out.fstride;
        if (out.dtype == SO_F64) {
            double* o = (double*)out.base + off;
            if (ok0 && ok1 && out.fstride == 1 && ((uintptr_t)o & 15) == 0) {
                double2 w;
                w.x = z0;
                w.y = z1;
                *reinterpret_cast<double2*>(o) = w;
            } else {
                if (ok0) o[0] = z0;
                if (ok1) o[out.fstride] = z1;
            }
        } else {  // a Float32 destination rounds at the store
            float* o = (float*)out.base + off;
            if (ok0 && ok1 && out.fstride == 1 && ((uintptr_t)o & 7) == 0) {
                float2 w;
                w.x = (float)z0;
                w.y = (float)z1;
                *reinterpret_cast<float2*>(o) = w;
            } else {
                if (ok0) o[0] = (float)z0;
                if (ok1) o[out.fstride] = (float)z1;
            }
        }
    }
}

void launch_randn_fill(const DPiece* d_pieces, int npieces, int64_t nblocks, const DLeaf* d_leaves, OutView out, hipStream_t st) {
    if (nblocks <= 0) return;
    hipLaunchKernelGGL(k_randn_fill, dim3((unsigned)nblocks), dim3(kBlock), 0, st, d_pieces, npieces, d_leaves, out);
}

}  // namespace so
