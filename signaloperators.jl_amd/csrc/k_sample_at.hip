// k_sample_at: `SampleAt(x, pos)` (signals.py; SO_NODE_SAMPLEAT of include/sigops.h) -- the table `x` read at the positions
// a second signal gives, with linear interpolation: a variable delay, varispeed, a wavetable.  The value is NumPy's
//     np.interp(p, arange(N), float64(x[:, c]), left, right)        or        np.interp(p, arange(N), ..., period=N)
// operation for operation (kmath.h so_interp restates arr_interp for any knots; here the knots are the integers, so
// there is no search: j = floor(p), the knot distance is exactly 1.0 and the slope is f1 - f0).  Compiled with
// -ffp-contract=off (build.py): every operation is rounded on its own, as in k_pointwise_math.hip.
//
// Lanes run over (frame pair, channel): grid.x over pairs of frames, grid.y over channels.  A lane owns the two frames of
// a 16-byte word of its channel's result row: one 16-byte load of `pos` where the row of positions has the same parity,
// one 16-byte store; a row that starts 8 bytes off a 16-byte boundary (an odd window base, an odd pitch) shifts its pairs
// by one frame and the two ends of the range are stored as 8-byte halves (k_randn_fill.hip handles its pairs the same way).
// The table is read with two plain loads per frame, x[j] and x[j + 1], j clamped into the table BEFORE any address is
// formed: no position -- NaN, +-Inf, 1e300, negative -- makes a lane read outside [0, N).  Neighbouring lanes of a slowly
// moving position read neighbouring words (coalesced like a copy); random positions cost a cache line per read.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kmath.h"

namespace so {

template <typename TX, bool WRAP>
__device__ __forceinline__ double sample_at_one(const TX* __restrict__ xc, int64_t xfs, int64_t N, double p, double left, double right) {
    if (WRAP) {
        // NumPy: x % period, the knots -1, 0 .. N-1, N with fp = x[N-1], x[0 .. N-1], x[0]
        const double pm = so_m_remainder(p, (double)N);  // in [0, N], or NaN (p NaN or infinite)
        double pc = pm > 0.0 ? pm : 0.0;                 // (NaN -> 0)
        pc = pc < (double)N ? pc : (double)N;
        const int64_t j = (int64_t)pc;
        const int64_t j0 = j >= N ? 0 : j;
        const int64_t j1 = j0 + 1 >= N ? 0 : j0 + 1;
        const double f0 = (double)xc[j0 * xfs], f1 = (double)xc[j1 * xfs];
        if (pm != pm) return pm;
        const double xlo = (double)j;
        if (pm == xlo) return f0;
        const double s = f1 - f0;
        double r = s * (pm - xlo) + f0;
        if (r != r) {
            r = s * (pm - (xlo + 1.0)) + f1;
            if (r != r && f0 == f1) r = f0;
        }
        return r;
    }
    if (N == 1) {  // (NumPy's one-knot rule: a NaN position is neither left nor right of the knot)
        const double f = (double)xc[0];
        return p < 0.0 ? left : p > 0.0 ? right : f;
    }
    const double top = (double)(N - 1);
    double pc = p > 0.0 ? p : 0.0;  // (NaN -> 0)
    pc = pc < top ? pc : top;
    int64_t j = (int64_t)pc;
    j = j > N - 2 ? N - 2 : j;
    const double f0 = (double)xc[j * xfs], f1 = (double)xc[(j + 1) * xfs];
    if (p != p) return p;
    if (p < 0.0) return left;
    if (p > top) return right;
    if (p == top) return f1;
    const double xlo = (double)j;
    if (p == xlo) return f0;
    const double s = f1 - f0;  // (f1 - f0) / (xp[j + 1] - xp[j]), the knot distance exactly 1.0
    double r = s * (p - xlo) + f0;
    if (r != r) {  // NumPy's fall-backs where a non-finite table value makes that NaN
        r = s * (p - (xlo + 1.0)) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    return r;
}

template <typename TX, bool WRAP>
__global__ __launch_bounds__(kBlock) void k_sample_at(SampleAtArgs a) {
    const int c = blockIdx.y;
    double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
    const double* __restrict__ pr = a.pos + (int64_t)c * a.pcs;
    const TX* __restrict__ xc = (const TX*)a.x + (int64_t)c * a.xcs;
    const int64_t s = (int64_t)(((uintptr_t)yr >> 3) & 1);  // the row starts 8 bytes off a 16-byte boundary: pairs shift by one frame
    const int64_t i0 = 2 * ((int64_t)blockIdx.x * kBlock + threadIdx.x) - s;
    const bool ok0 = i0 >= 0 && i0 < a.n, ok1 = i0 + 1 >= 0 && i0 + 1 < a.n;
    if (!ok0 && !ok1) return;
    double p0 = 0.0, p1 = 0.0;
    if (ok0 && ok1 && (((uintptr_t)(pr + i0)) & 15) == 0) {
        const double2 w = *reinterpret_cast<const double2*>(pr + i0);
        p0 = w.x;
        p1 = w.y;
    } else {
        if (ok0) p0 = pr[i0];
        if (ok1) p1 = pr[i0 + 1];
    }
    if (a.relative) {  // one Float64 addition, the frame index exact
        p0 = (double)(a.base + i0) + p0;
        p1 = (double)(a.base + i0 + 1) + p1;
    }
    double r0 = 0.0, r1 = 0.0;
    if (ok0) r0 = sample_at_one<TX, WRAP>(xc, a.xfs, a.N, p0, a.left, a.right);
    if (ok1) r1 = sample_at_one<TX, WRAP>(xc, a.xfs, a.N, p1, a.left, a.right);
    if (ok0 && ok1) {
        double2 w;
        w.x = r0;
        w.y = r1;
        *reinterpret_cast<double2*>(yr + i0) = w;
    } else if (ok0) yr[i0] = r0;
    else yr[i0 + 1] = r1;
}

int launch_sample_at(const SampleAtArgs& a, hipStream_t st) {
    if (a.n <= 0 || a.nch <= 0) return 0;
    if (a.N < 1 || a.nch > 65535) return -1;
    const int64_t nblocks = (a.n / 2 + 1 + kBlock - 1) / kBlock;
    if (nblocks >= ((int64_t)1 << 31)) return -1;
    const dim3 grid((unsigned)nblocks, (unsigned)a.nch);
    if (a.x_f32) {
        if (a.wrap) hipLaunchKernelGGL((k_sample_at<float, true>), grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_sample_at<float, false>), grid, dim3(kBlock), 0, st, a);
    } else {
        if (a.wrap) hipLaunchKernelGGL((k_sample_at<double, true>), grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_sample_at<double, false>), grid, dim3(kBlock), 0, st, a);
    }
    return 1;
}

}  // namespace so
