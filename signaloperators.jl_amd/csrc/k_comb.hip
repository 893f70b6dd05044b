// k_comb: `Comb(x, d, g)` / `Allpass(x, d, g)` (signals.py; SO_NODE_COMB of include/sigops.h) -- a feedback delay line of D
// frames.  Per channel, with xd = x[n - D] and yd = y[n - D] where n >= D and +0.0 before that,
//     y[n] = (b0 * x[n] + bD * xd) + a * yd
// every product and every sum rounded on its own (-ffp-contract=off, build.py), a term whose coefficient is exactly 0.0
// left out.  Frame n depends on frame n - D only, so the D residue classes of a channel are independent first-order
// recurrences: a lane that walks one class in order computes exactly what a sequential loop computes, bit for bit.
//
// Lanes run over (residue r in [0, D), channel): grid.x over blocks of kBlock residues, grid.y over channels.  A lane
// walks n = r, r + D, r + 2D, ... while n < a.n and carries xd and yd in registers: one read and one write per sample,
// neighbouring lanes on neighbouring words (512 contiguous bytes per wave and step where x has unit frame stride).  The
// only dependence between the steps of a lane runs through those two registers, so the loads are independent: the loads of
// kCombUnroll steps are issued before the arithmetic that consumes them (K1's chain path keeps eight in flight the same
// way).  The tail of a class -- fewer than kCombUnroll steps left -- clamps each frame index into [0, a.n) BEFORE an
// address is formed (k_sample_at.hip clamps its table index the same way) and stores under a guard: no lane forms an
// address outside its row for any D, a.n or r.  Frame arithmetic is 64-bit throughout; launch_comb passes D <= a.n (a
// longer delay leaves every class with one frame, as D = a.n does), so n + kCombUnroll * D cannot overflow.
//
// The resumed form (k_comb_resume; CombArgs::r, cin, cout; a stream's push): the rows start at frame r of the signal and
// lane j walks the class of frame r + j, residue (r + j) mod D, from the (xd, yd) its entry of the record cin holds --
// the x and the y of the class's last frame before r, +0.0 where it has none -- and leaves the pair it ends with in cout.
// The grid runs over all D classes, not min(D, n): a class without a frame in [r, r + n) -- a delay longer than what a push
// adds -- copies its entry from cin to cout.  cin and cout are different records and every entry of cout is written by
// exactly one lane with plain stores, so the same launch twice gives the same bytes.  launch_comb takes D < 2^40 there.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace so {

template <bool FF, bool FB>
__device__ __forceinline__ double comb_step(double x0, double& xd, double& yd, double b0, double bD, double a) {
    double t = b0 * x0;
    if (FF) t = t + bD * xd;
    if (FB) t = t + a * yd;
    xd = x0;
    yd = t;
    return t;
}

// the frames r, r + D, r + 2D, ... <= a.n - 1 of channel c, from (xd, yd), which leave as the class's last x and y
template <typename TX, bool FF, bool FB>
__device__ __forceinline__ void comb_walk(const CombArgs& a, int c, int64_t r, double& xd, double& yd) {
    const TX* __restrict__ xc = (const TX*)a.x + (int64_t)c * a.xcs;
    double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
    const int64_t D = a.D, xfs = a.xfs, last = a.n - 1;
    const double b0 = a.b0, bD = a.bD, g = a.a;
    int64_t n = r;
    TX v[kCombUnroll];
    while (n + (kCombUnroll - 1) * D <= last) {  // kCombUnroll whole steps
#pragma unroll
        for (int u = 0; u < kCombUnroll; ++u) v[u] = xc[(n + u * D) * xfs];
#pragma unroll
        for (int u = 0; u < kCombUnroll; ++u) yr[n + u * D] = comb_step<FF, FB>((double)v[u], xd, yd, b0, bD, g);
        n += kCombUnroll * D;
    }
    if (n > last) return;
#pragma unroll
    for (int u = 0; u < kCombUnroll - 1; ++u) {  // the tail: at most kCombUnroll - 1 steps
        const int64_t i = n + u * D;
        v[u] = xc[(i <= last ? i : last) * xfs];
    }
#pragma unroll
    for (int u = 0; u < kCombUnroll - 1; ++u) {
        const int64_t i = n + u * D;
        if (i <= last) yr[i] = comb_step<FF, FB>((double)v[u], xd, yd, b0, bD, g);
    }
}

template <typename TX, bool FF, bool FB>
__global__ __launch_bounds__(kBlock) void k_comb(CombArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.D || r >= a.n) return;
    double xd = 0.0, yd = 0.0;
    comb_walk<TX, FF, FB>(a, blockIdx.y, r, xd, yd);
}

template <typename TX, bool FF, bool FB>
__global__ __launch_bounds__(kBlock) void k_comb_resume(CombArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.D) return;
    const int c = blockIdx.y;
    const int64_t e = 2 * ((int64_t)c * a.D + (a.r + j) % a.D);  // the entry of the class of frame r + j
    double xd = 0.0, yd = 0.0;
    if (a.cin != nullptr) xd = a.cin[e], yd = a.cin[e + 1];
    if (j < a.n) comb_walk<TX, FF, FB>(a, c, j, xd, yd);
    if (a.cout != nullptr) a.cout[e] = xd, a.cout[e + 1] = yd;
}

template <typename TX>
static void launch_comb_t(const CombArgs& a, dim3 grid, hipStream_t st) {
    const bool ff = a.bD != 0.0, fb = a.a != 0.0;
    if (a.r > 0 || a.cout != nullptr) {
        if (ff && fb) hipLaunchKernelGGL((k_comb_resume<TX, true, true>), grid, dim3(kBlock), 0, st, a);
        else if (ff) hipLaunchKernelGGL((k_comb_resume<TX, true, false>), grid, dim3(kBlock), 0, st, a);
        else if (fb) hipLaunchKernelGGL((k_comb_resume<TX, false, true>), grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_comb_resume<TX, false, false>), grid, dim3(kBlock), 0, st, a);
        return;
    }
    if (ff && fb) hipLaunchKernelGGL((k_comb<TX, true, true>), grid, dim3(kBlock), 0, st, a);
    else if (ff) hipLaunchKernelGGL((k_comb<TX, true, false>), grid, dim3(kBlock), 0, st, a);
    else if (fb) hipLaunchKernelGGL((k_comb<TX, false, true>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_comb<TX, false, false>), grid, dim3(kBlock), 0, st, a);
}

int launch_comb(const CombArgs& a0, hipStream_t st) {
    if (a0.n <= 0 || a0.nch <= 0) return 0;
    if (a0.D < 1 || a0.nch > 65535) return -1;
    if (a0.r < 0 || (a0.r > 0 && a0.cin == nullptr)) return -1;
    CombArgs a = a0;
    if (a.r == 0) a.cin = nullptr;  // (from rest: no record is read)
    const bool resumed = a.r > 0 || a.cout != nullptr;
    if (resumed && a.D >= ((int64_t)1 << 40)) return -1;  // (the records have 2 D doubles a channel; n + kCombUnroll * D stays in range)
    if (!resumed) a.D = a.D < a.n ? a.D : a.n;  // (a delay of a.n frames or more: every class is its first frame)
    const int64_t nblocks = (a.D + kBlock - 1) / kBlock;
    if (nblocks >= ((int64_t)1 << 31)) return -1;
    const dim3 grid((unsigned)nblocks, (unsigned)a.nch);
    if (a.x_f32) launch_comb_t<float>(a, grid, st);
    else launch_comb_t<double>(a, grid, st);
    return 1;
}

}  // namespace so
