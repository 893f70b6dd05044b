// k_sample_at_fir: `SampleAt(x, pos, interp="cubic" | "sinc")` (signals.py; SO_NODE_SAMPLEAT i1 = 1 | 2 of include/sigops.h)
// -- the table `x` read at the positions a second signal gives through a four-point Catmull-Rom polynomial or through K taps
// of a 512-phase windowed-sinc table.  tests/sampleat_interp_ref.py is the definition, operation for operation; compiled
// with -ffp-contract=off (build.py): every product and every sum is rounded on its own, and the kernel evaluates `+` and
// `*` only -- the taps come from the host as bytes.
//
// The result discipline is k_sample_at.hip's: a lane owns the two frames of a 16-byte word of its channel's result row, one
// 16-byte load of `pos`, one 16-byte store, pairs shifted by one frame where the row starts 8 bytes off a 16-byte boundary.
// The position is clamped into the table BEFORE j = floor(p) is taken and every index j + o is clamped into [0, N) (walked
// modulo N under wrap) before an address is formed; left / right / NaN are selected afterwards, so no position -- NaN,
// +-Inf, 1e300, negative -- makes a lane read outside the table, and t = p - j lies in [0, 1), so the phase lies in
// [0, 512) and no lane reads outside the tap table either.
//
// k_sample_at_sinc<TX, WRAP, LDS>: the tap row of a frame is phase = floor(512 t) of the 513 rows h, and the same row of the
// 512 rows dh behind them.  LDS = false reads both rows where the plan put them (global memory; 1025 K doubles, L2-resident)
// on the grid of the linear kernel.  LDS = true (K <= 16, a result large enough to pay for the fill) is persistent: one
// workgroup of 1024 lanes per CU copies the table into LDS TRANSPOSED -- tap k of phase ph at double k * 513 + ph, the K
// rows of dh behind the K rows of h -- and walks the pairs of every channel with a grid stride.  Lanes of a half-wave
// read one tap k at their own phases: with the phase as the fast index, 32 phases that differ modulo 32 fall on 32
// different even banks of the 64 a ds_read_b64 sees (row-major rows of K = 16 doubles would all start on bank 0 or 32),
// and the row pitch of 513 doubles -- 512 phases, the 513th row of h, and with it an odd pitch -- keeps neighbouring taps
// too far apart, and off the 64-double stride, for the compiler to join them into ds_read2_b64 / ds_read2st64_b64, which
// move half the bytes per clock of ds_read_b64.
// Both forms issue the loads of four taps (x, h, dh) before the products that use them.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kcommon.h"
#include "kmath.h"

namespace so {

constexpr int kFirLdsBlock = 1024;
constexpr int kFirLdsMaxK = 16;                       // 2 * 16 rows of 513 doubles: 131328 bytes of the 160 KB
constexpr int kFirLdsPitch = kSampleAtPhases + 1;     // doubles between two taps of one phase in LDS
constexpr int64_t kFirLdsMinWork = (int64_t)1 << 17;  // frames x channels below which the fill costs more than it saves

// The clamped position of a frame: j = floor(pc), t = pc - j (exact).  Returns 0 where the arithmetic decides the result, 1
// where it is `over` whatever the table holds (left, right, a NaN position), 2 where it is x[0] by value (the one-knot rule
// of a table of one frame: a position that is neither left nor right of the knot, NaN included, as k_sample_at.hip has it).
template <bool WRAP>
__device__ __forceinline__ int fir_position(double p, int64_t N, double left, double right, int64_t& j, double& t, double& over) {
    if (WRAP) {
        const double pm = so_m_remainder(p, (double)N);  // in [0, N], or NaN (p NaN or infinite)
        double pc = pm > 0.0 ? pm : 0.0;                 // (NaN -> 0)
        pc = pc < (double)N ? pc : (double)N;
        j = (int64_t)pc;
        t = pc - (double)j;
        over = pm;
        return pm != pm ? 1 : 0;
    }
    const double top = (double)(N - 1);
    double pc = p > 0.0 ? p : 0.0;  // (NaN -> 0)
    pc = pc < top ? pc : top;
    j = (int64_t)pc;
    t = pc - (double)j;
    if (N == 1) {
        over = p < 0.0 ? left : right;
        return p < 0.0 || p > 0.0 ? 1 : 2;
    }
    over = p != p ? p : p < 0.0 ? left : right;
    return p != p || p < 0.0 || p > top ? 1 : 0;
}

// The table indices j + o for rising o: clamped into [0, N), or walked modulo N (a true modulo: a table shorter than the
// kernel is gone round several times).
template <bool WRAP>
struct FirIndex {
    int64_t i, N;
    __device__ __forceinline__ FirIndex(int64_t first, int64_t N_) : i(first), N(N_) {
        if (WRAP && (i < 0 || i >= N)) {
            i %= N;
            if (i < 0) i += N;
        }
    }
    __device__ __forceinline__ int64_t take() {
        const int64_t at = WRAP ? i : (i < 0 ? 0 : i > N - 1 ? N - 1 : i);
        ++i;
        if (WRAP && i == N) i = 0;
        return at;
    }
};

template <typename TX, bool WRAP>
__device__ __forceinline__ double fir_cubic(const TX* __restrict__ xc, int64_t xfs, int64_t N, int64_t j, double t) {
    FirIndex<WRAP> ix(j - 1, N);
    const int64_t am = ix.take(), a0 = ix.take(), a1 = ix.take(), a2 = ix.take();
    const double fm = (double)xc[am * xfs], f0 = (double)xc[a0 * xfs], f1 = (double)xc[a1 * xfs], f2 = (double)xc[a2 * xfs];
    const double c1 = 0.5 * (f1 - fm);
    const double c2 = ((fm - 2.5 * f0) + 2.0 * f1) - 0.5 * f2;
    const double c3 = 0.5 * (f2 - fm) + 1.5 * (f0 - f1);
    return ((c3 * t + c2) * t + c1) * t + f0;
}

// `h` and `dh`: the rows of the frame's phase.  The sum runs left to right from the first product.
template <typename TX, bool WRAP, int KS>
__device__ __forceinline__ double fir_sinc(const TX* __restrict__ xc, int64_t xfs, int64_t N, int64_t j, double alpha, const double* h, const double* dh, int K) {
    FirIndex<WRAP> ix(j - (K / 2 - 1), N);
    double acc;
    {
        const int64_t a0 = ix.take(), a1 = ix.take();
        const double x0 = (double)xc[a0 * xfs], x1 = (double)xc[a1 * xfs];
        const double h0 = h[0], h1 = h[(1) * KS], d0 = dh[0], d1 = dh[(1) * KS];
        acc = (h0 + alpha * d0) * x0;
        acc = acc + (h1 + alpha * d1) * x1;
    }
    int k = 2;
    for (; k + 4 <= K; k += 4) {
        const int64_t a0 = ix.take(), a1 = ix.take(), a2 = ix.take(), a3 = ix.take();
        const double x0 = (double)xc[a0 * xfs], x1 = (double)xc[a1 * xfs], x2 = (double)xc[a2 * xfs], x3 = (double)xc[a3 * xfs];
        const double h0 = h[(k) * KS], h1 = h[(k + 1) * KS], h2 = h[(k + 2) * KS], h3 = h[(k + 3) * KS];
        const double d0 = dh[(k) * KS], d1 = dh[(k + 1) * KS], d2 = dh[(k + 2) * KS], d3 = dh[(k + 3) * KS];
        acc = acc + (h0 + alpha * d0) * x0;
        acc = acc + (h1 + alpha * d1) * x1;
        acc = acc + (h2 + alpha * d2) * x2;
        acc = acc + (h3 + alpha * d3) * x3;
    }
    if (k < K) {  // (K even: two taps left)
        const int64_t a0 = ix.take(), a1 = ix.take();
        const double x0 = (double)xc[a0 * xfs], x1 = (double)xc[a1 * xfs];
        const double h0 = h[(k) * KS], h1 = h[(k + 1) * KS], d0 = dh[(k) * KS], d1 = dh[(k + 1) * KS];
        acc = acc + (h0 + alpha * d0) * x0;
        acc = acc + (h1 + alpha * d1) * x1;
    }
    return acc;
}

// One frame.  KIND 1: cubic; 2: sinc over `tab`: the plan's table (LDS = false: 513 rows h[phase][tap] of K doubles, then
// the 512 rows of dh) or its transposed image in LDS (LDS = true: tap k of phase ph at tab[k * kFirLdsPitch + ph], dh's K
// rows behind h's).
template <typename TX, bool WRAP, int KIND, bool LDS>
__device__ __forceinline__ double fir_one(const TX* __restrict__ xc, int64_t xfs, int64_t N, double p, double left, double right, const double* tab, int K) {
    int64_t j;
    double t, over;
    const int st = fir_position<WRAP>(p, N, left, right, j, t, over);
    double r;
    if (KIND == 1) {
        r = fir_cubic<TX, WRAP>(xc, xfs, N, j, t);
    } else {
        const double u = t * (double)kSampleAtPhases;  // exact; in [0, 512)
        const int ph = (int)u;
        const double alpha = u - (double)ph;
        if (LDS) r = fir_sinc<TX, WRAP, kFirLdsPitch>(xc, xfs, N, j, alpha, tab + ph, tab + K * kFirLdsPitch + ph, K);
        else r = fir_sinc<TX, WRAP, 1>(xc, xfs, N, j, alpha, tab + ph * K, tab + (kSampleAtPhases + 1 + ph) * K, K);
    }
    if (!WRAP && N == 1 && st == 2) return (double)xc[0];
    return st == 1 ? over : r;
}

// The pair of frames i0, i0 + 1 of channel c's row (either may lie outside [0, n)).
template <typename TX, bool WRAP, int KIND, bool LDS>
__device__ __forceinline__ void fir_pair(const SampleAtArgs& a, const double* tab, int K, const TX* __restrict__ xc, const double* __restrict__ pr,
                                         double* __restrict__ yr, int64_t i0) {
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
    // (a frame outside the range computes position 0.0 of the table and is not stored)
    const double r0 = fir_one<TX, WRAP, KIND, LDS>(xc, a.xfs, a.N, p0, a.left, a.right, tab, K);
    const double r1 = fir_one<TX, WRAP, KIND, LDS>(xc, a.xfs, a.N, p1, a.left, a.right, tab, K);
    if (ok0 && ok1) {
        double2 w;
        w.x = r0;
        w.y = r1;
        *reinterpret_cast<double2*>(yr + i0) = w;
    } else if (ok0) yr[i0] = r0;
    else yr[i0 + 1] = r1;
}

template <typename TX, bool WRAP>
__global__ __launch_bounds__(kBlock) void k_sample_at_cubic(SampleAtArgs a) {
    const int c = blockIdx.y;
    double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
    const int64_t s = (int64_t)(((uintptr_t)yr >> 3) & 1);  // the row starts 8 bytes off a 16-byte boundary: pairs shift by one frame
    fir_pair<TX, WRAP, 1, false>(a, nullptr, 4, (const TX*)a.x + (int64_t)c * a.xcs, a.pos + (int64_t)c * a.pcs, yr,
                                         2 * ((int64_t)blockIdx.x * kBlock + threadIdx.x) - s);
}

template <typename TX, bool WRAP, bool LDS>
__global__ __launch_bounds__(LDS ? kFirLdsBlock : kBlock) void k_sample_at_sinc(SampleAtFirArgs f) {
    const SampleAtArgs& a = f.a;
    const int K = f.K;
    if (!LDS) {
        const int c = blockIdx.y;
        double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
        const int64_t s = (int64_t)(((uintptr_t)yr >> 3) & 1);
        fir_pair<TX, WRAP, 2, false>(a, f.tab, K, (const TX*)a.x + (int64_t)c * a.xcs, a.pos + (int64_t)c * a.pcs, yr,
                                             2 * ((int64_t)blockIdx.x * kBlock + threadIdx.x) - s);
        return;
    }
    extern __shared__ double fir_lds[];  // 2 K rows of kFirLdsPitch doubles: h's taps, then dh's
    const int total = (2 * kSampleAtPhases + 1) * K;
    for (int e = threadIdx.x; e < total; e += kFirLdsBlock) {
        const int r = e / K, k = e - r * K;
        const int at = r <= kSampleAtPhases ? k * kFirLdsPitch + r : (K + k) * kFirLdsPitch + (r - (kSampleAtPhases + 1));
        fir_lds[at] = f.tab[e];
    }
    __syncthreads();
    const int64_t npairs = a.n / 2 + 1;
    for (int c = 0; c < a.nch; ++c) {
        double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
        const TX* __restrict__ xc = (const TX*)a.x + (int64_t)c * a.xcs;
        const double* __restrict__ pr = a.pos + (int64_t)c * a.pcs;
        const int64_t s = (int64_t)(((uintptr_t)yr >> 3) & 1);
        for (int64_t q = (int64_t)blockIdx.x * kFirLdsBlock + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * kFirLdsBlock)
            fir_pair<TX, WRAP, 2, true>(a, fir_lds, K, xc, pr, yr, 2 * q - s);
    }
}

bool sample_at_fir_uses_lds(const SampleAtFirArgs& f) {
    return f.kind == 2 && f.K <= kFirLdsMaxK && f.a.n * (int64_t)f.a.nch >= kFirLdsMinWork;
}

template <typename TX, bool WRAP>
static void launch_fir_one(const SampleAtFirArgs& f, const dim3& grid, hipStream_t st) {
    if (f.kind == 1) {
        hipLaunchKernelGGL((k_sample_at_cubic<TX, WRAP>), grid, dim3(kBlock), 0, st, f.a);
    } else if (!sample_at_fir_uses_lds(f)) {
        hipLaunchKernelGGL((k_sample_at_sinc<TX, WRAP, false>), grid, dim3(kBlock), 0, st, f);
    } else {
        static bool seen[64];
        static int cus[64];
        int dev = 0;
        (void)hipGetDevice(&dev);
        dev = dev < 0 ? 0 : (dev > 63 ? 63 : dev);
        if (first_use_on_device(seen)) {
            (void)hipFuncSetAttribute((const void*)k_sample_at_sinc<TX, WRAP, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            int n = 0;
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
            cus[dev] = n;
        }
        const int64_t npairs = f.a.n / 2 + 1;
        const int64_t want = (npairs + kFirLdsBlock - 1) / kFirLdsBlock;
        const size_t ldsb = (size_t)2 * f.K * kFirLdsPitch * sizeof(double);
        hipLaunchKernelGGL((k_sample_at_sinc<TX, WRAP, true>), dim3((unsigned)std::min<int64_t>(want, cus[dev])), dim3(kFirLdsBlock), ldsb, st, f);
    }
}

int launch_sample_at_fir(const SampleAtFirArgs& f, hipStream_t st) {
    const SampleAtArgs& a = f.a;
    if (a.n <= 0 || a.nch <= 0) return 0;
    if (a.N < 1 || a.nch > 65535) return -1;
    if (f.kind != 1 && (f.kind != 2 || f.K < 4 || f.K > 64 || (f.K & 1) || !f.tab)) return -1;
    const int64_t nblocks = (a.n / 2 + 1 + kBlock - 1) / kBlock;
    if (nblocks >= ((int64_t)1 << 31)) return -1;
    const dim3 grid((unsigned)nblocks, (unsigned)a.nch);
    if (a.x_f32) {
        if (a.wrap) launch_fir_one<float, true>(f, grid, st);
        else launch_fir_one<float, false>(f, grid, st);
    } else {
        if (a.wrap) launch_fir_one<double, true>(f, grid, st);
        else launch_fir_one<double, false>(f, grid, st);
    }
    return 1;
}

}  // namespace so
