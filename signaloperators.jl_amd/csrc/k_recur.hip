// k_recur: `Recur(a, b)`, `OnePole`, `Smooth`, `PeakDecay` (signals.py; SO_NODE_RECUR of include/sigops.h) -- per channel the
// first-order scan y[n] = J(a[n], y[n-1], b[n]), y[0] = b[0], in Float64 over Cumsum's tree, which depends on the frame
// index only (DESIGN.md "Recur"; tests/recur_ref.py is the definition), so a window, a stream block and the whole sink
// give the same bits.  J(a, v, w), m = a * v rounded once: OP 0 m + w (this file is compiled with -ffp-contract=off: an
// FMA would round once where the definition rounds twice), OP 1 the greater of m and w, NaN if either is.  An element of
// the scan is a pair (product of the a, value):
//   run    j of a tile: p = a, r = b at the first frame itself, then p[n] = a[n] p[n-1], r[n] = J(a[n], r[n-1], b[n]);
//          the run's totals (A, B) are its last (p, r)
//   tile   an inclusive Kogge-Stone scan over the 64 totals, d = 1 .. 32: (A, B)[j] <- (A[j] A[j-d], J(A[j], B[j-d], B[j])),
//          a lane without a source keeps its pair; q = p A[j-1], t = J(p, B[j-1], r) in run j >= 1
//   chunk  tile k >= 1: u = J(q, c, t), Q = q P with (P, c) the last (Q, u) of tile k - 1
//   signal chunk k >= 1: y = J(Q, C, u); C = u[last] after chunk 0, J(Q[last], C, u[last]) after each later one
//
// Reduce-then-scan in three launches like k_cumsum.hip, no workgroup waits for another:
//   k_recur_totals  one workgroup per (chunk, channel), every chunk but the last: the chunk's last (Q, u) -> tot
//   k_recur_carry   one workgroup per channel: u[last] -> C in place, chunk after chunk (lane 0, out of LDS)
//   k_recur_scan    one workgroup per (chunk, channel): the chunk-local scan again, C applied, stored
// A signal of one chunk is the third launch alone.
//
// The resumed form (RecurArgs::k0 > 0, a stream's push) is k_cumsum.hip's: the rows start at chunk k0, blockIdx.x and the
// index into tot are relative to it, the carry starts from cin, the C that enters chunk k0, and leaves the C that enters
// the last chunk in cout; "chunk 0 of the signal" (y[0] = b[0], no C applied) is relative chunk 0 without a cin.
//
// A lane holds the 16 p and the 16 r of its run: 64 VGPRs a tile, so the four tiles a wave that k_cumsum keeps in
// registers do not fit.  A workgroup is sixteen waves instead, a wave ONE tile of the chunk: both inputs are read once a
// pass, nothing is reloaded, and one barrier separates the tile scans from the carries.  A wave's LDS image (kscan.h)
// takes a's tile and then b's, one after the other; sixteen images are 144 KiB, one workgroup a CU, four waves a SIMD.
// A constant a fills the lane's p with the constant and runs the very multiplications a row of it would.  The vector
// paths are taken on tiles that lie whole inside [0, n); every other index is clamped into [0, n) before an address is
// formed and every store is guarded (kscan.h).  Frame arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kscan.h"

namespace so {

constexpr int kRecurWaves = kCumsumTiles;  // a wave a tile

template <int OP>
__device__ __forceinline__ double rc_join(double a, double v, double w) {
    const double m = a * v;
    if (OP == 0) return m + w;
    if (m != m || w != w) return __builtin_nan("");
    return m >= w ? m : w;
}

// The wave's tile, the one that starts at frame f0: the lane's run -> its tile-local (q, t), left in (p, r).
template <int OP, typename TB, bool AROW, bool VL>
__device__ __forceinline__ void rc_tile(const RecurArgs& g, const double* __restrict__ ar, const TB* __restrict__ br, int64_t f0, double* img, int lane,
                                        double (&p)[kCumsumRun], double (&r)[kCumsumRun]) {
    if (AROW) {
        cs_load_tile<double, VL>(ar, 1, f0, g.n, img, lane, p);
    } else {
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) p[m] = g.ac;
    }
    cs_load_tile<TB, VL>(br, g.bfs, f0, g.n, img, lane, r);
#pragma unroll
    for (int m = 1; m < kCumsumRun; ++m) {
        r[m] = rc_join<OP>(p[m], r[m - 1], r[m]);  // (p[m] is still a[m])
        p[m] = p[m] * p[m - 1];
    }
    double A = p[kCumsumRun - 1], B = r[kCumsumRun - 1];
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const double As = __shfl_up(A, d, 64), Bs = __shfl_up(B, d, 64);
        if (lane >= d) {
            B = rc_join<OP>(A, Bs, B);
            A = A * As;
        }
    }
    const double Ab = __shfl_up(A, 1, 64), Bb = __shfl_up(B, 1, 64);
    if (lane >= 1) {
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) {
            r[m] = rc_join<OP>(p[m], Bb, r[m]);
            p[m] = p[m] * Ab;
        }
    }
}

// the last (Q, u) of tile `upto - 1`, chunk-local, from the tiles' own last (q, t): tile after tile
template <int OP>
__device__ __forceinline__ void rc_carry(const double* tq, const double* tt, int upto, double& P, double& c) {
    P = tq[0], c = tt[0];
    for (int k = 1; k < upto; ++k) {
        c = rc_join<OP>(tq[k], c, tt[k]);
        P = tq[k] * P;
    }
}

// Pass 1: the last (Q, u) of chunk blockIdx.x (a whole chunk: the last chunk of a row has no total).
template <int OP, typename TB, bool AROW, bool VL>
__global__ __launch_bounds__(64 * kRecurWaves) void k_recur_totals(RecurArgs g) {
    __shared__ __attribute__((aligned(16))) double image[kRecurWaves * kCumsumImage];
    __shared__ double tq[kCumsumTiles], tt[kCumsumTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int c = blockIdx.y;
    const double* __restrict__ ar = AROW ? g.a + (int64_t)c * g.acs : nullptr;
    const TB* __restrict__ br = (const TB*)g.b + (int64_t)c * g.bcs;
    double p[kCumsumRun], r[kCumsumRun];
    rc_tile<OP, TB, AROW, VL>(g, ar, br, chunk * kCumsumChunk + (int64_t)wave * kCumsumTile, image + wave * kCumsumImage, lane, p, r);
    if (lane == 63) tq[wave] = p[kCumsumRun - 1], tt[wave] = r[kCumsumRun - 1];
    __syncthreads();
    if (threadIdx.x == 0) {
        double P, u;
        rc_carry<OP>(tq, tt, kCumsumTiles, P, u);
        double* e = g.tot + 2 * ((int64_t)c * g.tot_pitch + chunk);
        e[0] = P, e[1] = u;
    }
}

// The carries: entry k of a channel (blockIdx.x) holds (Q[last], u[last]) of chunk k; its second word becomes the C that
// chunk k + 1 starts from: C[0] = u[last] of chunk 0, C[k] = J(Q[last], C[k - 1], u[last]).  The pairs go through LDS
// kBlock at a time; lane 0 walks them.
template <int OP>
__global__ __launch_bounds__(kBlock) void k_recur_carry(double* tot, int64_t pitch, int64_t count, const double* cin, double* cout) {
    __shared__ double q[kBlock], u[kBlock];
    double* row = tot + 2 * (int64_t)blockIdx.x * pitch;
    const bool resumed = cin != nullptr;
    double C = resumed ? cin[blockIdx.x] : 0.0;  // (lane 0's; from rest: replaced, not joined, by the first chunk's)
    for (int64_t k0 = 0; k0 < count; k0 += kBlock) {
        const int64_t k = k0 + threadIdx.x;
        if (k < count) q[threadIdx.x] = row[2 * k], u[threadIdx.x] = row[2 * k + 1];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (int)(count - k0 < kBlock ? count - k0 : kBlock);  // (the entries past m are not read back)
            for (int j = 0; j < m; ++j) {
                C = (!resumed && k0 == 0 && j == 0) ? u[0] : rc_join<OP>(q[j], C, u[j]);
                u[j] = C;
            }
        }
        __syncthreads();
        if (k < count) row[2 * k + 1] = u[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0 && cout != nullptr) cout[blockIdx.x] = C;  // the C that enters chunk `count`, the last one
}

// Pass 2: chunk blockIdx.x of channel blockIdx.y, stored.
template <int OP, typename TB, bool AROW, bool VL, bool VS>
__global__ __launch_bounds__(64 * kRecurWaves) void k_recur_scan(RecurArgs g) {
    __shared__ __attribute__((aligned(16))) double image[kRecurWaves * kCumsumImage];
    __shared__ double tq[kCumsumTiles], tt[kCumsumTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int c = blockIdx.y;
    const double* __restrict__ ar = AROW ? g.a + (int64_t)c * g.acs : nullptr;
    const TB* __restrict__ br = (const TB*)g.b + (int64_t)c * g.bcs;
    double* __restrict__ yr = g.y + (int64_t)c * g.ycs;
    double* img = image + wave * kCumsumImage;
    const int64_t f0 = chunk * kCumsumChunk + (int64_t)wave * kCumsumTile;  // the wave's tile
    const bool exists = f0 < g.n;  // (a tile past the end: nothing reads its totals)
    double p[kCumsumRun], r[kCumsumRun];
    if (exists) {
        rc_tile<OP, TB, AROW, VL>(g, ar, br, f0, img, lane, p, r);
        if (lane == 63) tq[wave] = p[kCumsumRun - 1], tt[wave] = r[kCumsumRun - 1];
    }
    __syncthreads();
    if (!exists) return;
    const bool chunks_before = chunk > 0 || g.cin != nullptr;  // (the absolute chunk: launch_recur passes cin where k0 > 0 only)
    if (wave > 0) {
        double P, cy;
        rc_carry<OP>(tq, tt, wave, P, cy);
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) {
            r[m] = rc_join<OP>(p[m], cy, r[m]);
            if (chunks_before) p[m] = p[m] * P;  // (Q: only a carry C reads it)
        }
    }
    if (chunks_before) {
        const double C = chunk > 0 ? g.tot[2 * ((int64_t)c * g.tot_pitch + chunk - 1) + 1] : g.cin[c];
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) r[m] = rc_join<OP>(p[m], C, r[m]);
    }
    cs_store_tile<VS>(yr, f0, g.n, img, lane, r);
}

static bool rc_aligned(const void* p, int64_t cs, int nch, size_t esz) {
    return (uintptr_t)p % 16 == 0 && (nch == 1 || (cs * (int64_t)esz) % 16 == 0);
}

template <int OP, typename TB, bool AROW>
static void launch_recur_t(const RecurArgs& g, int64_t nchunks, hipStream_t st) {
    // one switch for both inputs: a tile is loaded 16 bytes a lane where b AND the row of a allow it
    const bool vl = g.bfs == 1 && rc_aligned(g.b, g.bcs, g.nch, sizeof(TB)) && (!AROW || rc_aligned(g.a, g.acs, g.nch, 8));
    const bool vs = rc_aligned(g.y, g.ycs, g.nch, 8);
    const dim3 block(64 * kRecurWaves);
    if (nchunks > 1) {
        const dim3 grid((unsigned)(nchunks - 1), (unsigned)g.nch);
        if (vl) hipLaunchKernelGGL((k_recur_totals<OP, TB, AROW, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((k_recur_totals<OP, TB, AROW, false>), grid, block, 0, st, g);
        hipLaunchKernelGGL((k_recur_carry<OP>), dim3((unsigned)g.nch), dim3(kBlock), 0, st, g.tot, g.tot_pitch, nchunks - 1, g.cin, g.cout);
    }
    const dim3 grid((unsigned)nchunks, (unsigned)g.nch);
    if (vl && vs) hipLaunchKernelGGL((k_recur_scan<OP, TB, AROW, true, true>), grid, block, 0, st, g);
    else if (vl) hipLaunchKernelGGL((k_recur_scan<OP, TB, AROW, true, false>), grid, block, 0, st, g);
    else if (vs) hipLaunchKernelGGL((k_recur_scan<OP, TB, AROW, false, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((k_recur_scan<OP, TB, AROW, false, false>), grid, block, 0, st, g);
}

template <int OP>
static void launch_recur_op(const RecurArgs& g, int64_t nchunks, hipStream_t st) {
    if (g.a) {
        if (g.b_f32) launch_recur_t<OP, float, true>(g, nchunks, st);
        else launch_recur_t<OP, double, true>(g, nchunks, st);
    } else {
        if (g.b_f32) launch_recur_t<OP, float, false>(g, nchunks, st);
        else launch_recur_t<OP, double, false>(g, nchunks, st);
    }
}

int launch_recur(const RecurArgs& g0, hipStream_t st) {
    if (g0.n <= 0 || g0.nch <= 0) return 0;
    if (g0.k0 < 0 || (g0.k0 > 0 && g0.cin == nullptr)) return -1;
    RecurArgs g = g0;
    if (g.k0 == 0) g.cin = nullptr;  // (from rest: no record is read)
    const int64_t nchunks = (g.n + kCumsumChunk - 1) / kCumsumChunk;
    if (g.nch > 65535 || nchunks >= ((int64_t)1 << 31) || (g.op != 0 && g.op != 1)) return -1;
    if (nchunks > 1 && (g.tot == nullptr || g.tot_pitch < nchunks - 1)) return -1;
    if (g.op == 0) launch_recur_op<0>(g, nchunks, st);
    else launch_recur_op<1>(g, nchunks, st);
    return nchunks > 1 ? 3 : 1;
}

}  // namespace so
