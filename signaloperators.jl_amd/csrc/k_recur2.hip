// k_recur2: `Recur2(a1, a2, b)`, `Resonator`, `Sweep` (signals.py; SO_NODE_RECUR2 of include/sigops.h) -- per channel the
// second-order scan y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n], y[0] = b[0], y[1] = (a1[1] y[0] + a2[1] (+0.0)) + b[1], in
// Float64 over Cumsum's tree, which depends on the frame index only (DESIGN.md "Recur2"; tests/recur2_ref.py is the
// definition), so a window, a stream block and the whole sink give the same bits.  Every product and every sum is rounded
// on its own (this file is compiled with -ffp-contract=off).  An element of the scan is E = (M, v), the affine map
// s -> M s + v on the state s = (y[n], y[n-1]); in the joins and where it is applied to a state its six entries are
// double-doubles (R2Elem below):
//   run    j of a tile: M = [[a1, a2], [1, 0]], v = (b, +0.0) at the first frame; every further frame shifts, row 0 <-
//          a1 row 0 + a2 row 1 (b added to v0 last), row 1 <- the old row 0; the run's total is its last (M, v)
//   tile   an inclusive Kogge-Stone scan over the 64 totals, d = 1 .. 32: E[j] <- E[j] o E[j-d] (r2_join), a lane without
//          a source keeps its element; the tile's total K is lane 63's
//   chunk  the state that enters tile k >= 1 is K[k-1] applied to the state that entered tile k - 1 (tile 0: the state S that
//          entered the chunk; no state: the v of K[k-1] alone), the state that enters run j >= 1 is E[j-1] applied to the
//          tile's (no state: its v alone); G[0] = K[0], G[k] = K[k] o G[k-1] is the chunk's own composite
//   signal S behind chunk 0 is the v of its G[15]; behind chunk c >= 1 it is G[15] applied to the S that entered it
//   output the recurrence itself, walked over the run from the state that entered it; run 0 of the signal starts with
//          y[0] = b[0] and goes on from (y[0], +0.0)
//
// Reduce-then-scan in three launches like k_recur.hip, no workgroup waits for another:
//   k_recur2_totals  one workgroup per (chunk, channel), every chunk but the last: the chunk's G[15] -> tot (twelve doubles)
//   k_recur2_carry   one workgroup per channel: (v0, v1) -> the state that enters the chunk behind, in place, chunk after
//                    chunk (lane 0, out of LDS)
//   k_recur2_scan    one workgroup per (chunk, channel): the tile scans again, the entering states, the outputs, stored
// A signal of one chunk is the third launch alone.
//
// The resumed form (Recur2Args::k0 > 0, a stream's push) is k_cumsum.hip's: the rows start at chunk k0, blockIdx.x and the
// index into tot are relative to it, the carry starts from cin, the state (s0, s1) that enters chunk k0, and leaves the
// state that enters the last chunk in cout.  That state is the carry's own -- composites applied in double-doubles -- and
// not the last two outputs, which walk the loop.  "No state yet" (`have`, run 0 of the signal) is relative chunk 0 without
// a cin.
//
// Registers: a lane's run of a1, a2 and b is 48 doubles and its composite six more, which k_recur.hip's geometry --
// sixteen waves a workgroup, a wave ONE tile, 128 VGPRs a wave -- does not hold.  So b stays in the wave's LDS image
// (kscan.h): the lane reads its run there, 16 bytes a read, in the composite's walk and again in the outputs' walk, and
// writes y[n] over b[n] in its own row, from where the tile is stored; only a1 and a2 are kept in registers (64 VGPRs,
// none for constants), and not during the joins, whose double-doubles need the room: the scan reads the lane's runs of
// a1 and a2 again, straight from memory, before it walks the outputs.  Sixteen images are 144 KiB: one workgroup a CU, four waves a SIMD.  The vector paths are taken on
// tiles that lie whole inside [0, n); every other index is clamped into [0, n) before an address is formed and every
// store is guarded (kscan.h).  Frame arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kscan.h"

namespace so {

constexpr int kRecur2Waves = kCumsumTiles;  // a wave a tile

// An element: (M00, M01, M10, M11, v0, v1), every entry the unevaluated sum h + l of two Float64 (a double-double).  A run's
// total has l = 0; the joins and the applications to a state are formed by the error-free transformations below -- plain
// Float64 operations in the order tests/recur2_ref.py gives them, nothing fused -- because in plain Float64 the
// cancellation of a join's products costs poles next to z = 1 four digits more than a loop loses (DESIGN.md "Recur2").
struct R2Elem {
    double h[6], l[6];
};

struct R2dd {
    double h, l;
};

// a low word that is not finite (an operand was, or the split overflowed) is 0: the high word stays what plain arithmetic gives
__device__ __forceinline__ double r2_fin(double e) { return __builtin_isfinite(e) ? e : 0.0; }

__device__ __forceinline__ R2dd r2_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, r2_fin((a - (s - bb)) + (b - bb))};
}

__device__ __forceinline__ R2dd r2_quick_two_sum(double a, double b) {
    const double s = a + b;
    return {s, r2_fin(b - (s - a))};
}

__device__ __forceinline__ R2dd r2_two_prod(double a, double b) {  // Dekker's product through Veltkamp's split: no FMA
    const double p = a * b;
    const double ca = 134217729.0 * a, ah = ca - (ca - a), al = a - ah;
    const double cb = 134217729.0 * b, bh = cb - (cb - b), bl = b - bh;
    return {p, r2_fin((((ah * bh - p) + ah * bl) + al * bh) + al * bl)};
}

__device__ __forceinline__ R2dd r2_mul(R2dd x, R2dd y) {
    const R2dd t = r2_two_prod(x.h, y.h);
    return r2_quick_two_sum(t.h, r2_fin(t.l + (x.h * y.l + x.l * y.h)));
}

__device__ __forceinline__ R2dd r2_mul_d(R2dd x, double y) {
    const R2dd t = r2_two_prod(x.h, y);
    return r2_quick_two_sum(t.h, r2_fin(t.l + x.l * y));
}

__device__ __forceinline__ R2dd r2_add(R2dd x, R2dd y) {
    const R2dd t = r2_two_sum(x.h, y.h);
    return r2_quick_two_sum(t.h, r2_fin(t.l + (x.l + y.l)));
}

__device__ __forceinline__ R2dd r2_at(const R2Elem& e, int i) { return {e.h[i], e.l[i]}; }

// (M2, v2) o (M1, v1): the later element l after the earlier e
__device__ __forceinline__ R2Elem r2_join(const R2Elem& l, const R2Elem& e) {
    R2Elem o;
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // row i of l: entries 2 i, 2 i + 1 and v[i] = entry 4 + i
        const R2dd a = r2_at(l, 2 * i), b = r2_at(l, 2 * i + 1);
        const R2dd m0 = r2_add(r2_mul(a, r2_at(e, 0)), r2_mul(b, r2_at(e, 2)));
        const R2dd m1 = r2_add(r2_mul(a, r2_at(e, 1)), r2_mul(b, r2_at(e, 3)));
        const R2dd v = r2_add(r2_add(r2_mul(a, r2_at(e, 4)), r2_mul(b, r2_at(e, 5))), r2_at(l, 4 + i));
        o.h[2 * i] = m0.h, o.l[2 * i] = m0.l, o.h[2 * i + 1] = m1.h, o.l[2 * i + 1] = m1.l, o.h[4 + i] = v.h, o.l[4 + i] = v.l;
    }
    return o;
}

// the state behind the element e where (s0, s1) entered it (the high words of the double-doubles); no state: the v of e alone
__device__ __forceinline__ void r2_enter(const R2Elem& e, bool have, double& s0, double& s1) {
    const R2dd t0 = r2_add(r2_add(r2_mul_d(r2_at(e, 0), s0), r2_mul_d(r2_at(e, 1), s1)), r2_at(e, 4));
    const R2dd t1 = r2_add(r2_add(r2_mul_d(r2_at(e, 2), s0), r2_mul_d(r2_at(e, 3), s1)), r2_at(e, 5));
    s0 = have ? t0.h : e.h[4];
    s1 = have ? t1.h : e.h[5];
}

__device__ __forceinline__ R2Elem r2_shfl_up(const R2Elem& e, int d) {
    R2Elem o;
#pragma unroll
    for (int i = 0; i < 6; ++i) o.h[i] = __shfl_up(e.h[i], d, 64), o.l[i] = __shfl_up(e.l[i], d, 64);
    return o;
}

constexpr int kR2Words = 12;  // doubles an element takes in memory: the six high words, then the six low words

__device__ __forceinline__ void r2_put(double* p, const R2Elem& e) {
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = e.h[i], p[6 + i] = e.l[i];
}

__device__ __forceinline__ R2Elem r2_get(const double* p) {
    R2Elem e;
#pragma unroll
    for (int i = 0; i < 6; ++i) e.h[i] = p[i], e.l[i] = p[6 + i];
    return e;
}

// the lane's run of a row of coefficients again, straight from memory (the image holds b by then): the values cs_load_tile gave
template <bool VL>
__device__ __forceinline__ void r2_reload(const double* __restrict__ ar, int64_t f0, int64_t n, int lane, double (&x)[kCumsumRun]) {
    if (VL && f0 + kCumsumTile <= n) {
#pragma unroll
        for (int q = 0; q < kCumsumRun / 2; ++q) {
            const cs_v2d w = *reinterpret_cast<const cs_v2d*>(ar + f0 + lane * kCumsumRun + 2 * q);
            x[2 * q] = w.x, x[2 * q + 1] = w.y;
        }
    } else {
        const int64_t last = n - 1;
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) {
            const int64_t f = f0 + lane * kCumsumRun + m;
            x[m] = ar[f <= last ? f : last];  // (past the end: a copy of the last frame, as cs_fill_image reads it)
        }
    }
}

// The wave's tile, the one that starts at frame f0: a1 and a2 of the lane's run -> x1, x2 (AROW), b -> the image, and the
// inclusive prefix of the lane's run within the tile -> returned.
template <typename TB, bool AROW, bool VL>
__device__ __forceinline__ R2Elem r2_tile(const Recur2Args& g, const double* __restrict__ a1r, const double* __restrict__ a2r, const TB* __restrict__ br, int64_t f0,
                                          double* img, int lane, double (&x1)[kCumsumRun], double (&x2)[kCumsumRun]) {
    if (AROW) {
        cs_load_tile<double, VL>(a1r, 1, f0, g.n, img, lane, x1);
        cs_load_tile<double, VL>(a2r, 1, f0, g.n, img, lane, x2);
    }
    cs_fill_image<TB, VL>(br, g.bfs, f0, g.n, img, lane);
    const double* row = img + lane * kCumsumPitch;
    double m00 = 0.0, m01 = 0.0, m10 = 0.0, m11 = 0.0, v0 = 0.0, v1 = 0.0;
#pragma unroll
    for (int q = 0; q < kCumsumRun / 2; ++q) {
        const cs_v2d w = *reinterpret_cast<const cs_v2d*>(row + 2 * q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = 2 * q + h;
            const double c1 = AROW ? x1[m] : g.ac[0], c2 = AROW ? x2[m] : g.ac[1], bm = h ? w.y : w.x;
            if (m == 0) {
                m00 = c1, m01 = c2, m10 = 1.0, m11 = 0.0, v0 = bm, v1 = 0.0;
            } else {
                const double n00 = c1 * m00 + c2 * m10, n01 = c1 * m01 + c2 * m11, nv0 = (c1 * v0 + c2 * v1) + bm;
                m10 = m00, m11 = m01, v1 = v0;
                m00 = n00, m01 = n01, v0 = nv0;
            }
        }
    }
    R2Elem e;  // the run's total: the walk's Float64 values, low words 0
    e.h[0] = m00, e.h[1] = m01, e.h[2] = m10, e.h[3] = m11, e.h[4] = v0, e.h[5] = v1;
#pragma unroll
    for (int i = 0; i < 6; ++i) e.l[i] = 0.0;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const R2Elem s = r2_shfl_up(e, d);
        if (lane >= d) e = r2_join(e, s);
    }
    return e;
}

// G[upto - 1], chunk-local, from the tiles' totals: tile after tile
__device__ __forceinline__ R2Elem r2_carry(const double* tk, int upto) {
    R2Elem G = r2_get(tk);
    for (int k = 1; k < upto; ++k) G = r2_join(r2_get(tk + kR2Words * k), G);
    return G;
}

// Pass 1: G[15] of chunk blockIdx.x (a whole chunk: the last chunk of a row has no total).
template <typename TB, bool AROW, bool VL>
__global__ __launch_bounds__(64 * kRecur2Waves) void k_recur2_totals(Recur2Args g) {
    __shared__ __attribute__((aligned(16))) double image[kRecur2Waves * kCumsumImage];
    __shared__ double tk[kR2Words * kCumsumTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int c = blockIdx.y;
    const double* __restrict__ a1r = AROW ? g.a[0] + (int64_t)c * g.acs[0] : nullptr;
    const double* __restrict__ a2r = AROW ? g.a[1] + (int64_t)c * g.acs[1] : nullptr;
    const TB* __restrict__ br = (const TB*)g.b + (int64_t)c * g.bcs;
    double x1[kCumsumRun], x2[kCumsumRun];
    const R2Elem e = r2_tile<TB, AROW, VL>(g, a1r, a2r, br, chunk * kCumsumChunk + (int64_t)wave * kCumsumTile, image + wave * kCumsumImage, lane, x1, x2);
    if (lane == 63) r2_put(tk + kR2Words * wave, e);
    __syncthreads();
    if (threadIdx.x == 0) r2_put(g.tot + kR2Words * ((int64_t)c * g.tot_pitch + chunk), r2_carry(tk, kCumsumTiles));
}

// The carries: entry k of a channel (blockIdx.x) holds G[15] of chunk k; its (v0, v1) become the state S that chunk k + 1
// starts from: S[0] = the v of chunk 0 as it is, S[k] = G[15] of chunk k applied to S[k - 1].  The elements go through
// LDS kBlock at a time; lane 0 walks them.
__global__ __launch_bounds__(kBlock) void k_recur2_carry(double* tot, int64_t pitch, int64_t count, const double* cin, double* cout) {
    __shared__ double el[kR2Words * kBlock];
    double* row = tot + kR2Words * (int64_t)blockIdx.x * pitch;
    const bool resumed = cin != nullptr;
    double s0 = resumed ? cin[2 * blockIdx.x] : 0.0, s1 = resumed ? cin[2 * blockIdx.x + 1] : 0.0;  // (lane 0's; from rest: replaced, not joined, by the first chunk's)
    for (int64_t k0 = 0; k0 < count; k0 += kBlock) {
        const int64_t k = k0 + threadIdx.x;
        if (k < count) {
#pragma unroll
            for (int i = 0; i < kR2Words; ++i) el[kR2Words * threadIdx.x + i] = row[kR2Words * k + i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (int)(count - k0 < kBlock ? count - k0 : kBlock);  // (the entries past m are not read back)
            for (int j = 0; j < m; ++j) {
                r2_enter(r2_get(el + kR2Words * j), resumed || !(k0 == 0 && j == 0), s0, s1);
                el[kR2Words * j + 4] = s0, el[kR2Words * j + 5] = s1;
            }
        }
        __syncthreads();
        if (k < count) row[kR2Words * k + 4] = el[kR2Words * threadIdx.x + 4], row[kR2Words * k + 5] = el[kR2Words * threadIdx.x + 5];
        __syncthreads();
    }
    if (threadIdx.x == 0 && cout != nullptr) cout[2 * blockIdx.x] = s0, cout[2 * blockIdx.x + 1] = s1;  // the state that enters chunk `count`, the last one
}

// Pass 2: chunk blockIdx.x of channel blockIdx.y, stored.
template <typename TB, bool AROW, bool VL, bool VS>
__global__ __launch_bounds__(64 * kRecur2Waves) void k_recur2_scan(Recur2Args g) {
    __shared__ __attribute__((aligned(16))) double image[kRecur2Waves * kCumsumImage];
    __shared__ double tk[kR2Words * kCumsumTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int c = blockIdx.y;
    const double* __restrict__ a1r = AROW ? g.a[0] + (int64_t)c * g.acs[0] : nullptr;
    const double* __restrict__ a2r = AROW ? g.a[1] + (int64_t)c * g.acs[1] : nullptr;
    const TB* __restrict__ br = (const TB*)g.b + (int64_t)c * g.bcs;
    double* __restrict__ yr = g.y + (int64_t)c * g.ycs;
    double* img = image + wave * kCumsumImage;
    const int64_t f0 = chunk * kCumsumChunk + (int64_t)wave * kCumsumTile;  // the wave's tile
    const bool exists = f0 < g.n;  // (a tile past the end: nothing reads its total)
    double x1[kCumsumRun], x2[kCumsumRun];
    R2Elem e{};
    if (exists) {
        e = r2_tile<TB, AROW, VL>(g, a1r, a2r, br, f0, img, lane, x1, x2);
        if (lane == 63) r2_put(tk + kR2Words * wave, e);
    }
    __syncthreads();
    if (!exists) return;
    // the state that enters the tile, then the one that enters the lane's run
    bool have = chunk > 0 || g.cin != nullptr;  // (the absolute chunk: launch_recur2 passes cin where k0 > 0 only)
    double s0 = 0.0, s1 = 0.0;
    if (chunk > 0) {
        const double* S = g.tot + kR2Words * ((int64_t)c * g.tot_pitch + chunk - 1);
        s0 = S[4], s1 = S[5];
    } else if (have) {
        s0 = g.cin[2 * c], s1 = g.cin[2 * c + 1];
    }
    for (int k = 0; k < wave; ++k) {  // tile after tile: the total of tile k applied to the state that entered it
        r2_enter(r2_get(tk + kR2Words * k), have, s0, s1);
        have = true;
    }
    const R2Elem before = r2_shfl_up(e, 1);
    if (lane >= 1) {
        r2_enter(before, have, s0, s1);
        have = true;
    }
    if (AROW) {  // (the coefficients' registers were free during the joins)
        r2_reload<VL>(a1r, f0, g.n, lane, x1);
        r2_reload<VL>(a2r, f0, g.n, lane, x2);
    }
    // the outputs: the recurrence itself, y[n] written over b[n] in the lane's row of the image
    double* row = img + lane * kCumsumPitch;
#pragma unroll
    for (int q = 0; q < kCumsumRun / 2; ++q) {
        cs_v2d w = *reinterpret_cast<const cs_v2d*>(row + 2 * q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = 2 * q + h;
            const double c1 = AROW ? x1[m] : g.ac[0], c2 = AROW ? x2[m] : g.ac[1], bm = h ? w.y : w.x;
            double y = (c1 * s0 + c2 * s1) + bm;
            if (m == 0) {  // (run 0 of the signal: the sample itself, and on from (y[0], +0.0))
                y = have ? y : bm;
                s1 = have ? s0 : 0.0;
            } else {
                s1 = s0;
            }
            s0 = y;
            if (h) w.y = y;
            else w.x = y;
        }
        *reinterpret_cast<cs_v2d*>(row + 2 * q) = w;
    }
    cs_drain_image<VS>(yr, f0, g.n, img, lane);
}

static bool r2_aligned(const void* p, int64_t cs, int nch, size_t esz) {
    return (uintptr_t)p % 16 == 0 && (nch == 1 || (cs * (int64_t)esz) % 16 == 0);
}

template <typename TB, bool AROW>
static void launch_recur2_t(const Recur2Args& g, int64_t nchunks, hipStream_t st) {
    // one switch for the three inputs: a tile is loaded 16 bytes a lane where b AND both rows of coefficients allow it
    const bool vl = g.bfs == 1 && r2_aligned(g.b, g.bcs, g.nch, sizeof(TB)) && (!AROW || (r2_aligned(g.a[0], g.acs[0], g.nch, 8) && r2_aligned(g.a[1], g.acs[1], g.nch, 8)));
    const bool vs = r2_aligned(g.y, g.ycs, g.nch, 8);
    const dim3 block(64 * kRecur2Waves);
    if (nchunks > 1) {
        const dim3 grid((unsigned)(nchunks - 1), (unsigned)g.nch);
        if (vl) hipLaunchKernelGGL((k_recur2_totals<TB, AROW, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((k_recur2_totals<TB, AROW, false>), grid, block, 0, st, g);
        hipLaunchKernelGGL(k_recur2_carry, dim3((unsigned)g.nch), dim3(kBlock), 0, st, g.tot, g.tot_pitch, nchunks - 1, g.cin, g.cout);
    }
    const dim3 grid((unsigned)nchunks, (unsigned)g.nch);
    if (vl && vs) hipLaunchKernelGGL((k_recur2_scan<TB, AROW, true, true>), grid, block, 0, st, g);
    else if (vl) hipLaunchKernelGGL((k_recur2_scan<TB, AROW, true, false>), grid, block, 0, st, g);
    else if (vs) hipLaunchKernelGGL((k_recur2_scan<TB, AROW, false, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((k_recur2_scan<TB, AROW, false, false>), grid, block, 0, st, g);
}

int launch_recur2(const Recur2Args& g0, hipStream_t st) {
    if (g0.n <= 0 || g0.nch <= 0) return 0;
    if (g0.k0 < 0 || (g0.k0 > 0 && g0.cin == nullptr)) return -1;
    Recur2Args g = g0;
    if (g.k0 == 0) g.cin = nullptr;  // (from rest: no record is read)
    const int64_t nchunks = (g.n + kCumsumChunk - 1) / kCumsumChunk;
    if (g.nch > 65535 || nchunks >= ((int64_t)1 << 31)) return -1;
    if ((g.a[0] == nullptr) != (g.a[1] == nullptr)) return -1;  // (both rows, or both constants)
    if (nchunks > 1 && (g.tot == nullptr || g.tot_pitch < nchunks - 1)) return -1;
    if (g.a[0]) {
        if (g.b_f32) launch_recur2_t<float, true>(g, nchunks, st);
        else launch_recur2_t<double, true>(g, nchunks, st);
    } else {
        if (g.b_f32) launch_recur2_t<float, false>(g, nchunks, st);
        else launch_recur2_t<double, false>(g, nchunks, st);
    }
    return nchunks > 1 ? 3 : 1;
}

}  // namespace so
