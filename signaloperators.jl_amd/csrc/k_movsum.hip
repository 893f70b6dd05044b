// k_movsum: `MovingSum(x, w)` / `MovingMean(x, w)` / `MovingRMS(x, w)` (signals.py; SO_NODE_MOVSUM of include/sigops.h) --
// sliding-window sums in Float64 over ONE summation tree fixed by the absolute frame numbers of x (tests/movingsum_ref.py is
// the definition; DESIGN.md "Moving sums").  Compiled with -ffp-contract=off: every + below is one rounded addition.
//
// Frames.  Input frame i in [0, n_in) is frame abs0 + i of x.  The addend of a frame is the sample widened to Float64 (its
// square for the rms, the product rounded once); what lies outside [0, n_in) is -0.0, the additive identity, so padding
// equals clipping.  (Frames of x below abs0 or past abs0 + n_in that exist but were not loaded are padded too: no window
// of the outputs asked for reaches them, and a table entry that does is never part of a cover -- stages.cpp.)
//
// Scans.  The LDS image holds 4096 addends and starts on a multiple of the segment length S in ABSOLUTE frames.  A lane
// takes a run of 16 neighbouring addends into registers (one addend of padding after every run spreads a half-wave over
// the banks), sums it left to right (right to left), and the run totals of a segment go through a Kogge-Stone scan in LDS:
// seg_scan is k_moving.hip's, with + in place of max -- the order of the additions IS the definition's (+ commutes bit
// for bit, so which operand comes first does not matter; it does not associate, so the tree may not change).
//
// Short windows (W - 1 <= kMsumHalo), k_movsum_short: the tile's 2048 windows, led in by the up to S - 1 frames back to a
// multiple of S: at most 2048 + 1024 + 1023 addends.  A window starts and ends in different segments with at most one
// whole segment between them: (Q(lo) + t) + P(hi), t that segment's total (the prefix at its last frame) or -0.0.
//
// Long windows (S = kMsumBlock), no workgroup waits for another: k_movsum_totals writes the total of every aligned block
// that holds an input frame (four blocks a workgroup, the same scan); k_movsum_level builds the aligned dyadic nodes of
// level l from level l - 1 (a child that holds no input frame is -0.0); k_movsum_long images the up to three blocks its
// tile's windows start in for Q and the three they end in for P and walks the canonical cover of the blocks in between: at
// block p the greatest l with 2^l | p and p + 2^l <= b, added left to right.  A node past the last block is -0.0 and is left
// out; a node of more levels than were built starts inside the input and reaches past it, and equals its leftmost built node.
//
// Addresses.  Every input index is clamped into [0, n_in) BEFORE an address is formed and every table index into its row;
// a 16-byte load is issued only for a group that lies whole inside the row, and only where the launcher found the row
// bases 16-byte aligned and the frame stride 1.  Stores are guarded by the tile's frame count.  launch_movsum clamps back
// and ahead to 2^61 for the index arithmetic (the segment length comes from the nominal window first): abs0 + n_in < 2^62.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace so {
namespace {

constexpr int kMsThreads = 256;
constexpr int kMsSpan = 4096;                         // addends of the LDS image
constexpr int kMsImg = kMsSpan + kMsSpan / kMsumRun;  // the image with one addend of padding after every run
constexpr int kMsOut = kMsumTile / kMsThreads;        // outputs of a lane
constexpr int kMsLongImg = 3 * kMsumBlock;            // the blocks a tile's windows start (end) in
constexpr int kMsBlockSh = 10;
static_assert(kMsSpan == kMsThreads * kMsumRun && kMsumRun == 16, "a lane's run is 16 addends");
static_assert(kMsumTile + kMsumHalo + kMsumBlock - 1 <= kMsSpan, "the short form's image: tile, halo and lead-in");
static_assert(kMsumHalo == kMsumBlock && (1 << kMsBlockSh) == kMsumBlock && kMsumBlock - 1 + kMsumTile <= kMsLongImg && kMsLongImg <= kMsSpan,
              "the short form ends where the segment is a block; a tile's windows start in three blocks at most");
static_assert((kMsImg + 2 * kMsThreads) * 8 <= 65536, "static LDS of at most 64 KiB");
__device__ __forceinline__ int pidx(int i) { return i + (i >> 4); }

template <typename F>
struct Vec;
template <>
struct Vec<float> {
    using V = float4;
    static constexpr int kVec = 4;
};
template <>
struct Vec<double> {
    using V = double2;
    static constexpr int kVec = 2;
};

template <typename F, bool SQ>
__device__ __forceinline__ double addend(F s) {
    const double d = (double)s;
    return SQ ? d * d : d;
}

// the addend of input frame i, -0.0 outside [0, n_in); the index is clamped before the address
template <typename F, bool SQ>
__device__ __forceinline__ double load_addend(const F* __restrict__ xr, int64_t xfs, int64_t n_in, int64_t i) {
    const bool inside = i >= 0 && i < n_in;
    const int64_t ic = i < 0 ? 0 : i < n_in ? i : n_in - 1;
    const F s = xr[ic * xfs];
    return inside ? addend<F, SQ>(s) : -0.0;
}

// a[pidx(k)] = the addend of input frame i0 + k for k in [0, cnt), -0.0 for k in [cnt, kMsSpan)
template <typename F, bool SQ>
__device__ __forceinline__ void load_image(double* a, const F* __restrict__ xr, int64_t xfs, int64_t n_in, int64_t i0, int cnt, bool vec) {
    const int tid = threadIdx.x;
    for (int k = cnt + tid; k < kMsSpan; k += kMsThreads) a[pidx(k)] = -0.0;
    if (!vec) {
        for (int k = tid; k < cnt; k += kMsThreads) a[pidx(k)] = load_addend<F, SQ>(xr, xfs, n_in, i0 + k);
        return;
    }
    constexpr int VE = Vec<F>::kVec;
    const int64_t ia = i0 - (((i0 % VE) + VE) % VE);  // the aligned group i0 lies in (i0 may be negative)
    const int ngroups = (int)((i0 + cnt - ia + VE - 1) / VE);
    for (int q = tid; q < ngroups; q += kMsThreads) {
        const int64_t is = ia + (int64_t)q * VE;
        const int k0 = (int)(is - i0);
        if (is >= 0 && is + VE <= n_in) {
            const typename Vec<F>::V v = *reinterpret_cast<const typename Vec<F>::V*>(xr + is);
            const F* e = reinterpret_cast<const F*>(&v);
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (k0 + k >= 0 && k0 + k < cnt) a[pidx(k0 + k)] = addend<F, SQ>(e[k]);
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (k0 + k >= 0 && k0 + k < cnt) a[pidx(k0 + k)] = load_addend<F, SQ>(xr, 1, n_in, is + k);
        }
    }
}

__device__ __forceinline__ void read_run(const double* img, double (&v)[kMsumRun]) {
#pragma unroll
    for (int e = 0; e < kMsumRun; ++e) v[e] = img[(int)threadIdx.x * (kMsumRun + 1) + e];
}
__device__ __forceinline__ void write_run(double* img, const double (&v)[kMsumRun]) {
#pragma unroll
    for (int e = 0; e < kMsumRun; ++e) img[(int)threadIdx.x * (kMsumRun + 1) + e] = v[e];
}

// Inclusive sums of the image inside aligned segments of S addends (a power of two, 1 .. kMsumBlock), v the lane's run:
// the prefix P (REV = false) or the suffix Q (REV) of the definition.  A segment shorter than a run is its own run.  Where
// a segment spans L = S / 16 > 1 lanes, the run totals go through the Kogge-Stone scan (tot: two rows of kMsThreads values,
// read from one and written to the other, one barrier a step: every lane of a segment takes step d at once), and each lane
// adds the scanned total of the run before (after) its own.  S is the same for every lane, so the barriers are uniform.
template <bool REV>
__device__ __forceinline__ void seg_scan(double (&v)[kMsumRun], int S, double* tot) {
    const int tid = threadIdx.x;
    if (!REV) {
#pragma unroll
        for (int e = 1; e < kMsumRun; ++e)
            if (e & (S - 1)) v[e] = v[e - 1] + v[e];
    } else {
#pragma unroll
        for (int e = kMsumRun - 2; e >= 0; --e)
            if ((e + 1) & (S - 1)) v[e] = v[e] + v[e + 1];
    }
    const int L = S / kMsumRun;  // lanes of a segment
    if (L <= 1) return;
    const int r = tid & (L - 1);  // the lane's place in its segment
    double x = REV ? v[0] : v[kMsumRun - 1];
    int p = 0;
    tot[tid] = x;
    __syncthreads();
    for (int d = 1; d < L; d <<= 1) {
        const bool ok = REV ? r + d < L : r >= d;
        if (ok) x = REV ? x + tot[p * kMsThreads + tid + d] : tot[p * kMsThreads + tid - d] + x;
        p ^= 1;
        tot[p * kMsThreads + tid] = x;
        __syncthreads();
    }
    const bool has = REV ? r + 1 < L : r >= 1;
    if (has) {
        const double c = tot[p * kMsThreads + (REV ? tid + 1 : tid - 1)];
#pragma unroll
        for (int e = 0; e < kMsumRun; ++e) v[e] = REV ? v[e] + c : c + v[e];
    }
}

// sum -> the node's value: the mean divides by the frames of the window [lo, hi] (input frames) clipped to [0, n_in), the
// rms takes the square root of that quotient; one IEEE division and one square root, each rounded once
template <int OP>
__device__ __forceinline__ double finish(double s, int64_t lo, int64_t hi, int64_t n_in) {
    if (OP == 0) return s;
    const int64_t l = lo > 0 ? lo : 0, h = hi < n_in - 1 ? hi : n_in - 1;
    const double q = s / (double)(h - l + 1);
    return OP == 2 ? sqrt(q) : q;
}

// tile frame of output (q, k) of a lane: groups of two neighbouring frames, group q at (tid + q * threads) * 2
__device__ __forceinline__ int out_frame(int q, int k) { return ((int)threadIdx.x + q * kMsThreads) * 2 + k; }

__device__ __forceinline__ void store_tile(double* __restrict__ yr, int64_t j0, int nt, const double* acc, bool vec) {
#pragma unroll
    for (int q = 0; q < kMsOut / 2; ++q) {
        const int jb = out_frame(q, 0);
        if (vec && jb + 2 <= nt) {
            *reinterpret_cast<double2*>(yr + j0 + jb) = make_double2(acc[q * 2], acc[q * 2 + 1]);
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (jb + k < nt) yr[j0 + jb + k] = acc[q * 2 + k];
        }
    }
}

template <typename F, int OP>
__global__ __launch_bounds__(kMsThreads) void k_movsum_short(MovsumArgs a, int vx, int vy) {
    __shared__ double img[kMsImg];
    __shared__ double tot[2 * kMsThreads];
    const int c = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kMsumTile;
    const int nt = (int)(a.n_out - j0 < kMsumTile ? a.n_out - j0 : kMsumTile);
    const int W = (int)(a.back + a.ahead) + 1;  // <= kMsumHalo + 1
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
    const int64_t lo0 = j0 + a.off - a.back;  // the input frame the tile's first window starts at (may be negative)
    double acc[kMsOut];
    if (W == 1) {
        load_image<F, OP == 2>(img, xr, a.xfs, a.n_in, lo0, nt, vx != 0);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kMsOut / 2; ++q)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int jb = out_frame(q, k), jl = jb < nt ? jb : nt - 1;
                acc[q * 2 + k] = finish<OP>(img[pidx(jl)], lo0 + jl, lo0 + jl, a.n_in);
            }
        store_tile(yr, j0, nt, acc, vy != 0);
        return;
    }
    // segments of S = the greatest power of two <= W - 1 in absolute frames: the image starts `lead` frames before the
    // first window, on a multiple of S (two's complement: & is the floor's remainder for a negative frame too)
    const int sh = 31 - __builtin_clz(W - 1), S = 1 << sh;
    const int lead = (int)((a.abs0 + lo0) & (int64_t)(S - 1));
    const int cnt = lead + nt + W - 1;  // <= kMsSpan - 1; the window of tile frame jl is the image's [lead + jl, lead + jl + W - 1]
    load_image<F, OP == 2>(img, xr, a.xfs, a.n_in, lo0 - lead, cnt, vx != 0);
    __syncthreads();
    double orig[kMsumRun], v[kMsumRun];
    read_run(img, orig);
#pragma unroll
    for (int e = 0; e < kMsumRun; ++e) v[e] = orig[e];
    seg_scan<true>(v, S, tot);
    write_run(img, v);  // (a lane overwrites the addends it alone has read)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMsOut / 2; ++q)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int jb = out_frame(q, k);
            acc[q * 2 + k] = img[pidx(lead + (jb < nt ? jb : nt - 1))];  // Q(lo) (clamped; the store is guarded)
        }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kMsumRun; ++e) v[e] = orig[e];
    seg_scan<false>(v, S, tot);
    write_run(img, v);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMsOut / 2; ++q)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int jb = out_frame(q, k), jl = jb < nt ? jb : nt - 1;
            const int il = lead + jl, ih = il + W - 1;
            // the whole segment in between, if there is one: its total is the prefix at its last frame; Q + -0.0 is Q
            const double t = (ih >> sh) - (il >> sh) == 2 ? img[pidx((((il >> sh) + 2) << sh) - 1)] : -0.0;
            const double s = (acc[q * 2 + k] + t) + img[pidx(ih)];
            acc[q * 2 + k] = finish<OP>(s, lo0 + jl, lo0 + jl + W - 1, a.n_in);
        }
    store_tile(yr, j0, nt, acc, vy != 0);
}

// level 0 of the table: t[m] = P((m + 1) B - 1) of every aligned block m in [m0, m0 + nb), four blocks a workgroup
template <typename F, bool SQ>
__global__ __launch_bounds__(kMsThreads) void k_movsum_totals(MovsumArgs a, int vx, int64_t m0, int64_t nb) {
    __shared__ double img[kMsImg];
    __shared__ double tot[2 * kMsThreads];
    constexpr int kPer = kMsSpan / kMsumBlock;  // blocks of an image
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kPer;
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    load_image<F, SQ>(img, xr, a.xfs, a.n_in, (m0 + b0) * kMsumBlock - a.abs0, kMsSpan, vx != 0);
    __syncthreads();
    double v[kMsumRun];
    read_run(img, v);
    seg_scan<false>(v, kMsumBlock, tot);
    constexpr int kLanes = kMsumBlock / kMsumRun;  // lanes of a block
    const int64_t b = b0 + tid / kLanes;
    if (tid % kLanes == kLanes - 1 && b < nb) a.tab[(int64_t)c * nb + b] = v[kMsumRun - 1];
}

// level l >= 1: node (l, q) = node (l - 1, 2 q) + node (l - 1, 2 q + 1) for every q in [m0 >> l, (m1 - 1) >> l]; a child
// outside level l - 1 holds no input frame and is -0.0.  Row l of the table starts at node (l, m0 >> l).
__global__ __launch_bounds__(kMsThreads) void k_movsum_level(double* tab, int l, int nch, int64_t m0, int64_t m1, int64_t nb) {
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kMsThreads + threadIdx.x;
    const int64_t q0 = m0 >> l, cnt = ((m1 - 1) >> l) - q0 + 1;
    if (i >= cnt) return;
    const int64_t p0 = m0 >> (l - 1), pcnt = ((m1 - 1) >> (l - 1)) - p0 + 1;
    const int64_t left = 2 * (q0 + i) - p0, right = left + 1;  // left >= -1, right <= pcnt
    const double* __restrict__ src = tab + ((int64_t)(l - 1) * nch + c) * nb;
    const double vl = src[left < 0 ? 0 : left], vr = src[right < pcnt ? right : pcnt - 1];
    tab[((int64_t)l * nch + c) * nb + i] = (left >= 0 ? vl : -0.0) + (right < pcnt ? vr : -0.0);
}

template <typename F, int OP>
__global__ __launch_bounds__(kMsThreads) void k_movsum_long(MovsumArgs a, int vx, int vy, int64_t m0, int64_t m1, int64_t nb, int levels, int64_t bcap) {
    __shared__ double img[kMsImg];
    __shared__ double tot[2 * kMsThreads];
    const int c = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kMsumTile;
    const int nt = (int)(a.n_out - j0 < kMsumTile ? a.n_out - j0 : kMsumTile);
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
    const double* __restrict__ tab = a.tab;
    // absolute frames.  A window that starts before frame 0 starts in block -1, which is all -0.0; one that ends in block
    // bcap (a power of two >= m1) or later ends in a block of -0.0, and its cover is the cover up to bcap
    auto lo_of = [&](int jl) { const int64_t l = a.abs0 + a.off + j0 + jl - a.back; return l > -1 ? l : (int64_t)-1; };
    auto hi_of = [&](int jl) { const int64_t h = a.abs0 + a.off + j0 + jl + a.ahead, cap = bcap << kMsBlockSh; return h < cap ? h : cap; };
    double v[kMsumRun], acc[kMsOut];
    // the blocks the windows start in: Q, and the whole blocks in between from the table
    const int64_t rs = (lo_of(0) >> kMsBlockSh) << kMsBlockSh;
    load_image<F, OP == 2>(img, xr, a.xfs, a.n_in, rs - a.abs0, kMsLongImg, vx != 0);
    __syncthreads();
    read_run(img, v);
    seg_scan<true>(v, kMsumBlock, tot);
    write_run(img, v);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMsOut / 2; ++q)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int jb = out_frame(q, k), jl = jb < nt ? jb : nt - 1;
            const int64_t lo = lo_of(jl), b = hi_of(jl) >> kMsBlockSh;
            int il = (int)(lo - rs);
            il = il < 0 ? 0 : il < kMsLongImg ? il : kMsLongImg - 1;  // (it lies inside: clamped all the same)
            double M = -0.0;  // -0.0 + v has the bits of v: the first node is taken as it is
            for (int64_t p = (lo >> kMsBlockSh) + 1; p < b && p < m1;) {
                const int tz = p == 0 ? 62 : __builtin_ctzll((unsigned long long)p);
                const int fl = 63 - __builtin_clzll((unsigned long long)(b - p));
                const int l = tz < fl ? tz : fl, le = l < levels ? l : levels;
                int64_t e = (p >> le) - (m0 >> le);
                e = e < 0 ? 0 : e < nb ? e : nb - 1;
                M = M + tab[((int64_t)le * a.nch + c) * nb + e];
                p += (int64_t)1 << l;
            }
            acc[q * 2 + k] = img[pidx(il)] + M;
        }
    __syncthreads();
    // the blocks the windows end in: P
    const int64_t re = (hi_of(0) >> kMsBlockSh) << kMsBlockSh;
    load_image<F, OP == 2>(img, xr, a.xfs, a.n_in, re - a.abs0, kMsLongImg, vx != 0);
    __syncthreads();
    read_run(img, v);
    seg_scan<false>(v, kMsumBlock, tot);
    write_run(img, v);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMsOut / 2; ++q)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int jb = out_frame(q, k), jl = jb < nt ? jb : nt - 1;
            int ih = (int)(hi_of(jl) - re);
            ih = ih < 0 ? 0 : ih < kMsLongImg ? ih : kMsLongImg - 1;
            const double s = acc[q * 2 + k] + img[pidx(ih)];
            const int64_t li = a.off + j0 + jl - a.back;
            acc[q * 2 + k] = finish<OP>(s, li, a.off + j0 + jl + a.ahead, a.n_in);
        }
    store_tile(yr, j0, nt, acc, vy != 0);
}

template <typename F, int OP>
int launch_movsum_t(const MovsumArgs& a, bool is_long, int vx, int vy, hipStream_t st) {
    const int64_t tiles = (a.n_out + kMsumTile - 1) / kMsumTile, nb = movsum_blocks(a.abs0, a.n_in);
    if (tiles >= ((int64_t)1 << 31) || nb >= ((int64_t)1 << 31)) return -1;
    const dim3 block(kMsThreads), grid((unsigned)tiles, (unsigned)a.nch);
    if (!is_long) {
        hipLaunchKernelGGL((k_movsum_short<F, OP>), grid, block, 0, st, a, vx, vy);
        return 1;
    }
    if (!a.tab) return -1;
    const int levels = movsum_levels(a.abs0, a.n_in, a.back, a.ahead);
    const int64_t m0 = a.abs0 / kMsumBlock, m1 = m0 + nb;
    int64_t bcap = 1;
    while (bcap < m1) bcap <<= 1;
    constexpr int kPer = kMsSpan / kMsumBlock;
    hipLaunchKernelGGL((k_movsum_totals<F, OP == 2>), dim3((unsigned)((nb + kPer - 1) / kPer), (unsigned)a.nch), block, 0, st, a, vx, m0, nb);
    for (int l = 1; l <= levels; ++l) {
        const int64_t cnt = ((m1 - 1) >> l) - (m0 >> l) + 1;
        hipLaunchKernelGGL(k_movsum_level, dim3((unsigned)((cnt + kMsThreads - 1) / kMsThreads), (unsigned)a.nch), block, 0, st, a.tab, l, (int)a.nch, m0, m1, nb);
    }
    hipLaunchKernelGGL((k_movsum_long<F, OP>), grid, block, 0, st, a, vx, vy, m0, m1, nb, levels, bcap);
    return 2 + levels;
}

template <typename F>
int launch_movsum_f(const MovsumArgs& a, bool is_long, int vx, int vy, hipStream_t st) {
    switch (a.op) {
    case 0: return launch_movsum_t<F, 0>(a, is_long, vx, vy, st);
    case 1: return launch_movsum_t<F, 1>(a, is_long, vx, vy, st);
    default: return launch_movsum_t<F, 2>(a, is_long, vx, vy, st);
    }
}

}  // namespace

int launch_movsum(const MovsumArgs& a0, hipStream_t st) {
    if (a0.n_out <= 0 || a0.nch <= 0) return 0;
    if (a0.nch > 65535 || a0.back < 0 || a0.ahead < 0 || a0.off < 0 || a0.abs0 < 0 || a0.n_in < 1 || a0.off > a0.n_in - a0.n_out || a0.op < 0 || a0.op > 2 ||
        a0.abs0 >= ((int64_t)1 << 62) - a0.n_in)
        return -1;
    MovsumArgs a = a0;
    const bool is_long = movsum_is_long(a.back, a.ahead);  // (the nominal window decides the form and the segment length)
    const int64_t cap = (int64_t)1 << 61;  // a longer reach ends in -0.0 all the same, and the cover up to bcap does not change
    a.back = a.back < cap ? a.back : cap;
    a.ahead = a.ahead < cap ? a.ahead : cap;
    const int64_t esz = a.x_f32 ? 4 : 8;
    const int vx = a.xfs == 1 && (uintptr_t)a.x % 16 == 0 && (a.nch == 1 || (a.xcs * esz) % 16 == 0);
    const int vy = (uintptr_t)a.y % 16 == 0 && (a.nch == 1 || (a.ycs * 8) % 16 == 0);
    return a.x_f32 ? launch_movsum_f<float>(a, is_long, vx, vy, st) : launch_movsum_f<double>(a, is_long, vx, vy, st);
}

}  // namespace so
