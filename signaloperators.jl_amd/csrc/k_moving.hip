// k_moving: `MovingMax(x, w)` / `MovingMin(x, w)` (signals.py; SO_NODE_MOVING of include/sigops.h) -- sliding-window extrema.
// Per channel, output j in [0, n_out) is the greatest (least) of the input frames
//     [max(0, j + off - back), min(n_in - 1, j + off + ahead)]
// under the order -Inf < .. < -0.0 < +0.0 < .. < +Inf, NaN if any of them is NaN, as a bit copy of that sample.
//
// Comparison.  A sample becomes a signed integer KEY of its own width that orders the same way: a non-negative float's
// bits are its key, a negative float's key is its bits with every bit but the sign inverted (-0.0 -> -1, -Inf just above
// the least integer), a NaN's key is the greatest integer.  The least integer is no sample's key: it pads what lies
// outside the signal.  The minimum is the maximum of the negated samples, negated: the sign bit is flipped on the way in
// and on the way out.  Integer max rounds nothing and is associative and commutative, so every decomposition below gives
// the definition's bits; the key converts back at the store (the greatest integer is a NaN pattern).
//
// Scans.  The LDS image holds up to 2 kMovTile keys.  A lane takes a run of 16 neighbouring keys into registers, scans it
// there, and the 256 run totals go through a Kogge-Stone scan in LDS (seg_scan): prefix or suffix maxima inside aligned
// segments of a power-of-two length cost one read and one write of the image and at most 8 barriers, whatever the length.
//
// Short windows (W - 1 <= kMovHalo), k_moving_short: a workgroup takes kMovTile outputs of one channel and loads the
// kMovTile + W - 1 keys they read into LDS.  With segments of S = the greatest power of two <= W - 1 (van Herk / Gil-Werman
// with a segment shorter than the window), a window starts and ends in different segments with at most one whole segment
// between them: it is the suffix maximum at its start, that segment's maximum (the prefix at its last key) and the prefix
// maximum at its end.  The lane keeps its run in registers, so the image is loaded once for both scans.
//
// Long windows, three kernels, no workgroup waits for another: k_moving_blockmax writes the maximum of every aligned block
// of kMovTile INPUT frames; k_moving_level builds level l of a sparse table over them (the maximum of 2^l blocks from b on)
// from level l - 1, one launch a level, only the levels a window of this length can ask for; k_moving_long forms an output
// from the suffix maximum of the block its window starts in, two table entries for the whole blocks in between and the
// prefix maximum of the block it ends in.  The starts of a tile's windows lie in two neighbouring blocks, and so do their
// ends: the workgroup recomputes those two blocks' suffix (prefix) maxima in LDS (segments of kMovTile).
// W > kMovTile + 1 here, so a window lies inside ONE block only where the signal clips it: at the
// front it starts on the block's first frame (the prefix alone), at the back it ends on the signal's last (the suffix).
//
// Addresses.  Every input index is clamped into [0, n_in) BEFORE an address is formed, and what lay outside becomes the
// padding key (k_comb.hip and k_sample_at.hip clamp the same way); a 16-byte load is issued only for a group that lies
// whole inside the row, and only where the launcher found the row bases 16-byte aligned and the frame stride 1.  Stores
// are guarded by the tile's frame count.  launch_moving clamps back and ahead to n_in, so no sum of frame indices exceeds
// 3 n_in; frame arithmetic is 64-bit, indices into LDS are int (< 2 kMovTile).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "kkey.h"

namespace so {
namespace {

constexpr int kMovThreads = kKeyThreads;  // (kkey.h: Key, to_key, from_key, pidx, load_key and load_image)
constexpr int kMovSpan = kMovTile + kMovHalo;      // keys of the LDS image
constexpr int kMovRun = kMovSpan / kMovThreads;    // neighbouring keys of the image a lane scans in registers
constexpr int kMovImg = kMovSpan + kMovSpan / kMovRun;  // the image with one key of padding after every run
constexpr int kMovOut = kMovTile / kMovThreads;    // outputs of a lane
static_assert((kMovTile & (kMovTile - 1)) == 0, "kMovTile is a power of two");
static_assert(kMovHalo >= kMovTile - 1 && kMovSpan == 2 * kMovTile, "the long form images two blocks; a longer window never lies inside one");
static_assert(kMovRun == 16 && (kMovImg + 2 * kMovThreads) * 8 <= 65536, "runs of 16 keys; static LDS of at most 64 KiB");
template <typename K>
__device__ __forceinline__ K kmax(K a, K b) {
    return a > b ? a : b;
}

// The lane's run of the image, img[pidx(16 tid + e)], into registers and back.
template <typename K>
__device__ __forceinline__ void read_run(const K* img, K (&v)[kMovRun]) {
#pragma unroll
    for (int e = 0; e < kMovRun; ++e) v[e] = img[(int)threadIdx.x * (kMovRun + 1) + e];
}
template <typename K>
__device__ __forceinline__ void write_run(K* img, const K (&v)[kMovRun]) {
#pragma unroll
    for (int e = 0; e < kMovRun; ++e) img[(int)threadIdx.x * (kMovRun + 1) + e] = v[e];
}

// Inclusive maxima of the image inside aligned segments of S keys (a power of two, 1 .. kMovSpan), v the lane's run:
// prefix maxima (REV = false: v[e] becomes the maximum from its segment's first key up to itself) or suffix maxima (REV:
// from itself up to its segment's last key).  The run is scanned in registers; where a segment spans L = S / 16 > 1 lanes
// the run totals go through a Kogge-Stone scan in LDS (tot: two rows of kMovThreads keys, read from one and written to the
// other, one barrier a step) and each lane adds what its segment holds before (after) its run.  S is the same for every
// lane, so the barriers are uniform.  The caller puts a barrier between two calls (it does: the image is written and read).
template <typename K, bool REV>
__device__ __forceinline__ void seg_scan(K (&v)[kMovRun], int S, K* tot) {
    const int tid = threadIdx.x;
    if (!REV) {
#pragma unroll
        for (int e = 1; e < kMovRun; ++e)
            if (e & (S - 1)) v[e] = kmax(v[e], v[e - 1]);  // (16 tid + e is no segment's first key)
    } else {
#pragma unroll
        for (int e = kMovRun - 2; e >= 0; --e)
            if ((e + 1) & (S - 1)) v[e] = kmax(v[e], v[e + 1]);  // (16 tid + e + 1 is no segment's first key)
    }
    const int L = S / kMovRun;  // lanes of a segment
    if (L <= 1) return;
    const int r = tid & (L - 1);  // the lane's place in its segment
    K x = REV ? v[0] : v[kMovRun - 1];
    int p = 0;
    tot[tid] = x;
    __syncthreads();
    for (int d = 1; d < L; d <<= 1) {
        const bool ok = REV ? r + d < L : r >= d;
        if (ok) x = kmax(x, tot[p * kMovThreads + (REV ? tid + d : tid - d)]);
        p ^= 1;
        tot[p * kMovThreads + tid] = x;
        __syncthreads();
    }
    const bool has = REV ? r + 1 < L : r >= 1;
    if (has) {
        const K c = tot[p * kMovThreads + (REV ? tid + 1 : tid - 1)];
#pragma unroll
        for (int e = 0; e < kMovRun; ++e) v[e] = kmax(v[e], c);
    }
}

// the outputs of a lane: kMovOut / kVec groups of kVec neighbouring frames, group q at tile frame (tid + q * threads) * kVec
template <typename F, bool MIN>
__device__ __forceinline__ void store_tile(F* __restrict__ yr, int64_t j0, int nt, const typename Key<F>::K* acc, bool vec) {
    using T = Key<F>;
    constexpr int VE = T::kVec;
#pragma unroll
    for (int q = 0; q < kMovOut / VE; ++q) {
        const int jb = ((int)threadIdx.x + q * kMovThreads) * VE;
        if (vec && jb + VE <= nt) {
            typename T::V v;
            F* e = reinterpret_cast<F*>(&v);
#pragma unroll
            for (int k = 0; k < VE; ++k) e[k] = from_key<F, MIN>(acc[q * VE + k]);
            *reinterpret_cast<typename T::V*>(yr + j0 + jb) = v;
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (jb + k < nt) yr[j0 + jb + k] = from_key<F, MIN>(acc[q * VE + k]);
        }
    }
}

template <typename F, bool MIN>
__global__ __launch_bounds__(kMovThreads) void k_moving_short(MovingArgs a, int vx, int vy) {
    using T = Key<F>;
    using K = typename T::K;
    constexpr int VE = T::kVec;
    __shared__ K img[kMovImg];
    __shared__ K tot[2 * kMovThreads];
    const int c = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kMovTile;
    const int nt = (int)(a.n_out - j0 < kMovTile ? a.n_out - j0 : kMovTile);
    const int W = (int)(a.back + a.ahead) + 1;  // <= kMovHalo + 1
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    F* __restrict__ yr = (F*)a.y + (int64_t)c * a.ycs;
    const int cnt = nt + W - 1;  // key i of the image is input frame j0 + off - back + i: the window of tile frame jl is [jl, jl + W - 1]
    load_image<F, MIN>(img, xr, a.xfs, a.n_in, j0 + a.off - a.back, cnt, vx != 0);
    for (int i = cnt + (int)threadIdx.x; i < kMovSpan; i += kMovThreads) img[pidx(i)] = T::kMin;
    __syncthreads();
    K acc[kMovOut];
    if (W == 1) {
#pragma unroll
        for (int q = 0; q < kMovOut / VE; ++q)
#pragma unroll
            for (int k = 0; k < VE; ++k) {
                const int jb = ((int)threadIdx.x + q * kMovThreads) * VE + k;
                acc[q * VE + k] = img[pidx(jb < nt ? jb : nt - 1)];
            }
        store_tile<F, MIN>(yr, j0, nt, acc, vy != 0);
        return;
    }
    // segments of S = the greatest power of two <= W - 1: a window starts and ends in different segments, with at most one
    // whole segment between them -- the suffix from its start, that segment's maximum (the prefix at its last key), the
    // prefix at its end
    const int sh = 31 - __builtin_clz(W - 1), S = 1 << sh;
    K orig[kMovRun], v[kMovRun];
    read_run(img, orig);
#pragma unroll
    for (int e = 0; e < kMovRun; ++e) v[e] = orig[e];
    seg_scan<K, true>(v, S, tot);
    write_run(img, v);  // (a lane overwrites the keys it alone has read)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMovOut / VE; ++q)
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            const int jb = ((int)threadIdx.x + q * kMovThreads) * VE + k;
            acc[q * VE + k] = img[pidx(jb < nt ? jb : nt - 1)];  // (clamped; the store is guarded)
        }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kMovRun; ++e) v[e] = orig[e];
    seg_scan<K, false>(v, S, tot);
    write_run(img, v);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMovOut / VE; ++q)
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            const int jb = ((int)threadIdx.x + q * kMovThreads) * VE + k;
            const int jl = jb < nt ? jb : nt - 1, hi = jl + W - 1;
            K r = kmax(acc[q * VE + k], img[pidx(hi)]);
            if ((hi >> sh) - (jl >> sh) == 2) r = kmax(r, img[pidx((((jl >> sh) + 2) << sh) - 1)]);
            acc[q * VE + k] = r;
        }
    store_tile<F, MIN>(yr, j0, nt, acc, vy != 0);
}

// level 0 of the table: the maximum of every aligned block of kMovTile input frames
template <typename F, bool MIN>
__global__ __launch_bounds__(kMovThreads) void k_moving_blockmax(MovingArgs a, int vx, int64_t nb) {
    using T = Key<F>;
    using K = typename T::K;
    constexpr int VE = T::kVec;
    __shared__ K part[kMovThreads / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t b = blockIdx.x, g0 = b * kMovTile;
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    K m = T::kMin;
    if (vx) {
        for (int q = tid; q < kMovTile / VE; q += kMovThreads) {
            const int64_t gs = g0 + (int64_t)q * VE;
            if (gs + VE <= a.n_in) {
                const typename T::V v = *reinterpret_cast<const typename T::V*>(xr + gs);
                const F* e = reinterpret_cast<const F*>(&v);
#pragma unroll
                for (int k = 0; k < VE; ++k) m = kmax(m, to_key<F, MIN>(e[k]));
            } else {
#pragma unroll
                for (int k = 0; k < VE; ++k) m = kmax(m, load_key<F, MIN>(xr, 1, a.n_in, gs + k));
            }
        }
    } else {
        for (int i = tid; i < kMovTile; i += kMovThreads) m = kmax(m, load_key<F, MIN>(xr, a.xfs, a.n_in, g0 + i));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = kmax(m, (K)__shfl_xor((long long)m, o, 64));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kMovThreads / 64; ++w) m = kmax(m, part[w]);
        ((K*)a.tab)[(int64_t)c * nb + b] = m;
    }
}

// level l >= 1: entry b = the maximum of the 2^l blocks from b on, for every b with b + 2^l <= nb
template <typename K>
__global__ __launch_bounds__(kMovThreads) void k_moving_level(K* tab, int l, int nch, int64_t nb) {
    const int c = blockIdx.y;
    const int64_t b = (int64_t)blockIdx.x * kMovThreads + threadIdx.x, half = (int64_t)1 << (l - 1);
    if (b + 2 * half > nb) return;
    const K* __restrict__ src = tab + ((int64_t)(l - 1) * nch + c) * nb;
    tab[((int64_t)l * nch + c) * nb + b] = kmax(src[b], src[b + half]);
}

template <typename F, bool MIN>
__global__ __launch_bounds__(kMovThreads) void k_moving_long(MovingArgs a, int vx, int vy, int64_t nb) {
    using T = Key<F>;
    using K = typename T::K;
    constexpr int VE = T::kVec;
    __shared__ K img[kMovImg];
    __shared__ K tot[2 * kMovThreads];
    const int c = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kMovTile;
    const int nt = (int)(a.n_out - j0 < kMovTile ? a.n_out - j0 : kMovTile);
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    F* __restrict__ yr = (F*)a.y + (int64_t)c * a.ycs;
    K v[kMovRun];
    const K* __restrict__ tab = (const K*)a.tab;
    const int64_t last = a.n_in - 1;
    auto lo_of = [&](int jl) { const int64_t l = j0 + jl + a.off - a.back; return l > 0 ? l : (int64_t)0; };
    auto hi_of = [&](int jl) { const int64_t h = j0 + jl + a.off + a.ahead; return h < last ? h : last; };
    K acc[kMovOut];
    // the blocks the windows start in: suffix maxima, and the whole blocks in between from the table
    const int64_t rs = lo_of(0) / kMovTile * kMovTile;
    load_image<F, MIN>(img, xr, a.xfs, a.n_in, rs, kMovSpan, vx != 0);
    __syncthreads();
    read_run(img, v);
    seg_scan<K, true>(v, kMovTile, tot);
    write_run(img, v);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMovOut / VE; ++q) {
        const int jb = ((int)threadIdx.x + q * kMovThreads) * VE;
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            const int jl = jb + k < nt ? jb + k : nt - 1;
            const int64_t l = lo_of(jl), h = hi_of(jl), bl = l / kMovTile, bh = h / kMovTile;
            K r = T::kMin;
            if (!(bl == bh && l == bl * kMovTile)) r = img[pidx((int)(l - rs))];
            if (bh - bl >= 2) {
                const int lv = 63 - __builtin_clzll((unsigned long long)(bh - bl - 1));
                const K* __restrict__ row = tab + ((int64_t)lv * a.nch + c) * nb;
                r = kmax(r, kmax(row[bl + 1], row[bh - ((int64_t)1 << lv)]));
            }
            acc[q * VE + k] = r;
        }
    }
    __syncthreads();
    // the blocks the windows end in: prefix maxima
    const int64_t re = hi_of(0) / kMovTile * kMovTile;
    load_image<F, MIN>(img, xr, a.xfs, a.n_in, re, kMovSpan, vx != 0);
    __syncthreads();
    read_run(img, v);
    seg_scan<K, false>(v, kMovTile, tot);
    write_run(img, v);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMovOut / VE; ++q) {
        const int jb = ((int)threadIdx.x + q * kMovThreads) * VE;
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            const int jl = jb + k < nt ? jb + k : nt - 1;
            const int64_t l = lo_of(jl), h = hi_of(jl), bl = l / kMovTile, bh = h / kMovTile;
            if (!(bl == bh && l != bl * kMovTile)) acc[q * VE + k] = kmax(acc[q * VE + k], img[pidx((int)(h - re))]);
        }
    }
    store_tile<F, MIN>(yr, j0, nt, acc, vy != 0);
}

template <typename F, bool MIN>
int launch_moving_t(const MovingArgs& a, int vx, int vy, hipStream_t st) {
    using K = typename Key<F>::K;
    const int64_t tiles = (a.n_out + kMovTile - 1) / kMovTile, nb = moving_blocks(a.n_in);
    if (tiles >= ((int64_t)1 << 31) || nb >= ((int64_t)1 << 31)) return -1;
    const dim3 block(kMovThreads), grid((unsigned)tiles, (unsigned)a.nch);
    if (!moving_is_long(a.n_in, a.back, a.ahead)) {
        hipLaunchKernelGGL((k_moving_short<F, MIN>), grid, block, 0, st, a, vx, vy);
        return 1;
    }
    if (!a.tab) return -1;
    const int levels = moving_levels(a.n_in, a.back, a.ahead);
    hipLaunchKernelGGL((k_moving_blockmax<F, MIN>), dim3((unsigned)nb, (unsigned)a.nch), block, 0, st, a, vx, nb);
    for (int l = 1; l <= levels; ++l) {
        const int64_t cnt = nb - ((int64_t)1 << l) + 1;  // >= 1: 2^levels <= nb
        hipLaunchKernelGGL((k_moving_level<K>), dim3((unsigned)((cnt + kMovThreads - 1) / kMovThreads), (unsigned)a.nch), block, 0, st, (K*)a.tab, l, (int)a.nch, nb);
    }
    hipLaunchKernelGGL((k_moving_long<F, MIN>), grid, block, 0, st, a, vx, vy, nb);
    return 2 + levels;
}

}  // namespace

int launch_moving(const MovingArgs& a0, hipStream_t st) {
    if (a0.n_out <= 0 || a0.nch <= 0) return 0;
    if (a0.nch > 65535 || a0.back < 0 || a0.ahead < 0 || a0.off < 0 || a0.n_in < 1 || a0.off > a0.n_in - a0.n_out) return -1;
    MovingArgs a = a0;
    a.back = moving_clamp(a.back, a.n_in);  // (a longer reach is clipped to the signal anyway; sums of frame indices stay below 3 n_in)
    a.ahead = moving_clamp(a.ahead, a.n_in);
    const int64_t esz = a.f32 ? 4 : 8;
    const int vx = a.xfs == 1 && (uintptr_t)a.x % 16 == 0 && (a.nch == 1 || (a.xcs * esz) % 16 == 0);
    const int vy = (uintptr_t)a.y % 16 == 0 && (a.nch == 1 || (a.ycs * esz) % 16 == 0);
    if (a.f32) return a.is_min ? launch_moving_t<float, true>(a, vx, vy, st) : launch_moving_t<float, false>(a, vx, vy, st);
    return a.is_min ? launch_moving_t<double, true>(a, vx, vy, st) : launch_moving_t<double, false>(a, vx, vy, st);
}

}  // namespace so
