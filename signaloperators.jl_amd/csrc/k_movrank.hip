// k_movrank: `MovingMedian(x, w)` / `MovingQuantile(x, w, q)` (signals.py; SO_NODE_MOVRANK of include/sigops.h) -- sliding rank
// filters.  Per channel, output j in [0, n_out) is a bit copy of the sample of rank floor(q (m - 1)), counted from 0, among
// the m input frames
//     [max(0, j + off - back), min(n_in - 1, j + off + ahead)]
// under the order -Inf < .. < -0.0 < +0.0 < .. < +Inf, NaN if any of them is NaN (tests/movingmedian_ref.py).
//
// Selection does not decompose like a maximum or a sum, so it is done by INCREMENTAL RANK COUNTING over k_moving.hip's
// monotone integer key (kkey.h): O(W) LDS reads a sample, no sorting, no divergence.
//
// Image.  A workgroup takes kRankTile outputs of one channel and loads the cnt = nt + W - 1 keys they read into LDS: entry i
// is input frame j0 + off - back + i, and the window of tile frame jl is the W entries [jl, jl + W - 1].  Frames before the
// signal hold the LEAST integer (no sample's key), frames after it the GREATEST, which is also a NaN's key.  The entries
// are ordered by (key, entry index), a strict total order: for element k an entry j < k is below it iff key[j] <= key[k],
// an entry j > k iff key[j] < key[k].  So the front pads rank below every sample and the back pads above, the ranks are
// counted over all W entries of a window, and output jl wants the element of rank
//     target(jl) = floor(q (m - 1)) + (front pads of its window),     the product ONE Float64 multiplication.
//
// Walk.  A lane owns ELEMENTS, entries k = tid, tid + 256, .. that are samples and not NaN.  Element k lies in the windows
// jl in [k - W + 1, k].  It counts its rank in window k - W + 1, where it is the last entry (W - 1 reads), and steps from
// window jl - 1 to jl: entry jl - 1 leaves, always before k (rank -= key <= key[k]), entry jl + W - 1 enters, always after k
// (rank += key < key[k]).  Where jl is a frame of the tile and the rank is the target, the lane writes k to sel[jl]:
// exactly one element an output does.  A guard of W - 1 entries of the greatest integer on either side of the image
// counts nothing in either comparison (no walking element holds that key), so the windows jl < 0 and jl >= nt are walked
// like the others, every lane runs the same 3 (W - 1) reads an element and no read is conditional.  Neighbouring lanes read
// neighbouring keys and write distinct outputs: no bank conflicts, the image is not padded.  A lane walks kRankGroup
// elements side by side and issues the reads of the next step before this step's claims, so 2 kRankGroup LDS reads are in
// flight.  A tile whose windows all lie inside the signal has ONE target, floor(q (W - 1)); the others read theirs from a
// table in LDS.
//
// NaN.  An element that IS NaN does not walk: as its lane sets it up it raises nanf[jl] for the frames whose window holds
// it (rare, so the divergence costs nothing where there is none).  A pad never does.
//
// Store.  After a barrier, lane-per-output: y = nanf ? NaN : the sample of key[sel], 16-byte stores guarded by the
// tile's frame count.
//
// Addresses.  kkey.h's loader clamps every input index into [0, n_in) before an address is formed.  launch_movrank clamps
// back and ahead to n_in and refuses W - 1 > kRankHalo; frame arithmetic is 64-bit, indices into LDS are int: the image's
// are at most kRankTile + 3 kRankHalo (k + s + W with k < cnt, s <= W - 1: the read ahead of the last step, in the entry the
// image has to spare), sel's and tgt's are checked against or clamped to nt.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "kkey.h"

namespace so {
namespace {

constexpr int kRankThreads = kKeyThreads;
constexpr int kRankSpan = kRankTile + kRankHalo;     // entries of the image at most: the elements
constexpr int kRankImg = kRankSpan + 2 * kRankHalo;  // ... and a guard of W - 1 entries on either side (and one entry to spare: the walk reads one step ahead)
constexpr int kRankEl = kRankSpan / kRankThreads;    // elements of a lane
constexpr int kRankGroup = 4;                        // elements a lane walks side by side
constexpr int kRankOut = kRankTile / kRankThreads;   // outputs of a lane
static_assert(kRankSpan % kRankThreads == 0 && kRankEl % kRankGroup == 0 && kRankOut % 4 == 0, "whole groups of elements, whole vectors of outputs");
static_assert(kRankSpan <= 65535 && kRankHalo <= 65535, "sel and tgt are 16-bit");
static_assert(3 * ((kRankImg + 1) * 8 + kRankTile * 5) <= 160 * 1024, "three workgroups of Float64 a compute unit");

// the walk of every element of the image (see the head of the file); UNI: every frame of the tile has the target tW
template <typename K, K kNaN, bool UNI>
__device__ __forceinline__ void walk(const K* img, int G, int nt, int r0, int r1, int tW, const uint16_t* tgt, uint16_t* sel, uint8_t* nanf) {
    constexpr int E = kRankGroup;
    for (int e0 = 0; e0 < kRankEl && e0 * kRankThreads < r1; e0 += E) {
        int k[E], r[E];
        K kk[E];
#pragma unroll
        for (int u = 0; u < E; ++u) {
            const int ku = (int)threadIdx.x + (e0 + u) * kRankThreads;
            const bool in = ku >= r0 && ku < r1;
            k[u] = in ? ku : r0;  // (a lane without an element walks a sample's entry ...)
            kk[u] = img[G + k[u]];
            if (in && kk[u] == kNaN) {  // a NaN: the frames of the tile whose window holds it
                const int hi = ku < nt - 1 ? ku : nt - 1;
#pragma unroll 1
                for (int jl = ku > G ? ku - G : 0; jl <= hi; ++jl) nanf[jl] = 1;
            }
            r[u] = in && kk[u] != kNaN ? 0 : -4 * kRankImg;  // (... from a rank that never reaches a target: it moves by W - 1 at most)
        }
        // the claim of window jl = k - (W - 1) + s; a clipped tile's target is read at a clamped frame, so the read is unconditional
        auto hit = [&](int u, int s) {
            const int jl = k[u] - G + s;
            const int jc = jl < 0 ? 0 : jl < nt ? jl : nt - 1;
            return (unsigned)jl < (unsigned)nt && r[u] == (UNI ? tW : (int)tgt[jc]);
        };
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
        for (int t = 0; t < G; ++t)
#pragma unroll
            for (int u = 0; u < E; ++u) r[u] += img[k[u] + t] <= kk[u] ? 1 : 0;  // entry k - (W - 1) + t of the image
        // The reads of step s + 1 are issued before the claims of step s: a claim is a store under a lane mask, which ends a
        // basic block, and the compiler moves no read over it -- without this the reads of one element at a time were in flight.
        // The reads of step W lie one entry behind the back guard (the image has one entry to spare) and are not used.
        K out[E], in[E];
#pragma unroll
        for (int u = 0; u < E; ++u) {
            out[u] = img[k[u]];
            in[u] = img[G + k[u] + 1];
        }
#pragma unroll
        for (int u = 0; u < E; ++u)
            if (hit(u, 0)) sel[k[u] - G] = (uint16_t)k[u];
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(2)
        for (int s = 1; s <= G; ++s) {
            bool h[E];
#pragma unroll
            for (int u = 0; u < E; ++u) {
                r[u] -= out[u] <= kk[u] ? 1 : 0;  // entry jl - 1 = k - W + s leaves
                r[u] += in[u] < kk[u] ? 1 : 0;    // entry jl + W - 1 = k + s enters
                h[u] = hit(u, s);
            }
#pragma unroll
            for (int u = 0; u < E; ++u) {
                out[u] = img[k[u] + s];
                in[u] = img[G + k[u] + s + 1];
            }
            bool any = false;
#pragma unroll
            for (int u = 0; u < E; ++u) any |= h[u];
            if (any) {  // (one branch a step: the four elements' arithmetic stays one basic block)
#pragma unroll
                for (int u = 0; u < E; ++u)
                    if (h[u]) sel[k[u] - G + s] = (uint16_t)k[u];
            }
        }
    }
}

template <typename F>
__global__ __launch_bounds__(kRankThreads) void k_movrank(MovrankArgs a, int vx, int vy) {
    using T = Key<F>;
    using K = typename T::K;
    constexpr int VE = T::kVec;
    __shared__ K img[kRankImg + 1];
    __shared__ uint16_t sel[kRankTile];  // the entry of the image an output copies
    __shared__ uint16_t tgt[kRankTile];  // the rank it wants, over the W entries of its window
    __shared__ uint8_t nanf[kRankTile];  // its window holds a NaN
    const int tid = threadIdx.x, c = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kRankTile;
    const int nt = (int)(a.n_out - j0 < kRankTile ? a.n_out - j0 : kRankTile);
    const int G = (int)(a.back + a.ahead);  // W - 1 <= kRankHalo
    const int cnt = nt + G;
    const int64_t g0 = j0 + a.off - a.back;  // the input frame of entry 0
    const F* __restrict__ xr = (const F*)a.x + (int64_t)c * a.xcs;
    F* __restrict__ yr = (F*)a.y + (int64_t)c * a.ycs;
    K* im = img + G;  // entry i of the image is im[i]; img[0, G) and im[cnt, cnt + G) are the guards
    // the entries [r0, r1) are samples: 0 <= r0 <= back < r1 <= cnt (entry `back` is the frame output 0 is centred on)
    const int r0 = (int)(g0 < 0 ? -g0 : 0);
    const int r1 = (int)(a.n_in - g0 < cnt ? a.n_in - g0 : cnt);
    const bool uni = g0 >= 0 && g0 + cnt <= a.n_in;  // no window of the tile is clipped: one target
    load_image<F, false, false>(im, xr, a.xfs, a.n_in, g0, cnt, vx != 0);
    for (int i = tid; i < G; i += kRankThreads) {
        img[i] = T::kMax;
        im[cnt + i] = T::kMax;
    }
    for (int jl = tid; jl < nt; jl += kRankThreads) nanf[jl] = 0;
    if (!uni)
        for (int jl = tid; jl < nt; jl += kRankThreads) {
            const int64_t n = j0 + a.off + jl;  // the input frame the window is centred on
            const int64_t lo = n > a.back ? n - a.back : 0, hi = n + a.ahead < a.n_in - 1 ? n + a.ahead : a.n_in - 1;
            const int64_t pads = a.back > n ? a.back - n : 0;
            tgt[jl] = (uint16_t)((int)floor(a.q * (double)(hi - lo)) + (int)pads);
        }
    __syncthreads();
    if (r1 < cnt) {  // (the same for every lane) what lies after the signal: the loader left the least integer there
        for (int i = r1 + tid; i < cnt; i += kRankThreads) im[i] = T::kMax;
        __syncthreads();
    }
    if (uni)
        walk<K, T::kMax, true>(img, G, nt, r0, r1, (int)floor(a.q * (double)G), tgt, sel, nanf);
    else
        walk<K, T::kMax, false>(img, G, nt, r0, r1, 0, tgt, sel, nanf);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kRankOut / VE; ++q) {
        const int jb = (tid + q * kRankThreads) * VE;
        typename T::V v;
        F* e = reinterpret_cast<F*>(&v);
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            const int jl = jb + k < nt ? jb + k : nt - 1;  // (clamped; the store is guarded)
            const int s = sel[jl] < r1 ? sel[jl] : r1 - 1;
            e[k] = from_key<F, false>(nanf[jl] ? T::kMax : im[s]);  // (the greatest integer is a NaN pattern)
        }
        if (vy && jb + VE <= nt) {
            *reinterpret_cast<typename T::V*>(yr + j0 + jb) = v;
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (jb + k < nt) yr[j0 + jb + k] = e[k];
        }
    }
}

}  // namespace

int launch_movrank(const MovrankArgs& a0, hipStream_t st) {
    if (a0.n_out <= 0 || a0.nch <= 0) return 0;
    if (a0.nch > 65535 || a0.back < 0 || a0.ahead < 0 || a0.off < 0 || a0.n_in < 1 || a0.off > a0.n_in - a0.n_out || !(a0.q >= 0.0 && a0.q <= 1.0)) return -1;
    if (!movrank_fits(a0.n_in, a0.back, a0.ahead)) return -1;
    MovrankArgs a = a0;
    a.back = moving_clamp(a.back, a.n_in);  // (a longer reach is clipped to the signal anyway)
    a.ahead = moving_clamp(a.ahead, a.n_in);
    const int64_t tiles = (a.n_out + kRankTile - 1) / kRankTile;
    if (tiles >= ((int64_t)1 << 31)) return -1;
    const int64_t esz = a.f32 ? 4 : 8;
    const int vx = a.xfs == 1 && (uintptr_t)a.x % 16 == 0 && (a.nch == 1 || (a.xcs * esz) % 16 == 0);
    const int vy = (uintptr_t)a.y % 16 == 0 && (a.nch == 1 || (a.ycs * esz) % 16 == 0);
    const dim3 block(kRankThreads), grid((unsigned)tiles, (unsigned)a.nch);
    if (a.f32)
        hipLaunchKernelGGL((k_movrank<float>), grid, block, 0, st, a, vx, vy);
    else
        hipLaunchKernelGGL((k_movrank<double>), grid, block, 0, st, a, vx, vy);
    return 1;
}

}  // namespace so
