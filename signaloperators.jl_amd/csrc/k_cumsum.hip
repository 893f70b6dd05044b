// k_cumsum: `Cumsum(x)` (signals.py; SO_NODE_CUMSUM of include/sigops.h) -- per channel y[n] = x[0] + ... + x[n] in Float64
// over ONE summation tree that depends on the frame index only (DESIGN.md "Cumsum"; tests/cumsum_ref.py is the
// definition), so a window, a stream block and the whole sink give the same bits:
//   run    j of a tile: the frames [16 j, 16 j + 16) summed left to right from the first sample itself -> r, total R[j]
//   tile   (64 runs): an inclusive Kogge-Stone scan v over R, d = 1 .. 32, a lane without a source keeps its value;
//          t = r in run 0, v[j - 1] + r in run j >= 1
//   chunk  (kCumsumTiles tiles): tile 0 is t, tile k >= 1 is c + t with c the last value of tile k - 1
//   signal chunk 0 is its chunk-local u, chunk k >= 1 is C + u with C the running sum of the chunks' last u
// Every + is one rounded Float64 addition; nothing is ever added to a zero that the tree does not have, so -0.0 survives.
//
// Reduce-then-scan, no workgroup waits for another (a look-back scan would sum whichever predecessors have published,
// which is another tree each time):
//   k_cumsum_totals  one workgroup per (chunk, channel), every chunk but the last: the chunk-local last value -> tot
//   k_cumsum_carry   one workgroup per channel: tot -> its running sum, in place (lane 0 adds, out of LDS)
//   k_cumsum_scan    one workgroup per (chunk, channel): the chunk-local scan again, + tot[chunk - 1], stored
// A signal of one chunk is the third launch alone.
//
// The resumed form (CumsumArgs::k0 > 0, a stream's push): the rows start at chunk k0 of the signal, so blockIdx.x is the
// chunk number relative to k0 and so is the index into tot; the carry starts from cin, the total that enters chunk k0,
// instead of from the first total, and the scan of the first chunk adds cin.  "The signal's chunk 0", which adds no carry,
// is keyed on the absolute chunk: relative chunk 0 without a cin.  The carry leaves the total that enters the last chunk
// in cout (one plain store a channel), never in cin: the same launch twice gives the same bytes.
//
// A workgroup is kCumsumWaves waves; a wave takes kCumsumTiles / kCumsumWaves consecutive tiles, one after the other, a
// lane one run of each and keeps its 16 values in registers until the tile carries are known (one barrier).  A lane's run
// is 128 contiguous bytes, so x is not loaded in run order: a full tile of a unit-stride, 16-byte aligned row is loaded 16
// bytes a lane, neighbouring lanes on neighbouring words (VL), written to the wave's own LDS image [64 runs][16 + 2 pad]
// and read back a run a lane with ds_read_b128 (the pad of 16 bytes puts the 16 lanes of a read group on 16 different
// slots); pass 2 stores the same way back (VS).  Everything else -- a frame stride, an unaligned row, the ragged last
// tile -- goes one element a lane, lanes on neighbouring frames, every frame index clamped into [0, n) BEFORE an address
// is formed and every store under a guard (k_comb.hip and k_sample_at.hip do the same).  The LDS image belongs to one
// wave; its writes and reads are ordered by a wavefront-scope fence.  Frame arithmetic is 64-bit.  The loads and stores
// are kscan.h's, shared with k_recur.hip.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kscan.h"

namespace so {

constexpr int kCumsumWaves = 4;
constexpr int kCumsumPerWave = kCumsumTiles / kCumsumWaves;  // tiles a wave carries in registers
static_assert(kCumsumTiles % kCumsumWaves == 0, "a wave takes a whole number of tiles");

// r: the lane's run -> its tile-local values t; returns the last of them (lane 63: the tile's last value, v[62] + R[63] --
// the value the next tile carries, which is not the scan's v[63])
__device__ __forceinline__ double cs_tile_scan(double (&r)[kCumsumRun], int lane) {
#pragma unroll
    for (int m = 1; m < kCumsumRun; ++m) r[m] = r[m - 1] + r[m];
    double v = r[kCumsumRun - 1];
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const double s = __shfl_up(v, d, 64);
        if (lane >= d) v = s + v;
    }
    const double before = __shfl_up(v, 1, 64);
    if (lane >= 1) {
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) r[m] = before + r[m];
    }
    return r[kCumsumRun - 1];
}

// Pass 1: the chunk-local last value of chunk blockIdx.x (a whole chunk: the last chunk of a row has no total).
template <typename TX, bool VL>
__global__ __launch_bounds__(64 * kCumsumWaves) void k_cumsum_totals(CumsumArgs a) {
    __shared__ __attribute__((aligned(16))) double image[kCumsumWaves * kCumsumImage];
    __shared__ double total[kCumsumTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int c = blockIdx.y;
    const TX* __restrict__ xr = (const TX*)a.x + (int64_t)c * a.xcs;
    double* img = image + wave * kCumsumImage;
#pragma unroll 1
    for (int i = 0; i < kCumsumPerWave; ++i) {
        const int tile = wave * kCumsumPerWave + i;
        double r[kCumsumRun];
        cs_load_tile<TX, VL>(xr, a.xfs, chunk * kCumsumChunk + (int64_t)tile * kCumsumTile, a.n, img, lane, r);
        const double v = cs_tile_scan(r, lane);
        if (lane == 63) total[tile] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = total[0];
#pragma unroll
        for (int k = 1; k < kCumsumTiles; ++k) s = s + total[k];
        a.tot[(int64_t)c * a.tot_pitch + chunk] = s;
    }
}

// The carries: tot[k] <- tot[0] + ... + tot[k], summed in that order, per channel (blockIdx.x), in place.  The totals go
// through LDS kBlock at a time; lane 0 reads 16 of them, adds, writes 16.
__global__ __launch_bounds__(kBlock) void k_cumsum_carry(double* tot, int64_t pitch, int64_t count, const double* cin, double* cout) {
    __shared__ double in[kBlock], out[kBlock];
    double* row = tot + (int64_t)blockIdx.x * pitch;
    const bool resumed = cin != nullptr;
    double s = resumed ? cin[blockIdx.x] : 0.0;  // (lane 0's; from rest: replaced, not added to, by the first total)
    for (int64_t k0 = 0; k0 < count; k0 += kBlock) {
        const int64_t k = k0 + threadIdx.x;
        if (k < count) in[threadIdx.x] = row[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (int)(count - k0 < kBlock ? count - k0 : kBlock);  // (the entries past m are not read back)
            for (int j0 = 0; j0 < m; j0 += 16) {
                double w[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) w[j] = in[j0 + j];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s = (!resumed && k0 == 0 && j0 == 0 && j == 0) ? w[0] : s + w[j];
                    out[j0 + j] = s;
                }
            }
        }
        __syncthreads();
        if (k < count) row[k] = out[threadIdx.x];
    }
    // the total that enters chunk `count`, the last one: the last entry written (lane 0's s has run on over the rest of its
    // group of 16, which nobody reads); lane 0 wrote `out` itself and count >= 1
    if (threadIdx.x == 0 && cout != nullptr) cout[blockIdx.x] = out[(count - 1) % kBlock];
}

// Pass 2: chunk blockIdx.x of channel blockIdx.y, stored.
template <typename TX, bool VL, bool VS>
__global__ __launch_bounds__(64 * kCumsumWaves) void k_cumsum_scan(CumsumArgs a) {
    __shared__ __attribute__((aligned(16))) double image[kCumsumWaves * kCumsumImage];
    __shared__ double total[kCumsumTiles];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int c = blockIdx.y;
    const TX* __restrict__ xr = (const TX*)a.x + (int64_t)c * a.xcs;
    double* __restrict__ yr = a.y + (int64_t)c * a.ycs;
    double* img = image + wave * kCumsumImage;
    const int64_t f00 = chunk * kCumsumChunk + (int64_t)wave * kCumsumPerWave * kCumsumTile;  // the wave's first frame
    double r[kCumsumPerWave][kCumsumRun];
#pragma unroll
    for (int i = 0; i < kCumsumPerWave; ++i) {
        const int64_t f0 = f00 + (int64_t)i * kCumsumTile;
        if (f0 < a.n) {  // (a tile past the end: nothing reads its total)
            cs_load_tile<TX, VL>(xr, a.xfs, f0, a.n, img, lane, r[i]);
            const double v = cs_tile_scan(r[i], lane);
            if (lane == 63) total[wave * kCumsumPerWave + i] = v;
        }
    }
    __syncthreads();
    // the carry into the wave's first tile: the last value of the tile before it, summed tile after tile
    double cy = 0.0;
    for (int k = 0; k < wave * kCumsumPerWave; ++k) cy = k == 0 ? total[0] : cy + total[k];
    const bool chunks_before = chunk > 0 || a.cin != nullptr;  // (the absolute chunk: launch_cumsum passes cin where k0 > 0 only)
    const double C = chunk > 0 ? a.tot[(int64_t)c * a.tot_pitch + chunk - 1] : a.cin != nullptr ? a.cin[c] : 0.0;
#pragma unroll
    for (int i = 0; i < kCumsumPerWave; ++i) {
        const int64_t f0 = f00 + (int64_t)i * kCumsumTile;
        if (f0 >= a.n) break;
        const int tile = wave * kCumsumPerWave + i;
        if (tile > 0) {
#pragma unroll
            for (int m = 0; m < kCumsumRun; ++m) r[i][m] = cy + r[i][m];
        }
        if (chunks_before) {
#pragma unroll
            for (int m = 0; m < kCumsumRun; ++m) r[i][m] = C + r[i][m];
        }
        cs_store_tile<VS>(yr, f0, a.n, img, lane, r[i]);
        cy = tile == 0 ? total[0] : cy + total[tile];  // the last value of this tile, chunk-local
    }
}

static bool cs_aligned(const void* p, int64_t cs, int nch, size_t esz) {
    return (uintptr_t)p % 16 == 0 && (nch == 1 || (cs * (int64_t)esz) % 16 == 0);
}

template <typename TX>
static void launch_cumsum_t(const CumsumArgs& a, int64_t nchunks, hipStream_t st) {
    const bool vl = a.xfs == 1 && cs_aligned(a.x, a.xcs, a.nch, sizeof(TX)), vs = cs_aligned(a.y, a.ycs, a.nch, 8);
    const dim3 block(64 * kCumsumWaves);
    if (nchunks > 1) {
        const dim3 grid((unsigned)(nchunks - 1), (unsigned)a.nch);
        if (vl) hipLaunchKernelGGL((k_cumsum_totals<TX, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_cumsum_totals<TX, false>), grid, block, 0, st, a);
        hipLaunchKernelGGL(k_cumsum_carry, dim3((unsigned)a.nch), dim3(kBlock), 0, st, a.tot, a.tot_pitch, nchunks - 1, a.cin, a.cout);
    }
    const dim3 grid((unsigned)nchunks, (unsigned)a.nch);
    if (vl && vs) hipLaunchKernelGGL((k_cumsum_scan<TX, true, true>), grid, block, 0, st, a);
    else if (vl) hipLaunchKernelGGL((k_cumsum_scan<TX, true, false>), grid, block, 0, st, a);
    else if (vs) hipLaunchKernelGGL((k_cumsum_scan<TX, false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_cumsum_scan<TX, false, false>), grid, block, 0, st, a);
}

int launch_cumsum(const CumsumArgs& a0, hipStream_t st) {
    if (a0.n <= 0 || a0.nch <= 0) return 0;
    if (a0.k0 < 0 || (a0.k0 > 0 && a0.cin == nullptr)) return -1;
    CumsumArgs a = a0;
    if (a.k0 == 0) a.cin = nullptr;  // (from rest: no record is read)
    const int64_t nchunks = (a.n + kCumsumChunk - 1) / kCumsumChunk;
    if (a.nch > 65535 || nchunks >= ((int64_t)1 << 31)) return -1;
    if (nchunks > 1 && (a.tot == nullptr || a.tot_pitch < nchunks - 1)) return -1;
    if (a.x_f32) launch_cumsum_t<float>(a, nchunks, st);
    else launch_cumsum_t<double>(a, nchunks, st);
    return nchunks > 1 ? 3 : 1;
}

}  // namespace so
