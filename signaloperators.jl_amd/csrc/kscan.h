// The data movement the scans over runs of 16 frames share (k_cumsum.hip, k_recur.hip, k_recur2.hip): a tile of 64 runs is loaded 16 bytes a
// lane, neighbouring lanes on neighbouring words, through a wave's own padded LDS image [64 runs][16 + 2 pad] and read back
// a run a lane with ds_read_b128 (the pad of 16 bytes puts the 16 lanes of a read group on 16 different slots), and stored
// the same way back.  Everything else -- a frame stride, an unaligned row, the ragged last tile -- goes one element a lane,
// lanes on neighbouring frames, every frame index clamped into [0, n) BEFORE an address is formed and every store under a
// guard.  The image belongs to one wave; its writes and reads are ordered by a wavefront-scope fence.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace so {

constexpr int kCumsumPitch = kCumsumRun + 2;                 // doubles per run of the LDS image
constexpr int kCumsumImage = 64 * kCumsumPitch;              // doubles per wave
static_assert(kCumsumRun == 16, "the loaders below are written for runs of 16 frames");

typedef double cs_v2d __attribute__((ext_vector_type(2)));
typedef float cs_v4f __attribute__((ext_vector_type(4)));

// the LDS image is one wave's: order its accesses among the lanes of the wave
__device__ __forceinline__ void cs_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// element e of a tile lies at this double of the image
__device__ __forceinline__ int cs_at(int e) { return (e >> 4) * kCumsumPitch + (e & 15); }

// the tile that starts at frame f0 of the row xr (n frames, frame stride xfs) -> the image, as Float64; the lane's run
// lies at img + lane * kCumsumPitch once the wave is synchronised
template <typename TX, bool VL>
__device__ __forceinline__ void cs_fill_image(const TX* __restrict__ xr, int64_t xfs, int64_t f0, int64_t n, double* img, int lane) {
    if (VL && f0 + kCumsumTile <= n) {
        if (sizeof(TX) == 8) {
#pragma unroll
            for (int i = 0; i < kCumsumTile / 128; ++i) {
                const int e = 128 * i + 2 * lane;
                *reinterpret_cast<cs_v2d*>(img + cs_at(e)) = *reinterpret_cast<const cs_v2d*>(xr + f0 + e);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kCumsumTile / 256; ++i) {
                const int e = 256 * i + 4 * lane;
                const cs_v4f w = *reinterpret_cast<const cs_v4f*>(xr + f0 + e);
                cs_v2d lo, hi;
                lo.x = (double)w.x, lo.y = (double)w.y, hi.x = (double)w.z, hi.y = (double)w.w;
                *reinterpret_cast<cs_v2d*>(img + cs_at(e)) = lo;
                *reinterpret_cast<cs_v2d*>(img + cs_at(e) + 2) = hi;
            }
        }
    } else {
        const int64_t last = n - 1;
        TX w[kCumsumRun];
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) {
            const int64_t f = f0 + 64 * m + lane;
            w[m] = xr[(f <= last ? f : last) * xfs];  // (past the end: a copy of the last frame, read by nothing that exists)
        }
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) img[cs_at(64 * m + lane)] = (double)w[m];
    }
    cs_wave_sync();
}

// the tile that starts at frame f0 of the row xr (n frames, frame stride xfs) -> the lane's run in r[0 .. 16)
template <typename TX, bool VL>
__device__ __forceinline__ void cs_load_tile(const TX* __restrict__ xr, int64_t xfs, int64_t f0, int64_t n, double* img, int lane,
                                             double (&r)[kCumsumRun]) {
    cs_fill_image<TX, VL>(xr, xfs, f0, n, img, lane);
#pragma unroll
    for (int q = 0; q < kCumsumRun / 2; ++q) {
        const cs_v2d w = *reinterpret_cast<const cs_v2d*>(img + lane * kCumsumPitch + 2 * q);
        r[2 * q] = w.x, r[2 * q + 1] = w.y;
    }
    cs_wave_sync();  // (the image is written again: by the next tile, or by cs_store_tile)
}

// the image, every lane's run written and not yet synchronised -> the frames [f0, f0 + 1024) of the row yr that exist
template <bool VS>
__device__ __forceinline__ void cs_drain_image(double* __restrict__ yr, int64_t f0, int64_t n, double* img, int lane) {
    cs_wave_sync();
    if (VS && f0 + kCumsumTile <= n) {
#pragma unroll
        for (int i = 0; i < kCumsumTile / 128; ++i) {
            const int e = 128 * i + 2 * lane;
            *reinterpret_cast<cs_v2d*>(yr + f0 + e) = *reinterpret_cast<const cs_v2d*>(img + cs_at(e));
        }
    } else {
#pragma unroll
        for (int m = 0; m < kCumsumRun; ++m) {
            const int64_t f = f0 + 64 * m + lane;
            if (f < n) yr[f] = img[cs_at(64 * m + lane)];
        }
    }
    cs_wave_sync();
}

// the lane's run r -> the frames [f0, f0 + 1024) of the row yr that exist
template <bool VS>
__device__ __forceinline__ void cs_store_tile(double* __restrict__ yr, int64_t f0, int64_t n, double* img, int lane,
                                              const double (&r)[kCumsumRun]) {
#pragma unroll
    for (int q = 0; q < kCumsumRun / 2; ++q) {
        cs_v2d w;
        w.x = r[2 * q], w.y = r[2 * q + 1];
        *reinterpret_cast<cs_v2d*>(img + lane * kCumsumPitch + 2 * q) = w;
    }
    cs_drain_image<VS>(yr, f0, n, img, lane);
}

}  // namespace so
