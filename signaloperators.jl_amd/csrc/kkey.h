// kkey.h: the monotone integer key of a sample and the loader of an LDS image of keys, shared by k_moving.hip (MovingMax /
// MovingMin) and k_movrank.hip (MovingMedian / MovingQuantile).
//
// A sample becomes a signed integer KEY of its own width that orders like -Inf < .. < -0.0 < +0.0 < .. < +Inf: a non-negative
// float's bits are its key, a negative float's key is its bits with every bit but the sign inverted (-0.0 -> -1, -Inf just
// above the least integer), a NaN's key is the greatest integer.  The least integer is no sample's key: it pads what lies
// outside the signal.  MIN flips the sign bit on the way in and on the way out: the order reversed.
//
// Addresses.  Every input index is clamped into [0, n_in) BEFORE an address is formed, and what lay outside becomes the
// padding key; a 16-byte load is issued only for a group that lies whole inside the row, and only where the launcher found
// the row bases 16-byte aligned and the frame stride 1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace so {
namespace {

constexpr int kKeyThreads = 256;  // lanes of a workgroup that loads an image
// key i of a padded image lies at img[pidx(i)]: a lane reads its run with a stride of 17 keys from its neighbour's, which
// spreads a half-wave's 8-byte (4-byte) accesses over all 64 (32) banks; consecutive keys stay consecutive but for the pad
__device__ __forceinline__ int pidx(int i) { return i + (i >> 4); }

template <typename F>
struct Key;
template <>
struct Key<float> {
    using K = int32_t;
    using V = float4;
    static constexpr int kBits = 32, kVec = 4;
    static constexpr K kMin = INT32_MIN, kMax = INT32_MAX, kInf = 0x7f800000;
};
template <>
struct Key<double> {
    using K = int64_t;
    using V = double2;
    static constexpr int kBits = 64, kVec = 2;
    static constexpr K kMin = INT64_MIN, kMax = INT64_MAX, kInf = 0x7ff0000000000000ll;
};

template <typename F, bool MIN>
__device__ __forceinline__ typename Key<F>::K to_key(F v) {
    using T = Key<F>;
    typename T::K b;
    __builtin_memcpy(&b, &v, sizeof b);
    if (MIN) b ^= T::kMin;
    const typename T::K k = b ^ ((b >> (T::kBits - 1)) & T::kMax);
    return (b & T::kMax) > T::kInf ? T::kMax : k;
}
template <typename F, bool MIN>
__device__ __forceinline__ F from_key(typename Key<F>::K k) {
    using T = Key<F>;
    typename T::K b = k ^ ((k >> (T::kBits - 1)) & T::kMax);
    if (MIN) b ^= T::kMin;
    F v;
    __builtin_memcpy(&v, &b, sizeof v);
    return v;
}

// one sample as a key: frame g of the row, the padding key outside [0, n_in); the index is clamped before the address
template <typename F, bool MIN>
__device__ __forceinline__ typename Key<F>::K load_key(const F* __restrict__ xr, int64_t xfs, int64_t n_in, int64_t g) {
    const bool inside = g >= 0 && g < n_in;
    const int64_t gc = g < 0 ? 0 : g < n_in ? g : n_in - 1;
    const F v = xr[gc * xfs];
    return inside ? to_key<F, MIN>(v) : Key<F>::kMin;
}

// a[pidx(i)] (PAD; a[i] without) = key of frame g0 + i for i in [0, cnt); `vec`: the row base is 16-byte aligned and the
// frame stride is 1
template <typename F, bool MIN, bool PAD = true>
__device__ __forceinline__ void load_image(typename Key<F>::K* a, const F* __restrict__ xr, int64_t xfs, int64_t n_in, int64_t g0, int cnt, bool vec) {
    using T = Key<F>;
    const int tid = threadIdx.x;
    auto at = [](int i) { return PAD ? pidx(i) : i; };
    if (!vec) {
        for (int i = tid; i < cnt; i += kKeyThreads) a[at(i)] = load_key<F, MIN>(xr, xfs, n_in, g0 + i);
        return;
    }
    constexpr int VE = T::kVec;
    const int64_t ga = g0 - (((g0 % VE) + VE) % VE);  // the aligned group g0 lies in (g0 may be negative)
    const int ngroups = (int)((g0 + cnt - ga + VE - 1) / VE);
    for (int q = tid; q < ngroups; q += kKeyThreads) {
        const int64_t gs = ga + (int64_t)q * VE;
        const int i0 = (int)(gs - g0);
        if (gs >= 0 && gs + VE <= n_in) {
            const typename T::V v = *reinterpret_cast<const typename T::V*>(xr + gs);
            const F* e = reinterpret_cast<const F*>(&v);
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (i0 + k >= 0 && i0 + k < cnt) a[at(i0 + k)] = to_key<F, MIN>(e[k]);
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (i0 + k >= 0 && i0 + k < cnt) a[at(i0 + k)] = load_key<F, MIN>(xr, 1, n_in, gs + k);
        }
    }
}

}  // namespace
}  // namespace so
