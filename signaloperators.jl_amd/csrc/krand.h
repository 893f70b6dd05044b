// Counter-based white noise (include/sigops.h SO_FN_RANDN: `Signal(randn, rng=DeviceRNG(seed, stream))`, reference
// src/functions.jl:98-114): frame i of a leaf is a pure function of (seed, stream, i), so windows, blocks, shards and
// repeated executes of a plan all see the same noise, and the generator keeps no state in memory.
//   p = i >> 1;  x0..x3 = Philox4x32-10(counter = (p lo, p hi, stream lo, stream hi), key = (seed lo, seed hi))
//   u1 = ((x1:x0 >> 11) + 1) * 2^-53 in (0, 1],  u2 = (x3:x2 >> 11) * 2^-53 in [0, 1)      (both exact)
//   r = sqrt(-2 log u1),  (s, c) = sincospi(2 u2);  frame 2p = r c, frame 2p + 1 = r s      (Box-Muller)
// Every operation is rounded on its own: the translation units that use this header are compiled with
// -ffp-contract=off (k_pointwise_math.hip, k_randn_fill.hip, the hipRTC kernels), and they all call these very
// functions, so the fill kernel, the interpreter and the hipRTC kernels give the same values bit for bit.
// Used by the ahead-of-time kernels and, as TEXT embedded by build.py into rtc_embed.inc, by the hipRTC sources of
// steps that contain such a leaf (rtc.cpp puts it behind kleaf.h, whose sincospi_c it calls).  No standard headers.
#pragma once

namespace so {

// Random123's Philox4x32 with ten rounds (Salmon et al., SC'11).  32 x 32 -> 64 products as mulhi + mul.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& x0, uint32_t& x1, uint32_t& x2, uint32_t& x3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x0 = c0;
    x1 = c1;
    x2 = c2;
    x3 = c3;
}

// frames 2p (z0) and 2p + 1 (z1) of the noise (seed, stream)
__device__ __forceinline__ void randn_pair(uint64_t seed, uint64_t stream, uint64_t p, double& z0, double& z1) {
    uint32_t x0, x1, x2, x3;
    philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), x0, x1, x2, x3);
    const uint64_t a = (((uint64_t)x1 << 32) | x0) >> 11, b = (((uint64_t)x3 << 32) | x2) >> 11;
    const double u1 = (double)(a + 1) * 1.1102230246251565e-16;  // 2^-53
    const double u2 = (double)b * 1.1102230246251565e-16;
    const double r = ::sqrt(-2.0 * ::log(u1));
    double s, c;
    sincospi_c(2.0 * u2, s, c);
    z0 = r * c;
    z1 = r * s;
}

// seed and stream of a noise leaf (bit patterns; written by the planner's set_randn_leaf, kernels.h)
__device__ __forceinline__ uint64_t randn_seed(const DLeaf& L) { return (uint64_t)L.modn; }
__device__ __forceinline__ uint64_t randn_stream(const DLeaf& L) { return (uint64_t)L.fstride; }

// the leaf's value at frame n: absolute frame index as in func_eval
__device__ __forceinline__ double randn_eval(const DLeaf& L, int64_t n) {
    const uint64_t i = (uint64_t)((L.sf ? n : 0) + L.df);
    double z0, z1;
    randn_pair(randn_seed(L), randn_stream(L), i >> 1, z0, z1);
    return (i & 1) ? z1 : z0;
}

}  // namespace so
