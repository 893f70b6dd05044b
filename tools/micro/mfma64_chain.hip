// The recurrence of k_rsos's chain wave in isolation: three v_mfma_f64_16x16x4_f64 per step whose result (registers
// 0..2 of the accumulator) is the B operand of the next step's three -- bare, and with the LDS traffic of the real
// loop (3 operand reads + 1 counter read requested a step ahead, 3 state writes + 1 counter write) placed in
// different spots.  Then the same recurrence on v_mfma_f64_4x4x4_4b_f64 (k4, k5: six, three or one instruction per step
// on the block lower triangular A^16) and a probe of that shape's lane map.  Cycles per step for one wave on a CU.
//   hipcc --offload-arch=gfx950 -O3 mfma64_chain.hip
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double v4d __attribute__((ext_vector_type(4)));
#define SO_LDS __attribute__((address_space(3)))

template <int MODE>
__global__ void k(long long* out, double* sink, int iters) {
    __shared__ double buf[64 * 64];
    __shared__ int flags[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 64; i += 64) buf[i] = 1e-6 * i;
    for (int i = lane; i < 64; i += 64) flags[i] = 1 << 30;
    __syncthreads();
    volatile SO_LDS double* xs = (volatile SO_LDS double*)buf;
    volatile SO_LDS double* ss = (volatile SO_LDS double*)buf + 32 * 64;
    volatile SO_LDS int* fl = (volatile SO_LDS int*)flags;
    double a0 = 1e-3 * threadIdx.x, a1 = 2e-3, a2 = 3e-3;
    v4d st = v4d{1e-3, 2e-3, 3e-3, 0};
    double cur[3] = {0.5, 0.25, 0.125}, nxt[3] = {0, 0, 0};
    int f1 = 1 << 30;
    long long t0 = clock64();
    int slot = 0;
    for (int it = 0; it < iters; ++it) {
        v4d acc = v4d{cur[0], cur[1], cur[2], 0};
        int f2 = 0;
        if (MODE == 2) {  // requests at the top, before the MFMAs
            if (f1 > it) {
                for (int v = 0; v < 3; ++v) nxt[v] = xs[slot * 192 + v * 64 + lane];
                f2 = fl[slot];
            }
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, st[0], acc, 0, 0, 0);
        if (MODE == 1 || MODE == 3) {  // everything under the first MFMA
            __builtin_amdgcn_sched_barrier(0);
            if (f1 > it) {
                for (int v = 0; v < 3; ++v) nxt[v] = xs[slot * 192 + v * 64 + lane];
                f2 = fl[slot];
            }
            for (int v = 0; v < 3; ++v) ss[slot * 192 + v * 64 + lane] = st[v];
            fl[32 + (slot & 7)] = it;
            __builtin_amdgcn_sched_barrier(0);
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, st[1], acc, 0, 0, 0);
        if (MODE == 2) {
            __builtin_amdgcn_sched_barrier(0);
            for (int v = 0; v < 3; ++v) ss[slot * 192 + v * 64 + lane] = st[v];
            fl[32 + (slot & 7)] = it;
            __builtin_amdgcn_sched_barrier(0);
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, st[2], acc, 0, 0, 0);
        if (MODE == 3) __builtin_amdgcn_sched_barrier(0);
        st = acc;
        if (MODE != 0) {
            for (int v = 0; v < 3; ++v) cur[v] = nxt[v];
            f1 = __builtin_amdgcn_readfirstlane(f2);
        }
        slot = slot + 1 == 21 ? 0 : slot + 1;
    }
    long long t1 = clock64();
    sink[blockIdx.x * blockDim.x + threadIdx.x] = st[0] + st[1] + st[2] + cur[0];
    if ((threadIdx.x & 63) == 0) out[blockIdx.x] = t1 - t0;
}

// The form the chain wave uses: two steps per loop iteration with the roles of the register sets swapped (no copies of
// the state or of the operands), every LDS request under a step's FIRST MFMA, and the counter read requested two steps
// before it is looked at (so that no wait ever stands between two MFMAs).
__global__ void k2(long long* out, double* sink, int iters) {
    __shared__ double buf[64 * 64];
    __shared__ int flags[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 64; i += 64) buf[i] = 1e-6 * i;
    for (int i = lane; i < 64; i += 64) flags[i] = 1 << 30;
    __syncthreads();
    volatile SO_LDS double* xs = (volatile SO_LDS double*)buf;
    volatile SO_LDS double* ss = (volatile SO_LDS double*)buf + 32 * 64;
    volatile SO_LDS int* fl = (volatile SO_LDS int*)flags;
    double a0 = 1e-3 * threadIdx.x, a1 = 2e-3, a2 = 3e-3;
    v4d sA = v4d{1e-3, 2e-3, 3e-3, 0}, sB = v4d{0, 0, 0, 0};
    double dA[3] = {0.5, 0.25, 0.125}, dB[3] = {0.1, 0.2, 0.3};
    int fA = 1 << 30, fB = 1 << 30;  // counter values requested in earlier steps (pending LDS loads)
    long long t0 = clock64();
    int slot = 0;
    auto step = [&](int it, v4d& sin, v4d& sout, double (&din)[3], int& fold, int& fnew) __attribute__((always_inline)) {
        v4d acc = v4d{din[0], din[1], din[2], 0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, sin[0], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        const int f = __builtin_amdgcn_readfirstlane(fold);  // requested two steps ago
        if (f > it) {
            for (int v = 0; v < 3; ++v) din[v] = xs[slot * 192 + v * 64 + lane];  // operands of step it + 2 into the set just read
            fnew = fl[slot];
        }
        for (int v = 0; v < 3; ++v) ss[slot * 192 + v * 64 + lane] = sin[v];
        fl[32 + (slot & 7)] = it;
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, sin[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, sin[2], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        sout = acc;
        slot = slot + 1 == 21 ? 0 : slot + 1;
    };
    for (int it = 0; it < iters; it += 2) {
        step(it, sA, sB, dA, fA, fA);
        step(it + 1, sB, sA, dB, fB, fB);
    }
    long long t1 = clock64();
    sink[blockIdx.x * blockDim.x + threadIdx.x] = sA[0] + sA[1] + sA[2] + dA[0] + sB[0] + dB[1];
    if ((threadIdx.x & 63) == 0) out[blockIdx.x] = t1 - t0;
}

// ... and with every VECTOR instruction (addresses, the counter's readfirstlane, the counter value to store) moved out
// from under the MFMAs into the gap before a step's first one: an fp64 MFMA keeps the vector ALU for its 64 cycles, so
// a v_mov "under" it waits for its end and pushes the next MFMA of the chain back by that much.
__global__ void k3(long long* out, double* sink, int iters) {
    __shared__ double buf[64 * 64];
    __shared__ int flags[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 64; i += 64) buf[i] = 1e-6 * i;
    for (int i = lane; i < 64; i += 64) flags[i] = 1 << 30;
    __syncthreads();
    const uint32_t xs0 = (uint32_t)(uintptr_t)(SO_LDS double*)buf + lane * 8, ss0 = xs0 + 32 * 64 * 8;
    const uint32_t fl0 = (uint32_t)(uintptr_t)(SO_LDS int*)flags;
    double a0 = 1e-3 * threadIdx.x, a1 = 2e-3, a2 = 3e-3;
    v4d sA = v4d{1e-3, 2e-3, 3e-3, 0}, sB = v4d{0, 0, 0, 0};
    double dA[3] = {0.5, 0.25, 0.125}, dB[3] = {0.1, 0.2, 0.3};
    int fA = 1 << 30, fB = 1 << 30;
    long long t0 = clock64();
    int slot = 0;
    auto step = [&](int it, v4d& sin, v4d& sout, double (&din)[3], int& fold) __attribute__((always_inline)) {
        // ---- the gap: vector instructions ----
        const int f = __builtin_amdgcn_readfirstlane(fold);
        uint32_t ax = xs0 + slot * 1536, as = ss0 + slot * 1536;
        uint32_t af = fl0 + slot * 4, ag = fl0 + 128 + (slot & 7) * 4;
        int itv = it;
        asm volatile("" : "+v"(ax), "+v"(as), "+v"(af), "+v"(ag), "+v"(itv));  // (in vector registers NOW)
        v4d acc = v4d{din[0], din[1], din[2], 0};
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, sin[0], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // ---- under the first MFMA: scalar and LDS instructions only ----
        if (f > it) {
            for (int v = 0; v < 3; ++v) din[v] = *(volatile SO_LDS double*)(uintptr_t)(ax + v * 512);
            fold = *(volatile SO_LDS int*)(uintptr_t)af;
        }
        for (int v = 0; v < 3; ++v) *(volatile SO_LDS double*)(uintptr_t)(as + v * 512) = sin[v];
        *(volatile SO_LDS int*)(uintptr_t)ag = itv;
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, sin[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, sin[2], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        sout = acc;
        slot = slot + 1 == 21 ? 0 : slot + 1;
    };
    for (int it = 0; it < iters; it += 2) {
        step(it, sA, sB, dA, fA);
        step(it + 1, sB, sA, dB, fB);
    }
    long long t1 = clock64();
    sink[blockIdx.x * blockDim.x + threadIdx.x] = sA[0] + sA[1] + sA[2] + dA[0] + sB[0] + dB[1];
    if ((threadIdx.x & 63) == 0) out[blockIdx.x] = t1 - t0;
}

// The same recurrence on v_mfma_f64_4x4x4_4b_f64: A^16 of a cascade is block lower triangular in 4 x 4 blocks, so a step is
// one instruction per block (r, c), c <= r, applied to all four groups of four sequences -- NI = 6 (three row blocks), 3
// (two) or 1 -- in the order (2,0) (1,0) (0,0) (2,1) (1,1) (2,2): every accumulate chain spaced, every B operand of the
// next step ready for several issue slots.  A row block of the state is ONE register pair (D is a B operand where it is).
// LDS 0: bare.  1: k3's traffic and rules -- vector instructions in the gap, the state writes behind the first
// instruction, the operand reads behind the last that takes the old operands as its C --, 2: all of it behind the first,
// 3: the reads behind the step's last instruction.
template <int NI, int LDS>
__global__ void k4(long long* out, double* sink, int iters) {
    constexpr int NK = NI == 6 ? 3 : NI == 3 ? 2 : 1;
    __shared__ double buf[64 * 64];
    __shared__ int flags[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 64; i += 64) buf[i] = 1e-6 * i;
    for (int i = lane; i < 64; i += 64) flags[i] = 1 << 30;
    __syncthreads();
    const uint32_t xs0 = (uint32_t)(uintptr_t)(SO_LDS double*)buf + lane * 8, ss0 = xs0 + 32 * 64 * 8;
    const uint32_t fl0 = (uint32_t)(uintptr_t)(SO_LDS int*)flags;
    double a[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[r][c] = 1e-3 * (threadIdx.x + 1) * (r + 1) - 2e-3 * c;
    double sA[3] = {1e-3, 2e-3, 3e-3}, sB[3] = {0, 0, 0};
    double dA[3] = {0.5, 0.25, 0.125}, dB[3] = {0.1, 0.2, 0.3};
    int fA = 1 << 30, fB = 1 << 30;
    long long t0 = clock64();
    int slot = 0;
    auto step = [&](int it, double (&sin)[3], double (&sout)[3], double (&din)[3], int& fold) __attribute__((always_inline)) {
        int f = 0, itv = it;
        uint32_t ax = 0, as = 0, af = 0, ag = 0;
        if (LDS) {  // ---- the gap: vector instructions ----
            f = __builtin_amdgcn_readfirstlane(fold);
            ax = xs0 + slot * 1536, as = ss0 + slot * 1536;
            af = fl0 + slot * 4, ag = fl0 + 128 + (slot & 7) * 4;
            asm volatile("" : "+v"(ax), "+v"(as), "+v"(af), "+v"(ag), "+v"(itv));
        }
        auto put = [&]() __attribute__((always_inline)) {
            if (!LDS) return;
            for (int v = 0; v < NK; ++v) *(volatile SO_LDS double*)(uintptr_t)(as + v * 512) = sin[v];
            *(volatile SO_LDS int*)(uintptr_t)ag = itv;
        };
        auto get = [&]() __attribute__((always_inline)) {
            if (!LDS) return;
            if (f > it) {
                for (int v = 0; v < NK; ++v) din[v] = *(volatile SO_LDS double*)(uintptr_t)(ax + v * 512);
                fold = *(volatile SO_LDS int*)(uintptr_t)af;
            }
        };
        double acc0, acc1 = 0, acc2 = 0;
        __builtin_amdgcn_sched_barrier(0);
        if (NK == 3) {
            acc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[2][0], sin[0], din[2], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            put();
            if (LDS == 2) get();
            __builtin_amdgcn_sched_barrier(0);
        }
        if (NK >= 2) {
            acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[1][0], sin[0], din[1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (NK == 2) {
                put();
                if (LDS == 2) get();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        acc0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[0][0], sin[0], din[0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (NK == 1) put();
        if (LDS == 1 || (LDS == 2 && NK == 1)) get();
        __builtin_amdgcn_sched_barrier(0);
        if (NK == 3) acc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[2][1], sin[1], acc2, 0, 0, 0);
        if (NK >= 2) acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[1][1], sin[1], acc1, 0, 0, 0);
        if (NK == 3) acc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[2][2], sin[2], acc2, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (LDS == 3) get();
        __builtin_amdgcn_sched_barrier(0);
        sout[0] = acc0, sout[1] = acc1, sout[2] = acc2;
        slot = slot + 1 == 10 ? 0 : slot + 1;  // (10 slots of 192 doubles: inside the half of buf each side has)
    };
    for (int it = 0; it < iters; it += 2) {
        step(it, sA, sB, dA, fA);
        step(it + 1, sB, sA, dB, fB);
    }
    long long t1 = clock64();
    sink[blockIdx.x * blockDim.x + threadIdx.x] = sA[0] + sA[1] + sA[2] + dA[0] + sB[0] + dB[1];
    if ((threadIdx.x & 63) == 0) out[blockIdx.x] = t1 - t0;
}

// k4's step with a hand-counted wait.  The small shape leaves no idle gap in front of a step's first instruction (the B
// operand has been ready for three issue slots), so whatever stands there is paid in full: k4<6, 1> is 226 cycles, 111 over
// the bare step.  Here:
//   * the reads are unconditional inline-asm ds_reads into the registers the step has just used, and the ONE wait of a step is
//     counted by hand: the requests of two steps ago are in when at most the 2 (NK + 1) of the step before are outstanding;
//   * all counters come with one ds_read_b32 (lane s = slot s's counter, a loop-invariant address), picked with v_readlane;
//   * the state counter's address is loop invariant; the next step's slot arithmetic stands under this step's last instructions.
// rsos_chain4 keeps the last two and leaves the waits to the compiler: in the kernel the counted wait measured no different
// (profiles/r17/chain4_forms.jsonl), and here it is the slower one.
template <int NI>
__global__ void k5(long long* out, double* sink, int iters) {
    constexpr int NK = NI == 6 ? 3 : NI == 3 ? 2 : 1;
    constexpr int NX = 10;
    __shared__ double buf[64 * 64];
    __shared__ int flags[64];
    const int lane = threadIdx.x;
    for (int i = lane; i < 64 * 64; i += 64) buf[i] = 1e-6 * i;
    for (int i = lane; i < 64; i += 64) flags[i] = 1 << 30;
    __syncthreads();
    const uint32_t xs0 = (uint32_t)(uintptr_t)(SO_LDS double*)buf + lane * 8, ss0 = xs0 + 32 * 64 * 8;
    const uint32_t fl0 = (uint32_t)(uintptr_t)(SO_LDS int*)flags;
    uint32_t afl = fl0 + 4 * (lane < NX ? lane : NX - 1), ag = fl0 + 128;
    asm volatile("" : "+v"(afl), "+v"(ag));
    double a[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[r][c] = 1e-3 * (threadIdx.x + 1) * (r + 1) - 2e-3 * c;
    double sA[3] = {1e-3, 2e-3, 3e-3}, sB[3] = {0, 0, 0};
    double dA[3] = {0.5, 0.25, 0.125}, dB[3] = {0.1, 0.2, 0.3};
    int fA = 1 << 30, fB = 1 << 30;
    long long t0 = clock64();
    int slot = 2;
    // (scalars: byte offsets of block it + 2's D . x slot and of the even / odd block's state slot -- the state slot of block
    //  it + 2 has the number of its D . x slot.  A wave issues an instruction every four cycles at best: the step is as long
    //  as its instruction count, and the slots' arithmetic is five scalar instructions)
    uint32_t offx = 2 * 1536, offsA = 0, offsB = 1536;
    int nbw = iters;
    asm volatile("" : "+s"(nbw));
    auto step = [&](int it, double (&sin)[3], double (&sout)[3], double (&din)[3], int& fpend, uint32_t& offs) __attribute__((always_inline)) {
        // ---- the gap ----
        if constexpr (NK == 3) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(din[0]), "+v"(din[1]), "+v"(din[2]), "+v"(fpend)::"memory");
        else if constexpr (NK == 2) asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(din[0]), "+v"(din[1]), "+v"(fpend)::"memory");
        else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(din[0]), "+v"(fpend)::"memory");
        const int f = __builtin_amdgcn_readlane(fpend, slot);  // (slot: of block it + 2)
        uint32_t ax = xs0 + offx, as = ss0 + offs;
        int itv = it;
        asm volatile("" : "+v"(ax), "+v"(as), "+v"(itv));
        auto put = [&]() __attribute__((always_inline)) {
            for (int v = 0; v < NK; ++v) *(volatile SO_LDS double*)(uintptr_t)(as + v * 512) = sin[v];
            *(volatile SO_LDS int*)(uintptr_t)ag = itv;
        };
        auto get = [&]() __attribute__((always_inline)) {
            if (__builtin_expect(f < it + 3, 0) && it + 3 <= nbw) __builtin_trap();  // (the place of the real loop's spin)
            asm volatile("ds_read_b64 %0, %1" : "=v"(din[0]) : "v"(ax) : "memory");
            if constexpr (NK >= 2) asm volatile("ds_read_b64 %0, %1 offset:512" : "=v"(din[1]) : "v"(ax) : "memory");
            if constexpr (NK >= 3) asm volatile("ds_read_b64 %0, %1 offset:1024" : "=v"(din[2]) : "v"(ax) : "memory");
            asm volatile("ds_read_b32 %0, %1" : "=v"(fpend) : "v"(afl) : "memory");
        };
        auto next_slot = [&]() __attribute__((always_inline)) {
            offs = offx;
            slot = slot + 1 == NX ? 0 : slot + 1;
            offx = (uint32_t)slot * 1536u;
            asm volatile("" : "+s"(offx), "+s"(offs));
        };
        double acc0, acc1 = 0, acc2 = 0;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (NK == 3) {
            acc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[2][0], sin[0], din[2], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            put();
            __builtin_amdgcn_sched_barrier(0);
            acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[1][0], sin[0], din[1], 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[0][0], sin[0], din[0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            get();
            __builtin_amdgcn_sched_barrier(0);
            acc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[2][1], sin[1], acc2, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            next_slot();
            __builtin_amdgcn_sched_barrier(0);
            acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[1][1], sin[1], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[2][2], sin[2], acc2, 0, 0, 0);
        } else if constexpr (NK == 2) {
            acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[1][0], sin[0], din[1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            put();
            __builtin_amdgcn_sched_barrier(0);
            acc0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[0][0], sin[0], din[0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            get();
            next_slot();
            __builtin_amdgcn_sched_barrier(0);
            acc1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[1][1], sin[1], acc1, 0, 0, 0);
        } else {
            acc0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a[0][0], sin[0], din[0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            put();
            get();
            next_slot();
        }
        __builtin_amdgcn_sched_barrier(0);
        sout[0] = acc0, sout[1] = acc1, sout[2] = acc2;
    };
    for (int it = 0; it < iters; it += 2) {
        step(it, sA, sB, dA, fA, offsA);
        step(it + 1, sB, sA, dB, fB, offsB);
    }
    long long t1 = clock64();
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(dA[0]), "+v"(dB[1])::"memory");
    sink[blockIdx.x * blockDim.x + threadIdx.x] = sA[0] + sA[1] + sA[2] + dA[0] + sB[0] + dB[1];
    if ((threadIdx.x & 63) == 0) out[blockIdx.x] = t1 - t0;
}

// Which lane holds what for v_mfma_f64_4x4x4_4b_f64: one launch with indicator operands.  ta[q][l]: B = 1 in lane q alone,
// A = 1 + lane -> D lane l holds 1 + (the A lane that met B lane q there) or 0; tb[p][l]: the same with A the indicator.
__global__ void k4_lanes(double* ta, double* tb) {
    const int lane = threadIdx.x;
    for (int q = 0; q < 64; ++q) {
        ta[q * 64 + lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(1.0 + lane, lane == q ? 1.0 : 0.0, 0.0, 0, 0, 0);
        tb[q * 64 + lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(lane == q ? 1.0 : 0.0, 1.0 + lane, 0.0, 0, 0, 0);
    }
}

// every way to spread (block, x, y) over the three base-4 digits of a lane, for A (x, y) = (i, k), B (k, j), D (i, j)
static int lane_of(int perm, int b, int x, int y) {
    static const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};  // digit of b, x, y
    return (b << (2 * P[perm][0])) | (x << (2 * P[perm][1])) | (y << (2 * P[perm][2]));
}
static const char* lane_name(int perm, const char* x, const char* y) {
    static char buf[8][64];
    static int n = 0;
    static const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const char* nm[3] = {"b", x, y};
    const char* d[3];
    for (int t = 0; t < 3; ++t) d[P[perm][t]] = nm[t];
    char* o = buf[n++ & 7];
    snprintf(o, 64, "16%s + 4%s + %s", d[2], d[1], d[0]);
    return o;
}

static void lane_probe() {
    double *ta, *tb;
    (void)hipMalloc(&ta, 8 * 4096);
    (void)hipMalloc(&tb, 8 * 4096);
    hipLaunchKernelGGL(k4_lanes, dim3(1), dim3(64), 0, 0, ta, tb);
    (void)hipDeviceSynchronize();
    static double ha[4096], hb[4096];
    (void)hipMemcpy(ha, ta, 8 * 4096, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hb, tb, 8 * 4096, hipMemcpyDeviceToHost);
    int found = 0;
    for (int pa = 0; pa < 6; ++pa)
        for (int pb = 0; pb < 6; ++pb)
            for (int pd = 0; pd < 6; ++pd) {
                static double wa[4096], wb[4096];
                for (int i = 0; i < 4096; ++i) wa[i] = wb[i] = 0.0;
                for (int b = 0; b < 4; ++b)
                    for (int i = 0; i < 4; ++i)
                        for (int j = 0; j < 4; ++j)
                            for (int k = 0; k < 4; ++k) {
                                const int la = lane_of(pa, b, i, k), lb = lane_of(pb, b, k, j), ld = lane_of(pd, b, i, j);
                                wa[lb * 64 + ld] = 1.0 + la;
                                wb[la * 64 + ld] = 1.0 + lb;
                            }
                bool ok = true;
                for (int i = 0; i < 4096 && ok; ++i) ok = wa[i] == ha[i] && wb[i] == hb[i];
                if (ok) {
                    ++found;
                    printf("lane map: A_b[i][k] in lane %s, B_b[k][j] in lane %s, D_b[i][j] in lane %s -- D %s a B operand where it is\n",
                           lane_name(pa, "i", "k"), lane_name(pb, "k", "j"), lane_name(pd, "i", "j"), pb == pd ? "IS" : "is NOT");
                }
            }
    if (!found) {
        printf("lane map: no digit permutation fits; raw table (B indicator lane q: D lane -> 1 + A lane)\n");
        for (int q = 0; q < 64; ++q) {
            printf("q %2d:", q);
            for (int l = 0; l < 64; ++l)
                if (ha[q * 64 + l] != 0.0) printf(" D%d<-A%d", l, (int)ha[q * 64 + l] - 1);
            printf("\n");
        }
    }
    (void)hipFree(ta);
    (void)hipFree(tb);
}

template <int NI, int LDS>
static double run4(long long* d, double* s, int iters, const char* what) {
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((k4<NI, LDS>), dim3(1), dim3(64), 0, 0, d, s, iters);
    (void)hipDeviceSynchronize();
    long long h;
    (void)hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    printf("k4<%d>: %.1f cycles per step  (4x4x4_4b, %d instructions per step, %s)\n", NI, (double)h / iters, NI, what);
    return (double)h / iters;
}

template <int NI>
static double run5(long long* d, double* s, int iters) {
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((k5<NI>), dim3(1), dim3(64), 0, 0, d, s, iters);
    (void)hipDeviceSynchronize();
    long long h;
    (void)hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    printf("k5<%d>: %.1f cycles per step  (... asm reads, one counted wait, scalar work under the last instructions)\n", NI, (double)h / iters);
    return (double)h / iters;
}

int main() {
    long long* d;
    double* s;
    (void)hipMalloc(&d, 8 * 4096);
    (void)hipMalloc(&s, 8 * 1024 * 1024);
    const int iters = 4000;
    lane_probe();
    const char* names[] = {"bare recurrence", "LDS traffic under the first MFMA", "reads before, writes under the second MFMA",
                           "under the first MFMA, fences around the third"};
    for (int mode = 0; mode < 4; ++mode) {
        for (int rep = 0; rep < 2; ++rep) {
            switch (mode) {
            case 0: hipLaunchKernelGGL(k<0>, dim3(1), dim3(64), 0, 0, d, s, iters); break;
            case 1: hipLaunchKernelGGL(k<1>, dim3(1), dim3(64), 0, 0, d, s, iters); break;
            case 2: hipLaunchKernelGGL(k<2>, dim3(1), dim3(64), 0, 0, d, s, iters); break;
            default: hipLaunchKernelGGL(k<3>, dim3(1), dim3(64), 0, 0, d, s, iters); break;
            }
        }
        (void)hipDeviceSynchronize();
        long long h;
        (void)hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
        printf("mode %d: %.1f cycles per step  (%s)\n", mode, (double)h / iters, names[mode]);
    }
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k2, dim3(1), dim3(64), 0, 0, d, s, iters);
    (void)hipDeviceSynchronize();
    long long h;
    (void)hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    printf("k2    : %.1f cycles per step  (two steps per iteration, register sets swapped, counter two steps ahead)\n", (double)h / iters);
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k3, dim3(1), dim3(64), 0, 0, d, s, iters);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    printf("k3    : %.1f cycles per step  (... and no vector instruction under an MFMA)\n", (double)h / iters);
    const double c3 = (double)h / iters;
    run4<6, 0>(d, s, iters, "bare");
    const double c61 = run4<6, 1>(d, s, iters, "LDS traffic: writes behind the first, reads behind the third");
    const double c62 = run4<6, 2>(d, s, iters, "LDS traffic: all behind the first");
    const double c63 = run4<6, 3>(d, s, iters, "LDS traffic: writes behind the first, reads behind the last");
    run4<3, 0>(d, s, iters, "bare");
    run4<3, 1>(d, s, iters, "LDS traffic");
    run4<1, 0>(d, s, iters, "bare");
    run4<1, 1>(d, s, iters, "LDS traffic");
    const double c5 = run5<6>(d, s, iters);
    run5<3>(d, s, iters);
    run5<1>(d, s, iters);
    (void)c62, (void)c63;
    printf("six instructions with LDS traffic / k3 = %.3f (k4), %.3f (k5) (go on at <= 0.75)\n", c61 / c3, c5 / c3);
    return 0;
}
