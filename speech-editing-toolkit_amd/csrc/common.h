// Shared device helpers for libset_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <type_traits>

#include "set_amd.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
template <int N> using ic = std::integral_constant<int, N>;

// ---- host-side error plumbing -------------------------------------------------------------
extern thread_local char g_set_err[512];

static inline int set_fail(int code, const char *what, const char *detail) {
    snprintf(g_set_err, sizeof(g_set_err), "%s: %s", what, detail ? detail : "");
    return code;
}
static inline int set_check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_fail(SET_E_LAUNCH, what, hipGetErrorString(e));
    return SET_OK;
}
#define SET_REQUIRE(cond, what)                                        \
    do {                                                               \
        if (!(cond)) return set_fail(SET_E_INVALID, what, #cond);      \
    } while (0)
#define SET_HIP(call, what)                                                        \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess) return set_fail(SET_E_LAUNCH, what, hipGetErrorString(e__)); \
    } while (0)

// ---- launch-time state set up once per device -----------------------------------------------
// Launches come from the main thread (forward) and torch's autograd device thread (backward), on any device.  A site keeps one
// `static SetDeviceOnce`; run(f) calls f() -> SET_OK | error on the current device unless f already succeeded there.  Success is one
// bit per device (release / acquire); a failure records nothing, so the next call retries.  Two threads racing on a first call may
// both run f: every f is idempotent (the same attribute value, the same constant bytes).  A device index beyond the mask, or none
// (hipGetDevice failed), runs f every time: correct, only slower.  Warm path: hipGetDevice and one atomic load.
struct SetDeviceOnce {
    std::atomic<uint64_t> done{0};
    template <typename F> int run(F &&f) {
        int dev = -1;
        const uint64_t bit = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 ? uint64_t(1) << dev : 0;
        if (done.load(std::memory_order_acquire) & bit) return SET_OK;
        const int rc = f();
        if (rc == SET_OK) done.fetch_or(bit, std::memory_order_release);
        return rc;
    }
};
// Opt `kernels` in to `bytes` of dynamic LDS on the current device, once per device.
template <typename... K>
static inline int set_lds_optin(SetDeviceOnce &once, int bytes, const char *what, K... kernels) {
    return once.run([&] {
        for (const void *k : {reinterpret_cast<const void *>(kernels)...})
            SET_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), what);
        return SET_OK;
    });
}
// The current device's CU count, queried once per device; on failure the query's error (nothing cached, *n_cu untouched).  The
// cached count, nonzero once known, is the per-device done flag; like SetDeviceOnce, a device beyond the table asks every time.
static inline hipError_t set_cu_count(int *n_cu) {
    static std::atomic<int> cached[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool slot = dev >= 0 && dev < 64;
    int n = slot ? cached[dev].load(std::memory_order_relaxed) : 0;
    if (n == 0) {
        e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        if (slot) cached[dev].store(n, std::memory_order_relaxed);
    }
    *n_cu = n;
    return hipSuccess;
}

const uint64_t *set_seed_delta_ptr();  // the device word of set_rng_seed_delta (csrc/diffusion_ops.hip), NULL when unset
// Clear `words` 32-bit words with a KERNEL.  Not hipMemsetAsync: as a memset node of a captured graph (training.GraphedTrainStep) a clear
// was not ordered against eager work enqueued between two replays (ROCm 7.2) -- buffers came out as uninitialised memory.
static __global__ void __launch_bounds__(256) set_zero_words_kernel(unsigned *p, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) p[i] = 0u;
}
static inline bool set_aligned16(const void *a, const void *b, const void *c) {  // 16-byte vector accesses are legal on all three
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
static inline hipError_t set_zero_async(void *p, size_t bytes, hipStream_t s) {
    const int64_t words = (int64_t)((bytes + 3) / 4);
    hipLaunchKernelGGL(set_zero_words_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, reinterpret_cast<unsigned *>(p), words);
    return hipGetLastError();
}
static inline unsigned set_blocks(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }
static inline int set_round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- activations (match torch CPU fp32 semantics) -----------------------------------------
__device__ __forceinline__ float dev_softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float dev_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float dev_act(float v, int act, float p) {
    switch (act) {
        case SET_ACT_RELU: return v > 0.0f ? v : 0.0f;
        case SET_ACT_GELU: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
        case SET_ACT_TANH: return tanhf(v);
        case SET_ACT_SOFTPLUS: return dev_softplus(v);
        case SET_ACT_MISH: return v * tanhf(dev_softplus(v));
        case SET_ACT_LRELU: return v > 0.0f ? v : v * p;
        default: return v;
    }
}
__device__ __forceinline__ float dev_pro(float v, int pro, float p) {
    switch (pro) {
        case SET_PRO_LRELU: return v > 0.0f ? v : v * p;
        case SET_PRO_DIV: return v / p;
        default: return v;
    }
}
// prologue with the code resolved at compile time: inside the staging loops a run-time `switch (pro)` per element turns
// into a scalar branch tree (+ an IEEE division sequence) per element -- measured 7.5 us per 32-channel stage against
// 0.3 us of MFMA work.  The callers switch ONCE per stage and instantiate the loop per code.
template <int PRO>
__device__ __forceinline__ float pro_c(float v, float p) {
    if constexpr (PRO == SET_PRO_LRELU) return v > 0.0f ? v : v * p;
    else if constexpr (PRO == SET_PRO_DIV) return v / p;
    else return v;
}
// the gate of the fused layer kernels (hardware exp and reciprocal) and their bf16 conversions
__device__ __forceinline__ float fsig(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float ftanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }
__device__ __forceinline__ unsigned short f2bf(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf2f(unsigned short u) { return __builtin_bit_cast(float, (unsigned)u << 16); }
__device__ __forceinline__ unsigned short f2h(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
__device__ __forceinline__ float h2f(unsigned short u) { return (float)__builtin_bit_cast(_Float16, u); }

// sum over the 64 lanes of a wave, every lane gets it
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- MFMA f32 32x32x2 fragment maps (cdna_hip_programming.md section 3) --------------------
//   A operand: lane l holds A[i = l & 31][k = l >> 5]
//   B operand: lane l holds B[k = l >> 5][j = l & 31]
//   C/D      : reg r of lane l is D[row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][col = l & 31]
__device__ __forceinline__ int mfma32_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
// Accumulator register r of the 32x32 block holds row  urow16(r) + 4*(lane>>5):  the first term is wave-uniform, so a
// global access can be  (uniform row pointer, SGPR) + (one per-lane 32-bit offset, VGPR)  -- no per-row 64-bit address
// registers (those spilled and serialised the epilogue stores behind vmcnt(0) reloads).
__device__ __forceinline__ int urow16(int r) { return (r & 3) + 8 * (r >> 2); }
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ---- 16-bit MFMAs 32x32x16: lane l holds A[i = l & 31][k = 8 (l >> 5) .. + 7] and B[k = 8 (l >> 5) .. + 7][j = l & 31] as four dwords; C/D as above
__device__ __forceinline__ f32x16 mfma_f16(u32x4_t a, u32x4_t b, f32x16 c) {
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_bf16(u32x4_t a, u32x4_t b, f32x16 c) {
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- raw buffer addressing: wave-uniform base (SGPR descriptor) + per-lane byte offset (one VGPR shared by every
//      row) + wave-uniform byte offset (SGPR).  hipcc otherwise materialises a 64-bit VGPR address per load/store
//      (v_lshl_add_u64 + 2 VGPRs each), which is what pushes row-looped tile code into spills.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)0x7fffffff, (int)0x00020000);
}
// a per-lane offset at or beyond the descriptor's num_records (0x7fffffff): raw-buffer loads return 0 there, stores are dropped
constexpr unsigned BUF_OOB = 0x80000000u;
__device__ __forceinline__ float buf_load(rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ f32x4 buf_load4(rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ u32x4_t buf_load_u4(rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ void buf_store4(f32x4 v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ void buf_store(float v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)voff, (int)soff, 0);
}
// streaming 16-byte accesses of data ONE CU writes and reads once per pass (a block's private buffer): nt load (evict-first at the
// L2), sc1 store (written through and dropped from the L2) -- they must not push the weights every CU of the XCD re-reads out of the L2
__device__ __forceinline__ f32x4 buf_load4_stream(rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 2));
}
__device__ __forceinline__ void buf_store4_stream(f32x4 v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, (int)voff, (int)soff, 16);
}
// fp32 add at the L2 without return (buffer_atomic_add_f32): for read-modify-write of data this block owns exclusively
__device__ __forceinline__ void buf_atomic_add(float v, rsrc_t r, unsigned voff, unsigned soff) {
    (void)__builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, r, (int)voff, (int)soff, 0);
}
// agent-scope write-through store (sc1): complete (vmcnt) = visible to every XCD, no L2 write-back needed later
__device__ __forceinline__ void buf_store_agent(float v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)voff, (int)soff, 16);
}
// ---- the channel-quad ("q4") layout of an fp32 [256][T] buffer: the x ping-pong and skip workspaces of the reverse loop (DESIGN 3.6 with fp32
// elements).  Element (c, t) is float q4f_index(c, t, T) of its utterance: the four channels of a quad at one frame are 16 contiguous bytes, which
// is what four consecutive accumulator registers of a 32x32 block hold (urow16).  Byte offset = (wave-uniform) 4 (c & ~3) T + (per-lane) 16 t.
__host__ __device__ inline int64_t q4f_index(int c, int t, int T) { return ((int64_t)(c >> 2) * T + t) * 4 + (c & 3); }
// 16-byte store with its row offset in an SGPR, plain or agent-scope write-through (sc1, as buf_store_agent).  gfx950 needs a wait state between such
// a store and a VALU instruction that rewrites its data registers, and the compiler does not insert it (tests/test_isa_schedule.py):
// the pad follows the store, and the scheduling barriers keep it there.
template <bool AGENT>
__device__ __forceinline__ void buf_store4_padded(f32x4 v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, (int)voff, (int)soff, AGENT ? 16 : 0);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 1" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// two fp32 values -> their two-piece fp16 splittings (a0 + a1 = a to 22 significand bits), each piece pair packed into one dword with the
// first value in the low half: v_cvt_pk_f16_f32, two back-conversions, v_pk_add_f32, v_cvt_pk_f16_f32 -- five instructions where two
// scalar splittings and their packing take ten.  Same roundings (to nearest even, twice) as `h0 = (f16)a; h1 = (f16)(a - (float)h0)`.
__device__ __forceinline__ void split2_f16(float a, float b, unsigned &p0, unsigned &p1) {
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
    typedef float f2_t __attribute__((ext_vector_type(2)));
    const f2_t v = {a, b};
    const h2_t h0 = __builtin_convertvector(v, h2_t);
    const h2_t h1 = __builtin_convertvector(v - __builtin_convertvector(h0, f2_t), h2_t);
    p0 = __builtin_bit_cast(unsigned, h0);
    p1 = __builtin_bit_cast(unsigned, h1);
}

// ---- shared fp32 MFMA GEMM inner loop -----------------------------------------------------------------------
// acc[RB][NCB] (32x32 blocks) += A * B over `ng` groups of GS k-steps (2 k values each).
//   A operand: packed image, one vector of RB floats per lane per k-step:  wp[u * 64] for k-step u of the group
//   B operand: LDS, bp[u * rstep + 32 * cb]
// Two operand sets ping-pong (no register copies): while the MFMAs of one group run, the loads of the next group are
// issued one k-step at a time, each pinned in front of its k-step's MFMAs with sched_barrier (otherwise the
// scheduler sinks them next to their use).  `advance(g)` moves wp / bp from group g to group g+1.  ng must be even.
template <int RB> struct AVec;
template <> struct AVec<1> { typedef float type; };
template <> struct AVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct AVec<4> { typedef float type __attribute__((ext_vector_type(4))); };

template <int RB>
__device__ __forceinline__ float avec_get(const typename AVec<RB>::type &v, int r) {
    if constexpr (RB == 1) return v; else return v[r];
}

template <int RB, int NCB, int GS>
struct KOps {
    typename AVec<RB>::type A[GS];
    float B[GS][NCB];
};

template <int RB, int NCB, int GS, typename Adv>
__device__ __forceinline__ void gemm_groups(f32x16 (&acc)[RB][NCB], const typename AVec<RB>::type *&wp, const float *&bp,
                                            int rstep, int ng, Adv advance) {
    KOps<RB, NCB, GS> P, Q;
    auto load_step = [&](KOps<RB, NCB, GS> &o, int u) {
        o.A[u] = wp[u * 64];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) o.B[u][cb] = bp[u * rstep + 32 * cb];
    };
    auto mma_step = [&](const KOps<RB, NCB, GS> &o, int u) {
        __builtin_amdgcn_s_setprio(1);  // co-resident blocks run out of phase: favour the wave that is in its MFMA burst (+3 %)
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[r][cb] = mfma32(avec_get<RB>(o.A[u], r), o.B[u][cb], acc[r][cb]);
        __builtin_amdgcn_s_setprio(0);
    };
#pragma unroll
    for (int u = 0; u < GS; ++u) load_step(P, u);
    for (int g = 0; g < ng; g += 2) {
        advance(g);  // -> group g+1 (always exists: ng is even)
#pragma unroll
        for (int u = 0; u < GS; ++u) {
            load_step(Q, u);
            __builtin_amdgcn_sched_barrier(0);
            mma_step(P, u);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (g + 2 < ng) advance(g + 1);  // last pair: re-load the final group (harmless, in bounds)
#pragma unroll
        for (int u = 0; u < GS; ++u) {
            load_step(P, u);
            __builtin_amdgcn_sched_barrier(0);
            mma_step(Q, u);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
