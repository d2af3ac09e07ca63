// Phase probes: the ONLY place a phase stamp is written.  The shipped library (SET_PHASE_PROBE = 0, the default) holds none: PhaseProbe and
// PhaseTimeline are empty there and every member is a no-op, so the call sites carry no #if and compile to nothing.
//   tools/build_exp.sh <tag> <file.hip> -DSET_PHASE_PROBE=1    instruments the kernels of that file (the library the probes in tools/ load)
//   ... -DSET_PHASE_PROBE=2                                     diffnet_x3.hip only: the one-task timeline of diffnet_stack_x3v_kernel
//
// PhaseProbe<N>: N sums of s_memtime ticks, taken by ONE wave of a block.  start(cond, wave) takes a wave-uniform condition and
// lap(p) a constant slot, so the sums and the last stamp live in scalar registers (s_memtime results are scalar); 32 bits each are enough:
// they hold 2 s even where the counter runs at 2 GHz (measured: ~2000 ticks per us), a launch takes milliseconds.  There is no memory operation between start() and the flush at the end of the kernel:
// one flat access near a k loop makes the wait-count pass treat every outstanding load as possibly out of order and drain the weight ring
// (s_waitcnt vmcnt(0)) at the top of every k-step group, i.e. the probe then measures a different kernel.  The flush is done by lane 0 of
// the sampling wave and ADDS the sums to the file's buffer, so a tool may sum over several launches: plain adds where one block samples,
// flush_atomic where several do.  Call sites pass nothing but the condition, the slot and the buffer: in a default build their arguments
// must fold away (the stack kernels' code generation is sensitive to as little as an empty `if` around a call).
#pragma once
#include "common.h"

#ifndef SET_PHASE_PROBE
#define SET_PHASE_PROBE 0
#endif

#if SET_PHASE_PROBE
template <int N>
struct PhaseProbe {
    uint32_t sum[N] = {}, prev = 0;
    bool on = false;
    // (again) at any point: from here on lap() and count() add in wave `wave` of the block, if `cond`; the sums are kept
    __device__ __forceinline__ void start(bool cond, int wave = 0) {
        on = cond && __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == wave;
        if (on) prev = (uint32_t)__builtin_amdgcn_s_memtime();
    }
    // sum[p] += now - prev; prev = now
    __device__ __forceinline__ void lap(int p) {
        if (on) {
            const uint32_t now = (uint32_t)__builtin_amdgcn_s_memtime();
            sum[p] += now - prev;
            prev = now;
        }
    }
    // a counter in a slot no lap() uses (tasks, layers, stages)
    __device__ __forceinline__ void count(int p, uint32_t n = 1) {
        if (on) sum[p] += n;
    }
    __device__ __forceinline__ void flush(uint64_t *buf) const {
        if (on && (threadIdx.x & 63) == 0)
            for (int p = 0; p < N; ++p) buf[p] += sum[p];
    }
    __device__ __forceinline__ void flush_atomic(uint64_t *buf) const {
        if (on && (threadIdx.x & 63) == 0)
            for (int p = 0; p < N; ++p) atomicAdd(reinterpret_cast<unsigned long long *>(buf + p), (unsigned long long)sum[p]);
    }
    // into int32 words, in units of 1024 ticks (the sync_ws diagnostics of the stack kernels)
    __device__ __forceinline__ void flush_atomic(int *words) const {
        if (on && (threadIdx.x & 63) == 0)
            for (int p = 0; p < N; ++p) atomicAdd(words + p, (int)(sum[p] >> 10));
    }
};
#else
template <int N>
struct PhaseProbe {
    __device__ __forceinline__ void start(bool, int = 0) {}
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ void count(int, uint32_t = 1) {}
    __device__ __forceinline__ void flush(uint64_t *) const {}
    __device__ __forceinline__ void flush_atomic(uint64_t *) const {}
    __device__ __forceinline__ void flush_atomic(int *) const {}
};
#endif

// PhaseTimeline<N> (SET_PHASE_PROBE == 2): absolute stamps of ONE task, kept in scalar registers by every wave and stored by the kernel's own
// #if SET_PHASE_PROBE == 2 block once the task is over -- a different measurement from the sums above (no sum, no sampled block).
template <int N>
struct PhaseTimeline {
#if SET_PHASE_PROBE == 2
    uint64_t ts[N] = {};
    __device__ __forceinline__ void mark(int p) {
        __builtin_amdgcn_sched_barrier(0);
        ts[p] = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
    }
#else
    __device__ __forceinline__ void mark(int) {}
#endif
};

// One per instrumented file (device symbols do not link across translation units): the file's buffer pointer `var` and its extern "C"
// setter.  A default build defines no __device__ symbol -- `var` is a null constant, so `var && ...` folds to false -- and its setter
// accepts NULL only.
#if SET_PHASE_PROBE
#define SET_PHASE_PROBE_BUFFER(var, setter)                                           \
    __device__ uint64_t *var = nullptr;                                               \
    extern "C" int setter(uint64_t *buf) {                                            \
        SET_HIP(hipMemcpyToSymbol(HIP_SYMBOL(var), &buf, sizeof(buf)), #setter);      \
        return SET_OK;                                                                \
    }
#else
#define SET_PHASE_PROBE_BUFFER(var, setter)                                           \
    constexpr uint64_t *var = nullptr;                                                \
    extern "C" int setter(uint64_t *buf) {                                            \
        return buf ? set_fail(SET_E_UNSUPPORTED, #setter, "library built without -DSET_PHASE_PROBE") : SET_OK; \
    }
#endif
