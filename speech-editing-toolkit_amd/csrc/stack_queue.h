// Scheduling of the six persistent layer-stack kernels (diffnet.hip: diffnet_stack_kernel, _wino_kernel, _split_kernel; diffnet_x3.hip:
// diffnet_stack_x3_kernel, _x3v_kernel, _split_x2_kernel): the sync_ws words, the bounded flag wait, the tile publish, the worker count
// and the split-operand kernels' per-task tile fill.  Hand-off protocol (cdna_hip_programming.md Guideline 16): a producer stores its tile agent-scope
// write-through, drains vmcnt, then publishes with ONE relaxed agent-scope store or add; a consumer's ONE lane polls relaxed and follows
// a successful wait with one acquire fence (or reads with agent-scope loads), a barrier hands the tile to the block.
#pragma once
#include <stdlib.h>

#include "common.h"

// ---- 1. sync_ws words (int32, cleared by every launch) ------------------------------------------------------------
constexpr int SQ_COUNTER = 0;      // next task of the (layer, tile) queue: one atomicAdd per claim
constexpr int SQ_ABORT = 1;        // != 0: a wait gave up; every other wait gives up too (the ABI's time-out word)
constexpr int SQ_WAIT_TICKS = 2;   // diagnostics: s_memtime ticks / 1024 the claiming lanes spent waiting ...
constexpr int SQ_FENCE_TICKS = 3;  // ... and publishing
constexpr int SQ_FLAGS = 4;        // [ntiles] per-tile flags: layers done (block-wide store) or parts / waves done (add)
// second per-tile array: the z rendezvous counters of the row-split kernels, the 9 phase sums of a -DSET_PHASE_PROBE=1 build
__host__ __device__ constexpr int sq_flags2(int ntiles) { return SQ_FLAGS + ntiles; }
constexpr int SQ_WINO_PHASE_WORDS = 12;
constexpr int SQ_GROUP_WORDS = 16;  // fixed words of one stack: set_diffusion_loop gives utterance group g, first utterance b0, the
                                    // slice at SQ_GROUP_WORDS * g + 2 * b0 * ceil(T / 32)

enum StackSync { SQ_QUEUE, SQ_ROW_SPLIT, SQ_WINO };
// Words a launch clears.  The ABI promises 16 + 2 B ceil(T / 32) words per stack (include/set_amd.h), and with n = B ceil(T / 32):
//   queue      4 + ntiles,       ntiles <= n (32-frame tiles at the most)
//   row split  4 + 2 ntiles,     ntiles == n
//   Winograd   4 + ntiles + 12,  ntiles <= B ceil(T / 64) <= n
// so every case fits 16 + 2 n.  A group of Bg utterances therefore ends at most where the next group's slice (b0 + Bg, g + 1) begins.
static inline size_t stack_sync_words(StackSync kind, int ntiles) {
    return kind == SQ_ROW_SPLIT ? (size_t)sq_flags2(ntiles) + ntiles : (size_t)sq_flags2(ntiles) + (kind == SQ_WINO ? SQ_WINO_PHASE_WORDS : 0);
}

// ---- 2. the bounded wait -----------------------------------------------------------------------------------------------
// relaxed agent-scope load of a flag that other blocks publish
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// polls before a wait gives up
constexpr unsigned STACK_SPIN_LIMIT = 1u << 22;  // task-queue dependency waits, s_sleep(8) per poll: ~1 s
constexpr unsigned SPLIT_SPIN_LIMIT = 1u << 20;  // row-split kernels (small batches), ~1 us per poll (agent-scope loads + s_sleep(1)): ~1-2 s

// ONE lane waits until all three flags reach `want` (three independent loads per poll, s_sleep(SLEEP) between polls) and returns `ok`;
// `fence`: one agent-scope acquire behind the wait (false: the caller reads what other blocks wrote with agent-scope loads).  Returns
// `gave_up` after LIMIT polls or because another block gave up: RAISE sets the abort flag and the caller's error word, which fails the
// launch; RAISE = false only leaves (blocks whose work nobody waits for).  The result is a value of the caller's (the next task number,
// an LDS word) and not a bool: the compiled loop is then the one the kernels had open-coded -- a bool return, an early return or a
// callback each moved loads and spill counts of the kernels around it.
template <int SLEEP, unsigned LIMIT, bool RAISE = true>
__device__ __forceinline__ int stack_wait(const int *f0, const int *f1, const int *f2, int want, int *abort_flag, int *err_flag, bool fence,
                                          int ok, int gave_up) {
    unsigned spins = 0;
    for (;;) {
        const int v0 = ld_agent(f0), v1 = ld_agent(f1), v2 = ld_agent(f2);
        if (min(v0, min(v1, v2)) >= want) break;
        __builtin_amdgcn_s_sleep(SLEEP);
        if (++spins > LIMIT || ld_agent(abort_flag) != 0) {
            if (RAISE) {
                __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (err_flag) __hip_atomic_store(err_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            ok = gave_up;
            break;
        }
    }
    if (fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return ok;
}
// the three settings in use.  Task queues: the producer tiles i-1, i, i+1 of the layer below
__device__ __forceinline__ int stack_wait_tiles(const int *f0, const int *f1, const int *f2, int want, int *abort_flag, int *err_flag, int ok = 1,
                                                int gave_up = 0) {
    return stack_wait<8, STACK_SPIN_LIMIT>(f0, f1, f2, want, abort_flag, err_flag, true, ok, gave_up);
}
// row-split kernels: the parts of the neighbouring tiles / of this tile (short polls: the wait is on the critical path of every layer)
__device__ __forceinline__ int stack_wait_parts(const int *f0, const int *f1, const int *f2, int want, int *abort_flag, int *err_flag, bool fence) {
    return stack_wait<1, SPLIT_SPIN_LIMIT>(f0, f1, f2, want, abort_flag, err_flag, fence, 1, 0);
}
// L2 warmers of the row-split fp16 kernel: paced by one tile's counter; nobody waits for them, so they give up without raising anything
__device__ __forceinline__ bool stack_wait_pace(const int *f, int want, int *abort_flag) {
    return stack_wait<8, SPLIT_SPIN_LIMIT, false>(f, f, f, want, abort_flag, nullptr, false, 1, 0) != 0;
}

// ---- 3. publish tile i of layer l (ONE lane, behind the vmcnt drain of every storing wave) ----------------------------
// Test hook SET_AMD_FAULT_TILE: that tile of layer 0 is never published, so its consumers must run into the spin limit and the launch
// must report it.  `hook` = false: this publish is not part of the hook (the direct fp32 kernel has none; one part's `ready` add
// withholds a tile of the row-split kernels).
constexpr int STACK_NO_FAULT_TILE = -1;
static inline int stack_fault_tile() {
    const char *e = getenv("SET_AMD_FAULT_TILE");
    return e ? atoi(e) : STACK_NO_FAULT_TILE;
}
// block-wide form: the flag holds the layers done
__device__ __forceinline__ void stack_publish_store(int *flags, int i, int l, int fault_tile, bool hook = true) {
    if (!(l == 0 && i == fault_tile && hook)) __hip_atomic_store(flags + i, l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// counting form: every part (row-split kernels: 4 blocks) or wave (x3v: X3V_FLAG_UNIT) of the tile adds one
__device__ __forceinline__ void stack_publish_add(int *flags, int i, int l, int fault_tile, bool hook = true) {
    if (!(l == 0 && i == fault_tile && hook)) (void)__hip_atomic_fetch_add(flags + i, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 4. workers of a task queue ----------------------------------------------------------------------------------------
// A task (l, i) needs tiles i-1 .. i+1 of layer l-1, so at most `ntiles` tasks are ever runnable and workers beyond ~0.8 ntiles mostly
// wait (`cap_4_5`); never fewer than min(floor, ntiles).  SET_AMD_STACK_GRID overrides; at most one worker per task, at least one.
static inline int stack_grid(int workers, int ntiles, int64_t ntasks, bool cap_4_5, int floor) {
    int grid = workers;
    if (cap_4_5 && grid > ntiles * 4 / 5) grid = ntiles * 4 / 5;
    if (grid < floor) grid = floor < ntiles ? floor : ntiles;
    if (const char *e = getenv("SET_AMD_STACK_GRID")) grid = atoi(e) > 0 ? atoi(e) : grid;
    if ((int64_t)grid > ntasks) grid = (int)ntasks;
    return grid < 1 ? 1 : grid;
}

// ---- 5. tile fill of task (l, i) -------------------------------------------------------------------------------------
// X3Tile (diffnet_x3.hip) of the split-operand queue kernels: tile i = `ncb` 32-frame column blocks of the batch's block list; `nimg` =
// 16-bit words of one layer's image
template <typename Tile>
__device__ __forceinline__ void stack_fill_x3_tile(Tile &lt, const SetDiffnetStackArgs &a, int l, int i, int ncb, int dil, int64_t nimg) {
    lt.xin = (l & 1) ? a.xb : a.xa;
    lt.xout = (l & 1) ? a.xa : a.xb;
    lt.skp = a.skip;
    lt.cp = a.condproj + (int64_t)l * a.cp_ls; lt.cp_bs = a.cp_bs;
    lt.dstep = a.dstep + (int64_t)l * a.d_ls; lt.d_bs = a.d_bs; lt.d_cs = a.d_cs;
    lt.img = reinterpret_cast<const unsigned short *>(a.wx3_all) + (int64_t)l * nimg;
    lt.b_dil = a.b_dil_all + (int64_t)l * 512;
    lt.b_out = a.b_out_all + (int64_t)l * 512;
    lt.err_flag = a.err_flag;
    lt.T = a.T; lt.dil = dil; lt.first = (l == 0);
    lt.nbu = (a.T + 31) / 32; lt.Q = a.B * lt.nbu; lt.q0 = i * ncb;
}
