// bf16-operand path of the training rows (BASELINE configs[1] "1xMI355X bf16"; the reference's AMP hooks are
// utils/commons/trainer.py:6,110,325,343-346 -- torch.autocast around the forward, fp32 master weights).
//
// What is bf16 here: the A / B fragments of the MFMA (v_mfma_f32_32x32x16_bf16, 16x the rate of the f32-input MFMA).
// Everything else stays fp32: activations and gradients in HBM, accumulation, bias / activation / residual epilogues,
// master weights and optimizer state.  Activations are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) on their way into LDS,
// weights once per optimizer step into a packed bf16 image.  At these shapes the GEMMs stop being the bound: the
// kernels below are sized to run near the rate at which their fp32 operands can be streamed from HBM / L2.
//
//   conv1d_bf16_kernel       forward conv and (with transposed weight addressing + negated dilation) input gradient
//   conv1d_wgrad_bf16_kernel weight gradient, reduction over frames, per-slice partial sums (no atomics)
//   wgrad_reduce_kernel      dW += sum over slices, in slice order  ->  run-to-run bit-stable gradients
//
// MFMA operand maps (32x32x16, cdna_hip_programming.md section 3): lane l holds A[i = l & 31][k = 8*(l>>5) .. +7] and
// B[k = 8*(l>>5) .. +7][j = l & 31] as 8 consecutive bf16 (one 16-byte LDS read); C/D as the f32 32x32 MFMA.  A and B use
// the SAME lane -> k map, so the contraction is right for any permutation of k the hardware applies inside an instruction.
#include <stdlib.h>

#include "weight_image.h"
#include "phase_probe.h"


namespace {

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// ---- epilogue (fp32) of the bf16 conv kernels: v = act((acc + bias) * alpha) + res ; * mask ; (+ previous output, / out_div) ----
// acc[i][j]: rows r0 + wm*64 + i*32 .., frames t0 + wn*64 + j*32 ..
template <int WM, int WN>
__device__ __forceinline__ void conv_bf16_epilogue(const SetConv1dArgs &a, const f32x16 (&acc)[2][2], int b, int t0, int r0, int wm, int wn,
                                                   int half, int l31) {
    // every optional operand is fetched as one batch of 16 on clamped addresses under ONE wave-uniform test, and the
    // activation code is resolved once per kernel (cheap ones as template instances, the transcendental ones in a
    // rolled loop): a per-element `if (ptr) v += ptr[i]` / `switch (act)` costs a branch (and a drained vmcnt) per element
    const bool has_div = a.accumulate && a.out_div != 0.0f;
    const bool has_res = a.res != nullptr, has_bias = a.bias != nullptr, has_acc = a.accumulate != 0;
    const rsrc_t d_out = make_rsrc(a.out + (int64_t)b * a.out_bs);
    const rsrc_t d_res = make_rsrc(has_res ? a.res + (int64_t)b * a.res_bs : a.out + (int64_t)b * a.out_bs);
    const rsrc_t d_bias = make_rsrc(has_bias ? a.bias : a.out);
    const bool has_mask = a.mask != nullptr;
    const rsrc_t d_mask = make_rsrc(has_mask ? a.mask + (int64_t)b * a.T_out : a.out);
    auto tile = [&](auto ACT, const f32x16 &av, int i, int j) __attribute__((always_inline)) {
        constexpr int kAct = decltype(ACT)::value;
        const int rbase = r0 + wm * 64 + i * 32 + 4 * half;  // register r of this lane is row rbase + (r&3) + 8*(r>>2)
        const int t = t0 + wn * 64 + j * 32 + l31;
        const bool tv = t < a.T_iter && t < a.T_out;
        const int tc = min(t, a.T_out - 1);
        float mk = 1.0f;
        if (has_mask) mk = buf_load(d_mask, (unsigned)tc * 4u, 0u);
        float bi[16], rv[16], ov[16];
        unsigned ro[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ro[r] = (unsigned)min(rbase + (r & 3) + 8 * (r >> 2), a.Cout - 1);
            bi[r] = rv[r] = ov[r] = 0.0f;
        }
        if (has_bias) {
#pragma unroll
            for (int r = 0; r < 16; ++r) bi[r] = buf_load(d_bias, ro[r] * 4u, 0u);
        }
        if (has_res) {
#pragma unroll
            for (int r = 0; r < 16; ++r) rv[r] = buf_load(d_res, (ro[r] * (unsigned)a.res_cs + (unsigned)tc) * 4u, 0u);
        }
        if (has_acc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) ov[r] = buf_load(d_out, (ro[r] * (unsigned)a.out_cs + (unsigned)tc) * 4u, 0u);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rbase + (r & 3) + 8 * (r >> 2);
            float y = (av[r] + bi[r]) * a.alpha;
            if constexpr (kAct == SET_ACT_RELU) y = y > 0.0f ? y : 0.0f;
            else if constexpr (kAct == SET_ACT_LRELU) y = y > 0.0f ? y : y * a.act_param;
            else if constexpr (kAct != SET_ACT_NONE) y = dev_act(y, a.act, a.act_param);
            y = (y + rv[r]) * mk + ov[r];
            if (has_div) y = y / a.out_div;
            // no branch around the store: a lane outside the tensor stores at an offset beyond the descriptor's range, which the buffer
            // unit drops.  (`if (valid) store` made every element its own exec-masked block, and the wait-count pass -- which cannot
            // know whether the previous block ran -- put s_waitcnt vmcnt(0) in each: 64 stores per lane, each waiting for the one before.)
            buf_store(y, d_out, (tv && row < a.Cout) ? (ro[r] * (unsigned)a.out_cs + (unsigned)tc) * 4u : BUF_OOB, 0u);
        }
    };
    auto finish = [&](auto ACT) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (r0 + wm * 64 + i * 32 >= a.Cout) continue;  // wave-uniform: a fully padded row block
#pragma unroll
            for (int j = 0; j < 2; ++j) tile(ACT, acc[i][j], i, j);
        }
    };
    switch (a.act) {
        case SET_ACT_NONE: finish(ic<SET_ACT_NONE>{}); break;
        case SET_ACT_RELU: finish(ic<SET_ACT_RELU>{}); break;
        case SET_ACT_LRELU: finish(ic<SET_ACT_LRELU>{}); break;
        default: finish(ic<-1>{}); break;  // gelu / tanh / softplus / mish: run-time dev_act (small layers only)
    }
}

// =====================================================================================================================
// conv1d, bf16 operands.  Block = 4 waves arranged WM x WN, wave tile 64 rows x 64 frames (2 x 2 accumulators of
// 32x32), block tile MB = 64*WM rows x NB = 64*WN frames.  One pipeline stage = KCH input channels x TG taps:
//   As[tl][row][KCH]  bf16, the weight rows of the block for tap tg0+tl          (copied from the packed image)
//   Bs[frame][KCH]    bf16, NB + halo frames of the input, prologue applied, rounded once per chunk of channels
// rows padded by 16 bytes: a 16-byte fragment read of 16 consecutive rows then hits 64 distinct banks.
// The loads of stage s+1 are issued (into registers) before the MFMAs of stage s; two barriers per stage.
// =====================================================================================================================
// Two shapes of stage: KCH = 32 with up to TGM = 4 taps (A tile <= 4 * 128 * 80 B = 40 KiB; every K, per-channel add
// supported) and KCH = 64 with one tap for the 1x1 convs (twice the MFMAs per pair of barriers; no halo rows, no
// per-channel add -- the staging registers of a 64-channel stage leave no room for them).
// VEC (round 6): the input tile is loaded in 16-byte units (4 frames of one channel; a thread owns 4 frames x 4 channels per unit = 4
// loads, four 8-byte LDS writes) instead of one frame per load (NPASS * KCH / 2 four-byte loads per thread and chunk): the same values
// in the same LDS cells.  Host: T_in, the strides and Cin multiples of 4, 16-byte aligned bases, halo <= 16 (launch_conv_bf16).
// probe builds (tools/build_exp.sh convprobe bf16.hip -DSET_PHASE_PROBE=1; tools/conv_phase_probe.py): wave 0 of block (1, 1, 1) of
// conv1d_bf16_kernel sums the s_memtime ticks of its per-stage phases and adds them to buf[0..5] (0 prologue, 1 barrier 1, 2 wait for the
// stage's loads + LDS writes, 3 barrier 2, 4 issue of the next stage's loads, 5 fragment reads + MFMAs), the stage count to buf[6]
SET_PHASE_PROBE_BUFFER(g_conv_phase_buf, set_debug_conv_phase_buffer)
template <int WM, int WN, int KCH, int TGM, bool HALO, bool ADD, bool VEC = false>
__global__ void __launch_bounds__(256, 2) conv1d_bf16_kernel(SetConv1dArgs a, int lo, int halo, int CinP, int CoutP) {
    PhaseProbe<7> pp;
    pp.start(g_conv_phase_buf && blockIdx.x == 1 && blockIdx.y == 1 && blockIdx.z == 1);
    static_assert(!VEC || KCH == 32, "16-byte input units: 32-channel stages");
    constexpr int BF_TG_MAX = TGM;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int MB = 64 * WM, NB = 64 * WN;
    constexpr int ROWB = KCH * 2 + 16;              // bytes per LDS row
    constexpr int CPT = KCH / 2;                    // channels per thread per staging pass (2 channel groups)
    constexpr int NPASS = NB / 128 + (HALO ? 1 : 0);  // frame passes of 128 rows (last one = halo rows)
    constexpr int AU_MAX = BF_TG_MAX * (KCH / 32) * MB * 4 / 256;  // 16-byte units of the A tile per thread
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z, t0 = blockIdx.x * NB, r0 = blockIdx.y * MB;
    const int R = NB + halo;                        // frame rows of the B tile
    unsigned char *As = smem_raw;                                   // [TG][MB][ROWB]
    unsigned char *Bs = smem_raw + BF_TG_MAX * MB * ROWB;           // [R][ROWB]
    const unsigned short *wimg = reinterpret_cast<const unsigned short *>(a.w);
    const float *inb = a.in + (int64_t)b * a.in_bs;
    const bool has_add = ADD && a.in_chan_add != nullptr;
    const float *addp = has_add ? a.in_chan_add + (int64_t)b * a.Cin : inb;  // dummy stays a valid address
    const int nchunk32 = CinP / 32;
    const int nchunks = (CinP + KCH - 1) / KCH;
    const int ngroups = (a.K + BF_TG_MAX - 1) / BF_TG_MAX;
    const int nstages = nchunks * ngroups;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};

    // ---- staging registers (one stage ahead) ----
    float pv[NPASS][CPT], pa[ADD ? CPT : 1];  // (dead under VEC)
    u32x4_t au[AU_MAX];
    // VEC: unit u = tid + 256 j -> frame quad u >> 3 (frames F0 + 4 (u >> 3) .., F0 = t0 + lo rounded down to a multiple of 4), channel
    // quad u & 7 of the 32-channel chunk; NQ quads cover the R rows of the tile
    constexpr int VQMAX = (64 * WN + 16 + 3) / 4 + 1, VJ = (VQMAX * 8 + 255) / 256;
    f32x4 vx[VEC ? VJ : 1][VEC ? 4 : 1], va[(VEC && ADD) ? VJ : 1];
    const int vF0 = (t0 + lo) & ~3, vsh = (t0 + lo) - vF0, vNQ = (R + vsh + 3) >> 2;
    const int sf = tid & 127, scg = tid >> 7;  // B staging: frame row sf (+128*pass), channel group scg

    // raw-buffer addressing (common.h): one VGPR byte offset per frame pass + a scalar byte offset per channel (the
    // thread's channel group is wave-uniform: waves 0,1 -> group 0, waves 2,3 -> group 1)
    const rsrc_t d_in = make_rsrc(inb);
    const rsrc_t d_add = make_rsrc(addp);
    const int scg_u = __builtin_amdgcn_readfirstlane(scg);
    auto issue_b = [&](int c0) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < VJ; ++j) {
                const int u = tid + 256 * j, q = min(u >> 3, vNQ - 1), cq = u & 7;
                const unsigned vo = (unsigned)min(max(vF0 + 4 * q, 0), a.T_in - 4) * 4u;
                const int cc = min(c0 + 4 * cq, a.Cin - 4);
                if constexpr (ADD) va[j] = buf_load4(d_add, (unsigned)cc * 4u, 0u);
#pragma unroll
                for (int i = 0; i < 4; ++i) vx[j][i] = buf_load4(d_in, vo + (unsigned)((cc + i) * (int)a.in_cs) * 4u, 0u);
            }
            return;
        }
        if constexpr (ADD) {
#pragma unroll
            for (int k = 0; k < CPT; ++k) pa[k] = buf_load(d_add, 0u, (unsigned)min(c0 + scg_u * CPT + k, a.Cin - 1) * 4u);
        }
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int ti = t0 + lo + p * 128 + sf;
            const unsigned vo = (unsigned)min(max(ti, 0), a.T_in - 1) * 4u;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int cc = min(c0 + scg_u * CPT + k, a.Cin - 1);
                pv[p][k] = buf_load(d_in, vo, (unsigned)(cc * (int)a.in_cs) * 4u);
            }
        }
    };
    auto commit_b = [&](auto PROC, int c0) __attribute__((always_inline)) {
        constexpr int kPro = decltype(PROC)::value;
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < VJ; ++j) {
                const int u = tid + 256 * j, q = u >> 3, cq = u & 7;
                const int f = vF0 + 4 * q;  // T_in % 4 == 0: the quad is entirely inside or outside; Cin % 4 == 0: so is the channel quad
                const bool ok = q < vNQ && f >= 0 && f < a.T_in && c0 + 4 * cq < a.Cin;
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // frame f + e -> tile row 4 q + e - vsh
                    float x[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v = vx[j][i][e];
                        if constexpr (ADD) v = has_add ? v + va[j][i] : v;
                        v = pro_c<kPro>(v, a.pro_param);
                        x[i] = ok ? v : 0.0f;
                    }
                    // (no branch around the write: rows outside the tile go to a spare row behind it -- twelve exec-masked blocks, each with its
                    // own wait, made the commit phase a third of a stage, profiles/r06_conv_phase_probe.log)
                    const int row = 4 * q + e - vsh;
                    const int rw = (q < vNQ && row >= 0 && row < R) ? row : R;
                    u32x2_t w;
                    w[0] = pack_bf16(x[0], x[1]); w[1] = pack_bf16(x[2], x[3]);
                    *reinterpret_cast<u32x2_t *>(Bs + rw * ROWB + cq * 8) = w;
                }
            }
            return;
        }
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int row = p * 128 + sf;
            const int ti = t0 + lo + row;
            const bool tv = ti >= 0 && ti < a.T_in;
            float x[CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                float v = pv[p][k];
                if constexpr (ADD) v = has_add ? v + pa[k] : v;
                v = pro_c<kPro>(v, a.pro_param);                          // unconditional, straight-line
                x[k] = (tv && c0 + scg_u * CPT + k < a.Cin) ? v : 0.0f;   // select, no branch
            }
            if (row < R) {
#pragma unroll
                for (int q = 0; q < CPT / 8; ++q) {
                    u32x4_t u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) u[e] = pack_bf16(x[8 * q + 2 * e], x[8 * q + 2 * e + 1]);
                    *reinterpret_cast<u32x4_t *>(Bs + row * ROWB + (scg * CPT + 8 * q) * 2) = u;
                }
            }
        }
    };
    // A tile of stage (chunk c0, taps tg0 .. tg0+tgn-1): unit u -> (tap tl, 32-channel sub-chunk h, row, 16-byte part)
    auto issue_a = [&](int c0, int tg0, int tgn) {
        const int units = tgn * (KCH / 32) * MB * 4;
#pragma unroll
        for (int q = 0; q < AU_MAX; ++q) {
            int u = tid + 256 * q;
            u = u < units ? u : 0;  // clamped duplicate load; not committed
            const int part = u & 3, row = (u >> 2) % MB, h = ((u >> 2) / MB) % (KCH / 32), tl = (u >> 2) / (MB * (KCH / 32));
            const int ch32 = min(c0 / 32 + h, nchunk32 - 1);
            const int64_t e = ((((int64_t)(tg0 + tl) * nchunk32 + ch32) * CoutP + r0 + row) * 32 + part * 8);
            au[q] = *reinterpret_cast<const u32x4_t *>(wimg + e);
        }
    };
    auto commit_a = [&](int c0, int tgn) {
        const int units = tgn * (KCH / 32) * MB * 4;
#pragma unroll
        for (int q = 0; q < AU_MAX; ++q) {
            const int u = tid + 256 * q;
            if (u < units) {
                const int part = u & 3, row = (u >> 2) % MB, h = ((u >> 2) / MB) % (KCH / 32), tl = (u >> 2) / (MB * (KCH / 32));
                u32x4_t v = au[q];
                if (c0 + 32 * h >= CinP) v = (u32x4_t){0u, 0u, 0u, 0u};  // KCH = 64 over an odd number of 32-channel chunks
                *reinterpret_cast<u32x4_t *>(As + (tl * MB + row) * ROWB + h * 64 + part * 16) = v;
            }
        }
    };
    auto stage_of = [&](int s, int &c0, int &tg0, int &tgn) {
        const int ch = s / ngroups, g = s % ngroups;
        c0 = ch * KCH;
        tg0 = g * BF_TG_MAX;
        tgn = min(BF_TG_MAX, a.K - tg0);
    };

    int c0, tg0, tgn;
    stage_of(0, c0, tg0, tgn);
    issue_b(c0);
    issue_a(c0, tg0, tgn);
    pp.lap(0);  // prologue: first loads issued
    for (int s = 0; s < nstages; ++s) {
        stage_of(s, c0, tg0, tgn);
        __syncthreads();  // MFMAs of the previous stage are done with the tiles
        pp.lap(1);  // barrier 1
        if (tg0 == 0) {
            switch (a.pro) {
                case SET_PRO_LRELU: commit_b(ic<SET_PRO_LRELU>{}, c0); break;
                case SET_PRO_DIV: commit_b(ic<SET_PRO_DIV>{}, c0); break;
                default: commit_b(ic<SET_PRO_NONE>{}, c0); break;
            }
        }
        commit_a(c0, tgn);
        pp.lap(2);  // wait for the stage's loads + LDS writes
        __syncthreads();
        pp.lap(3);  // barrier 2
        auto mfma_tap = [&](int tl) {
            const int off = (tg0 + tl) * a.dil - a.pad - lo;  // >= 0: frame-row shift of this tap inside the B tile
            const unsigned char *ap = As + (tl * MB + wm * 64 + l31) * ROWB + half * 16;
            const unsigned char *bp = Bs + (wn * 64 + l31 + off) * ROWB + half * 16;
#pragma unroll
            for (int ks = 0; ks < KCH / 16; ++ks) {
                const u32x4_t a0 = *reinterpret_cast<const u32x4_t *>(ap + ks * 32);
                const u32x4_t a1 = *reinterpret_cast<const u32x4_t *>(ap + 32 * ROWB + ks * 32);
                const u32x4_t b0 = *reinterpret_cast<const u32x4_t *>(bp + ks * 32);
                const u32x4_t b1 = *reinterpret_cast<const u32x4_t *>(bp + 32 * ROWB + ks * 32);
                acc[0][0] = mfma_bf16(a0, b0, acc[0][0]);
                acc[0][1] = mfma_bf16(a0, b1, acc[0][1]);
                acc[1][0] = mfma_bf16(a1, b0, acc[1][0]);
                acc[1][1] = mfma_bf16(a1, b1, acc[1][1]);
            }
        };
        if (s + 1 < nstages) {
            int c1, tg1, tgn1;
            stage_of(s + 1, c1, tg1, tgn1);
            if (tg1 == 0) issue_b(c1);
            issue_a(c1, tg1, tgn1);
        }
        pp.lap(4);  // issue of the next stage's loads
        // (rolled: unrolled over the taps of a stage it ran 8 - 16 % slower, profiles/r06_conv_unroll_ab.log; the next stage's loads issued in
        // slices between the taps' MFMA groups instead of one burst behind the barrier: 5 - 10 % slower, profiles/r06_conv_sliced_issue_ab.log)
        for (int tl = 0; tl < tgn; ++tl) mfma_tap(tl);
        pp.lap(5);  // fragment reads + MFMAs of the stage
    }

    pp.lap(5);  // (the last stage's MFMAs land here; per stage they are accounted below)
    pp.count(6, (uint32_t)nstages);
    pp.flush(g_conv_phase_buf);
    conv_bf16_epilogue<WM, WN>(a, acc, b, t0, r0, wm, wn, half, l31);
}

// ---- 1x1 conv, the input tile in one round trip per 256 input channels ----------------------------------------------------------------
// The 1x1 convs of the FFT / transformer blocks (attention projections, 192 or 256 channels, 12,800 - 25,600 frames) are ~200 blocks of
// a few MFMAs each: in the staged kernel above a block walks Cin / 64 stages of load -> convert -> barrier -> 16 MFMAs -> barrier with
// one stage of loads in flight, i.e. it spends its life in 3 - 4 dependent memory round trips (22 - 31 us per conv against 4 - 10 us of
// HBM time, tools/small_conv_probe.py).  Here every thread issues ALL its input loads at once (Cin / 2 dwords: frame tid & 127, channel
// half tid >> 7), the tile [128 frames][Cin] goes to LDS in one pass, and the GEMM runs over the whole K with the weight fragments
// straight from the packed image (L2-resident, ring of 4 k-steps): one input round trip, one barrier.
template <int CINP>
__global__ void __launch_bounds__(256, 2) conv1x1_oneshot_bf16_kernel(SetConv1dArgs a, int CoutP, int nchunk32) {
    constexpr int WM = 2, WN = 2, NB = 128;
    constexpr int ROWB = CINP * 2 + 16;  // bytes per frame row of the tile
    constexpr int CPT = CINP / 2;        // channels per thread (of one chunk of CINP channels)
    constexpr int NKS = CINP / 16;       // k-steps per chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char *Bs = smem_raw;        // [128][ROWB]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z, t0 = blockIdx.x * NB, r0 = blockIdx.y * 128;
    const unsigned short *wimg = reinterpret_cast<const unsigned short *>(a.w);
    const rsrc_t d_in = make_rsrc(a.in + (int64_t)b * a.in_bs);
    const int sf = tid & 127, scg = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int nchunks = (a.Cin + CINP - 1) / CINP;  // 1 for Cin <= CINP; wider inputs: chunks of CINP channels, one round trip each
    const unsigned vo = (unsigned)min(t0 + sf, a.T_in - 1) * 4u;
    const bool tv = t0 + sf < a.T_in;

    float pv[CPT];
    auto issue = [&](int c0) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) pv[k] = buf_load(d_in, vo, (unsigned)(min(c0 + scg * CPT + k, a.Cin - 1) * (int)a.in_cs) * 4u);
    };
    // weight fragments: lane (row l31 of row block i, k-half `half`) of k-step ks (counted over the whole K) reads 16 bytes of
    // wp[chunk ks / 2][row][32]   (k-steps beyond the image's last 32-channel chunk re-read it: their B rows are zero)
    const rsrc_t d_w = make_rsrc(wimg);
    auto a_off = [&](int ks, int i) {
        return (unsigned)(((min(ks >> 1, nchunk32 - 1) * CoutP + r0 + wm * 64 + i * 32 + l31) * 32 + (ks & 1) * 16 + half * 8) * 2);
    };
    constexpr int RING = NKS < 4 ? NKS : 4;
    u32x4_t A[RING][2];
    auto commit = [&](auto PROC, int c0) __attribute__((always_inline)) {
        constexpr int kPro = decltype(PROC)::value;
#pragma unroll
        for (int q = 0; q < CPT / 8; ++q) {
            u32x4_t u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v0 = pro_c<kPro>(pv[8 * q + 2 * e], a.pro_param), v1 = pro_c<kPro>(pv[8 * q + 2 * e + 1], a.pro_param);
                v0 = (tv && c0 + scg * CPT + 8 * q + 2 * e < a.Cin) ? v0 : 0.0f;
                v1 = (tv && c0 + scg * CPT + 8 * q + 2 * e + 1 < a.Cin) ? v1 : 0.0f;
                u[e] = pack_bf16(v0, v1);
            }
            *reinterpret_cast<u32x4_t *>(Bs + sf * ROWB + (scg * CPT + 8 * q) * 2) = u;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};
    const unsigned char *bp = Bs + (wn * 64 + l31) * ROWB + half * 16;
    issue(0);
    for (int c = 0; c < nchunks; ++c) {
        const int c0 = c * CINP, ks0 = c * NKS;
#pragma unroll
        for (int q = 0; q < RING; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i) A[q][i] = __builtin_amdgcn_raw_buffer_load_b128(d_w, (int)a_off(ks0 + q, i), 0, 0);
        if (c > 0) __syncthreads();  // the MFMAs of the previous chunk are done with the tile
        switch (a.pro) {
            case SET_PRO_LRELU: commit(ic<SET_PRO_LRELU>{}, c0); break;
            case SET_PRO_DIV: commit(ic<SET_PRO_DIV>{}, c0); break;
            default: commit(ic<SET_PRO_NONE>{}, c0); break;
        }
        __syncthreads();
        if (c + 1 < nchunks) issue(c0 + CINP);  // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {  // pinned k-step order (round 4): B reads | MFMAs straight from the ring slot | refill of that slot
            const u32x4_t b0 = *reinterpret_cast<const u32x4_t *>(bp + ks * 32);
            const u32x4_t b1 = *reinterpret_cast<const u32x4_t *>(bp + 32 * ROWB + ks * 32);
            acc[0][0] = mfma_bf16(A[ks % RING][0], b0, acc[0][0]);
            acc[0][1] = mfma_bf16(A[ks % RING][0], b1, acc[0][1]);
            acc[1][0] = mfma_bf16(A[ks % RING][1], b0, acc[1][0]);
            acc[1][1] = mfma_bf16(A[ks % RING][1], b1, acc[1][1]);
            if (ks + RING < NKS) {
#pragma unroll
                for (int i = 0; i < 2; ++i) A[ks % RING][i] = __builtin_amdgcn_raw_buffer_load_b128(d_w, (int)a_off(ks0 + ks + RING, i), 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    conv_bf16_epilogue<WM, WN>(a, acc, b, t0, r0, wm, wn, half, l31);
}

template <int CINP>
static int launch_conv1x1_oneshot(const SetConv1dArgs &a, hipStream_t s) {
    const int CoutP = set_round_up(a.Cout, BF16_IMG_ROWS);
    const size_t lds = (size_t)128 * (CINP * 2 + 16);
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, 96 * 1024, "conv 1x1 attr", conv1x1_oneshot_bf16_kernel<CINP>)) return rc;
    dim3 grid((a.T_iter + 127) / 128, (a.Cout + 127) / 128, a.B), block(256);
    hipLaunchKernelGGL((conv1x1_oneshot_bf16_kernel<CINP>), grid, block, lds, s, a, CoutP, set_round_up(a.Cin, BF16_IMG_CH) / 32);
    return set_check_launch("set_conv1d(bf16, 1x1)");
}

template <int WM, int WN, int KCH, int TGM, bool HALO, bool ADD, bool VEC = false>
static int launch_conv_bf16(const SetConv1dArgs &a, int lo, int halo, hipStream_t s) {
    if constexpr (KCH == 32 && !VEC) {  // 16-byte input units where the layout allows (SET_AMD_CONV_BF16_UNITS=0: one frame per load)
        const bool env = !(getenv("SET_AMD_CONV_BF16_UNITS") && atoi(getenv("SET_AMD_CONV_BF16_UNITS")) == 0);
        const bool al = ((uintptr_t)a.in & 15) == 0 && a.T_in % 4 == 0 && a.T_in >= 4 && a.in_cs % 4 == 0 && a.in_bs % 4 == 0 && a.Cin % 4 == 0 &&
                        (!a.in_chan_add || ((uintptr_t)a.in_chan_add & 15) == 0);
        if (env && al && halo <= 16) return launch_conv_bf16<WM, WN, KCH, TGM, HALO, ADD, true>(a, lo, halo, s);
    }
    constexpr int MB = 64 * WM, NB = 64 * WN, ROWB = KCH * 2 + 16, BF_TG_MAX = TGM;
    const int CinP = set_round_up(a.Cin, BF16_IMG_CH), CoutP = set_round_up(a.Cout, BF16_IMG_ROWS);
    const size_t lds = (size_t)BF_TG_MAX * MB * ROWB + (size_t)(NB + halo + (VEC ? 1 : 0)) * ROWB;  // (VEC: one spare row for the masked-out writes)
    static SetDeviceOnce lds_once;  // (96 KiB: two blocks per CU)
    if (int rc = set_lds_optin(lds_once, 96 * 1024, "conv bf16 attr", conv1d_bf16_kernel<WM, WN, KCH, TGM, HALO, ADD, VEC>)) return rc;
    if (lds > 96 * 1024) return set_fail(SET_E_UNSUPPORTED, "set_conv1d(bf16)", "tile does not fit LDS");
    dim3 grid((a.T_iter + NB - 1) / NB, (a.Cout + MB - 1) / MB, a.B), block(256);
    hipLaunchKernelGGL((conv1d_bf16_kernel<WM, WN, KCH, TGM, HALO, ADD, VEC>), grid, block, lds, s, a, lo, halo, CinP, CoutP);
    return set_check_launch("set_conv1d(bf16)");
}

// =====================================================================================================================
// weight gradient, bf16 operands:  dW[co][ci][tap] = sum_{b,t} G[b][co][t] * P(X[b][ci][t + tap*dil - pad])
// GEMM M = Cout (128 per block), N = Cin (128 per block) for ONE tap, reduction over frames in chunks of 64:
//   Gs[co][64 frames], Xs[ci][64 frames] bf16, rows padded to 144 bytes (conflict-free 16-byte fragment reads);
//   the chunk loads of step c+1 are in flight (registers) under the MFMAs of step c.
// Frames are split into `S` slices (grid.z); slice z writes its partial tile to partial[z][Cout][Cin][K] with plain
// stores.  wgrad_reduce_kernel then adds the slices to dW in slice order: no atomics, the same bits every run.
// =====================================================================================================================
constexpr int WGB_KT = 64;
constexpr int WGB_ROWB = WGB_KT * 2 + 16;

struct WgradBf16Args {
    const void *g, *x;  // fp32 [B][C][T], or bf16 when the kernel is instantiated with GB16 / XB16
    const float *chan_add;
    float *partial;  // [S][Cout][Cin][K]
    int B, Cin, Cout, K, dil, pad, T, T_in, pro;
    float pro_param;
    int chunks_per_slice, n_chunks_t, ci_tiles;
    // grouped launch (the same GEMM shape for every residual layer of the DiffNet: grid.z = group * S + slice): byte strides of g
    // and x between groups, float stride of chan_add; S = slices per group.  One group: S = gridDim.z, strides 0.
    int S;
    int64_t g_gs, x_gs, add_gs;
};

__device__ __forceinline__ unsigned buf_load_raw(rsrc_t r, unsigned voff, unsigned soff) {
    return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ unsigned buf_load_raw16(rsrc_t r, unsigned voff, unsigned soff) {
    return (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, (int)voff, (int)soff, 0);
}

// A bf16 operand in HBM (GB16 / XB16, the tensors the fused DiffNet layer kernels hand over) is CHANNEL-QUAD INTERLEAVED: element (c, t) of a
// batch slice at byte ((c >> 2) T + t) 8 + (c & 3) 2 (diffnet_bf16.hip).  q4_row / q4_frame: scalar / per-lane parts of that offset.
__device__ __forceinline__ unsigned q4_row(int c, int T) { return (unsigned)((c >> 2) * T) * 8u + (unsigned)(c & 3) * 2u; }
// 8 frames x 4 channels (four 16-byte units of 2 frames x 4 channels, consecutive in memory) -> channel c's 8 frames as one 16-byte row piece
template <int N>
__device__ __forceinline__ u32x4_t q4_channel(const unsigned (&u)[N], int c) {
    u32x4_t o;
#pragma unroll
    for (int k = 0; k < 4; ++k)  // unit k: dwords {f0: c0 c1 | c2 c3, f1: c0 c1 | c2 c3}
        o[k] = __builtin_amdgcn_perm(u[4 * k + 2 + (c >> 1)], u[4 * k + (c >> 1)], (c & 1) ? 0x07060302u : 0x05040100u);
    return o;
}

// GB16 / XB16: the operand already is bf16 in HBM (saved activations / gradients of the fused layer kernels): its bits
// go to LDS unchanged (no prologue, no per-channel add on such an operand).
template <bool GB16, bool XB16, bool GU = false, bool XU = false>  // GU / XU: that operand is copied in 16-byte units (host: wgrad_units_ok)
__global__ void __launch_bounds__(256, 2) conv1d_wgrad_bf16_kernel(WgradBf16Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char Gs[128 * WGB_ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Xs[128 * WGB_ROWB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const int tap = blockIdx.x / a.ci_tiles, ci0 = (blockIdx.x % a.ci_tiles) * 128;
    const int co0 = blockIdx.y * 128;
    const int shift = tap * a.dil - a.pad;
    const int total_chunks = a.B * a.n_chunks_t;
    const int grp = blockIdx.z / a.S;
    const int c_begin = (blockIdx.z - grp * a.S) * a.chunks_per_slice;
    const int c_end = min(c_begin + a.chunks_per_slice, total_chunks);
    const bool has_add = !XB16 && a.chan_add != nullptr;
    a.g = reinterpret_cast<const unsigned char *>(a.g) + grp * a.g_gs;
    a.x = reinterpret_cast<const unsigned char *>(a.x) + grp * a.x_gs;
    if (has_add) a.chan_add += grp * a.add_gs;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};

    // staging: lane = frame inside the chunk, the thread's wave owns rows wave, wave + 4, ... (32 rows per tile).
    // raw-buffer addressing: per-lane byte offset of the frame + scalar byte offset of the row (wave-uniform)
    const int sk = lane, sr0 = wave;
    unsigned gv[32], xv[32];  // raw bits (fp32 or bf16): converting at issue time would wait for the load
    float av[XB16 ? 1 : 32];
    constexpr unsigned GE = GB16 ? 2u : 4u, XE = XB16 ? 2u : 4u;  // element sizes
    // Round 4: an operand that already is bf16 in HBM is copied in 16-byte units (8 consecutive frames of a row; unit (row, ucol) of the
    // 128 x 64 tile = thread tid + 256 q) when its rows are 16-byte aligned (T a multiple of 8; the conv input also needs shift = 0):
    // 4 loads + 4 LDS writes per thread and chunk instead of 32 + 32 two-byte ones -- these kernels issue 16 MFMAs per chunk and were
    // bound by the staging instructions.  Same bits in the same LDS cells as the element-wise path (which stays for ragged T).
    // The path is a template parameter, not a run-time test: with both paths in one kernel the wait-count pass drained the next chunk's loads
    // in front of the MFMAs at the join of the two branches.
    // An fp32 operand takes the same route in units of 4 frames (16 bytes; 8 units per thread, converted at the LDS write: one 8-byte write).
    constexpr bool fastg = GU, fastx = XU;
    const int urow = tid >> 3, ucol = tid & 7;      // bf16 units: 8 per row, 32 rows per pass
    const int urow4 = tid >> 4, ucol4 = tid & 15;   // fp32 units: 16 per row, 16 rows per pass
    auto issue = [&](int ch) {
        const int b = ch / a.n_chunks_t, t0 = (ch % a.n_chunks_t) * WGB_KT;
        const unsigned vg = (unsigned)min(t0 + sk, a.T - 1) * (GB16 ? 8u : 4u);  // (bf16: quad-interleaved, 8 bytes per frame of a channel quad)
        const unsigned vx = (unsigned)min(max(t0 + sk + shift, 0), a.T_in - 1) * (XB16 ? 8u : 4u);
        const rsrc_t d_g = make_rsrc(reinterpret_cast<const unsigned char *>(a.g) + (int64_t)b * a.Cout * a.T * GE);
        const rsrc_t d_x = make_rsrc(reinterpret_cast<const unsigned char *>(a.x) + (int64_t)b * a.Cin * a.T_in * XE);
        const rsrc_t d_a = make_rsrc(has_add ? a.chan_add + (int64_t)b * a.Cin : reinterpret_cast<const float *>(a.x));
        if constexpr (fastg && GB16) {  // thread = (channel quad urow, 8 frames ucol): four consecutive 16-byte units (2 frames x 4 channels each)
            const unsigned vo = (unsigned)(min((co0 >> 2) + urow, (a.Cout >> 2) - 1) * a.T + min(t0 + 8 * ucol, a.T - 8)) * 8u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4_t v = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_g, (int)(vo + 16u * q), 0, 0);
                gv[4 * q] = v[0]; gv[4 * q + 1] = v[1]; gv[4 * q + 2] = v[2]; gv[4 * q + 3] = v[3];
            }
        } else if constexpr (fastg) {  // fp32: 16 bytes = 4 frames
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned vo = (unsigned)(min(co0 + urow4 + 16 * q, a.Cout - 1) * a.T + min(t0 + 4 * ucol4, a.T - 4)) * 4u;
                const u32x4_t v = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_g, (int)vo, 0, 0);
                gv[4 * q] = v[0]; gv[4 * q + 1] = v[1]; gv[4 * q + 2] = v[2]; gv[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int gr = min(co0 + sr0 + 4 * j, a.Cout - 1);
                gv[j] = GB16 ? buf_load_raw16(d_g, vg, q4_row(gr, a.T)) : buf_load_raw(d_g, vg, (unsigned)(gr * a.T) * 4u);
            }
        }
        if constexpr (fastx && XB16) {
            const unsigned vo = (unsigned)(min((ci0 >> 2) + urow, (a.Cin >> 2) - 1) * a.T_in + min(t0 + 8 * ucol, a.T_in - 8)) * 8u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4_t v = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_x, (int)(vo + 16u * q), 0, 0);
                xv[4 * q] = v[0]; xv[4 * q + 1] = v[1]; xv[4 * q + 2] = v[2]; xv[4 * q + 3] = v[3];
            }
        } else if constexpr (fastx) {  // fp32: 16 bytes = 4 frames; the per-channel add of the unit's row rides along (dummy address without one)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int cic = min(ci0 + urow4 + 16 * q, a.Cin - 1);
                const unsigned vo = (unsigned)(cic * a.T_in + min(t0 + 4 * ucol4, a.T_in - 4)) * 4u;
                const u32x4_t v = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_x, (int)vo, 0, 0);
                xv[4 * q] = v[0]; xv[4 * q + 1] = v[1]; xv[4 * q + 2] = v[2]; xv[4 * q + 3] = v[3];
                av[q] = buf_load(d_a, (unsigned)cic * 4u, 0u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int cic = min(ci0 + sr0 + 4 * j, a.Cin - 1);
                xv[j] = XB16 ? buf_load_raw16(d_x, vx, q4_row(cic, a.T_in)) : buf_load_raw(d_x, vx, (unsigned)(cic * a.T_in) * 4u);
                if constexpr (!XB16) av[j] = buf_load(d_a, 0u, (unsigned)cic * 4u);
            }
        }
    };
    auto commit = [&](auto PROC, int ch) __attribute__((always_inline)) {
        constexpr int kPro = decltype(PROC)::value;
        const int t0 = (ch % a.n_chunks_t) * WGB_KT;
        const int t = t0 + sk, ti = t + shift;
        const bool tv = t < a.T, tiv = tv && ti >= 0 && ti < a.T_in;
        if constexpr (fastg && GB16) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {  // the 8 frames of channel 4 urow + c, cut out of the thread's 8 frames x 4 channels
                const int row = 4 * urow + c;
                const bool ok = t0 + 8 * ucol < a.T && co0 + row < a.Cout;  // T % 8 == 0, Cout % 4 == 0: entirely inside or outside
                const u32x4_t w = q4_channel(gv, c);
                u32x4_t v;
                v[0] = ok ? w[0] : 0u; v[1] = ok ? w[1] : 0u; v[2] = ok ? w[2] : 0u; v[3] = ok ? w[3] : 0u;
                *reinterpret_cast<u32x4_t *>(Gs + row * WGB_ROWB + ucol * 16) = v;
            }
        } else if constexpr (fastg) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int row = urow4 + 16 * q;
                const bool ok = t0 + 4 * ucol4 < a.T && co0 + row < a.Cout;  // T % 4 == 0
                unsigned short h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = f2bf(__builtin_bit_cast(float, gv[4 * q + e]));
                u32x2_t w;
                w[0] = ok ? ((unsigned)h[0] | ((unsigned)h[1] << 16)) : 0u;
                w[1] = ok ? ((unsigned)h[2] | ((unsigned)h[3] << 16)) : 0u;
                *reinterpret_cast<u32x2_t *>(Gs + row * WGB_ROWB + ucol4 * 8) = w;
            }
        }
        if constexpr (fastx && XB16) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int row = 4 * urow + c;
                const bool ok = t0 + 8 * ucol < a.T && t0 + 8 * ucol < a.T_in && ci0 + row < a.Cin;
                const u32x4_t w = q4_channel(xv, c);
                u32x4_t v;
                v[0] = ok ? w[0] : 0u; v[1] = ok ? w[1] : 0u; v[2] = ok ? w[2] : 0u; v[3] = ok ? w[3] : 0u;
                *reinterpret_cast<u32x4_t *>(Xs + row * WGB_ROWB + ucol * 16) = v;
            }
        } else if constexpr (fastx) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int row = urow4 + 16 * q;
                const bool ok = t0 + 4 * ucol4 < a.T && t0 + 4 * ucol4 < a.T_in && ci0 + row < a.Cin;
                unsigned short h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xf = __builtin_bit_cast(float, xv[4 * q + e]);
                    h[e] = f2bf(pro_c<kPro>(has_add ? xf + av[q] : xf, a.pro_param));  // same arithmetic as the element-wise path
                }
                u32x2_t w;
                w[0] = ok ? ((unsigned)h[0] | ((unsigned)h[1] << 16)) : 0u;
                w[1] = ok ? ((unsigned)h[2] | ((unsigned)h[3] << 16)) : 0u;
                *reinterpret_cast<u32x2_t *>(Xs + row * WGB_ROWB + ucol4 * 8) = w;
            }
        }
        if constexpr (!fastg || !fastx) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int row = sr0 + 4 * j;
                unsigned short gb, xb;
                if constexpr (GB16) gb = (unsigned short)gv[j];
                else gb = f2bf(__builtin_bit_cast(float, gv[j]));
                if constexpr (XB16) xb = (unsigned short)xv[j];
                else {
                    const float xf = __builtin_bit_cast(float, xv[j]);
                    xb = f2bf(pro_c<kPro>(has_add ? xf + av[j] : xf, a.pro_param));  // unconditional, then select
                }
                if constexpr (!fastg) *reinterpret_cast<unsigned short *>(Gs + row * WGB_ROWB + sk * 2) = (tv && co0 + row < a.Cout) ? gb : (unsigned short)0;
                if constexpr (!fastx) *reinterpret_cast<unsigned short *>(Xs + row * WGB_ROWB + sk * 2) = (tiv && ci0 + row < a.Cin) ? xb : (unsigned short)0;
            }
        }
    };
    if (c_begin < c_end) issue(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        __syncthreads();
        switch (a.pro) {
            case SET_PRO_LRELU: commit(ic<SET_PRO_LRELU>{}, ch); break;
            case SET_PRO_DIV: commit(ic<SET_PRO_DIV>{}, ch); break;
            default: commit(ic<SET_PRO_NONE>{}, ch); break;
        }
        __syncthreads();
        if (ch + 1 < c_end) issue(ch + 1);
        const unsigned char *ap = Gs + (wm * 64 + l31) * WGB_ROWB + half * 16;
        const unsigned char *bp = Xs + (wn * 64 + l31) * WGB_ROWB + half * 16;
#pragma unroll
        for (int ks = 0; ks < WGB_KT / 16; ++ks) {
            const u32x4_t a0 = *reinterpret_cast<const u32x4_t *>(ap + ks * 32);
            const u32x4_t a1 = *reinterpret_cast<const u32x4_t *>(ap + 32 * WGB_ROWB + ks * 32);
            const u32x4_t b0 = *reinterpret_cast<const u32x4_t *>(bp + ks * 32);
            const u32x4_t b1 = *reinterpret_cast<const u32x4_t *>(bp + 32 * WGB_ROWB + ks * 32);
            acc[0][0] = mfma_bf16(a0, b0, acc[0][0]);
            acc[0][1] = mfma_bf16(a0, b1, acc[0][1]);
            acc[1][0] = mfma_bf16(a1, b0, acc[1][0]);
            acc[1][1] = mfma_bf16(a1, b1, acc[1][1]);
        }
    }
    // partial tile of this slice (zeros for an empty slice): plain stores
    float *pz = a.partial + (int64_t)blockIdx.z * a.Cout * a.Cin * a.K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 64 + i * 32 + mfma32_row(r, lane);
            if (co >= a.Cout) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ci = ci0 + wn * 64 + j * 32 + l31;
                if (ci < a.Cin) pz[((int64_t)co * a.Cin + ci) * a.K + tap] = acc[i][j][r];
            }
        }
}

// ---- 3-tap weight gradient with all taps in one block -----------------------------------------------------------------
// The one-tap-per-block kernel above re-reads the output gradient G once per (tap, ci tile) and the conv input X once per
// (tap, co tile): 470 MB for the DiffNet dilated conv at B=32, T=800 (dW = 512 x 256 x 3) against 52 MB of operands.
// Here a block owns a 128 (co) x 64 (ci) tile of dW for ALL three taps: G is staged once per 64-frame chunk, X once with
// its 2 dil halo frames, written to three LDS copies shifted by the tap offsets (copy k, column j = frame t0 + j + k dil
// - pad), so the MFMA fragment reads stay 16-byte aligned.  Traffic: G x Cin/64 + X x Cout/128 (208 MB for that conv).
template <bool GB16, bool GU = false>
__global__ void __launch_bounds__(256, 2) conv1d_wgrad3_bf16_kernel(WgradBf16Args a) {
    static_assert(!GU || GB16, "16-byte units need an operand that already is bf16");
    __shared__ __attribute__((aligned(16))) unsigned char Gs[128 * WGB_ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Xs[3 * 64 * WGB_ROWB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 128;
    const int sh0 = -a.pad, dil = a.dil;  // tap k reads frame t + k dil - pad
    const int total_chunks = a.B * a.n_chunks_t;
    const int grp = blockIdx.z / a.S;
    const int c_begin = (blockIdx.z - grp * a.S) * a.chunks_per_slice;
    const int c_end = min(c_begin + a.chunks_per_slice, total_chunks);
    const bool has_add = a.chan_add != nullptr;
    a.g = reinterpret_cast<const unsigned char *>(a.g) + grp * a.g_gs;
    a.x = reinterpret_cast<const unsigned char *>(a.x) + grp * a.x_gs;
    if (has_add) a.chan_add += grp * a.add_gs;
    constexpr unsigned GE = GB16 ? 2u : 4u;

    f32x16 acc[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[k][i] = (f32x16){0};

    const int sk = lane, sr0 = wave;
    unsigned gv[32];
    float xa[16], xb[16], av[16];
    constexpr bool fastg = GU;
    const int urow = tid >> 3, ucol = tid & 7;
    auto issue = [&](int ch) {
        const int b = ch / a.n_chunks_t, t0 = (ch % a.n_chunks_t) * WGB_KT;
        const unsigned vg = (unsigned)min(t0 + sk, a.T - 1) * (GB16 ? 8u : 4u);  // (bf16: quad-interleaved)
        const unsigned va = (unsigned)min(max(t0 + sh0 + sk, 0), a.T_in - 1) * 4u;
        const unsigned vb = (unsigned)min(max(t0 + sh0 + 64 + sk, 0), a.T_in - 1) * 4u;
        const rsrc_t d_g = make_rsrc(reinterpret_cast<const unsigned char *>(a.g) + (int64_t)b * a.Cout * a.T * GE);
        const rsrc_t d_x = make_rsrc(reinterpret_cast<const float *>(a.x) + (int64_t)b * a.Cin * a.T_in);
        const rsrc_t d_a = make_rsrc(has_add ? a.chan_add + (int64_t)b * a.Cin : reinterpret_cast<const float *>(a.x));
        if constexpr (fastg) {  // (see conv1d_wgrad_bf16_kernel: 16-byte units of the bf16 output gradient)
            const unsigned vo = (unsigned)(min((co0 >> 2) + urow, (a.Cout >> 2) - 1) * a.T + min(t0 + 8 * ucol, a.T - 8)) * 8u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4_t v = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_g, (int)(vo + 16u * q), 0, 0);
                gv[4 * q] = v[0]; gv[4 * q + 1] = v[1]; gv[4 * q + 2] = v[2]; gv[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int gr = min(co0 + sr0 + 4 * j, a.Cout - 1);
                gv[j] = GB16 ? buf_load_raw16(d_g, vg, q4_row(gr, a.T)) : buf_load_raw(d_g, vg, (unsigned)(gr * a.T) * 4u);
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int cic = min(ci0 + sr0 + 4 * j, a.Cin - 1);
            xa[j] = buf_load(d_x, va, (unsigned)(cic * a.T_in) * 4u);
            xb[j] = buf_load(d_x, vb, (unsigned)(cic * a.T_in) * 4u);
            av[j] = buf_load(d_a, 0u, (unsigned)cic * 4u);
        }
    };
    auto commit = [&](int ch) {
        const int t0 = (ch % a.n_chunks_t) * WGB_KT;
        const bool tv = t0 + sk < a.T;
        const int fa = t0 + sh0 + sk, fb = fa + 64;  // frames of the two loaded values
        const bool va = fa >= 0 && fa < a.T_in, vb = fb >= 0 && fb < a.T_in;
        if constexpr (fastg) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int row = 4 * urow + c;
                const bool ok = t0 + 8 * ucol < a.T && co0 + row < a.Cout;
                const u32x4_t w = q4_channel(gv, c);
                u32x4_t v;
                v[0] = ok ? w[0] : 0u; v[1] = ok ? w[1] : 0u; v[2] = ok ? w[2] : 0u; v[3] = ok ? w[3] : 0u;
                *reinterpret_cast<u32x4_t *>(Gs + row * WGB_ROWB + ucol * 16) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int row = sr0 + 4 * j;
                unsigned short gb;
                if constexpr (GB16) gb = (unsigned short)gv[j];
                else gb = f2bf(__builtin_bit_cast(float, gv[j]));
                *reinterpret_cast<unsigned short *>(Gs + row * WGB_ROWB + sk * 2) = (tv && co0 + row < a.Cout) ? gb : (unsigned short)0;
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = sr0 + 4 * j;
            const bool cv = ci0 + row < a.Cin;
            const float ad = has_add ? av[j] : 0.0f;
            const unsigned short ba = (va && cv) ? f2bf(xa[j] + ad) : (unsigned short)0;
            const unsigned short bb = (vb && cv) ? f2bf(xb[j] + ad) : (unsigned short)0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                // value at tile offset q (= sk or 64 + sk, frame t0 - pad + q) is column q - k dil of copy k
                const int ja = sk - k * dil, jb = 64 + sk - k * dil;
                unsigned char *base = Xs + (k * 64 + row) * WGB_ROWB;
                if (ja >= 0) *reinterpret_cast<unsigned short *>(base + ja * 2) = ba;
                if (jb < 64) *reinterpret_cast<unsigned short *>(base + jb * 2) = bb;
            }
        }
    };
    if (c_begin < c_end) issue(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        __syncthreads();
        commit(ch);
        __syncthreads();
        if (ch + 1 < c_end) issue(ch + 1);
        const unsigned char *ap = Gs + (wm * 64 + l31) * WGB_ROWB + half * 16;
#pragma unroll
        for (int ks = 0; ks < WGB_KT / 16; ++ks) {
            const u32x4_t a0 = *reinterpret_cast<const u32x4_t *>(ap + ks * 32);
            const u32x4_t a1 = *reinterpret_cast<const u32x4_t *>(ap + 32 * WGB_ROWB + ks * 32);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const u32x4_t bk = *reinterpret_cast<const u32x4_t *>(Xs + (k * 64 + wn * 32 + l31) * WGB_ROWB + half * 16 + ks * 32);
                acc[k][0] = mfma_bf16(a0, bk, acc[k][0]);
                acc[k][1] = mfma_bf16(a1, bk, acc[k][1]);
            }
        }
    }
    float *pz = a.partial + (int64_t)blockIdx.z * a.Cout * a.Cin * 3;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 64 + i * 32 + mfma32_row(r, lane);
            const int ci = ci0 + wn * 32 + l31;
            if (co < a.Cout && ci < a.Cin) {
                float *p = pz + ((int64_t)co * a.Cin + ci) * 3;
                p[0] = acc[0][i][r];
                p[1] = acc[1][i][r];
                p[2] = acc[2][i][r];
            }
        }
}

// ---- K-tap weight gradient (5 <= K <= 9, dilation 1, "same" or causal padding) with all taps in one block --------------------------------
// The FFN convs of the FFT blocks / CampNet layers are 9-tap convs (192 -> 768 at 12,800 frames, 256 -> 1024 at 25,600): with one
// tap per block the output gradient G is re-read K x (ci tiles) times and the conv input X K x (co tiles) times -- the blocks
// waited on operand loads (118 - 188 TFLOP/s against 330 - 440 of the forward kernel, tools/small_conv_probe.py).
// Here a block owns a 64 (co) x 64 (ci) tile of dW for ALL K taps (wave: 32 x 32 x K = K accumulators).  Per 64-frame chunk G is
// staged once and X once with 8 halo frames on either side; the taps are K views of the SAME LDS rows shifted by one frame each.
// A shifted view is not 16-byte aligned, so a lane reads the three aligned 8-frame groups around its k-group once and cuts the K
// windows out of those 12 registers (even shifts: a register renaming; odd shifts: 4 v_alignbit).  Operand traffic per chunk:
// (64 + 64 rows) x 64 frames for 36 MFMAs per wave instead of 4.
constexpr int WGT_XF = WGB_KT + 16;         // frames of an X row: chunk + 8 halo frames on either side
constexpr int WGT_XROWB = WGT_XF * 2 + 16;  // 176 bytes: conflict-free 16-byte reads (44 dwords per row)

template <int O>
__device__ __forceinline__ u32x4_t wgt_window(const u32x4_t (&W)[3]) {  // 8 bf16 starting at element O of the 24 in W
    unsigned w[12];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) w[4 * g + e] = W[g][e];
    u32x4_t o;
    if constexpr (O % 2 == 0) {
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = w[O / 2 + d];
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = __builtin_amdgcn_alignbit(w[(O - 1) / 2 + d + 1], w[(O - 1) / 2 + d], 16);
    }
    return o;
}

template <int K, int PAD, int TAP = 0>
__device__ __forceinline__ void wgt_taps(f32x16 (&acc)[K], u32x4_t av, const u32x4_t (&W)[3]) {
    if constexpr (TAP < K) {
        acc[TAP] = mfma_bf16(av, wgt_window<8 + TAP - PAD>(W), acc[TAP]);
        wgt_taps<K, PAD, TAP + 1>(acc, av, W);
    }
}

// PAD = frames of left padding: (K - 1) / 2 for the "same" convs, K - 1 for the causal ("LEFT"-padded) FFN convs of the decoders
template <int K, int PAD>
__global__ void __launch_bounds__(256, 2) conv1d_wgrad_taps_bf16_kernel(WgradBf16Args a) {
    static_assert(PAD >= 0 && PAD <= 8 && K - 1 - PAD >= 0 && K - 1 - PAD <= 8, "tap shifts must stay inside the 8-frame halo");
    __shared__ __attribute__((aligned(16))) unsigned char Gs[64 * WGB_ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Xs[64 * WGT_XROWB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
    const int total_chunks = a.B * a.n_chunks_t;
    const int c_begin = blockIdx.z * a.chunks_per_slice;
    const int c_end = min(c_begin + a.chunks_per_slice, total_chunks);

    f32x16 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = (f32x16){0};

    // staging (one chunk ahead, raw fp32 bits in registers): G rows wave, wave + 4, ... x frame t0 + lane; X the same rows x frame
    // t0 - 8 + lane, and the 16 frames t0 + 56 .. t0 + 71 of row tid >> 2 (4 frames per thread)
    unsigned gv[16], xv[16], xe[4];
    const int er = tid >> 2, ef = (tid & 3) * 4;
    auto issue = [&](int ch) {
        const int b = ch / a.n_chunks_t, t0 = (ch % a.n_chunks_t) * WGB_KT;
        const rsrc_t d_g = make_rsrc(reinterpret_cast<const float *>(a.g) + (int64_t)b * a.Cout * a.T);
        const rsrc_t d_x = make_rsrc(reinterpret_cast<const float *>(a.x) + (int64_t)b * a.Cin * a.T_in);
        const unsigned vg = (unsigned)min(t0 + lane, a.T - 1) * 4u;
        const unsigned vx = (unsigned)min(max(t0 - 8 + lane, 0), a.T_in - 1) * 4u;
#pragma unroll
        for (int j = 0; j < 16; ++j) gv[j] = buf_load_raw(d_g, vg, (unsigned)(min(co0 + wave + 4 * j, a.Cout - 1) * a.T) * 4u);
#pragma unroll
        for (int j = 0; j < 16; ++j) xv[j] = buf_load_raw(d_x, vx, (unsigned)(min(ci0 + wave + 4 * j, a.Cin - 1) * a.T_in) * 4u);
        const unsigned ro = (unsigned)(min(ci0 + er, a.Cin - 1) * a.T_in) * 4u;
#pragma unroll
        for (int e = 0; e < 4; ++e) xe[e] = buf_load_raw(d_x, ro + (unsigned)min(max(t0 + 56 + ef + e, 0), a.T_in - 1) * 4u, 0u);
    };
    auto commit = [&](auto PROC, int ch) __attribute__((always_inline)) {
        constexpr int kPro = decltype(PROC)::value;
        const int t0 = (ch % a.n_chunks_t) * WGB_KT;
        const bool tv = t0 + lane < a.T, xvld = t0 - 8 + lane >= 0 && t0 - 8 + lane < a.T_in;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = wave + 4 * j;
            const unsigned short gb = f2bf(__builtin_bit_cast(float, gv[j]));
            const unsigned short xb = f2bf(pro_c<kPro>(__builtin_bit_cast(float, xv[j]), a.pro_param));
            *reinterpret_cast<unsigned short *>(Gs + row * WGB_ROWB + lane * 2) = (tv && co0 + row < a.Cout) ? gb : (unsigned short)0;
            *reinterpret_cast<unsigned short *>(Xs + row * WGT_XROWB + lane * 2) = (xvld && ci0 + row < a.Cin) ? xb : (unsigned short)0;
        }
        unsigned short q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ti = t0 + 56 + ef + e;
            const unsigned short xb = f2bf(pro_c<kPro>(__builtin_bit_cast(float, xe[e]), a.pro_param));
            q[e] = (ti >= 0 && ti < a.T_in && ci0 + er < a.Cin) ? xb : (unsigned short)0;
        }
        u32x2_t u;
        u[0] = (unsigned)q[0] | ((unsigned)q[1] << 16); u[1] = (unsigned)q[2] | ((unsigned)q[3] << 16);
        *reinterpret_cast<u32x2_t *>(Xs + er * WGT_XROWB + (64 + ef) * 2) = u;
    };
    if (c_begin < c_end) issue(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        __syncthreads();
        switch (a.pro) {
            case SET_PRO_LRELU: commit(ic<SET_PRO_LRELU>{}, ch); break;
            case SET_PRO_DIV: commit(ic<SET_PRO_DIV>{}, ch); break;
            default: commit(ic<SET_PRO_NONE>{}, ch); break;
        }
        __syncthreads();
        if (ch + 1 < c_end) issue(ch + 1);
        // X row element e <-> frame t0 - 8 + e; the lane's k-group of G covers frames t0 + 16 ks + 8 half + (0 .. 7), tap `tap` pairs
        // them with X frames shifted by tap - PAD: elements 16 ks + 8 half + 8 + tap - PAD + (0 .. 7) -> offset 8 + tap - PAD in W
        const unsigned char *ap = Gs + (wm * 32 + l31) * WGB_ROWB + half * 16;
        const unsigned char *bp = Xs + (wn * 32 + l31) * WGT_XROWB + half * 16;
#pragma unroll
        for (int ks = 0; ks < WGB_KT / 16; ++ks) {
            const u32x4_t av = *reinterpret_cast<const u32x4_t *>(ap + ks * 32);
            u32x4_t W[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) W[g] = *reinterpret_cast<const u32x4_t *>(bp + ks * 32 + g * 16);
            wgt_taps<K, PAD>(acc, av, W);
        }
    }
    // partial tile of this slice (zeros for an empty slice): K consecutive floats per (co, ci)
    float *pz = a.partial + (int64_t)blockIdx.z * a.Cout * a.Cin * K;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 32 + mfma32_row(r, lane);
        const int ci = ci0 + wn * 32 + l31;
        if (co < a.Cout && ci < a.Cin) {
            float *o = pz + ((int64_t)co * a.Cin + ci) * K;
#pragma unroll
            for (int k = 0; k < K; ++k) o[k] = acc[k][r];
        }
    }
}

// ---- 3-tap weight gradient, one X copy (round 6) -------------------------------------------------------------------------------------
// conv1d_wgrad3_bf16_kernel stages the fp32 conv input one frame per load (32 four-byte loads per thread and chunk) and writes it to
// THREE shifted LDS copies with two-byte writes (96 per thread and chunk) for 24 MFMAs per wave: the vector-memory and LDS-write issue,
// not the matrix pipe, set its time (327 TFLOP/s on the DiffNet dilated conv).  Here, for the "same" convs (pad = dil in {1, 2, 4, 8},
// T a multiple of 8, bf16 output gradient): X is loaded in 16-byte units (4 frames: 5 loads per thread and chunk), converted once and
// written to ONE copy with an 8-frame halo on either side (5 eight-byte LDS writes); a lane reads the three aligned 8-frame groups
// around its k-group and cuts the tap windows out of those 12 registers, as conv1d_wgrad_taps_bf16_kernel does.  Same bf16 operand
// values, same chunk / k-step / tap order per accumulator as conv1d_wgrad3_bf16_kernel: the partial tiles are bit-identical.
template <int DIL>
__global__ void __launch_bounds__(256, 2) conv1d_wgrad3u_bf16_kernel(WgradBf16Args a) {
    static_assert(DIL == 1 || DIL == 2 || DIL == 4 || DIL == 8, "tap shifts must stay inside the 8-frame halo");
    __shared__ __attribute__((aligned(16))) unsigned char Gs[128 * WGB_ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Xs[64 * WGT_XROWB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 128;
    const int total_chunks = a.B * a.n_chunks_t;
    const int grp = blockIdx.z / a.S;
    const int c_begin = (blockIdx.z - grp * a.S) * a.chunks_per_slice;
    const int c_end = min(c_begin + a.chunks_per_slice, total_chunks);
    const bool has_add = a.chan_add != nullptr;
    a.g = reinterpret_cast<const unsigned char *>(a.g) + grp * a.g_gs;
    a.x = reinterpret_cast<const unsigned char *>(a.x) + grp * a.x_gs;
    if (has_add) a.chan_add += grp * a.add_gs;

    f32x16 acc[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[k][i] = (f32x16){0};

    // G: unit (row urow + 32 q, frames 8 ucol ..) as in conv1d_wgrad3_bf16_kernel; X: 64 rows x 20 units of 4 frames (frames t0 - 8 ..
    // t0 + 71), unit tid + 256 q = (row xr[q], unit column xc[q])
    constexpr int XU_ROW = WGT_XF / 4, XQ = 64 * XU_ROW / 256;  // 20 units per row, 5 per thread
    static_assert(64 * XU_ROW % 256 == 0, "whole units per thread");
    const int urow = tid >> 3, ucol = tid & 7;
    int xr[XQ], xc[XQ];
#pragma unroll
    for (int q = 0; q < XQ; ++q) { const int u = tid + 256 * q; xr[q] = u / XU_ROW; xc[q] = u - xr[q] * XU_ROW; }
    unsigned gv[16];
    u32x4_t xv[XQ];
    float av[XQ];
    auto issue = [&](int ch) {
        const int b = ch / a.n_chunks_t, t0 = (ch % a.n_chunks_t) * WGB_KT;
        const rsrc_t d_g = make_rsrc(reinterpret_cast<const unsigned char *>(a.g) + (int64_t)b * a.Cout * a.T * 2u);
        const rsrc_t d_x = make_rsrc(reinterpret_cast<const float *>(a.x) + (int64_t)b * a.Cin * a.T_in);
        const rsrc_t d_a = make_rsrc(has_add ? a.chan_add + (int64_t)b * a.Cin : reinterpret_cast<const float *>(a.x));
        const unsigned vog = (unsigned)(min((co0 >> 2) + urow, (a.Cout >> 2) - 1) * a.T + min(t0 + 8 * ucol, a.T - 8)) * 8u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // (quad-interleaved G: channel quad urow, 8 frames ucol = four consecutive 16-byte units)
            const u32x4_t v = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_g, (int)(vog + 16u * q), 0, 0);
            gv[4 * q] = v[0]; gv[4 * q + 1] = v[1]; gv[4 * q + 2] = v[2]; gv[4 * q + 3] = v[3];
        }
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int cic = min(ci0 + xr[q], a.Cin - 1);
            const unsigned vo = (unsigned)(cic * a.T_in + min(max(t0 - 8 + 4 * xc[q], 0), a.T_in - 4)) * 4u;
            xv[q] = (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(d_x, (int)vo, 0, 0);
            av[q] = buf_load(d_a, (unsigned)cic * 4u, 0u);
        }
    };
    auto commit = [&](int ch) {
        const int t0 = (ch % a.n_chunks_t) * WGB_KT;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int row = 4 * urow + c;
            const bool ok = t0 + 8 * ucol < a.T && co0 + row < a.Cout;  // T % 8 == 0, Cout % 4 == 0: entirely inside or outside
            const u32x4_t w = q4_channel(gv, c);
            u32x4_t v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ok ? w[e] : 0u;
            *reinterpret_cast<u32x4_t *>(Gs + row * WGB_ROWB + ucol * 16) = v;
        }
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int f0 = t0 - 8 + 4 * xc[q];
            const bool ok = f0 >= 0 && f0 < a.T_in && ci0 + xr[q] < a.Cin;  // T_in % 4 == 0
            const float ad = has_add ? av[q] : 0.0f;
            unsigned short h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned bits = xv[q][e];  // (a scalar copy first: __builtin_bit_cast of a vector-element lvalue reads element 0)
                h[e] = f2bf(__builtin_bit_cast(float, bits) + ad);  // the 3-copy kernel's arithmetic
            }
            u32x2_t w;
            w[0] = ok ? ((unsigned)h[0] | ((unsigned)h[1] << 16)) : 0u;
            w[1] = ok ? ((unsigned)h[2] | ((unsigned)h[3] << 16)) : 0u;
            *reinterpret_cast<u32x2_t *>(Xs + xr[q] * WGT_XROWB + xc[q] * 8) = w;
        }
    };
    if (c_begin < c_end) issue(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        __syncthreads();
        commit(ch);
        __syncthreads();
        if (ch + 1 < c_end) issue(ch + 1);
        // X row element e <-> frame t0 - 8 + e; the lane's k-group of G covers frames t0 + 16 ks + 8 half + (0 .. 7), tap k pairs them
        // with X frames shifted by (k - 1) DIL: elements 16 ks + 8 half + 8 + (k - 1) DIL + (0 .. 7) -> offset 8 + (k - 1) DIL in W
        const unsigned char *ap = Gs + (wm * 64 + l31) * WGB_ROWB + half * 16;
        const unsigned char *bp = Xs + (wn * 32 + l31) * WGT_XROWB + half * 16;
#pragma unroll
        for (int ks = 0; ks < WGB_KT / 16; ++ks) {
            const u32x4_t a0 = *reinterpret_cast<const u32x4_t *>(ap + ks * 32);
            const u32x4_t a1 = *reinterpret_cast<const u32x4_t *>(ap + 32 * WGB_ROWB + ks * 32);
            u32x4_t W[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) W[g] = *reinterpret_cast<const u32x4_t *>(bp + ks * 32 + g * 16);
            const u32x4_t b0 = wgt_window<8 - DIL>(W), b1 = W[1], b2 = wgt_window<8 + DIL>(W);
            acc[0][0] = mfma_bf16(a0, b0, acc[0][0]);
            acc[0][1] = mfma_bf16(a1, b0, acc[0][1]);
            acc[1][0] = mfma_bf16(a0, b1, acc[1][0]);
            acc[1][1] = mfma_bf16(a1, b1, acc[1][1]);
            acc[2][0] = mfma_bf16(a0, b2, acc[2][0]);
            acc[2][1] = mfma_bf16(a1, b2, acc[2][1]);
        }
    }
    float *pz = a.partial + (int64_t)blockIdx.z * a.Cout * a.Cin * 3;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 64 + i * 32 + mfma32_row(r, lane);
            const int ci = ci0 + wn * 32 + l31;
            if (co < a.Cout && ci < a.Cin) {
                float *p = pz + ((int64_t)co * a.Cin + ci) * 3;
                p[0] = acc[0][i][r];
                p[1] = acc[1][i][r];
                p[2] = acc[2][i][r];
            }
        }
}

// dw[i] += sum_{s < S} partial[s][i]   (one fixed association: four interleaved chains over the slices, combined pairwise -- four
// loads in flight per thread instead of one dependent add per memory round trip)
// (grid.y = group: partial[(group * S + z) * n + i], dw + group * dw_gs)
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float *partial, float *dw, int64_t n, int S, int64_t dw_gs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *pp = partial + (int64_t)blockIdx.y * S * n + i;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int z = 0;
    for (; z + 3 < S; z += 4) {
        s0 += pp[(int64_t)z * n];
        s1 += pp[(int64_t)(z + 1) * n];
        s2 += pp[(int64_t)(z + 2) * n];
        s3 += pp[(int64_t)(z + 3) * n];
    }
    for (; z < S; ++z) s0 += pp[(int64_t)z * n];
    dw[(int64_t)blockIdx.y * dw_gs + i] += (s0 + s1) + (s2 + s3);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// called by set_conv1d (conv1d.hip) for impl == SET_IMPL_BF16
int set_conv1d_bf16_dispatch(const SetConv1dArgs &a, hipStream_t s) {
    if (a.out_stride != 1 || a.out_off != 0)
        return set_fail(SET_E_UNSUPPORTED, "set_conv1d(bf16)", "strided output (polyphase transposed conv) is an fp32 path");
    const int o_first = -a.pad, o_last = (a.K - 1) * a.dil - a.pad;
    const int lo = o_first < o_last ? o_first : o_last;
    const int halo = (o_first < o_last ? o_last : o_first) - lo;
    if (halo > 128) return set_fail(SET_E_UNSUPPORTED, "set_conv1d(bf16)", "receptive field > 128");
    const int64_t cs = a.res && a.res_cs > a.out_cs ? a.res_cs : a.out_cs;
    if (((int64_t)set_round_up(a.Cout, BF16_IMG_ROWS) * cs + a.T_out) * 4 >= ((int64_t)1 << 31) ||
        ((int64_t)a.Cin * a.in_cs + a.T_in) * 4 >= ((int64_t)1 << 31))
        return set_fail(SET_E_UNSUPPORTED, "set_conv1d(bf16)", "one batch slice of in / out / res exceeds 2 GiB");
    // 64-row blocks waste less than 128-row ones on 129 .. 192 rows -- but they read the input once more, and the 1x1 convs of
    // that height (CampNet's 192-channel projections at 12,800 frames) wait on their input, not on MFMAs: 27 -> 22 us (192 -> 192),
    // 56 -> 45 us (768 -> 192) with 128-row blocks; the 9-tap convs keep the 64-row ones (146 vs 149 us)
    const bool narrow = a.Cout <= 64 || (a.Cout > 128 && a.Cout <= 192 && a.K > 1);
    if (a.K == 1 && a.Cin > 32 && a.Cout > 64 && halo == 0 && !a.in_chan_add && a.pad == 0) {
        const int cp = set_round_up(a.Cin, BF16_IMG_CH);
        if (cp <= 64) return launch_conv1x1_oneshot<64>(a, s);
        if (cp <= 128) return launch_conv1x1_oneshot<128>(a, s);
        if (cp <= 192) return launch_conv1x1_oneshot<192>(a, s);
        return launch_conv1x1_oneshot<256>(a, s);  // wider inputs: chunks of 256 channels
    }
    if (a.K == 1 && a.Cin > 32 && halo == 0 && !a.in_chan_add) {
        return narrow ? launch_conv_bf16<1, 4, 64, 1, false, false>(a, lo, halo, s)
                      : launch_conv_bf16<2, 2, 64, 1, false, false>(a, lo, halo, s);
    }
    // taps per stage: 5 and 9 taps (the predictor / FFN convs) are 1 and 2 stages per 32-channel chunk with 5 taps per stage, 2 and 3
    // with 4 -- these convs wait on their stage round trips, not on MFMAs (tools/small_conv_probe.py); all 9 taps in one stage of the
    // 64-row blocks (46 KB of weights per stage): 118 vs 125 us on 768 -> 192 at 12,800 frames, not kept (profiles/r06_conv_tg9_ab.log)
    if (a.K == 5 || a.K > 8)
        return narrow ? launch_conv_bf16<1, 4, 32, 5, true, true>(a, lo, halo, s) : launch_conv_bf16<2, 2, 32, 5, true, true>(a, lo, halo, s);
    return narrow ? launch_conv_bf16<1, 4, 32, 4, true, true>(a, lo, halo, s)
                  : launch_conv_bf16<2, 2, 32, 4, true, true>(a, lo, halo, s);
}

// fp32 deterministic path: kernel + slice plan live in train.hip
int wgrad_f32_slices(int B, int Cin, int Cout, int K, int T);
int launch_wgrad_f32_partial(const float *g, const float *x, const float *chan_add, float *partial, int B, int Cin, int Cout,
                             int K, int dil, int pad, int T, int T_in, int pro, float pro_param, hipStream_t s);

static bool wgrad3_applies(int K, int dil, int pad, int pro, int dtype) {
    const int d = dil < 0 ? -dil : dil;
    return K == 3 && dil > 0 && 2 * d <= 64 && pad >= 0 && pro == SET_PRO_NONE && (dtype == SET_DTYPE_BF16 || dtype == SET_DTYPE_BF16_G16);
}

static int wgrad_bf16_slices(int B, int Cin, int Cout, int K, int T, bool taps3 = false) {
    const int n_chunks_t = (T + WGB_KT - 1) / WGB_KT;
    const int64_t total_chunks = (int64_t)B * n_chunks_t;
    const int tiles = taps3 ? ((Cin + 63) / 64) * ((Cout + 127) / 128) : K * ((Cin + 127) / 128) * ((Cout + 127) / 128);
    int64_t S = (640 + tiles - 1) / tiles;  // ~2.5 blocks per CU
    if (S > total_chunks) S = total_chunks;
    if (S > (taps3 ? 32 : 64)) S = taps3 ? 32 : 64;
    if (S < 1) S = 1;
    const int64_t cps = (total_chunks + S - 1) / S;
    return (int)((total_chunks + cps - 1) / cps);  // no empty slices
}

// all-taps kernel (conv1d_wgrad_taps_bf16_kernel): K = 5, 7, 9, dilation 1, "same" (pad = (K - 1) / 2) or causal (pad = K - 1)
// padding, fp32 operands, no per-channel add
static bool wgrad_taps_applies(int K, int dil, int pad, int dtype, bool chan_add) {
    return dtype == SET_DTYPE_BF16 && !chan_add && (K == 5 || K == 7 || K == 9) && dil == 1 && (pad == (K - 1) / 2 || pad == K - 1);
}
static int wgrad_taps_slices(int B, int Cin, int Cout, int T) {
    const int64_t total_chunks = (int64_t)B * ((T + WGB_KT - 1) / WGB_KT);
    const int tiles = ((Cin + 63) / 64) * ((Cout + 63) / 64);
    const int target = 512;
    int64_t S = (target + tiles - 1) / tiles;  // two blocks per CU; every slice costs a K-tap partial image (write + read)
    if (S > total_chunks) S = total_chunks;
    if (S > 16) S = 16;
    if (S < 1) S = 1;
    const int64_t cps = (total_chunks + S - 1) / S;
    return (int)((total_chunks + cps - 1) / cps);  // no empty slices
}

// slices per group of a launch over `groups` equal GEMMs: with many groups a few slices fill the chip
static int wgrad_bf16_slices_grouped(int B, int Cin, int Cout, int K, int T, bool taps3, int groups) {
    const int n_chunks_t = (T + WGB_KT - 1) / WGB_KT;
    const int64_t total_chunks = (int64_t)B * n_chunks_t;
    const int64_t tiles = (int64_t)groups * (taps3 ? ((Cin + 63) / 64) * ((Cout + 127) / 128) : K * ((Cin + 127) / 128) * ((Cout + 127) / 128));
    // blocks of a grouped launch are long (each walks 1 / S of ALL frames): aim at ~2.5 full waves of the chip's 512 block slots,
    // not at the 2.5 blocks per CU of a single GEMM (measured, ms per bf16 training step: 640 blocks 15.75, 1280 15.16, 2048 15.29, 4096 15.39)
    const int target = 1280;
    int64_t S = (target + tiles - 1) / tiles;
    if (S > total_chunks) S = total_chunks;
    if (S > (taps3 ? 32 : 64)) S = taps3 ? 32 : 64;
    if (S < 1) S = 1;
    const int64_t cps = (total_chunks + S - 1) / S;
    return (int)((total_chunks + cps - 1) / cps);  // no empty slices
}

extern "C" int64_t set_conv1d_wgrad_scratch_floats(int32_t B, int32_t Cin, int32_t Cout, int32_t K, int32_t T, int32_t dtype) {
    // upper bound over the kernel variants of the dtype (the 3-tap variant is chosen from dil / pad / pro at call time)
    int S = dtype != SET_DTYPE_F32 ? wgrad_bf16_slices(B, Cin, Cout, K, T) : wgrad_f32_slices(B, Cin, Cout, K, T);
    if (dtype != SET_DTYPE_F32 && K == 3) { const int S3 = wgrad_bf16_slices(B, Cin, Cout, K, T, true); S = S3 > S ? S3 : S; }
    if (dtype == SET_DTYPE_BF16 && (K == 5 || K == 7 || K == 9)) { const int St = wgrad_taps_slices(B, Cin, Cout, T); S = St > S ? St : S; }
    return (int64_t)S * Cout * Cin * K;
}

extern "C" int64_t set_conv1d_wgrad_grouped_scratch_floats(int32_t groups, int32_t B, int32_t Cin, int32_t Cout, int32_t K, int32_t T) {
    if (groups < 1) return 0;
    int S = wgrad_bf16_slices_grouped(B, Cin, Cout, K, T, false, groups);
    if (K == 3) { const int S3 = wgrad_bf16_slices_grouped(B, Cin, Cout, K, T, true, groups); S = S3 > S ? S3 : S; }
    return (int64_t)groups * S * Cout * Cin * K;
}

// bf16 weight gradients of `groups` equal GEMMs in one launch (+ one ordered reduce): group q reads g + q g_gs, x + q x_gs,
// chan_add + q add_gs (element strides) and adds into dw + q dw_gs
static int wgrad_bf16_launch(const void *g, const void *x, const float *chan_add, float *dw, int B, int Cin, int Cout, int K, int dil,
                             int pad, int T, int T_in, int pro, float pro_param, int dtype, float *scratch, int groups, int64_t g_gs,
                             int64_t x_gs, int64_t add_gs, int64_t dw_gs, int S_plain, int S_taps3, hipStream_t s) {
    const int64_t n = (int64_t)Cout * Cin * K;
    const bool g16 = dtype != SET_DTYPE_BF16, x16 = dtype == SET_DTYPE_BF16_G16_X16;
    if ((g16 && Cout % 4) || (x16 && Cin % 4))  // bf16 operands are channel-quad interleaved (see q4_row)
        return set_fail(SET_E_UNSUPPORTED, "set_conv1d_wgrad_det(bf16 operand)", "channel count of a bf16 operand must be a multiple of 4");
    WgradBf16Args a;
    a.g = g; a.x = x; a.chan_add = chan_add; a.partial = scratch;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.K = K; a.dil = dil; a.pad = pad; a.T = T; a.T_in = T_in; a.pro = pro;
    a.pro_param = pro_param;
    a.n_chunks_t = (T + WGB_KT - 1) / WGB_KT;
    a.g_gs = g_gs * (g16 ? 2 : 4); a.x_gs = x_gs * (x16 ? 2 : 4); a.add_gs = add_gs;
    int S;
    if (groups == 1 && wgrad_taps_applies(K, dil, pad, dtype, chan_add != nullptr)) {
        S = wgrad_taps_slices(B, Cin, Cout, T);
        a.S = S;
        a.chunks_per_slice = (B * a.n_chunks_t + S - 1) / S;
        a.ci_tiles = (Cin + 63) / 64;
        dim3 grid(a.ci_tiles, (Cout + 63) / 64, S);
        const bool causal = pad == K - 1;
        if (K == 9 && !causal) hipLaunchKernelGGL((conv1d_wgrad_taps_bf16_kernel<9, 4>), grid, dim3(256), 0, s, a);
        else if (K == 9) hipLaunchKernelGGL((conv1d_wgrad_taps_bf16_kernel<9, 8>), grid, dim3(256), 0, s, a);
        else if (K == 7 && !causal) hipLaunchKernelGGL((conv1d_wgrad_taps_bf16_kernel<7, 3>), grid, dim3(256), 0, s, a);
        else if (K == 7) hipLaunchKernelGGL((conv1d_wgrad_taps_bf16_kernel<7, 6>), grid, dim3(256), 0, s, a);
        else if (!causal) hipLaunchKernelGGL((conv1d_wgrad_taps_bf16_kernel<5, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv1d_wgrad_taps_bf16_kernel<5, 4>), grid, dim3(256), 0, s, a);
        const int rc = set_check_launch("set_conv1d_wgrad_det(bf16, all taps)");
        if (rc != SET_OK) return rc;
    } else if (wgrad3_applies(K, dil, pad, pro, dtype)) {
        S = S_taps3;
        a.S = S;
        a.chunks_per_slice = (B * a.n_chunks_t + S - 1) / S;
        a.ci_tiles = (Cin + 63) / 64;
        dim3 grid(a.ci_tiles, (Cout + 127) / 128, S * groups);
        const bool gu = (T & 7) == 0 && T >= 8;  // rows of the bf16 output gradient are 16-byte aligned: copy it in 16-byte units
        // one-copy form (16-byte units of X): "same" convs with the tap shifts inside the 8-frame halo; SET_AMD_WGRAD3_UNITS=0 keeps the
        // three-copy kernel (the bit-identity test's reference)
        const bool units_env = !(getenv("SET_AMD_WGRAD3_UNITS") && atoi(getenv("SET_AMD_WGRAD3_UNITS")) == 0);
        const bool xu = units_env && dtype == SET_DTYPE_BF16_G16 && gu && pad == dil && T_in == T && (dil == 1 || dil == 2 || dil == 4 || dil == 8);
        if (xu && dil == 1) hipLaunchKernelGGL((conv1d_wgrad3u_bf16_kernel<1>), grid, dim3(256), 0, s, a);
        else if (xu && dil == 2) hipLaunchKernelGGL((conv1d_wgrad3u_bf16_kernel<2>), grid, dim3(256), 0, s, a);
        else if (xu && dil == 4) hipLaunchKernelGGL((conv1d_wgrad3u_bf16_kernel<4>), grid, dim3(256), 0, s, a);
        else if (xu) hipLaunchKernelGGL((conv1d_wgrad3u_bf16_kernel<8>), grid, dim3(256), 0, s, a);
        else if (dtype == SET_DTYPE_BF16) hipLaunchKernelGGL((conv1d_wgrad3_bf16_kernel<false>), grid, dim3(256), 0, s, a);
        else if (gu) hipLaunchKernelGGL((conv1d_wgrad3_bf16_kernel<true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv1d_wgrad3_bf16_kernel<true>), grid, dim3(256), 0, s, a);
        const int rc = set_check_launch("set_conv1d_wgrad_det(bf16, 3 taps)");
        if (rc != SET_OK) return rc;
    } else {
        S = S_plain;
        a.S = S;
        const int total_chunks = B * a.n_chunks_t;
        a.chunks_per_slice = (total_chunks + S - 1) / S;
        a.ci_tiles = (Cin + 127) / 128;
        dim3 grid(K * a.ci_tiles, (Cout + 127) / 128, S * groups);
        const bool gu = (T & 7) == 0 && T >= 8;                                     // (see the kernel: 16-byte units of an operand)
        const bool xu = gu && K == 1 && pad == 0 && T_in == T;                      // the conv input too when no tap shifts it
        if (dtype == SET_DTYPE_BF16) {
            if (xu) hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<false, false, true, true>), grid, dim3(256), 0, s, a);
            else if (gu) hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<false, false, true, false>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<false, false>), grid, dim3(256), 0, s, a);
        } else if (dtype == SET_DTYPE_BF16_G16) {
            if (xu) hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<true, false, true, true>), grid, dim3(256), 0, s, a);
            else if (gu) hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<true, false, true, false>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<true, false>), grid, dim3(256), 0, s, a);
        } else {
            if (xu) hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<true, true, true, true>), grid, dim3(256), 0, s, a);
            else if (gu) hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<true, true, true, false>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((conv1d_wgrad_bf16_kernel<true, true>), grid, dim3(256), 0, s, a);
        }
        const int rc = set_check_launch("set_conv1d_wgrad_det(bf16)");
        if (rc != SET_OK) return rc;
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(set_blocks(n, 256), groups), dim3(256), 0, s, scratch, dw, n, S, dw_gs);
    return set_check_launch("set_conv1d_wgrad_det(reduce)");
}

extern "C" int set_conv1d_wgrad_det(const void *g, const void *x, const float *chan_add, float *dw, int32_t B, int32_t Cin,
                                    int32_t Cout, int32_t K, int32_t dil, int32_t pad, int32_t T, int32_t T_in, int32_t pro,
                                    float pro_param, int32_t dtype, float *scratch, int64_t scratch_floats, void *stream) {
    SET_REQUIRE(g && x && dw && scratch && B > 0 && Cin > 0 && Cout > 0 && K > 0 && T > 0 && T_in > 0, "set_conv1d_wgrad_det");
    const int64_t n = (int64_t)Cout * Cin * K;
    const int64_t need = set_conv1d_wgrad_scratch_floats(B, Cin, Cout, K, T, dtype);
    SET_REQUIRE(scratch_floats >= need, "set_conv1d_wgrad_det (scratch too small)");
    SET_REQUIRE((int64_t)Cout * T * 4 < ((int64_t)1 << 31) && (int64_t)Cin * T_in * 4 < ((int64_t)1 << 31),
                "set_conv1d_wgrad_det (one batch slice exceeds 2 GiB)");
    hipStream_t s = (hipStream_t)stream;
    if (dtype != SET_DTYPE_F32) {
        SET_REQUIRE(dtype == SET_DTYPE_BF16 || dtype == SET_DTYPE_BF16_G16 || dtype == SET_DTYPE_BF16_G16_X16, "set_conv1d_wgrad_det (dtype)");
        SET_REQUIRE(dtype != SET_DTYPE_BF16_G16_X16 || (chan_add == nullptr && pro == SET_PRO_NONE), "set_conv1d_wgrad_det (bf16 x takes no prologue)");
        return wgrad_bf16_launch(g, x, chan_add, dw, B, Cin, Cout, K, dil, pad, T, T_in, pro, pro_param, dtype, scratch, 1, 0, 0, 0, 0,
                                 wgrad_bf16_slices(B, Cin, Cout, K, T), wgrad_bf16_slices(B, Cin, Cout, K, T, true), s);
    }
    const int S = (int)(need / n);
    const int rc = launch_wgrad_f32_partial(reinterpret_cast<const float *>(g), reinterpret_cast<const float *>(x), chan_add,
                                            scratch, B, Cin, Cout, K, dil, pad, T, T_in, pro, pro_param, s);
    if (rc != SET_OK) return rc;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(set_blocks(n, 256), 1), dim3(256), 0, s, scratch, dw, n, S, (int64_t)0);
    return set_check_launch("set_conv1d_wgrad_det(reduce)");
}

extern "C" int set_conv1d_wgrad_det_grouped(const void *g, const void *x, const float *chan_add, float *dw, int32_t groups,
                                            int64_t g_gs, int64_t x_gs, int64_t add_gs, int64_t dw_gs, int32_t B, int32_t Cin,
                                            int32_t Cout, int32_t K, int32_t dil, int32_t pad, int32_t T, int32_t T_in, int32_t dtype,
                                            float *scratch, int64_t scratch_floats, void *stream) {
    SET_REQUIRE(g && x && dw && scratch && groups > 0 && B > 0 && Cin > 0 && Cout > 0 && K > 0 && T > 0 && T_in > 0,
                "set_conv1d_wgrad_det_grouped");
    SET_REQUIRE(dtype == SET_DTYPE_BF16 || dtype == SET_DTYPE_BF16_G16 || dtype == SET_DTYPE_BF16_G16_X16, "set_conv1d_wgrad_det_grouped (dtype)");
    SET_REQUIRE(dtype != SET_DTYPE_BF16_G16_X16 || chan_add == nullptr, "set_conv1d_wgrad_det_grouped (bf16 x takes no per-channel add)");
    SET_REQUIRE(scratch_floats >= set_conv1d_wgrad_grouped_scratch_floats(groups, B, Cin, Cout, K, T), "set_conv1d_wgrad_det_grouped (scratch too small)");
    SET_REQUIRE((int64_t)Cout * T * 4 < ((int64_t)1 << 31) && (int64_t)Cin * T_in * 4 < ((int64_t)1 << 31),
                "set_conv1d_wgrad_det_grouped (one batch slice exceeds 2 GiB)");
    const int S1 = wgrad_bf16_slices_grouped(B, Cin, Cout, K, T, false, groups), S3 = wgrad_bf16_slices_grouped(B, Cin, Cout, K, T, true, groups);
    SET_REQUIRE((int64_t)groups * (S1 > S3 ? S1 : S3) <= 65535, "set_conv1d_wgrad_det_grouped (grid.z)");
    return wgrad_bf16_launch(g, x, chan_add, dw, B, Cin, Cout, K, dil, pad, T, T_in, SET_PRO_NONE, 0.0f, dtype, scratch, groups, g_gs, x_gs,
                             add_gs, dw_gs, S1, S3, (hipStream_t)stream);
}
