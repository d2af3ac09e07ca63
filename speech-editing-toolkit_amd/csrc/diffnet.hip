// DiffNet (FluentSpeech denoiser) layer kernels on the fp32 MFMA pipe for gfx950: one residual layer per launch (diffnet_layer_kernel),
// the persistent layer-stack kernels (diffnet_stack_kernel: direct; diffnet_stack_wino_kernel: Winograd F(2,3); diffnet_stack_split_kernel:
// row split for small batches), the kernels that pack their weight images, and the launcher of the stack kernels
// (set_launch_diffnet_stack_f32: which one runs is decided by plan_stack, csrc/diffusion_loop.hip).
//
// A layer (diffnet.py:60-81) fuses
//   x+d  ->  k=3 dilated conv (implicit GEMM, 512x768)  -> +bias +hoisted conditioner projection
//        ->  sigmoid*tanh gate  ->  1x1 conv (GEMM 512x256)  ->  residual/sqrt(2) + skip accumulate.
// fp32 end to end on v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain): the parity bar is |dmel| < 1e-4
// against the fp32 reference, which a bf16 path cannot meet.
//
// Work decomposition of diffnet_layer_kernel (64-wide waves, 256 CUs):
//   grid  = (ceil(T/64), B); block = 256 threads = 4 waves; block tile = all 512 rows x 64 frames.
//   wave w owns gate rows [64w,64w+64) and the matching filter rows [256+64w, 256+64w+64) so the
//   gate is lane-local in the accumulator layout; same split for residual/skip rows of GEMM 2.
//   8 accumulators (4 row blocks x 2 col blocks) of 32x32 per wave = 128 VGPRs -> 2 blocks per CU.
//   B operand (activations): LDS tile xs[256][64 + 2*dil], lanes read 32 consecutive frames ->
//   conflict free; the k=3 taps are column shifts of the same tile (im2col is free).
//   A operand (weights): pre-packed in fragment order so one k-step of a wave is a single 1 KiB
//   coalesced global_load_dwordx4 (L2 resident: 2 MiB per layer); prefetched 4 k-steps ahead.
//   z (gate output) overwrites the xs tile in LDS; x for the residual is re-read from L2.
#include <stdlib.h>

#include "common.h"
#include "diffnet_host.h"
#include "phase_probe.h"
#include "stack_queue.h"

// probe builds (-DSET_PHASE_PROBE=1, tools/split_phase_probe.py with X2=0): wave 0 of block (tile 1, part 1) of diffnet_stack_split_kernel sums
// the s_memtime ticks of its phases over the layers and adds them to buf[0..7] (0 wait for the previous layer, 1 stage, 2 GEMM 1, 3 gate +
// z publish, 4 wait for z, 5 z load, 6 GEMM 2, 7 epilogue + publish)
SET_PHASE_PROBE_BUFFER(g_split_phase_buf, set_debug_split_phase_buffer)

namespace {

constexpr int DC = 256;       // residual_channels this kernel is specialised for
constexpr int NT = 64;        // frames per block tile
constexpr int KS1 = 3 * DC / 2;  // 384 k-steps (K=768) of GEMM 1
constexpr int KS2 = DC / 2;      // 128 k-steps (K=256) of GEMM 2

__device__ __forceinline__ int layer_row(int w, int rb, int i) {
    // rb 0,1 -> first half rows (gate / residual); rb 2,3 -> second half (filter / skip)
    return (rb < 2 ? 64 * w + 32 * rb : DC + 64 * w + 32 * (rb - 2)) + i;
}

// fast gate math: v_exp_f32 / v_rcp_f32 (<= 1-2 ulp each); absolute error ~1e-7, far inside the 1e-4 mel bar
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// One (layer, 32*NCB-frame tile) unit of work; shared by the per-layer kernel (NCB = 2) and the persistent stack
// kernel (NCB = 1 or 2).
struct LayerTile {
    const float *xin;      // x_in  + b*256*T
    float *xout;           // x_out + b*256*T
    float *skp;            // skip  + b*256*T
    const float *cpb;      // condproj slab of this layer + b*cp_bs
    const float *dstep;    // d[c] = dstep[c*d_cs]  (already offset by b*d_bs)
    int64_t d_cs;
    const float *w1p, *b_dil, *w2p, *b_out;
    int T, t0, dil, first;
    uint64_t *dbg = nullptr;  // probe builds, diffnet_layer_kernel: the block's 8 words of SetDiffnetLayerArgs.dbg_clock
    // Winograd kernel only: tile geometry over frame offsets q = -1 .. 64 from the tile start.  Frames q >= o belong
    // to the NEXT utterance (cross-utterance tiling of the concatenated frame axis; o = 1 << 20 when the tile lies
    // inside one utterance): slab pointers above are those of the first utterance, x_bs4 / cp_bs4 the byte strides to
    // the next one.  nvalid = frames of the tile that exist, halo_l / halo_r = frames q = -1 / q = 64 exist (and, for
    // q = -1, belong to the same utterance as q = 0).
    int o, nvalid, halo_l, halo_r;
    unsigned x_bs4, cp_bs4;
    float *sy, *sz;  // optional: slabs [512][T] / [256][T] receiving the pre-gate values and the gated activations
};

// pair index p (0..31) -> frame offset of its first output: blocks of 2d frames, (q, q + d) paired inside a block
__device__ __forceinline__ int wn_pair_q(int p, int d) { return 2 * d * (p / d) + (p % d); }

// frame offset q (already clamped into the valid range) -> byte offset inside the first utterance's row
__device__ __forceinline__ unsigned wn_voff(const LayerTile &a, int q, unsigned slab4) {
    const bool side = q >= a.o;
    return 4u * (unsigned)(a.t0 + q - (side ? a.T : 0)) + (side ? slab4 : 0u);
}

// AGENT: tile outputs are stored agent-scope write-through (persistent kernel: the publish then needs no release fence)
template <int NCB, int GS, bool AGENT = false>
__device__ __forceinline__ void layer_tile(const LayerTile &a, float *smem) {
    constexpr int NTt = 32 * NCB;           // frames per tile;  GS = k-steps per operand group
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int t0 = a.t0;
    const int dil = a.dil;
    const int XW = NTt + 2 * dil;  // tile width incl. halo
    const int T = a.T;
    const float *xin = a.xin;
    PhaseProbe<6> pp;  // wave 0: 0 tile staged, 1 GEMM 1, 2 gate, 3 barrier + z staged, 4 GEMM 2, 5 epilogue
    pp.start(a.dbg);

    // NB every global load below is UNCONDITIONAL on a clamped (always in-bounds) address and the validity
    // select happens afterwards: a `cond ? load : 0` makes hipcc branch around each load and drain vmcnt(0)
    // per element (128 serialized round trips per lane).
    // All global traffic goes through raw-buffer instructions: SGPR descriptor of the slab + SGPR row offset + ONE
    // per-lane byte offset shared by every row (hipcc otherwise builds a 64-bit VGPR address per load / store).
    unsigned lo[NCB];  // per-lane byte offsets (clamped) relative to a wave-uniform row
    bool tv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        lo[cb] = 4u * (unsigned)(4 * half * T + min(t0 + 32 * cb + l31, T - 1));
        tv[cb] = t0 + 32 * cb + l31 < T;
    }
    const unsigned lb = 16u * (unsigned)half;
    const unsigned T4 = 4u * (unsigned)T;
    const rsrc_t rxin = make_rsrc(xin), rskp = make_rsrc(a.skp), rxout = make_rsrc(a.xout), rcp = make_rsrc(a.cpb),
                 rbd = make_rsrc(a.b_dil), rbo = make_rsrc(a.b_out);

    // ---- phase 0a: accumulators of GEMM 1 start at  b_dil + condproj  (so the gate needs no loads later);
    //      all loads are independent and issued together.
    f32x16 acc[4][NCB];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ur = (unsigned)layer_row(w, rb, urow16(r));  // wave-uniform
            const float bias = buf_load(rbd, lb, 4u * ur);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[rb][cb][r] = bias + buf_load(rcp, lo[cb], ur * T4);
        }
    // ---- phase 0b: stage the (x + d) tile: wave w owns channels [64w, 64w+64); one row = one coalesced
    //      64-lane load (+ a halo load when the row is wider than 64); 16 rows in flight.  Zero outside [0,T):
    //      the conv's zero padding applies to x + d (diffnet.py:71,74).
    {
        const int tA = t0 - dil + lane;       // columns 0..63
        const int tB = t0 - dil + 64 + lane;  // columns 64..XW-1
        const bool vA = tA >= 0 && tA < T;
        const bool vB = tB >= 0 && tB < T;
        const unsigned cA = 4u * (unsigned)min(max(tA, 0), T - 1), cB = 4u * (unsigned)min(max(tB, 0), T - 1);
        const bool laneA = lane < XW;
        const bool laneB = 64 + lane < XW;
        for (int r0 = 0; r0 < 64; r0 += 16) {
            float xa[16], xb[16], dd[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int c = 64 * w + r0 + u;
                xa[u] = buf_load(rxin, cA, (unsigned)c * T4);
                if constexpr (NCB == 2) xb[u] = buf_load(rxin, cB, (unsigned)c * T4);
                dd[u] = a.dstep[(int64_t)c * a.d_cs];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int c = 64 * w + r0 + u;
                if (laneA) smem[c * XW + lane] = vA ? xa[u] + dd[u] : 0.0f;
                if constexpr (NCB == 2) {
                    if (laneB) smem[c * XW + 64 + lane] = vB ? xb[u] + dd[u] : 0.0f;
                }
            }
        }
    }
    __syncthreads();
    pp.lap(0);

    // ---- phase 1: GEMM 1  y[512 x NTt] += Wdil[512 x 768] * im2col(xs): k-step ks -> tap ks/128, channels 2*(ks%128)+{0,1}
    {
        const f32x4 *wp = reinterpret_cast<const f32x4 *>(a.w1p) + (int64_t)w * KS1 * 64 + lane;
        const float *bp = smem + half * XW + l31;
        const int rstep = 2 * XW;  // LDS floats between consecutive k-steps (2 channels)
        constexpr int GPT = 128 / GS;  // groups per tap
        gemm_groups<4, NCB, GS>(acc, wp, bp, rstep, KS1 / GS, [&](int g) {
            wp += GS * 64;
            bp += GS * rstep;
            if ((g % GPT) == GPT - 1) bp += dil - 128 * rstep;  // next tap: back to channel 0, shift by dil columns
        });
    }
    pp.lap(1);

    // ---- phase 2: gate, lane-local (acc[rb] pairs with acc[rb+2]); bias + conditioner are already inside -----
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const float z = fast_sigmoid(acc[rb][cb][r]) * fast_tanh(acc[rb + 2][cb][r]);
                acc[rb][cb][r] = tv[cb] ? z : 0.0f;
            }
    pp.lap(2);
    __syncthreads();  // every wave is done reading xs
    // z tile zs[256][NTt] overlays the xs tile
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = 64 * w + 32 * rb + mfma32_row(r, lane);
                smem[c * NTt + cb * 32 + l31] = acc[rb][cb][r];
            }
    // ---- accumulators of GEMM 2 start at  x_in + b_out  (residual rows) /  skip + b_out  (skip rows): the
    //      epilogue is then store-only and these loads fly while the other waves finish their z stores.
    __builtin_amdgcn_sched_barrier(0);  // z registers are dead from here: keep the init loads below the z stores
    const bool first = a.first != 0;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ur = (unsigned)layer_row(w, rb, urow16(r));  // wave-uniform
            const float bias = buf_load(rbo, lb, 4u * ur);
            // residual rows read x_in, skip rows read the running skip sum (ignored by a select when first)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const float sv = rb < 2 ? buf_load(rxin, lo[cb], ur * T4) : buf_load(rskp, lo[cb], (ur - DC) * T4);
                acc[rb][cb][r] = (rb >= 2 && first) ? bias : bias + sv;
            }
        }
        if (rb == 1) __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    pp.lap(3);

    // ---- phase 3: GEMM 2  o[512 x NTt] += Wout[512 x 256] * zs ------------------------------------------------
    {
        const f32x4 *wp = reinterpret_cast<const f32x4 *>(a.w2p) + (int64_t)w * KS2 * 64 + lane;
        const float *bp = smem + half * NTt + l31;
        constexpr int rstep = 2 * NTt;
        gemm_groups<4, NCB, GS>(acc, wp, bp, rstep, KS2 / GS, [&](int) {
            wp += GS * 64;
            bp += GS * rstep;
        });
    }
    pp.lap(4);

    // ---- phase 4: store-only epilogue: x_out = (x + o_res) * 2^-1/2 ; skip = skip + o_skip ----------------------
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        if (tv[cb]) {  // one exec-mask region per column block, not one per store (valid frame: the clamp was a no-op)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned ur = (unsigned)layer_row(w, rb, urow16(r));  // wave-uniform
                    const float v = acc[rb][cb][r] * (rb < 2 ? 0.70710678118654752440f : 1.0f);
                    const unsigned so = rb < 2 ? ur * T4 : (ur - DC) * T4;
                    if constexpr (AGENT) buf_store_agent(v, rb < 2 ? rxout : rskp, lo[cb], so);
                    else buf_store(v, rb < 2 ? rxout : rskp, lo[cb], so);
                }
        }
    }
    pp.lap(5);
    pp.flush(a.dbg);
}

__global__ void __launch_bounds__(256, 2) diffnet_layer_kernel(SetDiffnetLayerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.y;
    LayerTile lt;
    lt.xin = a.x_in + (int64_t)b * DC * a.T;
    lt.xout = a.x_out + (int64_t)b * DC * a.T;
    lt.skp = a.skip + (int64_t)b * DC * a.T;
    lt.cpb = a.condproj + (int64_t)b * a.cp_bs;
    lt.dstep = a.dstep + (int64_t)b * a.d_bs;
    lt.d_cs = a.d_cs;
    lt.w1p = a.w1p; lt.b_dil = a.b_dil; lt.w2p = a.w2p; lt.b_out = a.b_out;
    lt.T = a.T; lt.t0 = blockIdx.x * NT; lt.dil = a.dil; lt.first = a.first;
    lt.dbg = a.dbg_clock ? a.dbg_clock + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 : nullptr;
    layer_tile<2, 4>(lt, smem);
}

// ---- Winograd F(2,3) variant of the layer tile (dilation 1) -----------------------------------------------------
// y[n] = g0 x[n-1] + g1 x[n] + g2 x[n+1].  For an output pair (y0, y1) with inputs d0..d3 = x[n-1..n+2]:
//   m1 = (d0 - d2) g0          m2 = (d1 + d2) (g0 + g1 + g2)/2
//   m3 = (d2 - d1) (g0 - g1 + g2)/2      m4 = (d1 - d3) g2          y0 = m1 + m2 + m3,  y1 = m2 - m3 - m4
// i.e. four 512x256 GEMMs over 32 pair-columns instead of one 512x768 GEMM over 64 frames: 2/3 of the MACs of the
// k=3 conv, 3/4 of the layer.  512 threads = 8 waves (2 per SIMD, so each hides the other's operand loads), one
// block per CU, 64-frame tiles.  Wave w owns gate rows [32w,32w+32) and filter rows 256+[32w,32w+32): 2 x 4 planes
// x 16 = 128 accumulator VGPRs.  The input transform is computed on the fly from the RAW (x + d) tile in LDS (two
// ds_read_b64 + 4 VALU per k-step); the filter transform is folded into the packed weights; bias + conditioner
// projection are folded into the M1 / M4 accumulator init.  GEMM 2 and the epilogue are as in layer_tile<2>.
constexpr int WN_NT = 64;
constexpr int WN_MAXD = STACK_WINO_MAX_DIL;  // largest dilation (dilation_cycle_length <= 4)
constexpr int WN_XW = WN_NT + 2 * WN_MAXD;  // 64 frames + a halo of d on each side (d = 1: + the 2-column boundary gap)
constexpr int WN_KS = DC / 2;  // 128 k-steps (2 channels each) for every GEMM here
constexpr int WN_GS = 2;       // k-steps per operand group of GEMM 1

// The phases are split so the persistent kernel can order them around its dependency wait:
//   wino_init   - accumulator init from bias + conditioner projection (does NOT depend on the previous layer)
//   wino_main   - stage x, GEMM 1, gate, GEMM 2, epilogue
__device__ __forceinline__ void wino_init(const LayerTile &a, f32x16 (&m)[2][4]) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int T = a.T;
    // output pair j = l31 -> frame offsets q_e ("even" slot) and q_e + d: the F(2,3) pairing runs over frames that are
    // d apart (d = 1: 2j, 2j + 1); clamped to the last existing frame
    const int qe0 = wn_pair_q(l31, a.dil);
    const int qe = min(qe0, a.nvalid - 1), qo = min(qe0 + a.dil, a.nvalid - 1);
    const unsigned rowh = 16u * (unsigned)half * (unsigned)T;  // + 4*half rows
    const unsigned loe = rowh + wn_voff(a, qe, a.cp_bs4), loo = rowh + wn_voff(a, qo, a.cp_bs4);
    const unsigned lb = 16u * (unsigned)half;
    const rsrc_t rcp = make_rsrc(a.cpb), rb = make_rsrc(a.b_dil);
    // M1 <- b + cp(even), M4 <- -(b + cp(odd)), M2 = M3 = 0
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
        m[rf][1] = (f32x16){0};
        m[rf][2] = (f32x16){0};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ur = (unsigned)(rf * DC + 32 * w + urow16(r));  // wave-uniform
            const float bias = buf_load(rb, lb, 4u * ur);
            m[rf][0][r] = bias + buf_load(rcp, loe, 4u * ur * (unsigned)T);
            m[rf][3][r] = -(bias + buf_load(rcp, loo, 4u * ur * (unsigned)T));
        }
    }
}

// xs = smem[0 .. 256*68), zs = smem + WN_ZS_OFF (own region: no barrier between the last xs read and the zs write)
constexpr int WN_ZS_OFF = DC * WN_XW;

template <bool UNIT_DIL>  // UNIT_DIL: every layer has dilation 1 (compile-time, keeps the shipped configuration's inner loop lean)
__device__ __forceinline__ void wino_main(const LayerTile &a, f32x16 (&m)[2][4], float *smem, PhaseProbe<9> &pp, int *s_task,
                                          int claimed) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
    const int half = lane >> 5, l31 = lane & 31;
    const int t0 = a.t0, T = a.T;
    const unsigned T4 = 4u * (unsigned)T;
    float *zs = smem + WN_ZS_OFF;
    constexpr int XW = UNIT_DIL ? WN_NT + 4 : WN_XW;  // LDS row of the x tile (68 keeps the dilation-1 layout)
    const int d = UNIT_DIL ? 1 : a.dil, qe = UNIT_DIL ? 2 * l31 : wn_pair_q(l31, d);
    const bool tve = qe < a.nvalid, tvo = qe + d < a.nvalid;
    const rsrc_t rxin = make_rsrc(a.xin), rskp = make_rsrc(a.skp), rxout = make_rsrc(a.xout);

    // ---- stage the raw (x + d) tile xs[256][XW]; wave w owns channels [32w, 32w+32).  Frame offset q sits in column
    //      q + d (+ 2 when it belongs to the next utterance, d = 1 only): the two columns in between stay zero, so the
    //      last pair of one utterance and the first pair of the next both see the conv's zero padding.
    {
        const int qA = lane;                                         // columns of frames 0..63
        const int qB = lane < d ? lane - d : 64 + lane - d;          // lanes 0..2d-1: the halo frames -d..-1, 64..64+d-1
        const bool isB = lane < 2 * d;
        // halo frames exist iff they lie in the same utterance (or, right halo in concatenated mode, in the batch)
        const bool vA = qA < a.nvalid;
        const bool vB = isB && (qB < 0 ? (d == 1 ? a.halo_l != 0 : a.t0 + qB >= 0)
                                       : (d == 1 ? a.halo_r != 0 : a.t0 + qB < a.T));
        const unsigned cA = wn_voff(a, min(qA, a.nvalid - 1), a.x_bs4);
        const unsigned cB = vB ? wn_voff(a, qB, a.x_bs4) : cA;  // (invalid: any valid address, value unused)
        const int colA = qA + d + (qA >= a.o ? 2 : 0), colB = qB + d + (qB >= a.o ? 2 : 0);
        const bool gap = a.o <= 64;                     // an utterance boundary lies in (or at the end of) this tile
        for (int r0 = 0; r0 < 32; r0 += 16) {
            float xa[16], xb[16], dd[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int c = 32 * w + r0 + u;
                xa[u] = buf_load(rxin, cA, (unsigned)c * T4);
                xb[u] = buf_load(rxin, cB, (unsigned)c * T4);
                dd[u] = a.dstep[(int64_t)c * a.d_cs];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int c = 32 * w + r0 + u;
                smem[c * XW + colA] = vA ? xa[u] + dd[u] : 0.0f;
                if (isB) smem[c * XW + colB] = vB ? xb[u] + dd[u] : 0.0f;
                if (gap && lane >= 32 && lane < 34) smem[c * XW + a.o + lane - 31] = 0.0f;  // columns o+1, o+2
            }
        }
    }
    __syncthreads();
    pp.lap(1);

    // ---- GEMM 1 (Winograd): m[rf][p] += G_p[rows][c] * D_p[c][pair],  k-step = channels (2ks, 2ks+1)
    {
        const rsrc_t rw = make_rsrc(a.w1p);
        const unsigned wv = 32u * (unsigned)lane;                // 8 floats per lane per k-step
        unsigned ws = (unsigned)w * (WN_KS * 64 * 8 * 4);        // wave-uniform byte offset of the current group
        // inputs of pair (q_e, q_e + d): frames q_e - d, q_e, q_e + d, q_e + 2d = columns c0, c0 + d, c0 + 2d, c0 + 3d
        const float *bpf = smem + half * XW + qe + (qe >= a.o ? 2 : 0);
        const f32x2 *bp = reinterpret_cast<const f32x2 *>(bpf);  // d = 1: two aligned 8-byte reads
        struct Ops { f32x4 A[WN_GS][2]; f32x2 D[WN_GS][2]; };
        Ops P, Q;
        auto load_step = [&](Ops &o, int u) {
            o.A[u][0] = buf_load4(rw, wv, ws + (unsigned)u * 2048u);
            o.A[u][1] = buf_load4(rw, wv + 16u, ws + (unsigned)u * 2048u);
            if (UNIT_DIL) {
                o.D[u][0] = bp[u * XW];      // (d0, d1): row stride 2*XW floats = XW float2
                o.D[u][1] = bp[u * XW + 1];  // (d2, d3)
            } else {
                const float *q = bpf + u * 2 * XW;
                o.D[u][0] = (f32x2){q[0], q[d]};
                o.D[u][1] = (f32x2){q[2 * d], q[3 * d]};
            }
        };
        auto mma_step = [&](const Ops &o, int u) {
            const float d0 = o.D[u][0][0], d1 = o.D[u][0][1], d2 = o.D[u][1][0], d3 = o.D[u][1][1];
            const float D1 = d0 - d2, D2 = d1 + d2, D3 = d2 - d1, D4 = d1 - d3;
            __builtin_amdgcn_s_setprio(1);
            m[0][0] = mfma32(o.A[u][0][0], D1, m[0][0]);
            m[0][1] = mfma32(o.A[u][0][1], D2, m[0][1]);
            m[0][2] = mfma32(o.A[u][0][2], D3, m[0][2]);
            m[0][3] = mfma32(o.A[u][0][3], D4, m[0][3]);
            m[1][0] = mfma32(o.A[u][1][0], D1, m[1][0]);
            m[1][1] = mfma32(o.A[u][1][1], D2, m[1][1]);
            m[1][2] = mfma32(o.A[u][1][2], D3, m[1][2]);
            m[1][3] = mfma32(o.A[u][1][3], D4, m[1][3]);
            __builtin_amdgcn_s_setprio(0);
        };
        constexpr int NG = WN_KS / WN_GS;
#pragma unroll
        for (int u = 0; u < WN_GS; ++u) load_step(P, u);
        for (int g = 0; g < NG; g += 2) {
            ws += WN_GS * 2048u;
            bp += WN_GS * XW;
            bpf += WN_GS * 2 * XW;
#pragma unroll
            for (int u = 0; u < WN_GS; ++u) {
                load_step(Q, u);
                __builtin_amdgcn_sched_barrier(0);
                mma_step(P, u);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (g + 2 < NG) { ws += WN_GS * 2048u; bp += WN_GS * XW; bpf += WN_GS * 2 * XW; }
#pragma unroll
            for (int u = 0; u < WN_GS; ++u) {
                load_step(P, u);
                __builtin_amdgcn_sched_barrier(0);
                mma_step(Q, u);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    pp.lap(2);
    // ---- output transform + gate (lane-local): even frame y0 = M1 + M2 + M3, odd frame y1 = M2 - M3 - M4
    {
        const bool save = a.sy != nullptr;  // training forward: keep y (gate | filter rows) and z for the backward pass
        const rsrc_t rsy = make_rsrc(save ? a.sy : a.xin), rsz = make_rsrc(save ? a.sz : a.xin);
        const unsigned rowh_s = 16u * (unsigned)half * (unsigned)T;
        const unsigned se = rowh_s + wn_voff(a, min(qe, a.nvalid - 1), 0u), so_ = rowh_s + wn_voff(a, min(qe + d, a.nvalid - 1), 0u);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float g0 = m[0][0][r] + m[0][1][r] + m[0][2][r], g1 = m[0][1][r] - m[0][2][r] - m[0][3][r];
            const float f0 = m[1][0][r] + m[1][1][r] + m[1][2][r], f1 = m[1][1][r] - m[1][2][r] - m[1][3][r];
            const float z0 = tve ? fast_sigmoid(g0) * fast_tanh(f0) : 0.0f;
            const float z1 = tvo ? fast_sigmoid(g1) * fast_tanh(f1) : 0.0f;
            const int c = 32 * w + mfma32_row(r, lane);
            if (UNIT_DIL) {
                *reinterpret_cast<f32x2 *>(zs + c * WN_NT + qe) = (f32x2){z0, z1};
            } else {
                zs[c * WN_NT + qe] = z0;
                zs[c * WN_NT + qe + d] = z1;
            }
            if (save) {  // (uniform branch; the saved tensors are per utterance, so only the per-utterance tiling gets here)
                const unsigned ur = (unsigned)(32 * w + urow16(r));
                if (tve) {
                    buf_store(g0, rsy, se, ur * T4);
                    buf_store(f0, rsy, se, (ur + DC) * T4);
                    buf_store(z0, rsz, se, ur * T4);
                }
                if (tvo) {
                    buf_store(g1, rsy, so_, ur * T4);
                    buf_store(f1, rsy, so_, (ur + DC) * T4);
                    buf_store(z1, rsz, so_, ur * T4);
                }
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- put the residual / running-skip tiles in flight (m is dead now); they are consumed after GEMM 2
    const unsigned rowh = 16u * (unsigned)half * (unsigned)T;  // + 4*half rows
    const unsigned lo0 = rowh + wn_voff(a, min(l31, a.nvalid - 1), a.x_bs4), lo1 = rowh + wn_voff(a, min(32 + l31, a.nvalid - 1), a.x_bs4);
    const bool tv0 = l31 < a.nvalid, tv1 = 32 + l31 < a.nvalid;
    const bool first = a.first != 0;
    f32x16 prev[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ur = (unsigned)(32 * w + urow16(r));  // wave-uniform row of x (rb 0) / skip (rb 1)
            prev[rb][0][r] = buf_load(rb == 0 ? rxin : rskp, lo0, ur * T4);
            prev[rb][1][r] = buf_load(rb == 0 ? rxin : rskp, lo1, ur * T4);
        }
    __builtin_amdgcn_sched_barrier(0);

    // ---- GEMM 2: o[512 x 64] = Wout * zs; wave w owns residual rows [32w, +32) and skip rows 256 + [32w, +32)
    f32x16 acc[2][2];
    {
        const rsrc_t rbo = make_rsrc(a.b_out);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float bias = buf_load(rbo, 16u * (unsigned)half, 4u * (unsigned)(rb * DC + 32 * w + urow16(r)));
                acc[rb][0][r] = bias;
                acc[rb][1][r] = bias;
            }
    }
    if (tid == 0) s_task[0] = claimed;  // next task of this block, read by everyone after the epilogue
    __syncthreads();
    pp.lap(3);
    {
        const AVec<2>::type *wp = reinterpret_cast<const AVec<2>::type *>(a.w2p) + (int64_t)w * WN_KS * 64 + lane;
        const float *bp = zs + half * WN_NT + l31;
        constexpr int rstep = 2 * WN_NT;
        gemm_groups<2, 2, 8>(acc, wp, bp, rstep, WN_KS / 8, [&](int) {
            wp += 8 * 64;
            bp += 8 * rstep;
        });
    }
    pp.lap(4);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        if (cb == 0 ? tv0 : tv1) {
            const unsigned so = cb == 0 ? lo0 : lo1;  // valid frame: the clamp was a no-op
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned ur = (unsigned)(32 * w + urow16(r));
                    const float v = (rb == 1 && first) ? acc[rb][cb][r] : acc[rb][cb][r] + prev[rb][cb][r];
                    // agent-scope write-through (sc1): once vmcnt drains, the tile is visible to every XCD, so the
                    // publish needs no L2 write-back (a release fence = buffer_wbl2 of the whole XCD L2: -5 %)
                    buf_store_agent(v * (rb == 0 ? 0.70710678118654752440f : 1.0f), rb == 0 ? rxout : rskp, so, ur * T4);
                }
        }
    }
    pp.lap(5);
}

// ---- persistent layer stack: (layer, tile) task queue + per-tile epoch flags -----------------------------------
// Inter-workgroup hand-off follows cdna_hip_programming.md Guideline 16: producer = every wave drains vmcnt,
// __syncthreads, ONE lane agent-scope release fence + asm vmcnt(0) + relaxed agent flag store; consumer = ONE lane
// polls relaxed, ONE agent-scope acquire, __syncthreads, then plain loads.  Every spin is bounded (stack_wait: stack_queue.h).
template <int NCB, int GS, int WPS>
__global__ void __launch_bounds__(256, WPS) diffnet_stack_kernel(SetDiffnetStackArgs a, int tiles_per_utt, int ntiles,
                                                                int ntasks, int task_slot) {
    constexpr int NTt = 32 * NCB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int *s_task = reinterpret_cast<int *>(smem + task_slot);  // inside the ONE dynamic LDS array
    int *counter = a.sync_ws + SQ_COUNTER, *abort_flag = a.sync_ws + SQ_ABORT, *done = a.sync_ws + SQ_FLAGS;
    const int tid = threadIdx.x;
    uint64_t wait_ticks = 0, fence_ticks = 0;  // diagnostics (lane 0 only): summed into SQ_WAIT_TICKS, SQ_FENCE_TICKS
    for (;;) {
        __syncthreads();  // LDS (tile + task slot) of the previous task is free
        if (tid == 0) {
            const uint64_t tw0 = __builtin_amdgcn_s_memtime();
            int n = atomicAdd(counter, 1);
            if (n < ntasks && n >= ntiles) {  // layer >= 1: wait for the three producer tiles of layer l-1
                const int l = n / ntiles, i = n - l * ntiles, j = i % tiles_per_utt;
                const int *f0 = done + i, *fl = done + (j > 0 ? i - 1 : i), *fr = done + (j < tiles_per_utt - 1 ? i + 1 : i);
                n = stack_wait_tiles(f0, fl, fr, l, abort_flag, a.err_flag, n, ntasks);
            }
            wait_ticks += __builtin_amdgcn_s_memtime() - tw0;
            *s_task = n;
        }
        __syncthreads();
        const int n = __builtin_amdgcn_readfirstlane(*s_task);
        if (n >= ntasks) {
            if (tid == 0) {  // units of 1024 ticks
                atomicAdd(a.sync_ws + SQ_WAIT_TICKS, (int)(wait_ticks >> 10));
                atomicAdd(a.sync_ws + SQ_FENCE_TICKS, (int)(fence_ticks >> 10));
            }
            break;
        }
        const int l = n / ntiles, i = n - l * ntiles;
        const int b = i / tiles_per_utt, j = i - b * tiles_per_utt;
        LayerTile lt;
        const float *xi = (l & 1) ? a.xb : a.xa;
        float *xo = (l & 1) ? a.xa : a.xb;
        lt.xin = xi + (int64_t)b * DC * a.T;
        lt.xout = xo + (int64_t)b * DC * a.T;
        lt.skp = a.skip + (int64_t)b * DC * a.T;
        lt.cpb = a.condproj + (int64_t)l * a.cp_ls + (int64_t)b * a.cp_bs;
        lt.dstep = a.dstep + (int64_t)l * a.d_ls + (int64_t)b * a.d_bs;
        lt.d_cs = a.d_cs;
        lt.w1p = a.w1p_all + (int64_t)l * (512 * 768);
        lt.w2p = a.w2p_all + (int64_t)l * (512 * 256);
        lt.b_dil = a.b_dil_all + (int64_t)l * 512;
        lt.b_out = a.b_out_all + (int64_t)l * 512;
        lt.T = a.T; lt.t0 = j * NTt; lt.dil = 1 << (l % a.dilation_cycle_length); lt.first = (l == 0);
        layer_tile<NCB, GS, true>(lt, smem);
        // publish tile i of layer l (outputs were stored agent-scope write-through: vmcnt drain = visible to every XCD)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
        __syncthreads();
        if (tid == 0) {
            const uint64_t tf0 = __builtin_amdgcn_s_memtime();
            stack_publish_store(done, i, l, STACK_NO_FAULT_TILE, false);
            fence_ticks += __builtin_amdgcn_s_memtime() - tf0;
        }
    }
}

// ---- small batches: every 32-frame tile split over FOUR co-operating blocks ---------------------------------------
// With a handful of utterances a layer has fewer tiles than the chip has CUs (B = 1, T = 800: 25 tiles on 256 CUs) and
// the time of a layer is the time of ONE tile on ONE CU: 4 row blocks x 512 MFMAs per SIMD.  Here block (tile i, part h)
// does the work of wave h of layer_tile<1>, one 32-row block per wave (wave j < 2: gate rows 64h + 32j.., then residual
// rows; j >= 2: the matching filter rows, then skip rows), i.e. a quarter of the MFMA chain per SIMD on four times as
// many CUs.  Blocks are bound to their (tile, part) for all L layers (grid = 4 x tiles, all co-resident) and meet twice
// per layer through agent-scope counters:
//   zcnt[i]  += 1 once the part's gated rows z[64h .. 64h+63] are stored (agent-scope write-through) to the tile's slot
//               of z_ws; GEMM 2 of every part reads all 256 rows after zcnt[i] reached 4 (l + 1);
//   ready[i] += 1 once the part's rows of x' are stored; layer l + 1 of tiles i-1, i, i+1 starts at ready >= 4 (l + 1).
// Every output element sees the same accumulation chain as in layer_tile (same initial value, same k order), the gate
// is the same product of the same two values (the tanh factor crosses from the filter wave to the gate wave through
// LDS): results are bit-identical to the direct kernels.  Weight images: one float per lane per k-step and 32-row block
// ([16][KS][64], set_diffnet_stack's w1s_all / w2s_all).
constexpr int SP_XW = 32 + 2 * WN_MAXD;      // widest x tile (d = 8)
constexpr int SP_LDS_FLOATS = DC * SP_XW + 64 * 32 + 4;

// GEMM of the row-split kernel: ONE 32x32 accumulator per wave, so one MFMA (64 cycles) per k-step and nothing else in
// the wave to hide operand latency behind.  The weight images are cold in L2 at every layer (2 MiB per layer, read once per
// XCD), i.e. A comes from the memory side at ~1.5-2 us: A is prefetched 64 k-steps ahead (two sets of 64 registers,
// ping-pong; the first set is loaded by split_preload BEFORE the inter-block wait that precedes the GEMM), B (LDS) 4 ahead.
//   A k-step ks: wp[ks * 64];  B k-step ks: *bq, bq += rstep per k-step, += tap_jump after every 128th (next conv tap)
__device__ __forceinline__ void split_preload(float (&A)[64], const float *wp) {
#pragma unroll
    for (int u = 0; u < 64; ++u) A[u] = wp[u * 64];
}

template <int KS>
__device__ __forceinline__ void split_gemm(f32x16 &acc, const float *wp, float (&Ap)[64], const float *bq, int rstep,
                                           int tap_jump) {
    static_assert(KS % 128 == 0, "two 64-k-step sets per iteration");
    float Aq[64], Bv[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        Bv[u] = *bq;
        bq += rstep;
    }
    for (int g = 0; g < KS / 64; g += 2) {
        const float *wq = wp + (int64_t)(g + 1) * 64 * 64;
#pragma unroll
        for (int u = 0; u < 64; ++u) {  // k-steps 64 g + u (g even: no tap boundary among the B prefetches of this half)
            Aq[u] = wq[u * 64];
            Bv[(u + 4) & 7] = *bq;
            bq += rstep;
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma32(Ap[u], Bv[u & 7], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
        const float *wn = wp + (int64_t)(g + 2 < KS / 64 ? g + 2 : g) * 64 * 64;  // last pair: harmless re-load
#pragma unroll
        for (int u = 0; u < 64; ++u) {  // k-steps 64 (g + 1) + u; the prefetch of k-step 64 (g + 2) starts the next tap
            Ap[u] = wn[u * 64];
            Bv[(u + 4) & 7] = *bq;  // (past the last k-step: a harmless read inside the tile)
            bq += rstep;
            if (u == 59) bq += tap_jump;
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma32(Aq[u], Bv[u & 7], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}


__global__ void __launch_bounds__(256, 2) diffnet_stack_split_kernel(SetDiffnetStackArgs a, int tiles_per_utt, int ntiles,
                                                                    int fault_tile) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // x tile [256][32 + 2d]; the z tile [256][32] overlays it
    float *gs = smem + DC * SP_XW;                                // [64][32] tanh(filter rows) of this part
    int *s_ok = reinterpret_cast<int *>(gs + 64 * 32);
    int *abort_flag = a.sync_ws + SQ_ABORT, *ready = a.sync_ws + SQ_FLAGS, *zcnt = a.sync_ws + sq_flags2(ntiles);
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int j = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = blockIdx.x >> 2, h = blockIdx.x & 3;
    const int b = i / tiles_per_utt, jt = i - b * tiles_per_utt;
    const int T = a.T, t0 = jt * 32;
    const int il = jt > 0 ? i - 1 : i, ir = jt < tiles_per_utt - 1 ? i + 1 : i;
    const unsigned T4 = 4u * (unsigned)T;
    const unsigned lo = 4u * (unsigned)(4 * half * T + min(t0 + l31, T - 1));  // per-lane byte offset, clamped
    const bool tv = t0 + l31 < T;
    const unsigned lb = 16u * (unsigned)half;
    const rsrc_t rz = make_rsrc(a.z_ws + (int64_t)i * (DC * 32));
    const rsrc_t rskp = make_rsrc(a.skip + (int64_t)b * DC * T);
    const int vr = 4 * h + j;  // 32-row block of the images
    PhaseProbe<8> pp;
    pp.start(g_split_phase_buf && blockIdx.x == 5);
    for (int l = 0; l < a.L; ++l) {
        const int dil = 1 << (l % a.dilation_cycle_length), XW = 32 + 2 * dil;
        const rsrc_t rxin = make_rsrc(((l & 1) ? a.xb : a.xa) + (int64_t)b * DC * T);
        const rsrc_t rxout = make_rsrc(((l & 1) ? a.xa : a.xb) + (int64_t)b * DC * T);
        const rsrc_t rcp = make_rsrc(a.condproj + (int64_t)l * a.cp_ls + (int64_t)b * a.cp_bs);
        const rsrc_t rbd = make_rsrc(a.b_dil_all + (int64_t)l * 512), rbo = make_rsrc(a.b_out_all + (int64_t)l * 512);
        const float *dstep = a.dstep + (int64_t)l * a.d_ls + (int64_t)b * a.d_bs;
        // ---- GEMM 1 accumulator = b_dil + conditioner projection: independent of the previous layer, issued before the wait
        f32x16 acc[1][1];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ur = (unsigned)layer_row(h, j, urow16(r));  // wave-uniform
            acc[0][0][r] = buf_load(rbd, lb, 4u * ur) + buf_load(rcp, lo, ur * T4);
        }
        float Ap[64];  // first 64 k-steps of the wave's weight rows (cold in L2): in flight during the wait and the staging
        const float *wp1 = a.w1s_all + (int64_t)l * (512 * 768) + (int64_t)vr * KS1 * 64 + lane;
        split_preload(Ap, wp1);
        if (tid == 0) *s_ok = l == 0 ? 1 : stack_wait_parts(ready + i, ready + il, ready + ir, 4 * l, abort_flag, a.err_flag, true);
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(*s_ok) == 0) return;
        pp.lap(0);
        // ---- stage x + d (wave j: channels 64j .. 64j+63; zero outside [0, T): the conv pads x + d).  All 64 row loads
        //      of the wave are in flight at once: one memory round trip
        {
            const int tA = t0 - dil + lane;
            const bool vA = tA >= 0 && tA < T, laneA = lane < XW;
            const unsigned cA = 4u * (unsigned)min(max(tA, 0), T - 1);
            float xa[64];
            // step offsets d[c] of the wave's 64 channels: ONE gather (lane u <-> channel 64j + u, stride d_cs: a table
            // column per diffusion step), broadcast per row with v_readlane -- 64 dependent scalar loads would serialise
            const float dv = dstep[(int64_t)(64 * j + lane) * a.d_cs];
#pragma unroll
            for (int u = 0; u < 64; ++u) xa[u] = buf_load(rxin, cA, (unsigned)(64 * j + u) * T4);
#pragma unroll
            for (int u = 0; u < 64; ++u) {
                const float dd = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dv), u));
                if (laneA) smem[(64 * j + u) * XW + lane] = vA ? xa[u] + dd : 0.0f;
            }
        }
        __syncthreads();
        pp.lap(1);
        // ---- GEMM 1: one 32-row block of  y = Wdil (*) (x + d)
        split_gemm<KS1>(acc[0][0], wp1, Ap, smem + half * XW + l31, 2 * XW, dil - 128 * 2 * XW);
        pp.lap(2);
        // ---- gate: the filter waves hand tanh(y_f) to the gate waves through LDS
        if (j >= 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) gs[(32 * (j - 2) + mfma32_row(r, lane)) * 32 + l31] = fast_tanh(acc[0][0][r]);
        }
        __syncthreads();  // gs complete; every wave is done reading the x tile
        if (j < 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float z = fast_sigmoid(acc[0][0][r]) * gs[(32 * j + mfma32_row(r, lane)) * 32 + l31];
                buf_store_agent(tv ? z : 0.0f, rz, 4u * (unsigned)(4 * half * 32 + l31),
                                4u * 32u * (unsigned)(64 * h + 32 * j + urow16(r)));
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the z rows of this wave are visible to every XCD
        __syncthreads();
        if (tid == 0) stack_publish_add(zcnt, i, l, fault_tile, false);
        pp.lap(3);
        // ---- GEMM 2 accumulator = b_out + x (residual rows) / + running skip sum (skip rows): these rows were written
        //      by this very wave one layer ago; the loads fly while lane 0 waits for the other parts' z rows
        {
            // rows 64h + 32(j & 1) + .. of x (gate waves) or of the skip sum (filter waves): one descriptor, no per-row branch
            const rsrc_t rsv = make_rsrc(j < 2 ? ((l & 1) ? a.xb : a.xa) + (int64_t)b * DC * T : a.skip + (int64_t)b * DC * T);
            float bias[16], sv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                bias[r] = buf_load(rbo, lb, 4u * (unsigned)layer_row(h, j, urow16(r)));
                sv[r] = buf_load(rsv, lo, (unsigned)(64 * h + 32 * (j & 1) + urow16(r)) * T4);
            }
            if (j >= 2 && l == 0) {  // first layer: the skip sum starts here (whatever the buffer held is ignored)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][0][r] = bias[r];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][0][r] = bias[r] + sv[r];
            }
        }
        const float *wp2 = a.w2s_all + (int64_t)l * (512 * 256) + (int64_t)vr * KS2 * 64 + lane;
        split_preload(Ap, wp2);
        if (tid == 0) *s_ok = stack_wait_parts(zcnt + i, zcnt + i, zcnt + i, 4 * (l + 1), abort_flag, a.err_flag, true);
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(*s_ok) == 0) return;
        pp.lap(4);
        // ---- the whole z tile [256][32] (one contiguous 32 KiB slot) -> LDS, same layout
        {
            f32x4 zv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) zv[k] = buf_load4(rz, 16u * (unsigned)tid, 4096u * (unsigned)k);
#pragma unroll
            for (int k = 0; k < 8; ++k) *reinterpret_cast<f32x4 *>(smem + 4 * tid + 1024 * k) = zv[k];
        }
        __syncthreads();
        pp.lap(5);
        // ---- GEMM 2: one 32-row block of  o = Wout z
        split_gemm<KS2>(acc[0][0], wp2, Ap, smem + half * 32 + l31, 64, 0);
        pp.lap(6);
        // ---- epilogue: x' = (x + o_res) / sqrt 2 (agent scope: the neighbours' next layer reads it), skip += o_skip
        if (tv && j < 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                buf_store_agent(acc[0][0][r] * 0.70710678118654752440f, rxout, lo, (unsigned)layer_row(h, j, urow16(r)) * T4);
        } else if (tv) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                buf_store(acc[0][0][r], rskp, lo, (unsigned)(layer_row(h, j, urow16(r)) - DC) * T4);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // every store of the block has completed; the LDS tile is free for the next layer
        if (tid == 0) stack_publish_add(ready, i, l, fault_tile, h == 0);
        pp.lap(7);
    }
    pp.flush(g_split_phase_buf);
}

// Winograd flavour of the persistent kernel: 512 threads, one block per CU, 64-frame tiles.  Same queue and flags
// as above, but each block claims its NEXT task while the current one is in GEMM 2, and issues the next task's
// producer-independent loads (bias + conditioner projection -> accumulator init) BEFORE it waits for the producer
// tiles, so that wait, the store drain and the release fence of the previous task overlap with them.  Claiming
// ahead is deadlock-free: a block finishes its claims in claim order, and a claim only ever waits on earlier ones.
template <bool UNIT_DIL>  // separate kernels: the dilation-1 one carries none of the dilated-layer code or registers
__global__ void __launch_bounds__(512, 2) diffnet_stack_wino_kernel(SetDiffnetStackArgs a, int tiles_per_utt, int ntiles,
                                                                    int ntasks, int concat, int fault_tile) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int *s_task = reinterpret_cast<int *>(smem + WN_ZS_OFF + DC * WN_NT);
    int *counter = a.sync_ws + SQ_COUNTER, *abort_flag = a.sync_ws + SQ_ABORT, *done = a.sync_ws + SQ_FLAGS;
    const int tid = threadIdx.x;
    uint64_t wait_ticks = 0, fence_ticks = 0;
    if (tid == 0) s_task[0] = atomicAdd(counter, 1);
    __syncthreads();
    int n = __builtin_amdgcn_readfirstlane(s_task[0]);
    int l = 0, i = 0, j = 0;
    LayerTile lt;
    auto decode = [&](int task) {
        l = task / ntiles;
        i = task - l * ntiles;
        int b;
        if (concat) {  // tile i covers frames [64 i, 64 i + 64) of the concatenated axis; tiles_per_utt == ntiles, j == i
            const int64_t f0 = (int64_t)WN_NT * i, F = (int64_t)a.B * a.T;
            b = (int)(f0 / a.T);
            j = i;
            lt.t0 = (int)(f0 - (int64_t)b * a.T);
            lt.o = (a.T - lt.t0 <= WN_NT && b + 1 < a.B) ? a.T - lt.t0 : (1 << 20);
            lt.nvalid = (int)min((int64_t)WN_NT, (b + 1 < a.B ? F : (int64_t)(b + 1) * a.T) - f0);
            lt.halo_l = lt.t0 > 0;
            lt.halo_r = f0 + WN_NT < F;
        } else {
            b = i / tiles_per_utt;
            j = i - b * tiles_per_utt;
            lt.t0 = j * WN_NT;
            lt.o = 1 << 20;
            lt.nvalid = min(WN_NT, a.T - lt.t0);
            lt.halo_l = lt.t0 > 0;
            lt.halo_r = lt.t0 + WN_NT < a.T;
        }
        lt.x_bs4 = 4u * (unsigned)DC * (unsigned)a.T;
        lt.cp_bs4 = 4u * (unsigned)a.cp_bs;
        const int64_t slab = (int64_t)a.B * DC * a.T;
        const float *xi = a.x_all ? a.x_all + l * slab : ((l & 1) ? a.xb : a.xa);
        float *xo = a.x_all ? a.x_all + (l + 1) * slab : ((l & 1) ? a.xa : a.xb);
        lt.xin = xi + (int64_t)b * DC * a.T;
        lt.xout = xo + (int64_t)b * DC * a.T;
        lt.skp = a.skip + (int64_t)b * DC * a.T;
        lt.sy = a.save_y ? a.save_y + 2 * l * slab + (int64_t)b * 2 * DC * a.T : nullptr;
        lt.sz = a.save_z ? a.save_z + l * slab + (int64_t)b * DC * a.T : nullptr;
        lt.cpb = a.condproj + (int64_t)l * a.cp_ls + (int64_t)b * a.cp_bs;
        lt.dstep = a.dstep + (int64_t)l * a.d_ls + (int64_t)b * a.d_bs;
        lt.d_cs = a.d_cs;
        lt.w1p = a.w1w_all + (int64_t)l * (512 * 256 * 4);
        lt.w2p = a.w2w_all + (int64_t)l * (512 * 256);
        lt.b_dil = a.b_dil_all + (int64_t)l * 512;
        lt.b_out = a.b_out_all + (int64_t)l * 512;
        lt.T = a.T; lt.dil = UNIT_DIL ? 1 : 1 << (l % a.dilation_cycle_length); lt.first = (l == 0);
    };
    // probe builds (-DSET_PHASE_PROBE=1, tools/wino_probe.py with WINO_PHASES=1): wave 0 of every block adds its phase sums, in units of 1024
    // ticks, to the 9 words behind the flags: 0 init loads + vmcnt drain, 6 barrier, 8 flag / dependency wait / claim + barrier, 1 stage,
    // 2 GEMM 1, 3 gate.., 4 GEMM 2, 5 epilogue
    PhaseProbe<9> pp;
    pp.start(true);
    int i_done = -1, l_done = 0;  // finished but not yet published tile of this block
    auto publish = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
        pp.lap(0);
        __syncthreads();
        pp.lap(6);
        if (tid == 0 && i_done >= 0) {
            const uint64_t tf0 = __builtin_amdgcn_s_memtime();
            // no release fence: the tile's stores are agent-scope write-through (wino_main's epilogue), drained above
            stack_publish_store(done, i_done, l_done, fault_tile);
            fence_ticks += __builtin_amdgcn_s_memtime() - tf0;
        }
    };
    while (n < ntasks) {
        decode(n);
        f32x16 m[2][4];
        wino_init(lt, m);  // issued before the previous tile's store drain / publish and before the dependency wait
        __builtin_amdgcn_sched_barrier(0);
        publish();
        int claimed = 0;
        if (tid == 0) {
            int ok_all = 1;
            if (l > 0) {
                const uint64_t tw0 = __builtin_amdgcn_s_memtime();
                const int *f0 = done + i, *fl = done + (j > 0 ? i - 1 : i), *fr = done + (j < tiles_per_utt - 1 ? i + 1 : i);
                ok_all = stack_wait_tiles(f0, fl, fr, l, abort_flag, a.err_flag);
                wait_ticks += __builtin_amdgcn_s_memtime() - tw0;
            }
            s_task[1] = ok_all;
            claimed = atomicAdd(counter, 1);  // claim the next task; the result is only needed after GEMM 1
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(s_task[1]) == 0) {
            i_done = -1;
            break;
        }
        pp.lap(8);
        wino_main<UNIT_DIL>(lt, m, smem, pp, s_task, claimed);
        i_done = i;
        l_done = l;
        n = __builtin_amdgcn_readfirstlane(s_task[0]);  // written by thread 0 before the barrier in front of GEMM 2
    }
    publish();
    pp.flush_atomic(a.sync_ws + sq_flags2(ntiles));
    if (tid == 0) {  // units of 1024 ticks
        atomicAdd(a.sync_ws + SQ_WAIT_TICKS, (int)(wait_ticks >> 10));
        atomicAdd(a.sync_ws + SQ_FENCE_TICKS, (int)(fence_ticks >> 10));
    }
}

// blockIdx.y = layer q of a stack: weights at w_dil + q wd_ls / w_out + q wo_ls (element strides), images at q * (their per-layer size)
__global__ void __launch_bounds__(256) pack_diffnet_layer_kernel(const float *w_dil, const float *w_out, float *w1p,
                                                                 float *w2p, int64_t wd_ls = 0, int64_t wo_ls = 0) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n1 = (int64_t)4 * KS1 * 64 * 4, n2 = (int64_t)4 * KS2 * 64 * 4;
    w_dil += (int64_t)blockIdx.y * wd_ls;
    w_out += (int64_t)blockIdx.y * wo_ls;
    w1p += (int64_t)blockIdx.y * n1;
    w2p += (int64_t)blockIdx.y * n2;
    if (idx < n1) {
        const int rb = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        const int ks = (int)((idx >> 8) % KS1), w = (int)((idx >> 8) / KS1);
        const int tap = ks >> 7, cp = ks & 127;
        const int row = layer_row(w, rb, lane & 31), c = 2 * cp + (lane >> 5);
        w1p[idx] = w_dil[((int64_t)row * DC + c) * 3 + tap];
    } else if (idx < n1 + n2) {
        const int64_t j = idx - n1;
        const int rb = (int)(j & 3), lane = (int)((j >> 2) & 63);
        const int ks = (int)((j >> 8) % KS2), w = (int)((j >> 8) / KS2);
        const int row = layer_row(w, rb, lane & 31), c = 2 * ks + (lane >> 5);
        w2p[j] = w_out[(int64_t)row * DC + c];
    }
}

// Winograd images: w1w[w][ks][lane][rf*4 + p] = G_p(Wdil[rf*256 + 32w + (lane&31)][2ks + (lane>>5)][0..2]),
//                  w2w[w][ks][lane][rb]       = Wout[rb*256 + 32w + (lane&31)][2ks + (lane>>5)]          (8 waves)
__global__ void __launch_bounds__(256) pack_diffnet_wino_kernel(const float *w_dil, const float *w_out, float *w1w,
                                                                float *w2w, int64_t wd_ls = 0, int64_t wo_ls = 0) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n1 = (int64_t)8 * WN_KS * 64 * 8, n2 = (int64_t)8 * WN_KS * 64 * 2;
    w_dil += (int64_t)blockIdx.y * wd_ls;  // (blockIdx.y = layer, as in pack_diffnet_layer_kernel)
    w_out += (int64_t)blockIdx.y * wo_ls;
    w1w += (int64_t)blockIdx.y * n1;
    w2w += (int64_t)blockIdx.y * n2;
    if (idx < n1) {
        const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
        const int ks = (int)((idx >> 9) % WN_KS), w = (int)((idx >> 9) / WN_KS);
        const int rf = e >> 2, p = e & 3;
        const int row = rf * DC + 32 * w + (lane & 31), c = 2 * ks + (lane >> 5);
        const float *g = w_dil + ((int64_t)row * DC + c) * 3;
        const double g0 = g[0], g1 = g[1], g2 = g[2];
        const double v = p == 0 ? g0 : (p == 1 ? 0.5 * (g0 + g1 + g2) : (p == 2 ? 0.5 * (g0 - g1 + g2) : g2));
        w1w[idx] = (float)v;
    } else if (idx < n1 + n2) {
        const int64_t j = idx - n1;
        const int rb = (int)(j & 1), lane = (int)((j >> 1) & 63);
        const int ks = (int)((j >> 7) % WN_KS), w = (int)((j >> 7) / WN_KS);
        const int row = rb * DC + 32 * w + (lane & 31), c = 2 * ks + (lane >> 5);
        w2w[j] = w_out[(int64_t)row * DC + c];
    }
}

}  // namespace

extern "C" int64_t set_diffnet_w1w_size(void) { return (int64_t)512 * 256 * 4; }
extern "C" int set_pack_diffnet_layer_wino(const float *w_dil, const float *w_out, float *w1w, float *w2w, void *stream) {
    SET_REQUIRE(w_dil && w_out && w1w && w2w, "set_pack_diffnet_layer_wino");
    const int64_t total = set_diffnet_w1w_size() + (int64_t)512 * 256;
    hipLaunchKernelGGL(pack_diffnet_wino_kernel, dim3(set_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, w_dil,
                       w_out, w1w, w2w);
    return set_check_launch("set_pack_diffnet_layer_wino");
}

extern "C" int64_t set_diffnet_w1p_size(void) { return (int64_t)512 * 768; }
extern "C" int64_t set_diffnet_w2p_size(void) { return (int64_t)512 * 256; }

// every layer of a stack in one launch per image family (the training forward re-packs all of them after each optimizer step: 2 x L
// launches of ~5 us otherwise).  Layer q's weights at w_dil + q wd_ls / w_out + q wo_ls (the flat optimizer's layout: one stride between
// the layers' tensors); w1p / w2p are [L][set_diffnet_w1p_size()] / [L][set_diffnet_w2p_size()], w1w / w2w (optional, both or neither) the
// Winograd images [L][set_diffnet_w1w_size()] / [L][512 * 256].
extern "C" int set_pack_diffnet_layers(const float *w_dil, const float *w_out, int64_t wd_ls, int64_t wo_ls, float *w1p, float *w2p,
                                       float *w1w, float *w2w, int32_t L, void *stream) {
    SET_REQUIRE(w_dil && w_out && w1p && w2p && L > 0 && L <= 65535 && (w1w == nullptr) == (w2w == nullptr), "set_pack_diffnet_layers");
    SET_REQUIRE((int64_t)8 * WN_KS * 64 * 8 == set_diffnet_w1w_size() && (int64_t)8 * WN_KS * 64 * 2 == (int64_t)512 * 256 &&
                    (int64_t)4 * KS1 * 64 * 4 == set_diffnet_w1p_size() && (int64_t)4 * KS2 * 64 * 4 == set_diffnet_w2p_size(),
                "set_pack_diffnet_layers(image sizes)");
    const int64_t total = set_diffnet_w1p_size() + set_diffnet_w2p_size();
    hipLaunchKernelGGL(pack_diffnet_layer_kernel, dim3(set_blocks(total, 256), L), dim3(256), 0, (hipStream_t)stream, w_dil, w_out, w1p,
                       w2p, wd_ls, wo_ls);
    int rc = set_check_launch("set_pack_diffnet_layers");
    if (rc != SET_OK || w1w == nullptr) return rc;
    const int64_t totw = set_diffnet_w1w_size() + (int64_t)512 * 256;
    hipLaunchKernelGGL(pack_diffnet_wino_kernel, dim3(set_blocks(totw, 256), L), dim3(256), 0, (hipStream_t)stream, w_dil, w_out, w1w,
                       w2w, wd_ls, wo_ls);
    return set_check_launch("set_pack_diffnet_layers(wino)");
}
extern "C" int set_pack_diffnet_layer(const float *w_dil, const float *w_out, float *w1p, float *w2p, void *stream) {
    SET_REQUIRE(w_dil && w_out && w1p && w2p, "set_pack_diffnet_layer");
    const int64_t total = set_diffnet_w1p_size() + set_diffnet_w2p_size();
    hipLaunchKernelGGL(pack_diffnet_layer_kernel, dim3(set_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       w_dil, w_out, w1p, w2p);
    return set_check_launch("set_pack_diffnet_layer");
}

extern "C" int set_diffnet_layer(const SetDiffnetLayerArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_diffnet_layer");
    const SetDiffnetLayerArgs &a = *args;
    SET_REQUIRE(a.x_in && a.condproj && a.dstep && a.w1p && a.b_dil && a.w2p && a.b_out && a.x_out && a.skip,
                "set_diffnet_layer");
    SET_REQUIRE(a.B > 0 && a.T > 0 && a.dil >= 1, "set_diffnet_layer");
    SET_REQUIRE(a.x_in != a.x_out, "set_diffnet_layer(x_in must not alias x_out)");
    if (a.dil > 8) return set_fail(SET_E_UNSUPPORTED, "set_diffnet_layer", "dilation > 8 (LDS tile > 80 KiB)");
    if (a.dbg_clock && !SET_PHASE_PROBE) return set_fail(SET_E_UNSUPPORTED, "set_diffnet_layer(dbg_clock)", "library built without -DSET_PHASE_PROBE");
    const size_t lds = (size_t)DC * (NT + 2 * a.dil) * sizeof(float);
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, 96 * 1024, "set_diffnet_layer(attr)", diffnet_layer_kernel)) return rc;
    dim3 grid((a.T + NT - 1) / NT, a.B);
    hipLaunchKernelGGL(diffnet_layer_kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
    return set_check_launch("set_diffnet_layer");
}


extern "C" int64_t set_sizeof_diffnet_stack_args(void) { return (int64_t)sizeof(SetDiffnetStackArgs); }
extern "C" int64_t set_sizeof_diffnet_layer_args(void) { return (int64_t)sizeof(SetDiffnetLayerArgs); }

// the fp32-pipe stack kernels (families 0 - 3 of the plan; the row-split one here is the fp32 launch, p.split_x2 goes to csrc/diffnet_x3.hip)
int set_launch_diffnet_stack_f32(const SetDiffnetStackArgs &a, const StackPlan &p, hipStream_t s) {
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, 150 * 1024, "set_diffnet_stack(attr)", diffnet_stack_kernel<1, 8, 2>, diffnet_stack_kernel<2, 4, 2>,
                               diffnet_stack_wino_kernel<true>, diffnet_stack_wino_kernel<false>, diffnet_stack_split_kernel))
        return rc;
    if (p.family == STACK_ROW_SPLIT) {
        const int tiles = (a.T + 31) / 32, nt = a.B * tiles;
        SET_HIP(set_zero_async(a.sync_ws, stack_sync_words(SQ_ROW_SPLIT, nt) * sizeof(int32_t), s), "set_diffnet_stack(memset)");
        hipLaunchKernelGGL(diffnet_stack_split_kernel, dim3(4 * nt), dim3(256), (size_t)SP_LDS_FLOATS * sizeof(float), s, a,
                           tiles, nt, stack_fault_tile());
        return set_check_launch("set_diffnet_stack");
    }
    // Tile width: a task (l, i) needs tiles i-1..i+1 of layer l-1, so at most `tiles per layer` tasks are ever
    // runnable.  Workers (2 per CU) must stay BELOW that or the youngest ones only wait (measured: 36 % wait time
    // with 512 workers on 416 64-frame tiles).  Use 64-frame tiles when a layer has >= 1.5x the workers, else
    // 32-frame tiles (B=32, T=800: 800 tiles, no tail waste); the grid is capped at 0.8x the tile count.
    const bool wino = p.family == STACK_WINO;
    const int ncb = p.family == STACK_DIRECT32 ? 1 : 2;
    const int ntt = 32 * ncb;
    int tiles_per_utt = (a.T + ntt - 1) / ntt;
    int ntiles = a.B * tiles_per_utt;
    // Winograd kernel: tile the CONCATENATED frame axis when an utterance boundary can only fall between output pairs
    // (T even) and at most once per tile (T >= 64): B*T/64 tiles instead of B*ceil(T/64) (T = 800: 400 vs 416).
    bool concat = wino && a.dilation_cycle_length == 1 && a.T % 2 == 0 && a.T >= WN_NT &&
                  (int64_t)a.cp_bs * 4 < (1ll << 31) && a.d_bs == 0 && !a.save_y && !a.save_z;
    if (concat) {
        ntiles = (int)(((int64_t)a.B * a.T + WN_NT - 1) / WN_NT);
        tiles_per_utt = ntiles;  // one chain of tiles: neighbours are i-1 / i+1 everywhere
    }
    const int64_t ntasks64 = (int64_t)ntiles * a.L;
    SET_REQUIRE(ntasks64 < (1ll << 30), "set_diffnet_stack(task count)");
    const int max_dil = 1 << (a.dilation_cycle_length - 1);
    const int task_slot = DC * (ntt + 2 * max_dil);  // float index of the task word
    const size_t lds = (size_t)(task_slot + 4) * sizeof(float);
    SET_HIP(set_zero_async(a.sync_ws, stack_sync_words(wino ? SQ_WINO : SQ_QUEUE, ntiles) * sizeof(int32_t), s),
            "set_diffnet_stack(memset)");
    const int wps = wino ? 1 : 2;  // resident blocks per CU (three 168-VGPR blocks per CU measured slower: see DESIGN.md)
    // capped at 0.8x the tile count (see above), but a block on every CU while there are tiles for them
    const int grid = stack_grid(wps * p.n_cu, ntiles, ntasks64, true, p.n_cu);
    const int fault_tile = stack_fault_tile();
    if (wino) {
        if (a.dilation_cycle_length == 1)
            hipLaunchKernelGGL(diffnet_stack_wino_kernel<true>, dim3(grid), dim3(512),
                               (size_t)(WN_ZS_OFF + DC * WN_NT + 4) * sizeof(float), s, a, tiles_per_utt, ntiles,
                               (int)ntasks64, concat ? 1 : 0, fault_tile);
        else
            hipLaunchKernelGGL(diffnet_stack_wino_kernel<false>, dim3(grid), dim3(512),
                               (size_t)(WN_ZS_OFF + DC * WN_NT + 4) * sizeof(float), s, a, tiles_per_utt, ntiles,
                               (int)ntasks64, 0, fault_tile);
    } else if (ncb == 1)
        hipLaunchKernelGGL((diffnet_stack_kernel<1, 8, 2>), dim3(grid), dim3(256), lds, s, a, tiles_per_utt, ntiles,
                           (int)ntasks64, task_slot);
    else
        hipLaunchKernelGGL((diffnet_stack_kernel<2, 4, 2>), dim3(grid), dim3(256), lds, s, a, tiles_per_utt, ntiles,
                           (int)ntasks64, task_slot);
    return set_check_launch("set_diffnet_stack");
}
