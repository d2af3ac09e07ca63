// Host side of the DiffNet layer stack and of the reverse diffusion loop (no kernel lives here):
//   plan_stack         which of the six persistent stack kernels a launch runs, and in which form -- decided in one place
//   set_diffnet_stack  validation, plan, dispatch to the launchers of csrc/diffnet.hip / csrc/diffnet_x3.hip, and the two shape queries
//   set_diffusion_loop enqueue steps x (in-projection, the L layers, skip projection, output head, posterior) for every utterance group
#include <stdlib.h>

#include "common.h"
#include "diffnet_host.h"
#include "loop_events.h"
#include "stack_queue.h"

namespace {

constexpr int DC = 256;  // residual_channels every kernel of the loop is specialised for

// an integer environment variable, read at every plan (tests set the environment between calls); false when unset
bool env_int(const char *name, int *v) {
    const char *e = getenv(name);
    if (e) *v = atoi(e);
    return e != nullptr;
}

// have_wino / have_split: the caller holds the Winograd / row-split images (and the z workspace); x3_mode: the split-operand images it
// holds (2 = two-piece fp16, 3 = three-piece bf16, else none); aligned8: condproj and both x buffers are 8-byte aligned with even strides
StackPlan plan_stack(int B, int T, int dcl, bool have_wino, bool have_split, int x3_mode, bool aligned8, int n_cu) {
    StackPlan p = {};
    p.n_cu = n_cu;
    int v = 0, wino_env = 0;
    const bool wino_set = env_int("SET_AMD_WINO", &wino_env);             // an explicit choice also rules out the row-split and x3 kernels
    const bool f32_pinned = env_int("SET_AMD_SPLIT_F32", &v) && v != 0;   // pins the row-split kernel to the fp32 pipe
    const bool have_x3 = x3_mode == 2 || x3_mode == 3;
    const int64_t tiles64 = (int64_t)B * ((T + 63) / 64);
    // row-split kernel: 4 blocks per 32-frame tile, all co-resident (2 per CU); SET_AMD_SPLIT=0 disables, =2 forces it (when it fits)
    // (measured at T = 800: one utterance 75 ms per 100 steps, two 79 ms; from three utterances on two blocks would share a CU
    // and the split-operand kernel, ~123 ms whatever the batch up to B = 16, is the faster one)
    const int64_t split_blocks = 4 * (int64_t)B * ((T + 31) / 32);
    // co-residency: two blocks per CU for the fp32-pipe kernel, ONE for the two-piece fp16 one (its A ring takes the whole register
    // file of a SIMD lane group: launch bounds (256, 1)) unless SET_AMD_SPLIT_F32 pins the fp32-pipe kernel
    const bool split_one_per_cu = have_x3 && !f32_pinned;
    const bool split_fits = have_split && dcl <= 4 && split_blocks <= (split_one_per_cu ? 1 : 2) * (int64_t)n_cu;
    const bool split_pays = split_blocks <= (int64_t)(have_x3 ? 1 : 2) * n_cu;
    int split_env = 1;
    (void)env_int("SET_AMD_SPLIT", &split_env);
    if (split_fits && (split_env == 2 || (split_env == 1 && !wino_set && split_pays))) {
        p.family = STACK_ROW_SPLIT;
        p.split_x2 = x3_mode == 2 && !f32_pinned;  // the same scheme on the two-piece fp16 operands
        return p;
    }
    // split-operand kernel: every batch the row-split kernel does not take (a task is 61 us against 77 us for a 32-frame
    // task of the direct fp32 kernel, so it wins even when the chip is far from full; tiny inputs stay on the fp32 kernels);
    // SET_AMD_X3=0 disables, =2 forces it at any size
    int x3_env = 1;
    (void)env_int("SET_AMD_X3", &x3_env);
    if (have_x3 && dcl <= 4 && (x3_env == 2 || (x3_env == 1 && !wino_set && tiles64 >= 8))) {
        p.family = x3_mode == 3 ? STACK_X3_BF16 : STACK_X3_F16;
        // tile width: 64 frames from ~0.6 tiles per CU on, below that 32-frame tiles; SET_AMD_X3_TILE=32|64 overrides
        bool narrow = 5 * tiles64 < 3 * (int64_t)n_cu;
        if (env_int("SET_AMD_X3_TILE", &v)) narrow = v == 32;
        p.x3_ncb = narrow ? 1 : 2;
        // Winograd form of GEMM 1: two-piece fp16, dilation 1, even T, never on 32-frame tiles; its 8-byte loads of frame pairs need
        // `aligned8`.  SET_AMD_X3_WINO=0 pins the direct form, =2 / =3 the tile width
        int wino = 1;
        (void)env_int("SET_AMD_X3_WINO", &wino);
        if (x3_mode == 2 && dcl == 1 && T % 2 == 0 && !narrow && wino > 0 && aligned8) {
            // 96-frame tiles once every CU has a tile chain of them (B = 32, T = 800: 267 chains for 256 CUs; below that the workers wait
            // for each other: B = 24 123 k frames/s on 96-frame tiles against 149 k on 64-frame ones, profiles/r06_x3v_nb2_ab.log)
            const int64_t tiles96 = ((int64_t)B * ((T + 31) / 32) + 2) / 3;
            p.x3_wino = true;
            p.x3_ncb = wino == 2 || wino == 3 ? wino : (tiles96 >= (int64_t)n_cu ? 3 : 2);
        }
        return p;
    }
    // fp32 pipe: Winograd when it has its images, dilation_cycle_length <= 4 and at least ~0.68 tiles per CU (the measured crossover
    // against the direct 32-frame kernel; SET_AMD_WINO=0 disables, =2 forces); else direct, on 64-frame tiles from 3 tiles per CU on
    int ncb = tiles64 < 3 * n_cu ? 1 : 2;
    if (env_int("SET_AMD_STACK_NCB", &v)) ncb = v == 2 ? 2 : 1;
    const bool wino_ok = have_wino && (1 << (dcl - 1)) <= STACK_WINO_MAX_DIL;
    bool wino = wino_ok && 25 * tiles64 >= 17 * n_cu;
    if (wino_set) wino = wino_ok && (wino_env == 2 || (wino && wino_env != 0));
    p.family = wino ? STACK_WINO : (ncb == 1 ? STACK_DIRECT32 : STACK_DIRECT64);
    return p;
}

// the plan of a shape alone (`images`: include/set_amd.h); assumes aligned tensors, and 256 CUs when no device answers
StackPlan plan_stack_of_images(int B, int T, int dcl, int images) {
    int n_cu = 256;
    (void)set_cu_count(&n_cu);
    return plan_stack(B, T, dcl, (images & 1) != 0, (images & 2) != 0, (images & 4) ? 3 : ((images & 8) ? 2 : 0), true, n_cu);
}

// the plan of one set_diffnet_stack launch: the tensors, strides and images of `a`
StackPlan stack_plan(const SetDiffnetStackArgs &a, int n_cu) {
    const bool plain = !a.x_all && !a.save_y && !a.save_z;  // the training outputs: only the fp32 queue kernels write them
    const bool aligned8 = ((reinterpret_cast<uintptr_t>(a.condproj) | reinterpret_cast<uintptr_t>(a.xa) | reinterpret_cast<uintptr_t>(a.xb)) & 7) == 0 &&
                          ((a.cp_bs | a.cp_ls) & 1) == 0;
    return plan_stack(a.B, a.T, a.dilation_cycle_length, a.w1w_all && a.w2w_all, a.w1s_all && a.w2s_all && a.z_ws && plain,
                      (a.wx3_all && plain) ? a.x3_mode : 0, aligned8, n_cu);
}

// what set_diffnet_stack requires of its arguments
int stack_validate(const SetDiffnetStackArgs &a) {
    SET_REQUIRE(a.xa && a.xb && a.skip && a.condproj && a.dstep && a.w1p_all && a.w2p_all && a.b_dil_all &&
                    a.b_out_all && a.sync_ws,
                "set_diffnet_stack");
    SET_REQUIRE(a.B > 0 && a.T > 0 && a.L > 0 && a.dilation_cycle_length >= 1 && a.dilation_cycle_length <= 4,
                "set_diffnet_stack");
    return SET_OK;
}

int stack_launch(const SetDiffnetStackArgs &a, const StackPlan &p, hipStream_t s) {
    SET_REQUIRE(!a.xs_q4 || p.x3_wino, "set_diffnet_stack(xs_q4: only the Winograd split-operand kernel reads the channel-quad layout)");
    if (p.family >= STACK_X3_BF16) return set_launch_diffnet_stack_x3(a, p, s);
    if (p.split_x2) return set_launch_diffnet_stack_split_x2(a, p, s);
    return set_launch_diffnet_stack_f32(a, p, s);
}

}  // namespace

extern "C" int set_diffnet_stack(const SetDiffnetStackArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_diffnet_stack");
    if (int rc = stack_validate(*args)) return rc;
    int n_cu = 0;
    SET_HIP(set_cu_count(&n_cu), "set_diffnet_stack");
    return stack_launch(*args, stack_plan(*args, n_cu), (hipStream_t)stream);
}
extern "C" int set_diffnet_stack_variant(int B, int T, int dilation_cycle_length, int images) {
    return plan_stack_of_images(B, T, dilation_cycle_length, images).family;
}
extern "C" int set_diffnet_stack_x3_winograd(int B, int T, int dilation_cycle_length, int images) {
    const StackPlan p = plan_stack_of_images(B, T, dilation_cycle_length, images);
    return p.family == STACK_X3_F16 && p.x3_wino ? p.x3_ncb : 0;
}

// ----------------------------------------------------------------------------------------------------------
// the reverse loop
// ----------------------------------------------------------------------------------------------------------
namespace {

SetConv1dArgs conv1x1_args(const float *in, const float *wp, const float *bias, float *out, int B, int Cin, int Cout, int T) {
    SetConv1dArgs c = {};
    c.in = in; c.w = wp; c.bias = bias; c.out = out;
    c.in_bs = (int64_t)Cin * T; c.in_cs = T; c.out_bs = (int64_t)Cout * T; c.out_cs = T;
    c.B = B; c.Cin = Cin; c.Cout = Cout; c.K = 1; c.dil = 1; c.pad = 0;
    c.T_in = T; c.T_iter = T; c.T_out = T; c.out_stride = 1; c.out_off = 0;
    c.alpha = 1.0f; c.impl = SET_IMPL_MFMA;
    return c;
}

// auxiliary streams for utterance groups (created once, never destroyed)
hipStream_t g_aux_streams[8] = {nullptr};
int aux_stream(int i, hipStream_t *out) {
    if (!g_aux_streams[i]) SET_HIP(hipStreamCreateWithFlags(&g_aux_streams[i], hipStreamNonBlocking), "aux stream");
    *out = g_aux_streams[i];
    return SET_OK;
}

// how the L layers of a step run
enum StepBody {
    STEP_STACK,        // one persistent stack launch (fp32-equivalent kernels)
    STEP_BF16_GROUPS,  // opt-in bf16 operands, `fuse` layers per launch (csrc/diffnet_bf16.hip: the tile stays on chip between them)
    STEP_BF16_LAYERS,  // opt-in bf16 operands, one launch per layer (conditioner projection inside the layer GEMM)
    STEP_F32_LAYERS,   // fp32, one launch per layer
};
// what is the same for every step of a chain; the environment is read here, once per set_diffusion_loop call and group
struct StepPlan {
    StepBody body;
    int fuse;             // STEP_BF16_GROUPS: layers per launch
    bool fused_boundary;  // the step boundary (and the next step's in-projection) as one launch
    bool boundary_x2;     // ... on two-piece fp16 operands
    bool ws_q4;           // ws_x0, ws_x1 and ws_skip in the channel-quad layout (common.h, q4f_index): STEP_STACK on the Winograd split-operand
                          // kernel between fused two-piece fp16 boundaries, the only kernels that read it
    StackPlan stack;      // STEP_STACK
};

// the chain of one utterance group [b0, b0 + Bg): its slices of the loop's tensors
struct Chain {
    const SetDiffLoopArgs &a;
    int b0, Bg;
    hipStream_t s;
    float *x, *ws_x0, *ws_x1, *ws_skip, *ws_h, *ws_x0pred;
    const float *condproj;
    StepPlan plan;
    SetDiffnetStackArgs stack;  // STEP_STACK: the launch of a step but for its dstep column
    int64_t bf16_per_utt;       // STEP_BF16_GROUPS: scratch floats of one utterance
};

int plan_steps(Chain &c, int g) {
    const SetDiffLoopArgs &a = c.a;
    const int T = a.T, L = a.L, dcl = a.dilation_cycle_length;
    StepPlan &p = c.plan;
    int n_cu = 0;
    SET_HIP(set_cu_count(&n_cu), "set_diffusion_loop");
    p.fused_boundary = boundary_fusable(a);
    const bool x2_images = p.fused_boundary && a.w_skip_x2 && a.w_outp_x2 && a.w_in_x2 && a.M <= 96;
    if (a.img16_all) {
        p.fuse = 1;
        if (a.bf16_ws && dcl <= 2) {
            p.fuse = set_diffnet_layers_bf16_plan(c.Bg, T, L, dcl);  // 10 (128-frame tiles fill the chip) or 5
            if (env_int("SET_AMD_BF16_FUSE", &p.fuse)) p.fuse = p.fuse < 1 ? 1 : (p.fuse > 16 ? 16 : p.fuse);
            if (p.fuse > 1 && a.bf16_ws_floats < set_diffnet_layers_bf16_scratch_floats(a.B, T, 0, p.fuse, dcl)) p.fuse = 1;
        }
        p.body = p.fuse > 1 ? STEP_BF16_GROUPS : STEP_BF16_LAYERS;
        // utterance groups (n_groups > 1) run concurrently on their own streams and the 128-frame kernel indexes its private skip
        // rows by (blockIdx.y, blockIdx.x) of its own launch: every group gets its own slice (per-utterance floats do not depend on B)
        if (p.fuse > 1) c.bf16_per_utt = set_diffnet_layers_bf16_scratch_floats(1, T, 0, p.fuse, dcl);
        // the bf16-operand loop takes the split-operand boundary whenever its images are given (round 4: 85 -> 37 us per step at B = 32,
        // T = 800; it is the fp32-equivalent one, and it raises the same range word, which the caller must read)
        p.boundary_x2 = x2_images;
    } else if (a.persistent) {
        p.body = STEP_STACK;
        SetDiffnetStackArgs &sa = c.stack;
        sa.xa = c.ws_x0; sa.xb = c.ws_x1; sa.skip = c.ws_skip;
        sa.condproj = c.condproj; sa.cp_bs = (int64_t)L * 512 * T; sa.cp_ls = (int64_t)512 * T;
        sa.dstep = a.dstep; sa.d_bs = 0; sa.d_cs = a.steps; sa.d_ls = (int64_t)DC * a.steps;  // (dstep: + the step's column)
        sa.w1p_all = a.w1p_all; sa.w2p_all = a.w2p_all; sa.b_dil_all = a.b_dil_all; sa.b_out_all = a.b_out_all;
        sa.w1w_all = a.w1w_all; sa.w2w_all = a.w2w_all;
        sa.w1s_all = a.w1s_all; sa.w2s_all = a.w2s_all; sa.wx3_all = a.wx3_all; sa.x3_mode = a.x3_mode;
        sa.z_ws = a.z_ws ? a.z_ws + (int64_t)c.b0 * DC * 32 * ((T + 31) / 32) : nullptr;
        sa.err_flag = a.err_flag;
        sa.sync_ws = a.sync_ws ? a.sync_ws + SQ_GROUP_WORDS * (int64_t)g + 2 * (int64_t)c.b0 * ((T + 31) / 32) : nullptr;  // per-group slice
        sa.B = c.Bg; sa.T = T; sa.L = L; sa.dilation_cycle_length = dcl;
        if (int rc = stack_validate(sa)) return rc;
        p.stack = stack_plan(sa, n_cu);
        // the step boundary on two-piece fp16 operands whenever the layer stack runs on them (same splitting, same range guard)
        p.boundary_x2 = x2_images && p.stack.two_piece_fp16();
    } else {
        p.body = STEP_F32_LAYERS;
    }
    int v = 0;
    if (env_int("SET_AMD_BOUNDARY_X2", &v)) p.boundary_x2 = p.boundary_x2 && v != 0;
    // the workspace layout, decided here once for the chain.  SET_AMD_WS_Q4=0 keeps the plain layout (the A/B switch)
    int q4_env = 1;
    (void)env_int("SET_AMD_WS_Q4", &q4_env);
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(c.ws_x0) | reinterpret_cast<uintptr_t>(c.ws_x1) | reinterpret_cast<uintptr_t>(c.ws_skip)) & 15) == 0;
    p.ws_q4 = a.ws_q4 != 0 && q4_env != 0 && p.body == STEP_STACK && p.stack.x3_wino && p.fused_boundary && p.boundary_x2 && aligned16;
    c.stack.xs_q4 = p.ws_q4 ? 1 : 0;
    return SET_OK;
}

// ---- the four step bodies: layers 0 .. L-1 of diffusion step `sid`, ws_x0 -> (ws_x0 | ws_x1), skip sum -> ws_skip
int step_stack(const Chain &c, int sid) {
    SetDiffnetStackArgs sa = c.stack;
    sa.dstep += sid;
    return stack_launch(sa, c.plan.stack, c.s);
}

// launch(l, x_in, x_out) for l = 0, stride, .. < L, the x buffers ping-ponging from ws_x0
template <typename Launch> int for_layers(const Chain &c, int stride, Launch launch) {
    float *cur = c.ws_x0, *nxt = c.ws_x1;
    int rc = SET_OK;
    for (int l = 0; l < c.a.L && rc == SET_OK; l += stride) {
        rc = launch(l, cur, nxt);
        float *tmp = cur; cur = nxt; nxt = tmp;
    }
    return rc;
}

int step_bf16_groups(const Chain &c, int sid) {
    const SetDiffLoopArgs &a = c.a;
    const int L = a.L, fuse = c.plan.fuse;
    return for_layers(c, fuse, [&](int l, float *cur, float *nxt) {
        SetDiffnetLayersBf16Args fa = {};
        fa.x_in = cur; fa.x_out = nxt; fa.skip = c.ws_skip;
        fa.cond = a.cond + (int64_t)c.b0 * 192 * a.T;
        fa.dstep = a.dstep + sid; fa.d_bs = 0; fa.d_cs = a.steps; fa.d_ls = (int64_t)DC * a.steps;
        fa.img = reinterpret_cast<const uint16_t *>(a.img16_all) + (int64_t)l * set_diffnet_layer_bf16_image_size();
        fa.b_dil = a.b_dil_all + (int64_t)l * 512; fa.b_cond = a.b_cond_all + (int64_t)l * 512; fa.b_out = a.b_out_all + (int64_t)l * 512;
        fa.scratch = a.bf16_ws + (int64_t)c.b0 * c.bf16_per_utt; fa.scratch_floats = (int64_t)c.Bg * c.bf16_per_utt;
        fa.B = c.Bg; fa.T = a.T; fa.l0 = l; fa.nl = L - l < fuse ? L - l : fuse; fa.dilation_cycle_length = a.dilation_cycle_length;
        fa.first = (l == 0);
        return set_diffnet_layers_fwd_bf16(&fa, c.s);
    });
}

int step_bf16_layers(const Chain &c, int sid) {
    const SetDiffLoopArgs &a = c.a;
    return for_layers(c, 1, [&](int l, float *cur, float *nxt) {
        SetDiffnetLayerBf16Args la = {};
        la.x_in = cur; la.x_out = nxt; la.skip = c.ws_skip;
        la.cond = a.cond + (int64_t)c.b0 * 192 * a.T;
        la.dstep = a.dstep + (int64_t)l * DC * a.steps + sid;
        la.d_bs = 0; la.d_cs = a.steps;
        la.img = reinterpret_cast<const uint16_t *>(a.img16_all) + (int64_t)l * set_diffnet_layer_bf16_image_size();
        la.b_dil = a.b_dil_all + (int64_t)l * 512; la.b_cond = a.b_cond_all + (int64_t)l * 512;
        la.b_out = a.b_out_all + (int64_t)l * 512;
        la.B = c.Bg; la.T = a.T; la.dil = 1 << (l % a.dilation_cycle_length); la.first = (l == 0);
        return set_diffnet_layer_fwd_bf16(&la, c.s);
    });
}

int step_f32_layers(const Chain &c, int sid) {
    const SetDiffLoopArgs &a = c.a;
    return for_layers(c, 1, [&](int l, float *cur, float *nxt) {
        SetDiffnetLayerArgs la = {};
        la.x_in = cur; la.x_out = nxt; la.skip = c.ws_skip;
        la.condproj = c.condproj + (int64_t)l * 512 * a.T;
        la.cp_bs = (int64_t)a.L * 512 * a.T;
        la.dstep = a.dstep + (int64_t)l * DC * a.steps + sid;
        la.d_bs = 0; la.d_cs = a.steps;
        la.w1p = a.w1p_all + (int64_t)l * (512 * 768); la.b_dil = a.b_dil_all + (int64_t)l * 512;
        la.w2p = a.w2p_all + (int64_t)l * (512 * 256); la.b_out = a.b_out_all + (int64_t)l * 512;
        la.B = c.Bg; la.T = a.T; la.dil = 1 << (l % a.dilation_cycle_length); la.first = (l == 0);
        return set_diffnet_layer(&la, c.s);
    });
}

// enqueue the chain of utterance group g = [b0, b0+Bg) on stream s; ev (optional): two events per step around its layers
int diffusion_chain(const SetDiffLoopArgs &a, int g, int b0, int Bg, hipStream_t s, hipEvent_t *ev) {
    const int T = a.T, M = a.M, L = a.L;
    const int64_t per_batch = (int64_t)M * T;
    Chain c = {a, b0, Bg, s};
    c.x = a.x + (int64_t)b0 * per_batch;
    c.ws_x0 = a.ws_x0 + (int64_t)b0 * DC * T; c.ws_x1 = a.ws_x1 + (int64_t)b0 * DC * T;
    c.ws_skip = a.ws_skip + (int64_t)b0 * DC * T; c.ws_h = a.ws_h + (int64_t)b0 * DC * T;
    c.ws_x0pred = a.ws_x0pred + (int64_t)b0 * per_batch;
    c.condproj = a.condproj ? a.condproj + (int64_t)b0 * L * 512 * T : nullptr;
    if (int rc = plan_steps(c, g)) return rc;
    const StepPlan &p = c.plan;
    const uint64_t quads_before = (uint64_t)((int64_t)b0 * per_batch / 4);
    const uint64_t quads_total = (uint64_t)(((int64_t)a.B * per_batch + 3) / 4);
    int rc = SET_OK;
    for (int k = 0; k < a.steps && rc == SET_OK; ++k) {
        const int sid = a.steps - 1 - k;  // diffusion step id t = steps-1 .. 0 (spec_denoiser.py:181)
        // input projection + ReLU (diffnet.py:118-120); with the fused boundary it is part of the previous step's
        // boundary launch
        if (!p.fused_boundary || k == 0) {
            // (channel-quad workspaces: projected into ws_x1, which layer 0 overwrites, and re-laid into ws_x0 -- once per loop)
            SetConv1dArgs cin = conv1x1_args(c.x, a.w_in_p, a.b_in, p.ws_q4 ? c.ws_x1 : c.ws_x0, Bg, M, DC, T);
            cin.act = SET_ACT_RELU;
            rc = set_conv1d(&cin, s);
            if (rc == SET_OK && p.ws_q4) rc = launch_relayout_q4(c.ws_x1, c.ws_x0, Bg, T, s);
            if (rc != SET_OK) break;
        }
        if (ev) (void)hipEventRecord(ev[2 * k], s);
        switch (p.body) {
            case STEP_STACK: rc = step_stack(c, sid); break;
            case STEP_BF16_GROUPS: rc = step_bf16_groups(c, sid); break;
            case STEP_BF16_LAYERS: rc = step_bf16_layers(c, sid); break;
            case STEP_F32_LAYERS: rc = step_f32_layers(c, sid); break;
        }
        if (ev) (void)hipEventRecord(ev[2 * k + 1], s);
        if (rc != SET_OK) break;
        const float *eps = a.noise ? a.noise + (int64_t)k * a.B * per_batch + (int64_t)b0 * per_batch : nullptr;
        // Philox counters are global element quads, so the noise does not depend on the grouping
        const uint64_t quad_offset = (uint64_t)(k + 1) * quads_total + quads_before;
        if (p.fused_boundary) {
            // only the skip sum feeds the output head (diffnet.py:128); the next step's stack input buffer is ws_x0
            rc = launch_boundary(a, Bg, c.ws_skip, c.x, eps, sid, quad_offset, k + 1 < a.steps ? c.ws_x0 : nullptr, p.boundary_x2, p.ws_q4, s);
            continue;
        }
        // skip sum / sqrt(L) -> skip_projection -> ReLU -> output_projection (diffnet.py:128-131)
        SetConv1dArgs cs = conv1x1_args(c.ws_skip, a.w_skip_p, a.b_skip, c.ws_h, Bg, DC, DC, T);
        cs.pro = SET_PRO_DIV; cs.pro_param = sqrtf((float)L); cs.act = SET_ACT_RELU;
        rc = set_conv1d(&cs, s);
        if (rc != SET_OK) break;
        SetConv1dArgs co = conv1x1_args(c.ws_h, a.w_outp_p, a.b_outp, c.ws_x0pred, Bg, DC, M, T);
        rc = set_conv1d(&co, s);
        if (rc != SET_OK) break;
        rc = set_posterior_step(c.ws_x0pred, c.x, eps, a.coef4 + 4 * sid, 0, c.x, Bg, per_batch, a.seed, quad_offset, s);
    }
    return rc;
}

}  // namespace

extern "C" int set_diffusion_loop(const SetDiffLoopArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_diffusion_loop");
    const SetDiffLoopArgs &a = *args;
    SET_REQUIRE(a.B > 0 && a.T > 0 && a.M > 0 && a.L > 0 && a.steps > 0 && a.dilation_cycle_length >= 1,
                "set_diffusion_loop");
    SET_REQUIRE(a.x && a.dstep && a.coef4 && a.w_in_p && a.b_in && a.b_dil_all && a.b_out_all && a.w_skip_p && a.b_skip &&
                    a.w_outp_p && a.b_outp, "set_diffusion_loop");
    if (a.img16_all) {
        SET_REQUIRE(a.cond && a.b_cond_all, "set_diffusion_loop(bf16 loop needs cond and b_cond_all)");
        // the bf16 layer kernels take dilations up to 8: refuse a longer cycle here, before the in-projection and the first layers are
        // enqueued (set_diffnet_layer_fwd_bf16 would refuse layer 4 with x's workspaces half written); stack_validate asks the same
        SET_REQUIRE(a.dilation_cycle_length <= 4, "set_diffusion_loop(bf16 loop: dilation_cycle_length <= 4)");
    } else {
        SET_REQUIRE(a.condproj && a.w1p_all && a.w2p_all, "set_diffusion_loop");
        SET_REQUIRE(!a.persistent || a.sync_ws, "set_diffusion_loop(persistent needs sync_ws)");
    }
    SET_REQUIRE(a.ws_x0 && a.ws_x1 && a.ws_skip && a.ws_h && a.ws_x0pred, "set_diffusion_loop");
    hipStream_t s = (hipStream_t)stream;
    const int64_t per_batch = (int64_t)a.M * a.T;
    int G = a.n_groups < 1 ? 1 : (a.n_groups > 8 ? 8 : a.n_groups);
    if (G > a.B) G = a.B;
    if (per_batch % 4 != 0) G = 1;  // group slices must start on a Philox quad boundary
    const bool timing = a.layer_span_ms != nullptr;
    LoopEvents events;  // every event below; destroyed on every return path
    std::vector<hipEvent_t> ev(timing ? (size_t)2 * a.steps * G : 0);  // [group][step][begin, end of the layers]
    for (hipEvent_t &e : ev) SET_HIP(events.create(&e, true), "set_diffusion_loop(event)");
    hipEvent_t loop_ev[2] = {nullptr, nullptr};
    if (a.loop_ms) {
        SET_HIP(events.create(&loop_ev[0], true), "set_diffusion_loop(event)");
        SET_HIP(events.create(&loop_ev[1], true), "set_diffusion_loop(event)");
        (void)hipEventRecord(loop_ev[0], s);
    }
    int rc = SET_OK;
    if (G == 1) {
        rc = diffusion_chain(a, 0, 0, a.B, s, timing ? ev.data() : nullptr);
    } else {
        hipEvent_t fork = nullptr, join = nullptr;
        SET_HIP(events.create(&fork, false), "set_diffusion_loop(fork)");
        SET_HIP(hipEventRecord(fork, s), "set_diffusion_loop(fork)");
        for (int g = 0; g < G && rc == SET_OK; ++g) {
            const int b0 = (int)((int64_t)a.B * g / G), b1 = (int)((int64_t)a.B * (g + 1) / G);
            hipStream_t sg;
            rc = aux_stream(g, &sg);
            if (rc != SET_OK) break;
            SET_HIP(hipStreamWaitEvent(sg, fork, 0), "set_diffusion_loop(fork wait)");
            rc = diffusion_chain(a, g, b0, b1 - b0, sg, timing ? ev.data() + (size_t)2 * a.steps * g : nullptr);
            SET_HIP(events.create(&join, false), "set_diffusion_loop(join)");
            SET_HIP(hipEventRecord(join, sg), "set_diffusion_loop(join)");
            SET_HIP(hipStreamWaitEvent(s, join, 0), "set_diffusion_loop(join wait)");
        }
    }
    if (a.loop_ms) (void)hipEventRecord(loop_ev[1], s);
    if (timing || a.loop_ms) {
        if (rc == SET_OK) {
            hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = set_fail(SET_E_LAUNCH, "set_diffusion_loop(sync)", hipGetErrorString(e));
        }
        if (rc == SET_OK && timing) {
            for (int k = 0; k < a.steps; ++k) {
                float acc_ms = 0.0f;
                for (int g = 0; g < G; ++g) {
                    float ms = 0.0f;
                    (void)hipEventElapsedTime(&ms, ev[(size_t)2 * a.steps * g + 2 * k], ev[(size_t)2 * a.steps * g + 2 * k + 1]);
                    acc_ms += ms;
                }
                a.layer_span_ms[k] = acc_ms / (float)G;
            }
        }
        if (rc == SET_OK && a.loop_ms) (void)hipEventElapsedTime(a.loop_ms, loop_ev[0], loop_ev[1]);
    }
    return rc;
}

extern "C" int64_t set_sizeof_diff_loop_args(void) { return (int64_t)sizeof(SetDiffLoopArgs); }
