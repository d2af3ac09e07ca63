/*
 * set_amd.h -- C ABI of libset_amd.so: the MI355X (gfx950) implementation of the
 * Speech-Editing-Toolkit acoustic hot path (FluentSpeech spec_denoiser diffusion
 * loop + HiFi-GAN generator forward).
 *
 * The reference (Zain-Jiang/Speech-Editing-Toolkit) is pure Python/PyTorch and has
 * NO native/FFI boundary of its own; its extension points
 * are Python registries.  This header is therefore the boundary a maintainer of
 * the reference would bind with ctypes.  Every entry point
 * cites the reference code whose arithmetic it replaces (paths relative to the
 * upstream repo root).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc'd / torch CUDA tensors) unless
 *     a parameter is documented as host;
 *   - activations are fp32, channel-major: [B][C][T] with T contiguous (the
 *     layout nn.Conv1d uses in the reference); index tensors are int64;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*);
 *     the caller keeps all buffers alive until it synchronises the stream;
 *   - return value: 0 = ok, negative = SET_E_* error code; nothing throws;
 *   - no global mutable state except a lazily created pool of auxiliary HIP streams (set_diffusion_loop
 *     with n_groups > 1); thread-compatible (one caller thread per stream).
 */
#ifndef SET_AMD_H
#define SET_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SET_AMD_ABI_VERSION 5

/* error codes */
#define SET_OK 0
#define SET_E_INVALID (-1)     /* bad argument (null pointer, shape out of range) */
#define SET_E_UNSUPPORTED (-2) /* shape not supported by the requested implementation */
#define SET_E_LAUNCH (-3)      /* hipLaunch / hip runtime error */

/* activation codes (epilogue `act`) */
#define SET_ACT_NONE 0
#define SET_ACT_RELU 1
#define SET_ACT_GELU 2     /* exact erf GELU (nn.GELU default) */
#define SET_ACT_TANH 3
#define SET_ACT_SOFTPLUS 4 /* beta=1, threshold=20 (nn.Softplus default) */
#define SET_ACT_MISH 5     /* x*tanh(softplus(x)), diffnet.py:14-16 */
#define SET_ACT_LRELU 6    /* leaky_relu(x, act_param) */

/* input prologue codes (`pro`) applied to every in-range input sample */
#define SET_PRO_NONE 0
#define SET_PRO_LRELU 1 /* leaky_relu(x, pro_param)   (hifigan.py:53,55,129,138) */
#define SET_PRO_DIV 2   /* x / pro_param              (diffnet.py:128, / sqrt(L)) */

/* implementation selector for set_conv1d (0 is treated as NAIVE) */
#define SET_IMPL_NAIVE 1 /* one thread per output sample; any shape; device-side cross-check */
#define SET_IMPL_MFMA 2  /* implicit-GEMM on v_mfma_f32_32x32x2_f32; needs packed weights */
#define SET_IMPL_MFMA2 3 /* big-tile variant for wide layers (128*RB rows x 64 frames per block, RB = 4/2/1 for
                            Cout >= 384 / >= 192 / else); needs the image of set_pack_conv_weight_v2;
                            receptive field (K-1)*|dil| <= 64 */

#define SET_IMPL_BF16 4  /* bf16 MFMA operands (v_mfma_f32_32x32x16_bf16), fp32 accumulate / epilogue / HBM tensors; `w` =
                            the image of set_pack_conv_weight_bf16; stride-1 output only.  The training rows' "bf16"
                            arithmetic (BASELINE configs[1]; the reference's autocast hooks: utils/commons/trainer.py:325,343) */
#define SET_IMPL_F16X2 5 /* fp32 operands carried as two fp16 pieces, three fp16 MFMAs per product, fp32 accumulate (fp32-
                          * equivalent results, see SetDiffnetStackArgs.wx3_all); `w` = the image of
                          * set_pack_conv_weight_x2; no in_chan_add; an activation of magnitude >= 32768 raises the sticky
                          * flag of set_conv_x2_range_flag (the caller repeats on an fp32 impl) */

#define SET_IMPL_FEWOUT 6 /* Cout <= 2 over a long sequence (HiFi-GAN conv_post): one thread per four output samples, fp32 VALU,
                          * input streamed once with 16-byte loads; `w` = the RAW weight (w_base / w_s* addressing, as the naive
                          * kernel); needs K <= 9, dil 1, 0 <= pad <= 4, K - pad <= 5, T_in == T_out, T % 4 == 0, no res / mask /
                          * in_chan_add / accumulate, 16-byte aligned in / out */

/* operand type selector of the training GEMMs */
#define SET_DTYPE_F32 0
#define SET_DTYPE_BF16 1         /* fp32 tensors in HBM, rounded to bf16 on the way into LDS */
#define SET_DTYPE_BF16_G16 2     /* weight gradient only: the output gradient g already is bf16 [B][Cout][T] in HBM */
#define SET_DTYPE_BF16_G16_X16 3 /* ... and so is the conv input x (no prologue / per-channel add then) */

int set_abi_version(void);
/* last hip error string of the calling thread's most recent failing call (host pointer, static storage) */
const char *set_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Generic 1-D convolution, stride 1, with fused prologue/epilogue.  Replaces every
 * F.conv1d / nn.Conv1d / nn.Linear / nn.ConvTranspose1d (as u polyphase convs) call on the path:
 * modules/commons/conv.py:45-49,94 ; nar_tts_modules.py:17,22,83,88 ; mel_encoder.py:7-13 ;
 * diffnet.py:49-52,94,106-107 ; hifigan.py:108,114-115,122 and ResBlock1/2 (:31-48,71-76).
 *
 *   for t in [0, T_iter):  n = t*out_stride + out_off   (skipped unless 0 <= n < T_out)
 *     acc  = sum_{ci,tap} W[co][ci][tap] * P(in[b][ci][t + tap*dil - pad])   (0 outside [0,T_in))
 *            where P(x) = pro(x + in_chan_add[b][ci])      (in_chan_add optional)
 *     v    = act((acc + bias[co]) * alpha)
 *     v    = v + res[b][co][n]                              (res optional)
 *     v    = v * mask[b][n]                                 (mask optional, [B][T_out])
 *     out[b][co][n] = accumulate ? out[b][co][n] + v : v
 *     (accumulate && out_div != 0:  out = (out + v) / out_div -- the last term of a running mean, e.g. the MRF mean
 *      `xs / num_kernels` of hifigan.py:131-137 folded into the last ResBlock's final conv; same summation order)
 *
 * `dil` may be negative (ConvTranspose polyphase taps read in[q - j]).
 * Weights: impl NAIVE reads w[w_base + co*w_sco + ci*w_sci + tap*w_stap];
 *          impl MFMA reads `w` as the packed image written by set_pack_conv_weight.
 * ------------------------------------------------------------------------------------------------ */
typedef struct SetConv1dArgs {
    const float *in;          /* [B][Cin][T_in], batch stride in_bs, channel stride in_cs */
    const float *w;           /* see above */
    const float *bias;        /* [Cout] or NULL */
    const float *res;         /* optional residual, batch stride res_bs, channel stride res_cs */
    const float *mask;        /* optional [B][T_out] */
    const float *in_chan_add; /* optional [B][Cin] (batch stride Cin) */
    float *out;               /* [B][Cout][T_out], batch stride out_bs, channel stride out_cs */
    int64_t in_bs, in_cs, out_bs, out_cs, res_bs, res_cs;
    int64_t w_base, w_sco, w_sci, w_stap; /* NAIVE weight addressing */
    int32_t B, Cin, Cout, K, dil, pad;
    int32_t T_in, T_iter, T_out, out_stride, out_off;
    int32_t pro, act, accumulate, impl;
    float pro_param, act_param, alpha;
    float out_div;            /* see above; 0 = plain accumulate */
} SetConv1dArgs;

int set_conv1d(const SetConv1dArgs *args, void *stream);

/* number of floats of the packed image for (Cout, Cin, K) */
int64_t set_packed_conv_weight_size(int32_t Cout, int32_t Cin, int32_t K);
/* pack w[w_base + co*w_sco + ci*w_sci + tap*w_stap] into MFMA A-fragment order:
 * wp[rb][tap][cp][lane] = W[32*rb + (lane&31)][2*cp + (lane>>5)][tap], zero padded
 * (rb < ceil(Cout/32), cp < CinP/2, CinP = Cin rounded up to 16). */
int set_pack_conv_weight(const float *w, float *wp, int32_t Cout, int32_t Cin, int32_t K,
                         int64_t w_base, int64_t w_sco, int64_t w_sci, int64_t w_stap, void *stream);

/* image for SET_IMPL_F16X2: [32-row block][16-channel group][tap][piece][lane][8 fp16] + 4 floats {2^k, 2^-k, 0, 0}; the
 * weights are multiplied by 2^scale_exp before they are split (pick it so that max |w| 2^k is in [8, 16)); ..._size in fp16
 * ELEMENTS */
int64_t set_packed_conv_weight_x2_size(int32_t Cout, int32_t Cin, int32_t K);
int set_pack_conv_weight_x2(const float *w, void *wp, int32_t Cout, int32_t Cin, int32_t K, int64_t w_base, int64_t w_sco,
                            int64_t w_sci, int64_t w_stap, int32_t scale_exp, void *stream);
/* nn.ConvTranspose1d(Cin, Cout, k, stride u, padding P) on the same kernel, EVERY output phase in one launch (the fp32 path
 * runs one strided-output conv per phase): the rows of the GEMM are (channel, phase) pairs, so with u % 4 == 0 the four rows
 * of an accumulator register group are four consecutive output samples -> 16-byte stores instead of stride-u scatters.
 * w: the module's weight [Cin][Cout][k]; out[b][co][n] = bias[co] + sum_ci sum_j w[ci][co][u j + p] pro(in[b][ci][q - j]),
 * n + P = u q + p (hifigan.py:114-115); in / out contiguous [B][C][T], T_out = (T_in - 1) u - 2 P + k. */
int64_t set_packed_conv_transpose_x2_size(int32_t Cout, int32_t Cin, int32_t k, int32_t u);
int set_pack_conv_transpose_x2(const float *w, void *wp, int32_t Cout, int32_t Cin, int32_t k, int32_t u, int32_t scale_exp,
                               void *stream);
int set_conv_transpose1d_x2(const float *in, const void *wp, const float *bias, float *out, int32_t B, int32_t Cin, int32_t Cout,
                            int32_t k, int32_t u, int32_t P, int32_t T_in, int32_t pro, float pro_param, void *stream);
/* *flag = sticky "an activation left the fp16 range of the F16X2 splitting" word (synchronises); reset != 0 clears it */
int set_conv_x2_range_flag(int32_t *flag, int32_t reset);

/* One iteration of HiFi-GAN's ResBlock1 loop, fused (replaces modules/vocoder/hifigan/hifigan.py:51-58
 *     xt = leaky_relu(x, slope); xt = c1(xt); xt = leaky_relu(xt, slope); xt = c2(xt); x = xt + x
 * with c1 = Conv1d(C, C, K, dilation=dil, padding=dil (K-1)/2), c2 = Conv1d(C, C, K, dilation=1, padding=(K-1)/2)):
 *     out = (c2(lrelu(c1(lrelu(x)) )) + x  [+ previous out if accumulate]) [/ out_div if != 0]
 * accumulate / out_div carry the MRF sum and mean of hifigan.py:131-137 like SetConv1dArgs does.  Two-piece fp16 operands
 * (SET_IMPL_F16X2 arithmetic; w1 / w2 = images of set_pack_conv_weight_x2(C, C, K)); the intermediate xt lives in LDS only
 * (20 C T bytes of HBM traffic per pair become 8 C T).  Results are bit-identical to the two set_conv1d(F16X2) launches.
 * x / out: [B][C][T] with unit frame stride; out must not alias x.  Shapes: see set_resblock_pair_x2_supported.
 * An activation of magnitude >= 32768 raises the sticky flag of set_conv_x2_range_flag. */
typedef struct SetResblockPairArgs {
    const float *x;
    const void *w1;
    const float *b1;
    const void *w2;
    const float *b2;
    float *out;
    int64_t x_bs, x_cs, out_bs, out_cs;  /* batch / channel strides in elements */
    int32_t B, C, K, dil, T;
    int32_t accumulate;
    float slope, out_div;
} SetResblockPairArgs;
int64_t set_sizeof_resblock_pair_args(void);
/* SET_OK if the fused kernel takes the shape (16 <= C <= 256, odd 3 <= K <= 15 -- <= 5 above 128 channels --, dil (K-1) <= 128,
 * T >= 64) */
int set_resblock_pair_x2_supported(int32_t C, int32_t K, int32_t dil, int32_t T);
int set_resblock_pair_x2(const SetResblockPairArgs *args, void *stream);

/* packed image for SET_IMPL_MFMA2 (layout depends on Cout, K and |dil| as well as on the weights) */
int64_t set_packed_conv_weight_v2_size(int32_t Cout, int32_t Cin, int32_t K);
int set_pack_conv_weight_v2(const float *w, float *wp, int32_t Cout, int32_t Cin, int32_t K, int32_t dil,
                            int64_t w_base, int64_t w_sco, int64_t w_sci, int64_t w_stap, void *stream);

/* weight-norm fold  w[i][...] = g[i] * v[i][...] / ||v[i][...]||_2   (torch.nn.utils.weight_norm, dim=0;
 * hifigan.py:32-47,108,114,122).  v,w: [n0][inner]; g: [n0]. */
int set_weight_norm_fold(const float *g, const float *v, float *w, int32_t n0, int64_t inner, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Conditioner glue kernels (FastSpeech-style encoder path; all tiny)
 * ------------------------------------------------------------------------------------------------ */
/* LayerNorm over the channel dim of [B][C][T] (modules/commons/layers.py:5-24 with dim=1),
 * then optional * mask[b][t].  */
int set_layernorm_ch(const float *x, const float *gamma, const float *beta, const float *mask, float *out,
                     int32_t B, int32_t C, int32_t T, float eps, void *stream);
/* out[b][c][t] (+)= scale * table[idx[b][t]][c]     (layers.py:45-50, conv.py:138, fs.py:138,164,188) */
int set_embedding_bct(const int64_t *idx, const float *table, float *out, int32_t B, int32_t T, int32_t C,
                      int32_t n_rows, float scale, int32_t accumulate, void *stream);
/* the same with the scale read from device memory (scale_dev[0]): a learnable scale -- the decoder's pos_embed_alpha,
 * transformer.py:795-796 -- without a device-to-host read in the middle of the step */
int set_embedding_bct_dev_scale(const int64_t *idx, const float *table, float *out, int32_t B, int32_t T, int32_t C,
                                int32_t n_rows, const float *scale_dev, int32_t accumulate, void *stream);
/* mask[b][t] = (sum_c |x[b][c][t]|) > 0 ? 1 : 0     (conv.py:58,108) */
int set_abs_sum_mask(const float *x, float *mask, int32_t B, int32_t C, int32_t T, void *stream);
/* mask[i] = idx[i] > 0 ? 1 : 0                       (fs.py:87,93 ; spec_denoiser.py:163,166) */
int set_index_mask(const int64_t *idx, float *mask, int64_t n, void *stream);
/* out[b][c][t] = mel2ph[b][t] > 0 ? enc[b][c][mel2ph[b][t]-1] : 0   (align_ops.py:21-25) */
int set_expand_states(const float *enc, const int64_t *mel2ph, float *out, int32_t B, int32_t C,
                      int32_t T_txt, int32_t T, void *stream);
/* out[b][c][t] = (x[b][c][t] + (add ? add[b][c] : 0)) * (mask ? mask[b][t] : 1)   (fs.py:91,98,102) */
int set_add_chan_mask(const float *x, const float *add, const float *mask, float *out, int32_t B, int32_t C,
                      int32_t T, void *stream);
/* masked_dur[b][j] = #{t : mel2ph[b][t]*(1-(int)tmask[b][t]) == j+1} * (txt[b][j] != 0)
 * (fs.py:136-137, utils/audio/align.py:71-90).  int64 out [B][T_txt]. */
int set_masked_dur(const int64_t *mel2ph, const float *tmask, const int64_t *txt, int64_t *out, int32_t B,
                   int32_t T, int32_t T_txt, void *stream);
/* pitch bins: f = clamp(2^f0,50,900); f = 0 where uv>0 or pad; mel-scale -> bin 1..255
 * (utils/audio/pitch/utils.py:17-28,71-82 ; fs.py:160-163,182-183).
 * f0_in/uv_in [B][T]; tmask optional: inputs are first multiplied by (1-tmask) (fs.py:160-161);
 * uv_from_logit: treat uv_in as logits (uv = uv_in > 0, fs.py:186); pad optional int64 mel2ph (pad where == 0);
 * outputs optional: f0_denorm fp32 [B][T], coarse int64 [B][T]. */
int set_pitch_coarse(const float *f0_in, const float *uv_in, const float *tmask, const int64_t *mel2ph_pad,
                     int32_t uv_from_logit, float *f0_denorm, int64_t *coarse, int64_t n, void *stream);
/* [B][T][C] <-> [B][C][T] */
int set_transpose_btc_to_bct(const float *in, float *out, int32_t B, int32_t T, int32_t C, void *stream);
int set_transpose_bct_to_btc(const float *in, float *out, int32_t B, int32_t C, int32_t T, void *stream);
/* out = (a + b + c) / div  (b, c optional)           (hifigan.py:131-137 MRF mean `xs / num_kernels`) */
int set_sum_scale(const float *a, const float *b, const float *c, float *out, float div, int64_t n, void *stream);
/* out[i] = a[i]*(1-m[i]) + b[i]*m[i] ; m broadcast over `inner` trailing elements
 * (fs.py:176-177 ; tasks/speech_editing/spec_denoiser.py:53) */
int set_blend_mask(const float *a, const float *b, const float *m, float *out, int64_t n, int64_t inner, void *stream);
/* out[i] = x[i] * (1 - m[i / inner])                 (spec_denoiser.py:164 ref_mels*(1-mask)) */
int set_mul_one_minus_mask(const float *x, const float *m, float *out, int64_t n, int64_t inner, void *stream);
/* LengthRegulator: mel2ph[b][p] = sum_j (j+1) * [cs_prev_j <= p < cs_j], dur = round(dur)*(1-pad)
 * (nar_tts_modules.py:42-72).  Two calls: set_dur_total writes total[b] (int64) = sum_j dur_j;
 * the host reads max(total) to size the output (the reference sizes a tensor the same way, :69). */
int set_dur_total(const float *dur, const int64_t *txt, int64_t *total, int32_t B, int32_t T_txt, void *stream);
int set_length_regulate(const float *dur, const int64_t *txt, int64_t *mel2ph, int32_t B, int32_t T_txt,
                        int32_t T_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * DiffNet + diffusion loop
 * ------------------------------------------------------------------------------------------------ */
/* out[j][n] = sin(t[n]*w_j) (j < dim/2), cos(t[n]*w_{j-dim/2}) (j >= dim/2), w_j = exp(-j ln(1e4)/(dim/2-1))
 * (diffnet.py:34-46).  t: fp32 [n] (host fills it with the integer step ids).  out: [dim][n]. */
int set_sinusoid_embed(const float *t, float *out, int32_t dim, int32_t n, void *stream);

/* z = sigmoid(y[:, :C]) * tanh(y[:, C:])   y [B][2C][T] -> z [B][C][T]    (diffnet.py:76-77) */
int set_gate(const float *y, float *z, int32_t B, int32_t C, int32_t T, void *stream);
/* x_out = (x_in + o[:, :C]) / sqrt(2) ; skip (+)= o[:, C:]               (diffnet.py:80-81,128) */
int set_res_skip(const float *x_in, const float *o, float *x_out, float *skip, int32_t B, int32_t C, int32_t T,
                 int32_t first, void *stream);

/* One fused DiffNet residual layer (diffnet.py:60-81) for residual_channels == 256:
 *   y   = W_dil (*) (x_in + d) + b_dil + condproj      k=3, dilation `dil`, zero padded
 *   z   = sigmoid(y[:256]) * tanh(y[256:])
 *   o   = W_out z + b_out
 *   x_out = (x_in + o[:256]) / sqrt(2);  skip = first ? o[256:] : skip + o[256:]
 * x_in/x_out/skip: [B][256][T] (must not alias); condproj: [B][512][T] slab with batch stride cp_bs
 * (= conditioner_projection(cond) + its bias, hoisted out of the step loop: it does not depend on t);
 * d[b][c] = dstep[b*d_bs + c*d_cs]  (diffusion_projection(mlp(emb(t)))[b][c]);
 * w1p / w2p: images written by set_pack_diffnet_layer. */
typedef struct SetDiffnetLayerArgs {
    const float *x_in;
    const float *condproj;
    const float *dstep;
    const float *w1p;
    const float *b_dil;
    const float *w2p;
    const float *b_out;
    float *x_out;
    float *skip;
    int64_t cp_bs, d_bs, d_cs;
    int32_t B, T, dil, first;
    /* diagnostic, NULL unless the library was built with -DSET_PHASE_PROBE=1 (SET_E_UNSUPPORTED otherwise):
     * [gridDim.y*gridDim.x][8] uint64, wave 0 of every block ADDS the s_memtime ticks of its phases to words 0..5
     * (tile staged, GEMM1, gate, barrier + z staged, GEMM2, epilogue) */
    uint64_t *dbg_clock;
} SetDiffnetLayerArgs;
int set_diffnet_layer(const SetDiffnetLayerArgs *args, void *stream);
/* floats needed for w1p (512x768) and w2p (512x256) */
int64_t set_diffnet_w1p_size(void);
int64_t set_diffnet_w2p_size(void);
/* pack dilated_conv.weight [512][256][3] and output_projection.weight [512][256][1] (diffnet.py:63,66) */
int set_pack_diffnet_layer(const float *w_dil, const float *w_out, float *w1p, float *w2p, void *stream);
/* every layer of a stack in one launch per image family: layer q's weights at w_dil + q wd_ls / w_out + q wo_ls (element strides),
 * w1p / w2p = [L][set_diffnet_w1p_size()] / [L][set_diffnet_w2p_size()]; w1w / w2w (both or neither) = the Winograd images
 * [L][set_diffnet_w1w_size()] / [L][512 * 256] of set_pack_diffnet_layer_wino */
int set_pack_diffnet_layers(const float *w_dil, const float *w_out, int64_t wd_ls, int64_t wo_ls, float *w1p, float *w2p,
                            float *w1w, float *w2w, int32_t L, void *stream);

/* All L residual layers of one DiffNet pass in ONE persistent launch (residual_channels == 256).
 * Up to 2 x #CU resident blocks pull (layer, tile) tasks in layer-major order from an atomic queue; a task
 * (l, i) starts when tiles i-1, i, i+1 of layer l-1 are published (per-tile epoch flags; agent-scope
 * release/acquire), so no CU idles at layer boundaries (a 416-tile layer does not divide over 256 CUs).
 * Tiles are 64 frames when a layer has >= 3 x #CU of them, else 32 frames (keeps runnable tasks > workers).
 * Layer l reads (l even ? xa : xb) and writes the other buffer; skip accumulates in place; results are
 * bit-identical to L calls of set_diffnet_layer.  sync_ws: >= 16 + 2*B*ceil(T/32) int32, zeroed by the call;
 * sync_ws[1] != 0 afterwards means a dependency wait timed out (SET_E_LAUNCH is NOT raised asynchronously). */
typedef struct SetDiffnetStackArgs {
    float *xa, *xb, *skip;        /* [B][256][T] each */
    const float *condproj;        /* layer l, batch b slab at condproj + l*cp_ls + b*cp_bs : [512][T] */
    const float *dstep;           /* d[l][b][c] = dstep[l*d_ls + b*d_bs + c*d_cs] */
    const float *w1p_all;         /* [L][512*768]  packed (set_pack_diffnet_layer) */
    const float *w2p_all;         /* [L][512*256] */
    const float *b_dil_all;       /* [L][512] */
    const float *b_out_all;       /* [L][512] */
    int32_t *sync_ws;
    int64_t cp_bs, cp_ls, d_bs, d_cs, d_ls;
    int32_t B, T, L, dilation_cycle_length;
    /* optional Winograd F(2,3) images (set_pack_diffnet_layer_wino), [L][512*256*4] and [L][512*256]: when both are
     * given, dilation_cycle_length <= 4 and the batch has at least 0.68 64-frame tiles per CU, the k=3 conv runs as four
     * 512x256 GEMMs over output pairs (2/3 of its MACs); results then agree with the direct kernels to fp32
     * rounding (a few 1e-6), not bit for bit.  SET_AMD_WINO=0 in the environment disables it. */
    const float *w1w_all;
    const float *w2w_all;
    /* optional, Winograd kernel only (training forward): x_all [L+1][B][256][T] replaces the xa/xb ping-pong (layer l
     * reads slab l, writes slab l+1; slab 0 = input), save_y [L][B][512][T] receives the gate/filter pre-activations
     * and save_z [L][B][256][T] the gated activations, i.e. what the backward pass needs (diffnet.py:73-77). */
    float *x_all;
    float *save_y;
    float *save_z;
    /* optional sticky error word (never cleared by the library): set to 1 if a dependency wait ran into its spin
     * limit and the launch gave up (sync_ws[1] says the same for the last launch only) */
    int32_t *err_flag;
    /* optional, small batches (4*B*ceil(T/32) <= 2 x #CU): row-split images [L][512*768] / [L][512*256] in the layout
     * [32-row block v = 4w + rb][k-step][lane] (the same values as w1p_all / w2p_all, which are [w][k-step][lane][rb])
     * plus a workspace z_ws of B*ceil(T/32)*256*32 floats.  Every 32-frame tile is then computed by four co-operating
     * blocks (one 32-row block per wave), bit-identical to the direct kernels.  SET_AMD_SPLIT=0 disables it. */
    const float *w1s_all;
    const float *w2s_all;
    float *z_ws;
    /* optional split-operand images [L][set_diffnet_layer_x3_image_size(x3_mode)] 16-bit (set_pack_diffnet_layer_x3): every
     * fp32 weight and activation is carried as a sum of 16-bit pieces and every product is formed by several 16-bit MFMAs
     * with fp32 accumulation -- fp32-equivalent accuracy (error against fp64 not larger than the fp32 MFMA chain's) at a
     * fraction of the fp32 matrix-pipe time:
     *   x3_mode 3: three bf16 pieces, six products (fp32 range, error ~2^-23 per product);
     *   x3_mode 2: two fp16 pieces, three products (error ~2^-21 per product; an activation of magnitude >= 32768 sets
     *              *err_flag = 2 instead of overflowing silently; weights are pre-scaled by a power of two at pack time).
     * Used from the Winograd crossover on (batches that fill the chip); results agree with the fp32 kernels to fp32
     * rounding, not bit for bit.  SET_AMD_X3=0 disables it, =2 forces it at any size. */
    const void *wx3_all;
    int32_t x3_mode;
    /* != 0: xa, xb and skip are in the channel-quad layout on input and output -- element (b, c, t) at float
     * b*256*T + ((c >> 2)*T + t)*4 + (c & 3), 16-byte aligned -- so that the kernel's accesses are 16 bytes wide.  Only the Winograd
     * form of the two-piece fp16 split-operand kernel (x3_mode 2, dilation_cycle_length 1, even T, 64- or 96-frame tiles) honours it;
     * with any other plan the call returns SET_E_INVALID.  0 (the default): [B][256][T]. */
    int32_t xs_q4;
} SetDiffnetStackArgs;
int set_diffnet_stack(const SetDiffnetStackArgs *args, void *stream);
int64_t set_sizeof_diffnet_stack_args(void);

/* which kernel set_diffnet_stack picks for this shape on the current device: 0 direct/64-frame tiles,
 * 1 direct/32-frame tiles, 2 Winograd, 3 row-split (diagnostics: bench.py names the kernel in its roofline object);
 * 4 split-operand 3 x bf16, 5 split-operand 2 x fp16; images: bit 0 = Winograd images given, bit 1 = row-split images +
 * z_ws given, bit 2 = split-operand images of mode 3 given, bit 3 = of mode 2 */
int64_t set_diffnet_layer_x3_image_size(int32_t mode); /* 16-bit elements per layer (mode 2 or 3; -1 otherwise) */
/* k1 / k2: the weights of the dilated conv / the output projection are multiplied by 2^k before they are split (mode 2: pick
 * k so that max |w| 2^k is in [8, 16), which keeps the residual pieces of all but the tiniest weights normal; mode 3: 0) */
int set_pack_diffnet_layer_x3(const float *w_dil /*[512][256][3]*/, const float *w_out /*[512][256]*/, void *img, int32_t mode,
                              int32_t k1, int32_t k2, void *stream);
int set_diffnet_stack_variant(int B, int T, int dilation_cycle_length, int images);
/* Non-zero when the split-operand kernel of variant 5 runs GEMM 1 in its Winograd F(2,3) form for this shape (diffnet_stack_x3v_kernel: the
 * k = 3 dilated conv of diffnet.py:70 over output pairs, 3/4 of the layer's matrix instructions; dilation 1, even T): the number of 32-frame
 * column blocks per tile -- 3 (96-frame tiles: shapes with a tile chain for every CU) or 2 (64-frame tiles); 0 = the direct form
 * (SET_AMD_X3_WINO=0 pins it, =2 / =3 pin the tile width).  `images` as for set_diffnet_stack_variant. */
int set_diffnet_stack_x3_winograd(int B, int T, int dilation_cycle_length, int images);
int64_t set_diffnet_w1w_size(void);
int set_pack_diffnet_layer_wino(const float *w_dil, const float *w_out, float *w1w, float *w2w, void *stream);

/* posterior step (spec_denoiser.py:86-101):  x_prev = c1*x0 + c2*x_t + (t != 0) * exp(0.5*logvar) * eps
 * per-batch scalars coef4[b*coef_bs + {0,1,2,3}] = {c1, c2, logvar, nonzero} (coef_bs = 0: shared by the
 * batch); eps == NULL -> counter-based Philox4x32-10 + Box-Muller noise keyed by (seed, offset + i/4).
 * x_prev may alias x_t. */
int set_posterior_step(const float *x0, const float *x_t, const float *eps, const float *coef4, int64_t coef_bs,
                       float *x_prev, int32_t B, int64_t per_batch, uint64_t seed, uint64_t offset, void *stream);
/* x_t = a[b]*x_start + s[b]*eps   (q_sample, spec_denoiser.py:126-132); ab2[b] = {a, s}; optional * nonpad[b][t] */
int set_q_sample(const float *x_start, const float *eps, const float *ab2, const float *nonpad, float *x_t,
                 int32_t B, int32_t M, int32_t T, void *stream);
/* fill with N(0,1): Philox4x32-10 + Box-Muller (throughput runs; spec_denoiser.py:180) */
int set_randn(float *out, int64_t n, uint64_t seed, uint64_t offset, void *stream);
/* Graph capture of a training step: every Philox kernel launched through set_randn / set_posterior_step / set_dropout, and the fused
 * step boundary of set_diffusion_loop (which replaces set_posterior_step there), adds the device word *dev_word to its seed argument
 * (NULL = off, the default).  A captured step carries the seeds of the step it was captured at; the
 * replay of step k stores (seed_k - seed_captured) in the word before it launches the graph and draws exactly the numbers the eager
 * step k draws.  Process-wide; the word must stay allocated while it is set. */
int set_rng_seed_delta(const uint64_t *dev_word);
/* Host-side stream ordering (the training path's leaf stream, leaf_stream.leaf_work): work enqueued on `after` from now on waits for
 * everything enqueued on `first` so far (hipEventRecord + hipStreamWaitEvent on a cached event; slot < 32 selects the event, one per
 * direction and device: slot s belongs to device s / 2 and its event is created there, whatever the calling thread's current device is).
 * Capturable: inside a stream capture the pair is a cross-stream edge. */
int set_stream_order(void *first, void *after, int32_t slot);
/* Progress markers of a stream (round 6; the leaf stream's operand bookkeeping, leaf_stream.leaf_work -- the reference's autograd engine
 * frees a backward operand as soon as its node has run, utils/commons/trainer.py:340-350 `loss.backward()`): set_stream_mark records marker
 * `slot` (0 .. 63, an event of device `dev`, created on first use) on `stream`; set_stream_mark_done(slot) returns 1 once everything enqueued on
 * that stream before the mark has finished, 0 while it has not, < 0 on error (never blocks). */
int set_stream_mark(void *stream, int32_t slot, int32_t dev);
int set_stream_mark_done(int32_t slot);
/* a non-blocking stream of the lowest priority of the current device (the leaf stream); never destroyed */
int set_stream_create_low_priority(void **out);

/* Whole reverse loop (spec_denoiser.py:178-184 + p_sample :103-108 + DiffNet.forward diffnet.py:110-132)
 * for residual_channels == 256.  All weights pre-packed by the caller; workspaces provided by the caller.
 * Launch sequence: input projection once, then per step {layer stack (set_diffnet_stack, or L set_diffnet_layer
 * launches when persistent == 0), step boundary}.  The step boundary -- skip projection + output projection +
 * posterior update (explicit or Philox noise) + the NEXT step's input projection -- is one fused kernel when
 * T % 4 == 0 and M <= 96 (bit-identical to the separate set_conv1d / set_posterior_step launches it replaces, which
 * remain the path for other shapes; SET_AMD_FUSED_BOUNDARY=0 forces them). */
typedef struct SetDiffLoopArgs {
    /* problem */
    int32_t B, T, M, L, steps, dilation_cycle_length;
    /* state */
    float *x;              /* [B][M][T]  in: x_T, out: x_0 */
    const float *noise;    /* optional explicit eps: [steps][B][M][T] in execution order (i = steps-1..0); NULL -> Philox */
    uint64_t seed;
    const float *condproj; /* [B][L*512][T]  hoisted conditioner projections (+bias) */
    const float *dstep;    /* [L*256][steps] : column s = diffusion_projection_l(mlp(emb(s))) */
    const float *coef4;    /* [steps][4] host-computed {c1, c2, logvar, nonzero} per step id, DEVICE pointer */
    /* packed weights */
    const float *w_in_p;   /* input_projection packed (Cout 256, Cin M, K 1) */
    const float *b_in;
    const float *w1p_all;  /* [L][512*768] packed dilated-conv weights (set_pack_diffnet_layer) */
    const float *w2p_all;  /* [L][512*256] packed output-projection weights */
    const float *b_dil_all; /* [L][512] */
    const float *b_out_all; /* [L][512] */
    const float *w1w_all;   /* optional Winograd images (see SetDiffnetStackArgs), used by the persistent path */
    const float *w2w_all;
    const float *w1s_all;   /* optional row-split images + workspace (see SetDiffnetStackArgs), small batches */
    const float *w2s_all;
    float *z_ws;
    const void *wx3_all;    /* optional split-operand images (see SetDiffnetStackArgs), batches that fill the chip */
    int32_t x3_mode;
    /* optional set_pack_conv_weight_x2 images of skip_projection (256 x 256), output_projection (M x 256) and
     * input_projection (256 x M): with x3_mode == 2 the fused step boundary then runs on the two-piece fp16 operands as well
     * (SET_AMD_BOUNDARY_X2=0 keeps the fp32 MFMA boundary kernel); the opt-in bf16 loop (img16_all) takes it whenever the images are
     * given -- it can raise err_flag = 2 (an activation outside the fp16 split range), which the caller must read and answer by
     * repeating the loop without these images */
    const void *w_skip_x2, *w_outp_x2, *w_in_x2;
    const float *w_skip_p; /* skip_projection packed */
    const float *b_skip;
    const float *w_outp_p; /* output_projection packed (Cout M, Cin 256) */
    const float *b_outp;
    /* workspaces, each [B][256][T] floats */
    float *ws_x0, *ws_x1, *ws_skip, *ws_h;
    float *ws_x0pred; /* [B][M][T] */
    /* optional: HOST array [steps] receiving the wall time in ms of the L-layer span of each step (hipEvent
     * pairs on the launching stream; mean over utterance groups); the call then synchronises before returning */
    float *layer_span_ms;
    /* optional: HOST float receiving the wall time in ms of the whole loop (event pair on `stream`); synchronises */
    float *loop_ms;
    /* utterance groups (<= 8; 0/1 = one): the batch is split into n_groups contiguous slices that run as
     * independent chains on auxiliary HIP streams (forked from / joined to `stream` with events), so the tail of one
     * group's layer launch overlaps the next layer of another group.  Results are bit-identical for any n_groups. */
    int32_t n_groups;
    /* persistent != 0: run the L layers of every step as one set_diffnet_stack launch (needs sync_ws,
     * >= 160 + 2*B*ceil(T/32) int32); 0: one set_diffnet_layer launch per layer */
    int32_t persistent;
    int32_t *sync_ws;
    int32_t *err_flag; /* optional sticky error word, see SetDiffnetStackArgs.err_flag (1: time-out, 2: activation out of the
                        * fp16 split range) */
    /* bf16-operand loop (opt-in, NOT the parity path; img16_all != NULL selects it): every residual layer runs as one
     * set_diffnet_layer_fwd_bf16 launch reading cond [B][192][T] (the conditioner projection is a K-chunk of the layer's
     * GEMM, condproj is not used), images [L][set_diffnet_layer_bf16_image_size()], conditioner biases [L][512] */
    const float *cond;
    const void *img16_all;
    const float *b_cond_all;
    /* bf16 loop: with bf16_ws_floats >= set_diffnet_layers_bf16_scratch_floats(B, T, 0, n, dilation_cycle_length) for the group size
     * n in use and dilation_cycle_length <= 2 the layers run set_diffnet_layers_bf16_plan() per launch
     * (set_diffnet_layers_fwd_bf16); NULL: one launch per layer.  SET_AMD_BF16_FUSE=n overrides the group size (1 = per layer). */
    float *bf16_ws;
    int64_t bf16_ws_floats;
    /* != 0: the library may keep ws_x0, ws_x1 and ws_skip in the channel-quad layout of SetDiffnetStackArgs.xs_q4 (they are scratch: only
     * their layout changes, x does not).  It does so for a chain whose layer stack runs the Winograd split-operand kernel and whose step
     * boundary is the fused two-piece fp16 one; every other chain keeps [B][256][T].  The workspaces must then be 16-byte aligned.
     * SET_AMD_WS_Q4=0 in the environment keeps the plain layout.  0 (the default): plain. */
    int32_t ws_q4;
} SetDiffLoopArgs;
int set_diffusion_loop(const SetDiffLoopArgs *args, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Training: backward kernels, losses, optimizer.
 * Input gradients of a convolution are a set_conv1d call on the output gradient with transposed weight
 * addressing (w_sco <-> w_sci) and negated dil / pad; the pieces below are what set_conv1d cannot express.
 * ------------------------------------------------------------------------------------------------ */
/* dW[co][ci][tap] += sum_{b,t} G[b][co][t] * P(X[b][ci][t + tap*dil - pad]),  P as in set_conv1d
 * (chan_add, pro).  impl SET_IMPL_MFMA: split-K GEMM on fp32 MFMA with fp32 atomics; else one thread per weight. */
int set_conv1d_wgrad(const float *g, const float *x, const float *chan_add, float *dw, int32_t B, int32_t Cin,
                     int32_t Cout, int32_t K, int32_t dil, int32_t pad, int32_t T, int32_t T_in, int32_t pro,
                     float pro_param, int32_t impl, void *stream);

/* Deterministic weight gradient (same arithmetic contract as set_conv1d_wgrad, MFMA path): the frames are cut into S
 * slices, slice z writes its partial dW to scratch[z][Cout][Cin][K] with plain stores, then dW += sum_z scratch[z] in
 * slice order -- no atomics, bit-identical from run to run.  dtype SET_DTYPE_F32: fp32 MFMA operands; SET_DTYPE_BF16:
 * g and x rounded to bf16 (RNE) on the way into LDS, fp32 accumulation.  `scratch` must hold
 * set_conv1d_wgrad_scratch_floats(...) floats and may be reused by the next call on the same stream. */
int64_t set_conv1d_wgrad_scratch_floats(int32_t B, int32_t Cin, int32_t Cout, int32_t K, int32_t T, int32_t dtype);
int set_conv1d_wgrad_det(const void *g, const void *x, const float *chan_add, float *dw, int32_t B, int32_t Cin,
                         int32_t Cout, int32_t K, int32_t dil, int32_t pad, int32_t T, int32_t T_in, int32_t pro,
                         float pro_param, int32_t dtype, float *scratch, int64_t scratch_floats, void *stream);
/* The same for `groups` equal GEMMs in ONE launch (+ one ordered reduce) -- the weight gradients of all L residual layers of the
 * DiffNet at once: group q reads g + q g_gs, x + q x_gs, chan_add + q add_gs and ADDS into dw + q dw_gs (strides in elements of the
 * respective type).  With L x the tiles a few frame slices per group fill the chip: 13 - 64 slices per GEMM become 2 - 4 (as much
 * less partial-sum traffic), 120 launches become 6.  bf16 dtypes only, no prologue. */
int64_t set_conv1d_wgrad_grouped_scratch_floats(int32_t groups, int32_t B, int32_t Cin, int32_t Cout, int32_t K, int32_t T);
int set_conv1d_wgrad_det_grouped(const void *g, const void *x, const float *chan_add, float *dw, int32_t groups, int64_t g_gs,
                                 int64_t x_gs, int64_t add_gs, int64_t dw_gs, int32_t B, int32_t Cin, int32_t Cout, int32_t K,
                                 int32_t dil, int32_t pad, int32_t T, int32_t T_in, int32_t dtype, float *scratch,
                                 int64_t scratch_floats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused DiffNet residual layer, bf16 MFMA operands, for the TRAINING path (residual_channels 256, hidden_size 192,
 * kernel 3; modules/speech_editing/spec_denoiser/diffnet.py:60-81 and its transpose).  One launch per layer and
 * direction; see csrc/diffnet_bf16.hip for the arithmetic and the HBM traffic it removes.
 *   img    packed bf16 weight images of ONE layer (set_pack_diffnet_layer_bf16; set_diffnet_layer_bf16_image_size()
 *          bf16 elements): forward GEMM 1 / GEMM 2 and the three transposed images of the backward
 *   y16/z16/dy16/do16   bf16 [B][512|256][T]: pre-gate, gated activation, and their gradients (MFMA operands of the
 *          weight-gradient GEMMs, inputs of the gate derivative)
 *   dstep  d[b][c] = dstep[b*d_bs + c*d_cs]   (diffusion_projection(step embedding), per utterance)
 * ------------------------------------------------------------------------------------------------ */
typedef struct SetDiffnetLayerBf16Args {
    const float *x_in;   /* [B][256][T] */
    float *x_out;        /* [B][256][T] = (x_in + o_res) / sqrt2 */
    float *skip;         /* [B][256][T] += o_skip (first != 0: = o_skip) */
    const float *cond;   /* [B][192][T] */
    const float *dstep;
    const void *img;
    const float *b_dil, *b_cond, *b_out; /* [512] each */
    uint16_t *y16;       /* [B][512][T] bf16 out (both NULL: inference, nothing is saved) */
    uint16_t *z16;       /* [B][256][T] bf16 out */
    int64_t d_bs, d_cs;
    int32_t B, T, dil, first;
} SetDiffnetLayerBf16Args;
int64_t set_sizeof_diffnet_layer_bf16_args(void);
int64_t set_diffnet_layer_bf16_image_size(void);
int set_pack_diffnet_layer_bf16(const float *wdil /*[512][256][3]*/, const float *wcond /*[512][192]*/,
                                const float *wout /*[512][256]*/, void *img, void *stream);
/* L layers in one launch: layer q reads wdil + q * sdil (etc., element strides between the layers' tensors) and writes image q of
 * img [L][image_size] -- the flat optimizer lays every layer's parameters out at one stride, so the whole stack is re-rounded by ONE
 * launch after an update instead of L. */
int set_pack_diffnet_layers_bf16(const float *wdil, const float *wcond, const float *wout, int64_t sdil, int64_t scond, int64_t sout,
                                 void *img, int32_t L, void *stream);
int set_diffnet_layer_fwd_bf16(const SetDiffnetLayerBf16Args *args, void *stream);
/* Several consecutive residual layers per launch (bf16 operands, inference: nothing is saved): a block keeps its tile on chip for
 * `nl` (<= 16) layers l0 .. l0 + nl - 1 (x and the conditioner are read once; the fp32 residual rows stay in registers; the running
 * skip sum stays in registers (64-frame tiles) or goes through L2 per layer (128-frame tiles)) and stores the tile - 2 H frames whose
 * receptive field stayed inside the tile, H = sum of the dilations 2^((l0 + m) % dilation_cycle_length), m = 1 .. nl - 1.  The tile
 * width is chosen per launch: 128 frames when B * ceil(T / (128 - 2 H)) blocks still fill 3/4 of the CUs, else 64.  Same arithmetic
 * per frame as nl set_diffnet_layer_fwd_bf16 launches (x AND the skip sum bit-identical at both tile widths: the 128-frame shape adds
 * the layers' skip contributions in layer order as well).  Arrays are the per-layer operands of those launches laid out one layer after the other: img
 * [nl][image_size], b_dil / b_cond / b_out [nl][512], dstep of layer l at dstep + l * d_ls (l counted from layer 0 of the network).
 * x_in != x_out.  scratch >= set_diffnet_layers_bf16_scratch_floats(B, T, l0, nl, dilation_cycle_length) floats (128-frame tiles:
 * a block's private copy of its skip rows between the layers of the group).
 * set_diffnet_layers_bf16_plan(B, T, L, dilation_cycle_length): the group size the reverse loop uses for a stack of L layers. */
typedef struct SetDiffnetLayersBf16Args {
    const float *x_in;   /* [B][256][T] input of layer l0 */
    float *x_out;        /* [B][256][T] output of layer l0 + nl - 1 */
    float *skip;         /* [B][256][T] += sum of the nl skip contributions (first != 0: =) */
    const float *cond;   /* [B][192][T] */
    const float *dstep;
    const void *img;
    const float *b_dil, *b_cond, *b_out;
    float *scratch;
    int64_t scratch_floats;
    int64_t d_bs, d_cs, d_ls;
    int32_t B, T, l0, nl, dilation_cycle_length, first;
} SetDiffnetLayersBf16Args;
int64_t set_sizeof_diffnet_layers_bf16_args(void);
int64_t set_diffnet_layers_bf16_scratch_floats(int32_t B, int32_t T, int32_t l0, int32_t nl, int32_t dilation_cycle_length);
int32_t set_diffnet_layers_bf16_plan(int32_t B, int32_t T, int32_t L, int32_t dilation_cycle_length);
int set_diffnet_layers_fwd_bf16(const SetDiffnetLayersBf16Args *args, void *stream);
/* Phase probes.  The shipped library holds no phase stamps: these setters return SET_OK for NULL and SET_E_UNSUPPORTED otherwise.  A
 * library whose source file was built with -DSET_PHASE_PROBE=1 (tools/build_exp.sh) takes a device buffer of uint64 words; the sampled
 * wave sums the s_memtime ticks (100 MHz) of its phases in registers and ADDS them to the buffer when the kernel ends (NULL = off).
 * bf16: block (1,1), wave 0 of set_diffnet_layer_fwd_bf16 -> buf[0..4] = stage, GEMM 1, gate, GEMM 2, epilogue; of
 * set_diffnet_layers_fwd_bf16, layers m >= 1 of the group -> buf[0..4] = init + barrier, GEMM 1, gate, GEMM 2, epilogue, layer count in
 * buf[7], and the same of wave 4 in buf[8..15] */
int set_debug_bf16_phase_buffer(uint64_t *buf);
/* wave 0 of one block (tile 1, part 1) of the fp32 row-split stack kernel, summed over the layers: buf[0..7] = wait for the previous
 * layer, stage, GEMM 1, gate + z publish, wait for z, z load, GEMM 2, epilogue + publish */
int set_debug_split_phase_buffer(uint64_t *buf);
/* wave 0 of block 0 of the split-operand stack kernels, summed over its tasks: buf[0..5] = claim + wait, stage, GEMM 1, gate, GEMM 2,
 * epilogue + publish, task count in buf[7], sub-phases in buf[8..12] (csrc/diffnet_x3.hip); the two-piece row-split kernel: the eight
 * phases of set_debug_split_phase_buffer.  -DSET_PHASE_PROBE=2: rows of 32 dwords, the one-task timeline of tools/x3_timeline_probe.py */
int set_debug_x3_phase_buffer(uint64_t *buf);
/* wave 0 of every 16th block of batch row 1 of the fused ResBlock-pair kernel (atomic adds): buf[0..4] = x chunk wait + split, GEMM 1
 * issue, GEMM 1 drain + epilogue 1, GEMM 2 issue, GEMM 2 drain + epilogue 2, block count in buf[7] */
int set_debug_resblock_phase_buffer(uint64_t *buf);
/* wave 0 of block (1,1,1) of the staged bf16 conv kernel: buf[0] = prologue, buf[1..5] = barrier 1, wait for the stage's loads + LDS
 * writes, barrier 2, issue of the next stage's loads, fragment reads + MFMAs (summed over the stages), stage count in buf[6] */
int set_debug_conv_phase_buffer(uint64_t *buf);

typedef struct SetDiffnetLayerBf16BwdArgs {
    const float *dx_out; /* [B][256][T] gradient w.r.t. x_out; NULL = zero (the last layer's x_out feeds nothing) */
    const float *dskip;  /* [B][256][T] gradient w.r.t. the skip sum (the same tensor for every layer) */
    const uint16_t *y16; /* saved by the forward */
    const void *img;
    float *dx;           /* [B][256][T] out: gradient w.r.t. x_in (= w.r.t. x_in + d) */
    uint16_t *dy16;      /* [B][512][T] bf16 out: gradient w.r.t. the pre-gate y */
    uint16_t *do16;      /* [B][512][T] bf16 out: [dx_out / sqrt2 ; dskip] */
    float *dcond;        /* [B][192][T] (+)= Wcond^T dy   (dcond_first != 0: written, not accumulated) */
    float *part_dbo;     /* [B * tiles][512] per-tile sums of d_o over frames  (bias gradient of the output projection) */
    float *part_dby;     /* [B * tiles][512] per-tile sums of dy               (bias gradient of dilated conv = conditioner) */
    float *part_dd;      /* [B * tiles][256] per-tile sums of Wdil^T (*) dy    (gradient of the per-utterance step offsets) */
    int32_t B, T, dil, dcond_first;
} SetDiffnetLayerBf16BwdArgs;
int64_t set_sizeof_diffnet_layer_bf16_bwd_args(void);
int32_t set_diffnet_layer_bwd_bf16_tiles(int32_t T, int32_t dil); /* tiles per utterance = rows per b of the part_* arrays */
int set_diffnet_layer_bwd_bf16(const SetDiffnetLayerBf16BwdArgs *args, void *stream);
/* the ordered partial sums of one layer's backward in one launch: db_out[512] += sum part_dbo, db_dil[512] and db_cond[512] +=
 * sum part_dby (over all B*tiles rows), dd[b*dd_bs + c] = sum over the tiles of utterance b of part_dd (c < 256) */
int set_diffnet_layer_bwd_reduce(const float *part_dbo, const float *part_dby, const float *part_dd, int32_t B, int32_t tiles,
                                 float *db_out, float *db_dil, float *db_cond, float *dd, int64_t dd_bs, void *stream);
/* the same for L layers swept with one tile count, in ONE launch: partials [L][B*tiles][512|512|256], layer q's targets at
 * db_* + q * s_* (element strides between the layers' bias gradients) and dd + q * dd_ls */
int set_diffnet_layers_bwd_reduce(const float *part_dbo, const float *part_dby, const float *part_dd, int32_t B, int32_t tiles, int32_t L,
                                  float *db_out, int64_t s_out, float *db_dil, int64_t s_dil, float *db_cond, int64_t s_cond, float *dd,
                                  int64_t dd_bs, int64_t dd_ls, void *stream);
/* out[g][j] (+)= scale * sum_{r < rows} part[(g*rows + r)*cols + j]  in row order (deterministic reduction of per-tile partials) */
int set_partial_rows_sum(const float *part, float *out, int32_t groups, int32_t rows, int32_t cols, int32_t accumulate,
                         float scale, void *stream);

/* Every residual layer's diffusion_projection of the step embedding in one launch (reference: modules/speech_editing/spec_denoiser/
 * diffnet.py:66,72 -- one Linear(C, C) per layer on the [N, C] embedding):  out[n][l*C + co] = b_l[co] + sum_ci W_l[co][ci] h[ci][n]
 * with h [C][N], W_l = w + l*w_ls ([C][C] row-major), b_l = b + l*b_ls, out [N][L*C].  fp32 FMAs.  C % 64 == 0, N <= 64.
 * ..._bwd: dh[ci][n] = sum_{l,co} W_l[co][ci] g[n][l*C+co] (partials in scratch, summed in (l, co-quarter) order),
 * dW_l[co][ci] += sum_n g[n][l*C+co] h[ci][n], db_l[co] += sum_n g[n][l*C+co]; scratch >= set_step_proj_bwd_scratch_floats floats. */
int set_step_proj_fwd(const float *h, const float *w, int64_t w_ls, const float *b, int64_t b_ls, float *out, int32_t L, int32_t C,
                      int32_t N, void *stream);
int64_t set_step_proj_bwd_scratch_floats(int32_t L, int32_t C, int32_t N);
/* the backward in two entry points: dh feeds the backward chain, dW / db are parameter gradients the host side may launch on its
 * second stream */
int set_step_proj_bwd_dh(const float *g, const float *w, int64_t w_ls, float *dh, float *scratch, int32_t L, int32_t C, int32_t N,
                         void *stream);
int set_step_proj_bwd_dw(const float *h, const float *g, float *dw, int64_t dw_ls, float *db, int64_t db_ls, int32_t L, int32_t C,
                         int32_t N, void *stream);

/* bf16 weight image for SET_IMPL_BF16: wp[tap][chunk][row][32] bf16, row < Cout rounded up to 128, chunk < ceil(Cin/32),
 * zero padded; ..._size returns the number of bf16 ELEMENTS (2 bytes each). */
int64_t set_packed_conv_weight_bf16_size(int32_t Cout, int32_t Cin, int32_t K);
int set_pack_conv_weight_bf16(const float *w, void *wp, int32_t Cout, int32_t Cin, int32_t K, int64_t w_base,
                              int64_t w_sco, int64_t w_sci, int64_t w_stap, void *stream);
/* Every weight image of the three layouts below in ONE launch (after an optimizer step, instead of one pack launch per image).
 * descs_dev: n descriptors IN DEVICE MEMORY, sorted by `start` = index of the image's first element in the concatenated element
 * space [0, total); the kinds may be mixed (elements are 4 bytes for the fp32 kinds, 2 for bf16; `start` counts elements).
 * The caller sets w, wp, w_base .. w_stap, Cout, Cin, K and `start`; set_fill_pack_desc (host) fills kind and the layout fields --
 * it is the one place that holds the padding rules of the images -- and returns the image's element count, which is what the
 * set_packed_conv_weight*_size entries return (-1: bad arguments).  `dil` matters to SET_IMG_F32_BIG only. */
#define SET_IMG_F32 0     /* fp32 small-tile: the image of set_pack_conv_weight (SET_IMPL_MFMA) */
#define SET_IMG_F32_BIG 1 /* fp32 big-tile: the image of set_pack_conv_weight_v2 (SET_IMPL_MFMA2) */
#define SET_IMG_BF16 2    /* bf16: the image of set_pack_conv_weight_bf16 (SET_IMPL_BF16) */
typedef struct SetPackDesc {
    const float *w;
    void *wp;
    int64_t w_base, w_sco, w_sci, w_stap, start;
    int32_t Cout, Cin, K, kind;
    int32_t CinP, CoutP, RB, ch_max; /* padded channels / rows; big-tile: rows per block / 128, channels per LDS chunk */
} SetPackDesc;
int64_t set_sizeof_pack_desc(void);
int64_t set_fill_pack_desc(SetPackDesc *d, int32_t kind, int32_t dil);
int set_pack_conv_weights_batch(const SetPackDesc *descs_dev, int32_t n, int64_t total, void *stream);

/* Reductions of the training path.  Every sum that feeds a loss or a gradient is ordered: the entry points below write one
 * partial result per block / slice into `scratch` and combine them in a fixed order, so the result is bit-identical from
 * run to run (what makes a resumed training run repeat the uninterrupted one exactly).  There is no form that accumulates
 * with fp32 atomics, whose last bits would depend on the arrival order of the blocks; the one exception is the split-K
 * branch of set_conv1d_wgrad (SET_IMPL_MFMA), which the training path does not take (it uses set_conv1d_wgrad_det).
 * `scratch` is required; it may be reused by the next call on the same stream.  Sizes (floats): channel_sum 2048 + C;
 * weighted_sum 1024; sumsq 2048; dur 4 B; pitch 4 ceil(B T / 256); scatter_rows B * set_scatter_rows_segments(T) * n_rows * C.
 *   set_channel_sum_det:  out[c] += sum_{b,t} x[b][c][t]   (bias gradients)
 *   set_weighted_sum_det: out[0] += sum_i x[i] * (w ? w[i/inner] : 1)
 *   set_sumsq_det:        out[0] += sum g[i]^2
 *   set_dur_loss_sums_det (speech_editing_base.py:58-90):    sums[0..3] += {sum nonpad*d^2, sum nonpad, sum wordmask*dw^2, sum wordmask}
 *   set_pitch_loss_sums_det (speech_editing_base.py:92-108): sums[0..3] += {sum nonpad*bce, sum nonpad, sum nv*|df0|, sum nv}
 *                         on channel-major pitch_pred [B][2][T] (row 0 f0, row 1 uv logit) */
int set_channel_sum_det(const float *x, float *out, int32_t B, int32_t C, int32_t T, float *scratch, void *stream);
int set_weighted_sum_det(const float *x, const float *w, float *out, int64_t n, int64_t inner, float *scratch, void *stream);
int set_sumsq_det(const float *g, float *out, int64_t n, float *scratch, void *stream);
int set_dur_loss_sums_det(const float *dur_pred, const int64_t *mel2ph, const int64_t *txt, const int64_t *word_id,
                          float *sums, int32_t B, int32_t T, int32_t T_txt, int32_t n_words, float *scratch, void *stream);
int set_pitch_loss_sums_det(const float *pp, const float *f0, const float *uv, const int64_t *mel2ph, float *sums,
                            int32_t B, int32_t T, float *scratch, void *stream);
/* Scatter-add of gradient rows, no atomics.  doutT: the gradient TRANSPOSED to [B][T][C].
 * mode 0 (embedding backward, layers.py:45-50): table[idx[b][t]][c] += scale * doutT[b][t][c]  (idx clamped to the table,
 *        padding_idx skipped), table [n_rows][C];
 * mode 1 (expand_states backward, align_ops.py:21-25): table[b][idx[b][t] - 1][c] += doutT[b][t][c] for idx > 0,
 *        table [B][n_rows][C] (the gradient of the encoder output, transposed). */
int32_t set_scatter_rows_segments(int32_t T);
int set_scatter_rows_det(const int64_t *idx, const float *doutT, float *table, int32_t B, int32_t T, int32_t C,
                         int32_t n_rows, float scale, int32_t padding_idx, int32_t mode, float *scratch, void *stream);
/* out[row] = scale * sum_t x[row][t] */
int set_row_sum(const float *x, float *out, int64_t rows, int32_t T, float scale, void *stream);
/* G = dY * mask[b][t] * alpha * [act == RELU: y > 0]   (epilogue backward of set_conv1d; act NONE or RELU) */
int set_conv_epilogue_bwd(const float *dy, const float *y, const float *mask, float *g, int32_t B, int32_t C,
                          int32_t T, int32_t act, float alpha, void *stream);
/* y = act(z) / dz = dy * act'(z)  for the SET_ACT_* codes */
int set_act_fwd(const float *z, float *y, int64_t n, int32_t act, float p, void *stream);
int set_act_bwd(const float *z, const float *dy, float *dz, int64_t n, int32_t act, float p, void *stream);
/* dz = (dy * act'(z)) * scale: act backward followed by the producing conv's output scale alpha (set_conv1d's `alpha`), one launch */
int set_act_bwd_scaled(const float *z, const float *dy, float *dz, int64_t n, int32_t act, float p, float scale, void *stream);
/* backward of set_gate: y [B][2C][T] (saved pre-gate), dz [B][C][T] -> dy [B][2C][T] */
int set_gate_bwd(const float *y, const float *dz, float *dy, int32_t B, int32_t C, int32_t T, void *stream);
/* backward of set_res_skip: dx = dx_out/sqrt2 ; d_o[:, :C] = dx_out/sqrt2 ; d_o[:, C:] = dskip */
int set_res_skip_bwd(const float *dx_out, const float *dskip, float *dx, float *d_o, int32_t B, int32_t C, int32_t T,
                     void *stream);
/* backward of set_layernorm_ch; dgamma/dbeta are accumulated (+=).  `partial` is required: scratch of
 * set_layernorm_ch_bwd_scratch(B, C, T) floats (contents irrelevant) that takes one row of dgamma/dbeta partial sums per
 * block; a second launch adds the rows in block order (NULL: SET_E_INVALID). */
int64_t set_layernorm_ch_bwd_scratch(int32_t B, int32_t C, int32_t T);
int set_layernorm_ch_bwd(const float *x, const float *gamma, const float *mask, const float *dy, float *dx,
                         float *dgamma, float *dbeta, float *partial, int32_t B, int32_t C, int32_t T, float eps,
                         void *stream);
/* the same with dx = (LayerNorm gradient) + add [B][C][T]: the residual branch of a pre-LN sub-block joins inside the launch */
int set_layernorm_ch_bwd_add(const float *x, const float *gamma, const float *mask, const float *dy, const float *add, float *dx,
                             float *dgamma, float *dbeta, float *partial, int32_t B, int32_t C, int32_t T, float eps, void *stream);
/* inverted dropout with a Philox keep-mask keyed by (seed, offset + i/4): y = keep ? x/(1-p) : 0.  Calling it on the
 * output gradient with the same (seed, offset) is the backward (nar_tts_modules.py:20,86 predictor dropout). */
int set_dropout(const float *x, float *y, int64_t n, float p, uint64_t seed, uint64_t offset, void *stream);
/* dropout on the branch of a residual sub-block (modules/commons/conv.py:57-65): y = (x + keep z/(1-p)) * mask[b][t] on [B][C][T],
 * keep = set_dropout's decision for the same (seed, offset, element index); mask may be NULL */
int set_residual_dropout(const float *x, const float *z, const float *mask, float *y, int32_t B, int32_t C, int32_t T, float p,
                         uint64_t seed, uint64_t offset, void *stream);
/* its backward: g2 = dy * mask (the residual's gradient), gz = keep g2/(1-p) (the branch's) */
int set_conv_epilogue_bwd_dropout(const float *dy, const float *mask, float *g2, float *gz, int32_t B, int32_t C, int32_t T, float p,
                                  uint64_t seed, uint64_t offset, void *stream);
/* StutterSpeech head + losses (csrc/stutter.hip): h [B][C][T] (post_net1 output), w [3][C], bias [3], labels int64 [B][T] in {0,1,2}
 * (2 = pad).  Writes logits [B][T][3]; with labels, stats[3] = {ce (mean over label != 2), focal (mean over all B*T rows), n_valid}
 * from per-block partials in scratch (set_stutter_head_scratch_floats), combined in block order.  labels NULL: logits only. */
int64_t set_stutter_head_scratch_floats(int32_t B, int32_t C, int32_t T);
int set_stutter_head_loss(const float *h, const float *w, const float *bias, const int64_t *labels, float *logits, float *stats,
                          float *scratch, int32_t B, int32_t C, int32_t T, void *stream);
/* backward from the saved logits and stats: g_ce / g_focal are device scalars (either may be NULL = 0); writes dh [B][C][T] and the
 * per-(utterance, 256-frame chunk) weight / bias partials into scratch; dw / db non-NULL: also dw[3][C] += , db[3] += (set_stutter_head_bwd_reduce) */
int set_stutter_head_loss_bwd(const float *h, const float *w, const float *logits, const int64_t *labels, const float *stats,
                              const float *g_ce, const float *g_focal, float *dh, float *dw, float *db, float *scratch, int32_t B,
                              int32_t C, int32_t T, void *stream);
int set_stutter_head_bwd_reduce(const float *scratch, float *dw, float *db, int32_t B, int32_t C, int32_t T, void *stream);
/* w[f] = (sum_m |target[f][m]|) != 0    (weights_nonzero_speech, utils/nn/seq_utils.py:33-37) */
int set_frame_weight(const float *target, float *w, int64_t frames, int32_t M, void *stream);
/* absd = |pred - target|, sgn = sign(pred - target)  (either may be NULL)   (l1_loss, speech_base.py:223-229) */
int set_l1_elem(const float *pred, const float *target, float *absd, float *sgn, int64_t n, void *stream);
/* out[i] = a[i] * (w ? w[i/inner] : 1) * (scale_dev ? scale_dev[0] : 1) * scale */
int set_scale_bcast(const float *a, const float *w, float *out, int64_t n, int64_t inner, const float *scale_dev,
                    float scale, void *stream);
/* SSIM (utils/metrics/ssim.py:12-44) on [B][H][W] images: 11x11 gaussian (sigma 1.5), zero padded.
 * `bias` (6.0, speech_base.py:247) is added to the in-range pixels of both images.
 * filter: mu1, mu2, E[x^2], E[y^2], E[xy];  map: 1 - ssim and d ssim / d(mu1, E[x^2], E[xy]);
 * bwd: dimg1 = F(gm) + 2 img1 F(g11) + img2 F(g12). */
int set_ssim_filter(const float *img1, const float *img2, float bias, float *mu1, float *mu2, float *s11, float *s22,
                    float *s12, int32_t B, int32_t H, int32_t W, void *stream);
int set_ssim_map(const float *mu1, const float *mu2, const float *s11, const float *s22, const float *s12,
                 float *one_minus, float *d_mu1, float *d_s11, float *d_s12, int64_t n, void *stream);
int set_ssim_bwd(const float *img1, const float *img2, float bias, const float *gm, const float *g11, const float *g12,
                 float *dimg1, int32_t B, int32_t H, int32_t W, void *stream);
/* Gradients of the duration and pitch losses.  `final_sums` (required): the four sums of set_dur_loss_sums_det /
 * set_pitch_loss_sums_det.  ddur = gscale * d(lam_p*s0/s1 + lam_w*s2/s3)/d dur_pred;  dpp [B][2][T] = gscale * d(lam_f0*s2/s3 +
 * lam_uv*s0/s1)/d pitch_pred. */
int set_dur_loss(const float *dur_pred, const int64_t *mel2ph, const int64_t *txt, const int64_t *word_id,
                 const float *final_sums, float *ddur, int32_t B, int32_t T, int32_t T_txt, int32_t n_words, float lam_p,
                 float lam_w, float gscale, void *stream);
int set_pitch_loss(const float *pp, const float *f0, const float *uv, const int64_t *mel2ph, const float *final_sums,
                   float *dpp, int32_t B, int32_t T, float lam_uv, float lam_f0, float gscale, void *stream);
/* torch.optim.AdamW step (speech_base.py:163-170) over flat buffers on the gradient g*grad_scale (grad_scale =
 * 1/world after a SUM all-reduce), with clip_grad_norm_ folded in (base_task.py:129-133): the gradient is further
 * scaled by min(1, max_norm / (sqrt(sumsq[0])*grad_scale + 1e-6)) when sumsq != NULL (sumsq = sum g^2). */
int set_adamw(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int32_t step, const float *sumsq, float max_norm, float grad_scale, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Attention building blocks (CampNet rows; modules/speech_editing/commons/transformer.py)
 * ------------------------------------------------------------------------------------------------ */
/* Strided batched fp32 GEMM on MFMA:  C[b](m,n) = alpha * sum_k A[b](m,k) * B[b](k,n)  (+ C if accumulate).
 * Batch index b = bo * n_inner + bi; every operand is addressed base + bo*X_bo + bi*X_bi + row*rs + col*cs, so the
 * heads of a [B][heads*d][T] activation are batches and Q, K^T, V, O need no transposes (transformer.py:344-347,365,
 * 403-405 do view/transpose/contiguous instead).  The same entry point serves the four gradient products. */
typedef struct SetBmmArgs {
    const float *A, *B;
    float *C;
    int64_t a_bo, a_bi, a_ms, a_ks;
    int64_t b_bo, b_bi, b_ks, b_ns;
    int64_t c_bo, c_bi, c_ms, c_ns;
    int32_t n_outer, n_inner, M, N, K;
    float alpha;
    int32_t accumulate;
} SetBmmArgs;
int64_t set_sizeof_bmm_args(void);
int set_bmm(const SetBmmArgs *args, void *stream);
/* Fused multi-head attention (replaces the bmm -> softmax -> bmm of modules/speech_editing/commons/transformer.py:361-406 and
 * the self-attention of torch's multi_head_attention_forward that EncSALayer / DecSALayer call, :505-513,:566-575):
 *     o[b][h] = softmax_keys(scale q[b][h] k[b][h]^T  (+ key padding -> fill)) v[b][h]
 * on the channel-major layout: element (b, head h, channel c < head_dim, frame t) of q sits at q + b q_bs + (h head_dim + c) q_cs
 * + t, likewise k / v (Tk frames) and o; q / k / v may be channel slices of one packed projection.  The scores never reach HBM
 * (online softmax over 32-key tiles); lse [B][heads][2][Tq] = the softmax statistics the backward needs: row max m and sum l = sum exp(s - m)
 * (log-sum-exp = m + log l; kept apart because log l vanishes in fp32 next to a -1e8 fill).  p (optional):
 * the probabilities [B][heads][Tq][Tk] for callers that return them (transformer.py:396-410).  kpm (optional) [B][Tk], != 0 =
 * padded key; fill = -inf (torch: a fully padded row is NaN) or -1e8 (transformer.py:381-386: a fully padded row is uniform).
 * bf16 != 0: bf16 MFMA operands (fp32 scores / softmax / accumulation), else fp32 MFMA throughout.  head_dim: 32, 64 or 96. */
typedef struct SetAttnArgs {
    const float *q, *k, *v;
    float *o, *lse, *p;
    const float *kpm;
    int64_t q_bs, k_bs, v_bs, o_bs;
    int32_t q_cs, k_cs, v_cs, o_cs;
    int32_t B, heads, head_dim, Tq, Tk;
    float scale, fill;
    int32_t bf16;
} SetAttnArgs;
int64_t set_sizeof_attn_args(void);
int set_attention(const SetAttnArgs *args, void *stream);
/* Gradients of set_attention: P is recomputed from q, k and fwd.lse (fwd.o = the forward's output, fwd.p unused).  d_o has o's
 * layout; dq / dk / dv are addressed like q / k / v with their own strides and are overwritten; delta [B][heads][Tq] is scratch
 * (sum_c dO O).  Two launches (per query tile: dq; per key tile: dk, dv), no atomics: bit-stable from run to run. */
typedef struct SetAttnBwdArgs {
    SetAttnArgs fwd;
    const float *d_o;
    float *delta, *dq, *dk, *dv;
    int64_t dq_bs, dk_bs, dv_bs;
    int32_t dq_cs, dk_cs, dv_cs;
} SetAttnBwdArgs;
int64_t set_sizeof_attn_bwd_args(void);
int set_attention_bwd(const SetAttnBwdArgs *args, void *stream);
/* y[row] = softmax_fp32(x[row]) over `cols`; logits where key_padding_mask[row / rows_per_batch][col] != 0 are
 * replaced by `fill` first (-inf: F.multi_head_attention_forward; -1e8: transformer.py:381-386).  mask may be NULL. */
int set_softmax_rows(const float *x, const float *key_padding_mask, float *y, int64_t rows, int32_t cols,
                     int64_t rows_per_batch, float fill, void *stream);
/* ds = p * (dp - sum_cols(p * dp)) */
int set_softmax_rows_bwd(const float *p, const float *dp, float *ds, int64_t rows, int32_t cols, void *stream);
/* make_positions with padding_idx 0 (utils/nn/seq_utils.py:6-18): pos[b][t] = rank of entry t among the non-zero
 * entries of row b (1-based), 0 where the entry is 0.  Entries: int64 tokens[B][T], or (tokens == NULL) the fp32
 * values x[b*x_bs + t] (first channel of a [B][C][T] tensor: transformer.py:795 numbers frames by `x[..., 0]`). */
int set_make_positions(const int64_t *tokens, const float *x, int64_t x_bs, int64_t *pos, int32_t B, int32_t T,
                       void *stream);
/* out[b][i] = mean over heads of p[b][h][i]   (transformer.py:414-416, need_head_weights=False) */
int set_head_mean(const float *p, float *out, int32_t B, int32_t heads, int64_t n, void *stream);
/* out[b][c][t] = x[b][c][t]*(1-m[b][t]) + e[c]*m[b][t]   (campnet.py:56 `mels*(1-mask) + mask_emb*mask`) */
int set_mask_fill_chan(const float *x, const float *e, const float *m, float *out, int32_t B, int32_t C, int32_t T,
                       void *stream);
/* out[c] += sum_{b,t} d[b][c][t] * m[b][t]   (gradient of mask_emb) */
int set_masked_channel_sum(const float *d, const float *m, float *out, int32_t B, int32_t C, int32_t T, void *stream);

/* Log-mel front end: wav [B][wav_bs >= N] fp32 -> mel [B][T][n_mels] fp32 in one launch (the layout of the reference's item['mel']):
 * Hann-windowed STFT, magnitude sqrt(re^2 + im^2 + mag_eps), filterbank product, log_scale * log(max(mel, floor)).  Replaces
 * utils/audio/__init__.py:64-75 (librosa_wav2spec: pad = n_fft / 2, reflect = 0, clamp_input = 0, mag_eps = 0, floor = 1e-6,
 * log_scale = 1 / ln 10) and modules/vocoder/hifigan/mel_utils.py:59-76 (pad = (n_fft - hop) / 2, reflect = 1, clamp_input = 1,
 * mag_eps = 1e-9, floor = 1e-5, log_scale = 1).  Both GEMMs run on v_mfma_f32_32x32x2_f32; the spectrum stays on chip.
 *   lengths   int64 [B] samples per row (NULL: N each), clamped to [0, N]; nothing past a row's length is read.  Row b has
 *             T_b = 1 + (len_b + 2 pad - n_fft) / hop frames (0 when negative); frames T_b .. T-1 are written as 0.0.  With reflect = 1
 *             the caller guarantees len_b > pad (the entry checks N only: lengths live on the device).
 *   T         = 1 + (N + 2 pad - n_fft) / hop
 *   table     image of W[2][nbins rounded up to 32s][n_fft], W[0][f][n] = win[n] cos(2 pi (bin_lo + f) n / n_fft),
 *             W[1][f][n] = -win[n] sin(...), rows of bins >= bin_lo + nbins zero: set_log_mel_table_size(n_fft, nbins) floats ordered
 *             [32-bin chunk][n / 4][lane 0..63][4], element e = W[e & 1][32 chunk + (lane & 31)][4 (n / 4) + 2 (e >> 1) + (lane >> 5)]
 *   basis     image of mel_basis [n_mels][n_fft / 2 + 1], ordered [32-bin chunk][r 0..15][lane][4], element e < 3 =
 *             mel_basis[32 e + (lane & 31)][bin_lo + 32 chunk + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)] (0 outside the matrix), e = 3: 0
 *   bin_lo    first bin computed, a multiple of 32; nbins bins from there (bin_lo + nbins <= n_fft / 2 + 1)
 * Built for n_fft = 1024, hop = 256, n_mels <= 96: anything else is SET_E_UNSUPPORTED.  No atomics: bit-reproducible, and a row of a
 * ragged batch equals the same waveform run alone.  table / basis 16-byte aligned; mel too when n_mels is a multiple of 4. */
typedef struct SetLogMelArgs {
    const float *wav;
    const int64_t *lengths;
    const float *table, *basis;
    float *mel;
    int64_t wav_bs;
    double log_scale;
    int32_t B, N, T;
    int32_t n_fft, hop, n_mels;
    int32_t bin_lo, nbins;
    int32_t pad, reflect, clamp_input;
    float mag_eps, floor;
    int32_t pad_;
} SetLogMelArgs;
int64_t set_sizeof_log_mel_args(void);
int64_t set_log_mel_table_size(int32_t n_fft, int32_t nbins);
int set_log_mel(const SetLogMelArgs *args, void *stream);

/* Mel-cepstral distortion (csrc/mcd.hip; utils/eval/mcd.py `get_metrics_mels`, utils/metrics/dtw.py).  All tensors fp32 and contiguous
 * unless stated; every `len*` is int64 [B] on the device or NULL (every row full).  A length is read as clamped into [1, T] ([0, T] for
 * set_mfcc): no kernel leaves its buffers whatever the device holds.  No atomics anywhere: two runs agree bit for bit, and a row of a ragged
 * batch equals the same pair run alone.
 *
 * set_mfcc: mel [B][T][M] -> out [B][T][K], out[b][t][k-1] = sum_n x[n] table[k-1][n] in ascending n (fp32 FMA), x = mel or, with
 *   take_log, log10(mel) rounded once from double.  table [K][M] = cos(pi k (2n+1) / (2M)), k = 1..K (metrics.dct_table).  Rows
 *   t >= lengths[b] are written as +0.0.  K <= 64, M <= 96, else SET_E_UNSUPPORTED.
 * set_dtw: x [B][Tx][K], y [B][Ty][K] -> dist [B] = D[len_x-1][len_y-1], steps [B] int32 = the length of the optimal path, and, when
 *   dir != NULL, dir [B][Tx][Ty] uint8 = the predecessor chosen per cell (0 diagonal, 1 row above, 2 column before).
 *   C[i][j] = sqrt(sum_k (x_ik - y_jk)^2) in the difference form; D[i][j] = C[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]), +inf outside
 *   the matrix, D[0][0] = C[0][0]; ties go to the first of the three in that order; L[i][j] = 1 + L[chosen], L[0][0] = 1.  Rows >= len_x and
 *   columns >= len_y are never read, and dir outside [0, len_x) x [0, len_y) is not written.  One 256-thread block per pair, dynamic LDS
 *   (320 (KP + 1) + 2 Ty + 16) * 4 bytes with KP = 40 (K <= 40) or 64.  K <= 64, Ty <= 8192, else SET_E_UNSUPPORTED.
 * set_dtw_path: dir, steps -> path [B][Tx + Ty - 1][2] int32: entries 0 .. steps[b]-1 are (i, j) from (0, 0) to (len_x-1, len_y-1);
 *   entries beyond are not written.
 * set_zero_fill_dist: sum [B] = sum over t < max(len_x, len_y) of ||x_t - y_t||, a side read as zeros at and beyond its length.
 * set_mcd_finish: frames [B] int64 = steps[b] (steps int32, from set_dtw) or, with steps == NULL, max(len_1, len_2);
 *   mcd = num / frames and penalty = 2 - (len_1 + len_2) / frames, each computed in double and rounded once. */
int set_mfcc(const float *mel, const int64_t *lengths, const float *table, float *out, int32_t B, int32_t T, int32_t M, int32_t K,
             int32_t take_log, void *stream);
int set_dtw(const float *x, const float *y, const int64_t *len_x, const int64_t *len_y, float *dist, int32_t *steps, uint8_t *dir, int32_t B,
            int32_t Tx, int32_t Ty, int32_t K, void *stream);
int set_dtw_path(const uint8_t *dir, const int64_t *len_x, const int64_t *len_y, const int32_t *steps, int32_t *path, int32_t B, int32_t Tx,
                 int32_t Ty, void *stream);
int set_zero_fill_dist(const float *x, const float *y, const int64_t *len_x, const int64_t *len_y, float *sum, int32_t B, int32_t Tx,
                       int32_t Ty, int32_t K, void *stream);
int set_mcd_finish(const float *num, const int32_t *steps, const int64_t *len_1, const int64_t *len_2, float *mcd, float *penalty,
                   int64_t *frames, int32_t B, int32_t T1, int32_t T2, void *stream);

/* Short-time objective intelligibility (csrc/stoi.hip; eval/stoi.py `stoi(x, y, 22050, extended=False)` with eval/utils.py).  Four
 * launches: x, y [B][in_bs >= N] fp32 -> d [B] fp32, valid [B] uint8.  Every `lengths` / `lens` is int64 [B] on the device or NULL (every
 * row full) and is read clamped into [0, N]: no kernel leaves its buffers whatever the device holds.  No atomics anywhere: two runs agree bit
 * for bit, and a row of a ragged batch equals the same pair run alone.  win [1024] fp32 is the SYMMETRIC Hann np.hanning(1026)[1:-1],
 * float64 rounded once (not the periodic window of the log-mel).  Sizes follow from N alone: F_max = ceil((N - 1024) / 512) energy frames,
 * rows of 512 (F_max + 1) compacted samples, T = 2 (F_max - 1) envelope frames.  N > 1024.
 *
 * set_stoi_select: a row of len samples has F = ceil((len - 1024) / 512) frames (0 when len <= 1024), frame f from sample 512 f.
 *   e2[f] = sum_n fl(fl(w[n] x[512 f + n])^2) in fp32: lane l of a wave sums n = l, l + 64, ... ascending, then the butterfly 32, 16, .., 1;
 *   nrm[b][f] = sqrtf(e2[f]) (nrm [B][F_max], written for f < F).  Frame f is kept iff nrm[f] + EPS > 0.01f (max_f nrm[f] + EPS) in fp32,
 *   EPS = 2.220446e-16f: the reference's 20 log10(a + EPS) > 20 log10(m + EPS) - 40 in the linear domain (an all-zero row keeps every
 *   frame, as the reference does).  kept [B][F_max] int32: kept[b][j] = the j-th kept frame, ascending, written for j < K[b]; K [B] int32.
 *   One block per row, the scan in LDS.
 * set_stoi_compact: the reference's `_overlap_and_add` of the kept windowed frames at hop 512, for x and for y with x's list.
 *   sil [2 B][sil_bs >= 512 (F_max + 1)], row b = x's and row B + b = y's signal: for j = 0 .. K, r < 512
 *     sil[512 j + r] = fl(fl(w[r] s[512 kept[j] + r]) + fl(w[r + 512] s[512 kept[j-1] + 512 + r])),
 *   the first product +0.0 at j = K and the second at j = 0 (two separately rounded products, one rounded add: numpy float32 gives the
 *   same bits).  Nothing at or beyond L = 512 (K + 1) is written.  sil_len [2 B] int64 = L of each row.  K and kept are read clamped.
 * set_stoi_bands: sil [R][sil_bs >= N] with lens [R] -> tob [R][T][n_bands], T = ceil((N - 1024) / 256).  Row r has
 *   T_r = ceil((len_r - 1024) / 256) frames (0 when len_r <= 1024; 2 (K - 1) for len = 512 (K + 1)), frame m from sample 256 m, no padding:
 *     tob[m][i] = sqrtf(sum_bin basis[i][bin] (re^2 + im^2)),
 *   the windowed DFT and the band sum both on v_mfma_f32_32x32x2_f32 by the kernel body of set_log_mel (csrc/dft_gemm.h), the spectrum kept
 *   on chip; frames m >= T_r are written as +0.0.  table / basis are the images of set_log_mel (melspec.pack_dft_table over the window
 *   above, melspec.pack_mel_basis of the 0/1 band matrix), 16-byte aligned.  n_fft = 1024, hop = 256, n_bands <= 32, else SET_E_UNSUPPORTED.
 * set_stoi_score: tob [2 B][T][n_bands] (row b = x, row B + b = y) and lens [B] (compacted samples, as sil_len) -> d, valid.
 *   T_b = ceil((len_b - 1024) / 256) clamped to T; J = T_b - 29 segments; T_b < 30: valid = 0, d = NaN.  Else, for every segment m and band i,
 *   with the 30-vectors X = tob_x[m .. m+29][i], Y likewise: c = ||Y|| > 0 ? ||X|| / ||Y|| : 0; Y' = min(Y c, X (1 + 10^0.75)); both minus
 *   their means; rho = <X, Y'> / (||X|| ||Y'||), 0 when a norm is 0; d = sum rho / (n_bands J), valid = 1.  Every segment is evaluated
 *   directly, in double from the fp32 envelopes; a thread's sum and the block's tree depend on T_b only.  seg = 30, n_bands <= 32, else
 *   SET_E_UNSUPPORTED.  T = 0 (tob may be NULL) marks every row invalid. */
int set_stoi_select(const float *x, int64_t x_bs, const int64_t *lengths, const float *win, float *nrm, int32_t *kept, int32_t *K, int32_t B,
                    int32_t N, int32_t n_frame, void *stream);
int set_stoi_compact(const float *x, const float *y, int64_t in_bs, const float *win, const int32_t *kept, const int32_t *K, float *sil,
                     int64_t sil_bs, int64_t *sil_len, int32_t B, int32_t N, int32_t n_frame, void *stream);
int set_stoi_bands(const float *sil, int64_t sil_bs, const int64_t *lens, const float *table, const float *basis, float *tob, int32_t R,
                   int32_t N, int32_t T, int32_t n_fft, int32_t hop, int32_t n_bands, int32_t bin_lo, int32_t nbins, void *stream);
int set_stoi_score(const float *tob, const int64_t *lens, float *d, uint8_t *valid, int32_t B, int32_t T, int32_t n_bands, int32_t seg,
                   void *stream);

/* Wav-level mel-cepstral distortion of the reference's eval script (csrc/wav_mcd.hip; eval/mcd.py `cal_mcd` on
 * librosa.feature.mfcc(sr=22050, n_mfcc=34, n_fft=1024, hop_length=256, n_mels=80, fmin=55, fmax=7600, htk=True), librosa 0.8.0).  All
 * tensors fp32 and contiguous; every `frames*` is int64 [B] on the device or NULL (every row full) and is read clamped into [0, T]: no
 * kernel leaves its buffers whatever the device holds.  No atomics anywhere: two runs agree bit for bit, and a row of a ragged batch equals
 * the same pair run alone.
 *
 * set_db_mel: SetLogMelArgs as for set_log_mel, with pad = n_fft / 2 and reflect = 1 (librosa 0.8.0's center=True), else
 *   SET_E_UNSUPPORTED; mag_eps is not read.  A row of len_b samples has T_b = 1 + len_b / hop frames when len_b > pad and none otherwise;
 *   T = 1 + N / hop, N > pad.  mel[b][t][m] = fl(log_scale * log(max(S, floor))) evaluated in double, S = sum_bin basis[m][bin] (re^2 + im^2)
 *   with both products on v_mfma_f32_32x32x2_f32 by the kernel body of set_log_mel (csrc/dft_gemm.h); frames t >= T_b are +0.0.  dB of a
 *   power is floor = 1e-10, log_scale = 10 / ln 10.  table / basis are the images of set_log_mel.
 * set_db_peak: db [B][T][M], frames [B] -> peak [B] = max over t < T_b and all m of db[b][t][m]; -inf for a row without frames.  Frames at
 *   or beyond T_b are not read.
 * set_db_mfcc: out [B][T][K], out[b][t][k] = sum_n x[n] table[k][n] in ascending n (fp32 FMA), x[n] = max(db[b][t][n], fl(peak[b] -
 *   top_db)).  table [K][M] = s_k cos(pi k (2n+1) / (2M)), k = 0..K-1, s_0 = 1/sqrt(M), s_k = sqrt(2/M) (metrics.dct_ortho_table).  Rows
 *   t >= frames[b] are written as +0.0.  K <= 64, M <= 96, else SET_E_UNSUPPORTED.
 * set_coef_rms_dist: x [B][Tx][K], y [B][Ty][K] -> mcd [B], valid [B] uint8.  A pair with frames_x != frames_y, or without frames, has
 *   valid = 0 and mcd = NaN.  Else, with T_b the common count: s_k = sum_{t < T_b} (x[t][k] - y[t][k])^2 in double (thread q of 4 sums
 *   t = q, q + 4, ... ascending; s_k = (p_0 + p_1) + (p_2 + p_3)); mcd = fl((sum_k 10 / ln 10 sqrt(2 s_k)) / K / T_b), the sum over k
 *   ascending in double; valid = 1.  The sum inside the root runs over the FRAMES, as the reference's axis=1 on [K, T] arrays does.
 *   K <= 64, else SET_E_UNSUPPORTED. */
int set_db_mel(const SetLogMelArgs *args, void *stream);
int set_db_peak(const float *db, const int64_t *frames, float *peak, int32_t B, int32_t T, int32_t M, void *stream);
int set_db_mfcc(const float *db, const int64_t *frames, const float *peak, const float *table, float *out, int32_t B, int32_t T, int32_t M,
                int32_t K, float top_db, void *stream);
int set_coef_rms_dist(const float *x, const float *y, const int64_t *frames_x, const int64_t *frames_y, float *mcd, uint8_t *valid, int32_t B,
                      int32_t Tx, int32_t Ty, int32_t K, void *stream);

/* HiFi-GAN mel loss and its waveform gradient (csrc/mel_loss.hip; tasks/vocoder/hifigan.py:35-38, F.l1_loss of two
 * modules/vocoder/hifigan/mel_utils.py:59-76 `mel_spectrogram`s).  All tensors fp32 and contiguous.  No atomics anywhere: two runs agree bit
 * for bit, every sum has one fixed order, and a row's gradient depends on the other rows only through the factor 1 / count.
 *
 * set_mel_linear: SetLogMelArgs as for set_log_mel (floor and log_scale are not read); mel [B][T][n_mels] = the filterbank product itself,
 *   the value set_log_mel takes the log of, bit for bit.
 * set_mel_loss_fwd: mel_hat, mel_y [B][T][n_mels] (set_mel_linear's) -> loss [1], g_mel [B][T][n_mels] and, when not NULL, log_hat / log_y.
 *   With L = fl(log_scale * log(max(mel, floor))) evaluated in double (set_log_mel's own value), d = fl(L_hat - L_y), count = B T n_mels:
 *     g_mel = (mel_hat >= floor && d != 0) ? copysign(fl(log_scale), d) / mel_hat : 0                  (torch: sign(0) = 0, clamp(min=)
 *   passes the gradient at mel >= floor) -- count times d loss / d mel_hat: set_mel_loss_bwd divides by count once, at the end, so a
 *   row's gradient has the same bits before that whatever the batch -- and loss = fl(S / count) with S = sum |d| in this order: block k of 4096 elements, thread tid of 256
 *   sums elements 4096 k + 256 i + tid in ascending i = 0..15 (elements beyond count add nothing); column c = tid & 63 of the block is
 *   ((s[c] + s[64 + c]) + s[128 + c]) + s[192 + c]; the blocks' columns are summed by csrc/rows_sum.h (16 row groups of four chains), and
 *   the 64 column sums in ascending order.  part: set_mel_loss_fwd_scratch_floats(count) floats of scratch.
 * set_mel_loss_bwd: g_mel [B][T][n_mels] and the waveform wav [B][wav_bs >= N] (the y_hat the forward saw) -> g_wav [B][N], every sample
 *   written: 1 / count times d/d wav of sum g_mel[b][t][m] mel[b][t][m] through the filterbank, the magnitude sqrt(re^2 + im^2 + mag_eps), the windowed DFT,
 *   the reflect padding of pad = (n_fft - hop) / 2 and the clamp to [-1, 1] (gradient passed where -1 <= wav <= 1, both ends included).
 *   Three launches: (1) per 64-frame tile re / im again by GEMM 1 of set_log_mel on the same `table`, g_mag = basis^T g_mel, g_re = g_mag
 *   re / mag, g_im likewise -> spec [B][2][nbins rounded up to 32s][T rounded up to 64s] (set_mel_loss_bwd_spec_floats); (2) the padded
 *   gradient g_pad [B][(T + 3) hop], g_pad[hop u + c] = sum_{q < 4} sum_f W[0][f][hop q + c] g_re[f][u - q] + W[1][f][hop q + c]
 *   g_im[f][u - q], a gather (a block owns 64 hops); (3) g_wav[j] = (g_pad[j + pad] + g_pad[pad - j] for 1 <= j <= pad) + g_pad[pad +
 *   2 (N - 1) - j] for N - 1 - pad <= j <= N - 2, g_pad read as 0 beyond its end, divided by count (fp32; 1 for a g_mel that carries
 *   its own scale), times the clamp mask.
 *   basis_t  image of mel_basis^T: [32-bin chunk][k-step s 0..47][lane], = mel_basis[2 s + (lane >> 5)][bin_lo + 32 chunk + (lane & 31)],
 *            0 outside the matrix and for bins beyond bin_lo + nbins
 *   itable   image of the table W of set_log_mel for launch (2): set_mel_idft_table_size(n_fft, nbins) floats ordered
 *            [32-bin chunk][wave 0..3][q 0..3][part 0..1][s 0..15][lane][2], element e = W[part][32 chunk + 2 s + (lane >> 5)][256 q +
 *            64 wave + 32 e + (lane & 31)]
 * Built for n_fft = 1024, hop = 256, n_mels <= 96, pad = 384: anything else is SET_E_UNSUPPORTED.  table / itable / g_pad 16-byte aligned. */
typedef struct SetMelLossFwdArgs {
    const float *mel_hat, *mel_y;
    float *g_mel, *log_hat, *log_y, *part, *loss;
    double log_scale;
    int32_t B, T, n_mels;
    float floor;
} SetMelLossFwdArgs;
typedef struct SetMelLossBwdArgs {
    const float *wav, *table, *basis_t, *itable, *g_mel;
    float *spec, *g_pad, *g_wav;
    int64_t wav_bs;
    int32_t B, N, T;
    int32_t n_fft, hop, n_mels;
    int32_t bin_lo, nbins, pad;
    float mag_eps, count;
    int32_t pad_;
} SetMelLossBwdArgs;
int64_t set_sizeof_mel_loss_fwd_args(void);
int64_t set_sizeof_mel_loss_bwd_args(void);
int set_mel_linear(const SetLogMelArgs *args, void *stream);
int64_t set_mel_loss_fwd_scratch_floats(int64_t count);
int set_mel_loss_fwd(const SetMelLossFwdArgs *args, void *stream);
int64_t set_mel_idft_table_size(int32_t n_fft, int32_t nbins);
int64_t set_mel_loss_bwd_spec_floats(int32_t B, int32_t T, int32_t nbins);
int set_mel_loss_bwd(const SetMelLossBwdArgs *args, void *stream);

/* Multi-resolution STFT loss and its waveform gradient, one resolution per call (csrc/stft_loss.hip; tasks/vocoder/hifigan.py:46-47 on
 * modules/vocoder/hifigan/stft_loss.py).  All tensors fp32 and contiguous unless said.  With mag(s) = sqrt(max(re^2 + im^2, 1e-7)) of the
 * windowed DFT of the reflect-padded (n_fft / 2 each side) row, periodic Hann of `win` samples centred in n_fft, T = 1 + N / hop frames,
 * n_fft / 2 + 1 bins, count = B T (n_fft / 2 + 1):
 *     sc = sqrt(S_d) / sqrt(S_g), mag = S_l / count;  S_d = sum (y_mag - x_mag)^2, S_g = sum y_mag^2, S_l = sum |ln y_mag - ln x_mag|
 * over the whole batch.  No atomics anywhere: two runs agree bit for bit and every sum has one fixed order.  A row's magnitudes do not
 * depend on the batch; the losses and the gradient couple the rows through exactly three scalars: D = sqrt(S_d), G = sqrt(S_g), count.
 *
 * Geometries are compiled in: set_stft_geometries writes up to max_triples (n_fft, hop, win) triples and returns how many exist; any
 * other triple is SET_E_UNSUPPORTED with the list in the message.  set_stft_sizes -> out8 = {T, floats of `table`, floats of `itable`,
 * doubles of `part`, floats of the kept magnitudes `mag`, floats of `spec`, floats of `g_pad`, Ts = T rounded up to 64s}.
 *   table    [32-bin chunk][k-step s < win/2][lane][2], element e = W[e][32 chunk + (lane & 31)][left + 2 s + (lane >> 5)], left = (n_fft -
 *            win) / 2: only the win non-zero window samples; W = melspec.dft_table's [2][bins][n_fft], rows beyond the last bin zero
 *   itable   [32-bin chunk][wave vw < NW][k-step kk < 32 Q][lane], Q = ceil(win / hop), q = kk >> 5, part = (kk >> 4) & 1, s = kk & 15:
 *            W[part][32 chunk + 2 s + (lane >> 5)][left + hop q + c], c = 32 rb + (lane & 31); rb = vw with NW = ceil(hop / 32) when a hop
 *            has 4 or 8 row blocks of 32 samples, rb = vw >> 1 with NW = 4 when it has 2; zero where c >= hop, hop q + c >= win or the
 *            bin does not exist
 * set_stft_magnitude: x [B][x_bs >= N] -> mag [B][T][n_fft/2 + 1].  Each (bin, frame) is one accumulator that takes the win window samples
 *   in ascending order (v_mfma_f32_32x32x2_f32); re^2 + im^2 = fl(fl(re re) + fl(im im)).
 * set_stft_loss_fwd: x, y -> loss [2] = {sc, mag}, stats [6] doubles = {D, G, count, S_d, S_g, S_l}; when `mag` is not NULL it receives
 *   the magnitudes of the signal that is not differentiated (x when which = 1, y when which = 0) as [B][chunks x 32][Ts] for
 *   set_stft_loss_bwd.  Order of the sums: block (z, b, tile) = 64 frames x bin chunks 4 z .. 4 z + 3 of row b, one chunk per wave; lane l
 *   of a wave adds its entries in double in the order column block cb = 0, 1 (frame 64 tile + 32 cb + (l & 31)), register r = 0..15 (bin
 *   32 chunk + (r & 3) + 8 (r >> 2) + 4 (l >> 5)); an entry is d = fl(y_mag - x_mag) squared, y_mag squared (both exact in double) and
 *   |fl(ln y_mag) - fl(ln x_mag)| with ln evaluated in double and rounded to fp32 once, the difference in fp32; frames >= T and bins
 *   beyond the last add 0.  The 64 lanes by v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1; the waves as ((w0 + w1) + w2) + w3 -> part[((z B
 *   + b) tiles + tile)][3].  Then thread t of 256 adds blocks t, t + 256, ... in ascending order and the 256 thread sums are added in
 *   ascending order.  D, G by double sqrt; sc = fl32(D / G), mag = fl32(S_l / count).
 * set_stft_loss_bwd: d (u_sc scale sc + u_mag scale mag) / d (y when which = 1, x when which = 0) -> g_wav [B][N], every sample written
 *   (accumulate = 0) or added to (accumulate = 1).  u_sc, u_mag: device scalars (never read by the host); stats: set_stft_loss_fwd's.
 *   With m the differentiated signal's magnitude, r the other's (from `mag`, or by a second DFT when mag is NULL):
 *     g_m = (c1 (m - r) - c2 m) + c3 sign(m - r) / m,   c1 = u_sc scale / (D G) (0 when D = 0), c2 = u_sc scale D / G^3 (0 when which = 0),
 *     c3 = u_mag scale / count, the coefficients evaluated in double and rounded to fp32 once;  g_re = g_m re / m, g_im = g_m im / m where
 *     re^2 + im^2 >= 1e-7, else 0 -> spec [B][2][chunks x 32][Ts]; then g_pad [B][(T + Q - 1) hop] (padded sample left + i at i) = the
 *     inverse windowed DFT as a gather (one accumulator per sample; order: chunk, tap q, part, bin), and the fold g_wav[j] = (g_p[j + P] +
 *     g_p[P - j] for 1 <= j <= P) + g_p[P + 2 (N - 1) - j] for N - 1 - P <= j <= N - 2, P = n_fft / 2, g_p = 0 where no window sample lies.
 *   A g_m [B][T][n_fft/2 + 1] that is not NULL is used as the magnitude gradient instead (stats, u_sc, u_mag are then not read).
 * N > n_fft / 2 (reflect padding), B <= 65535.  table / itable / g_pad 16-byte aligned. */
typedef struct SetStftLossArgs {
    const float *x, *y, *table, *itable, *u_sc, *u_mag, *g_m;
    float *mag, *loss, *spec, *g_pad, *g_wav;
    double *part, *stats;
    int64_t x_bs, y_bs;
    int32_t B, N, T;
    int32_t n_fft, hop, win;
    int32_t which, accumulate;
    float scale;
    int32_t pad_;
} SetStftLossArgs;
int64_t set_sizeof_stft_loss_args(void);
int32_t set_stft_geometries(int32_t *triples, int32_t max_triples);
int set_stft_sizes(int32_t n_fft, int32_t hop, int32_t win, int64_t B, int64_t N, int64_t *out8);
int set_stft_magnitude(const SetStftLossArgs *args, void *stream);
int set_stft_loss_fwd(const SetStftLossArgs *args, void *stream);
int set_stft_loss_bwd(const SetStftLossArgs *args, void *stream);

/* ------------------------------------------------------------------------------------------------
 * HiFi-GAN's multi-period discriminator as the generator step uses it (modules/vocoder/hifigan/hifigan.py:154-223 and the loss
 * functions :301-338; tasks/vocoder/hifigan.py:26-50): forward on the real and the generated waveform with every feature map, the
 * adversarial and feature-matching losses, and their gradient with respect to the generated waveform.  csrc/sconv.hip.
 *
 * Layout: the reference folds [B, 1, T] into [B, 1, H, p] (right reflect pad to Tp = ceil(T / p) p, H = Tp / p) and runs (K, 1)
 * Conv2d layers, which never mix the p columns.  Here every (b, w) column is a row of its own: activations are [R][C][H], contiguous,
 * R = 2 B p, row (sig B + b) p + w, the real signal's rows (sig = 0) first.  t.view(B, p, C, H).permute(0, 2, 3, 1) of one signal's
 * rows is the reference's [B, C, H, p] tensor without a copy.  H_out = (H_in + 2 pad - K) / s + 1.
 *
 * set_sconv1d_fwd:  out[r][co][h] = act(bias[co] + sum_ci sum_k W[co][ci][k] x[r][ci][s h + k - pad]), x = 0 outside [0, H_in);
 *   act = 0: identity, act = 1: v > 0 ? v : slope v;  1 <= s <= 4, 1 <= K <= 7, 0 <= pad < K, any Cin / Cout; bias may be NULL.
 *   wp: the image of set_pack_conv_weight(W).  fp32 operands on v_mfma_f32_32x32x2_f32: each output is one fp32 fma chain over
 *   (16-channel chunk ascending, tap ascending, channel ascending), from 0, then + bias, then act.
 * set_sconv1d_dgrad:  dz_in[r][ci][j] = gate(f_in[r][ci][j]) (add[r][ci][j] + sum_co sum_k W[co][ci][k] dz_out[r][co][(j + pad - k) / s])
 *   over the k with (j + pad - k) % s == 0 and 0 <= (j + pad - k) / s < H_out;  gate(v) = v > 0 ? 1 : slope (slope at exactly 0, as
 *   torch's leaky_relu backward);  f_in NULL: no gate;  add NULL: none.  wtp: the image of set_pack_conv_weight of the transposed
 *   weight W'[ci][co][k] (Cout' = Cin, Cin' = Cout).  Cin, Cout, H_in, K, s, pad are the FORWARD layer's.  One fma chain per element
 *   over (16-channel chunk of co, tap k ascending among the element's taps, co ascending), from 0, then + add, then the gate.
 * set_mpd_fold_conv_fwd:  the first layer (one input channel) straight from the waveforms y, y_hat [B][T] (contiguous):
 *   xpad[n] = y[n] for n < T, y[2 (T - 1) - n] for T <= n < Tp;  out[(sig B + b) p + w][c][h] = act(bias[c] + sum_k w[c][k]
 *   xpad[(s h + k - pad) p + w]) with rows outside [0, H) zero; w: the RAW weight [C][K]; T > p.  One fma chain over k ascending.
 * set_mpd_fold_conv_bwd:  dz [B p][C][H_out] (the generated rows' gradient at the first layer's pre-activation) -> g_wav [B][T], every
 *   sample written:  G(i, w) = fma chain over c ascending, inside it k ascending, of w[c][k] dz[b p + w][c][(i + pad - k) / s] (taps
 *   that hit no output frame add an exact 0);  g_wav[b][n] = G(n / p, n % p) + G(m / p, m % p), the second term only where the mirror
 *   m = 2 (T - 1) - n lies in [T, Tp).
 * One row's [C][H] slice must stay below 2 GiB (SET_E_UNSUPPORTED).  No atomics; results do not depend on R or on the run. */
int32_t set_sconv1d_out_len(int32_t H_in, int32_t K, int32_t s, int32_t pad);
int set_sconv1d_fwd(const float *x, const float *wp, const float *bias, float *out, int32_t R, int32_t Cin, int32_t Cout, int32_t H_in,
                    int32_t K, int32_t s, int32_t pad, int32_t act, float slope, void *stream);
int set_sconv1d_dgrad(const float *dz_out, const float *wtp, const float *f_in, const float *add, float *dz_in, int32_t R, int32_t Cin,
                      int32_t Cout, int32_t H_in, int32_t K, int32_t s, int32_t pad, float slope, void *stream);
int set_mpd_fold_conv_fwd(const float *y, const float *y_hat, const float *w, const float *bias, float *out, int32_t B, int32_t T,
                          int32_t p, int32_t C, int32_t K, int32_t s, int32_t pad, int32_t act, float slope, void *stream);
int set_mpd_fold_conv_bwd(const float *dz, const float *w, float *g_wav, int32_t B, int32_t T, int32_t p, int32_t C, int32_t K,
                          int32_t s, int32_t pad, void *stream);

/* The three loss forms of hifigan.py:301-338 over a list of tensors.  `items`: a DEVICE array of n_items x SET_MULTI_LOSS_WORDS
 * 64-bit words (plain words, not structs):
 *   [0] address of a   [1] address of b (L1 only)   [2] address of grad_a (backward; 0 = none)   [3] mode (SET_LOSS_*)
 *   [4..7] extents, outermost first (unused ones 1)   [8..11] element strides of a (and of grad_a)   [12..15] element strides of b
 *   [16] the item's first chunk: the chunks of the items before it, ceil(numel / SET_MULTI_LOSS_CHUNK) each   [17] result slot
 * total_chunks = the chunks of all items.  Modes: L1 mean |a - b|, SQ1 mean (1 - a)^2, SQ0 mean a^2.
 * set_multi_loss_fwd: loss[k] = fp32(scale * sum over the items of slot k, in list order, of sum_i / numel_i), k < n_slots <= 4, left on
 *   the device.  Order of an item's sum (all in double; a term is |a - b|, (1 - a)^2 or a^2 of the operands converted to double):
 *   element li is the row-major index over the extents; block c (a chunk) has thread t add the terms of elements CHUNK c + t + 256 u,
 *   u = 0..7 ascending, then the 256 thread sums are halved (red[t] += red[t + st], st = 128, 64, .. 1) -> part[first chunk + c];
 *   then thread t of one block adds the item's partials t, t + 256, .. ascending and the thread sums are halved the same way.
 *   part: total_chunks doubles of scratch.  Two kernels (partials, finish).
 * set_multi_loss_bwd: grad_a = coef {sign(a - b), 2 (a - 1), 2 a} in fp32, sign(0) = 0, coef = fp32(u[slot] scale / numel) with the
 *   product and the quotient in double; u: n_slots device floats (the upstream gradients; never read by the host); written at a's
 *   strides, for the items whose word [2] is not 0.  One kernel. */
#define SET_MULTI_LOSS_WORDS 18
#define SET_MULTI_LOSS_CHUNK 2048
#define SET_LOSS_L1 0
#define SET_LOSS_SQ1 1
#define SET_LOSS_SQ0 2
int set_multi_loss_fwd(const int64_t *items, int32_t n_items, int64_t total_chunks, float scale, int32_t n_slots, double *part,
                       float *loss, void *stream);
int set_multi_loss_bwd(const int64_t *items, int32_t n_items, int64_t total_chunks, float scale, const float *u, void *stream);

/* ------------------------------------------------------------------------------------------------
 * HiFi-GAN's multi-scale discriminator as the generator step uses it (modules/vocoder/hifigan/hifigan.py:226-298): grouped strided
 * convs with up to 41 taps, the first layer straight from the waveforms, and AvgPool1d(4, 2, padding = 1).  csrc/msd.hip.  Activations
 * are [R][C][H] rows as above (R = 2 B, the real signal's rows first); the dense layers 7 and 8 run on set_sconv1d_*.
 *
 * set_gconv1d_fwd:  out[r][co][h] = act(bias[co] + sum_{ci in group(co)} sum_k W[co][ci][k] x[r][g Cin/G + ci][s h + k - pad]), W
 *   [Cout][Cin / G][K], g = co / (Cout / G), x = 0 outside [0, H_in);  1 <= K <= SET_GCONV_KMAX, 1 <= s <= 4, 0 <= pad < K, any G
 *   dividing Cin and Cout, any Cin / G and Cout / G (ragged sizes are zero-padded inside the image).  wp: G images of
 *   set_pack_conv_weight back to back, image g that of the dense [Cout / G][Cin / G][K] weight of group g
 *   (set_packed_gconv_weight_size floats in all).  One fp32 fma chain per output over (16-channel chunk of the group's input channels
 *   ascending, tap ascending, channel ascending), from 0, then + bias, then act (as set_sconv1d_fwd).
 * set_gconv1d_dgrad:  dz_in = gate(f_in) (add + conv^T(dz_out)) as set_sconv1d_dgrad, per group; wtp: G images of the groups'
 *   transposed weights W'[ci][co][k].  One fma chain per element over (16-channel chunk of the group's co, tap ascending among the
 *   element's taps, co ascending), from 0, then + add, then the gate (gate(0) = slope).  All output phases in one launch.
 * The frames of one block: the forward works on SET_GCONV_TILE_1 output frames when Cout / G fits one 32-row block, else on
 *   SET_GCONV_TILE_2; the dgrad on s times that many input frames by the 32-row blocks of Cin / G (set_gconv1d_tile(rows per group)).
 * set_wave_conv_fwd:  the first layer from y, y_hat [B][T]: out[sig B + b][c][h] = act(bias[c] + sum_k w[c][k] wav[h + k - pad]), zeros
 *   outside; w: the raw weight [C][K], K <= SET_WAVE_CONV_KMAX odd, pad = (K - 1) / 2.  One fma chain over k ascending.  y_hat NULL:
 *   the B rows of y alone (out [B][C][T]).
 * set_wave_conv_bwd:  dz [B][C][T] (the generated rows' gradient at the first layer's pre-activation) -> g_wav [B][T], every sample
 *   written: one fma chain over c ascending, inside it k ascending, of w[c][k] dz[b][c][n + pad - k] (a frame outside adds an exact 0).
 * set_avgpool4s2_fwd:  x [B][T] -> out [B][T_out], T_out = (T - 2) / 2 + 1 (T >= 2):
 *   out[j] = 0.25 (((x[2 j - 1] + x[2 j]) + x[2 j + 1]) + x[2 j + 2]), zeros outside (the divisor is 4 at the edges too).
 * set_avgpool4s2_bwd:  g_in[i] = add[i] + (0.25 g_out[lo] + 0.25 g_out[hi]), lo = (i + 1) / 2 - 1, hi = lo + 1, a term outside
 *   [0, T_out) an exact 0; add NULL: the bracket alone.  T is the INPUT length.
 * No atomics; results do not depend on R, B or on the run. */
#define SET_GCONV_KMAX 41
#define SET_WAVE_CONV_KMAX 15
#define SET_GCONV_TILE_1 128
#define SET_GCONV_TILE_2 64
int32_t set_gconv1d_out_len(int32_t H_in, int32_t K, int32_t s, int32_t pad);
int32_t set_gconv1d_tile(int32_t rows_per_group);
int64_t set_packed_gconv_weight_size(int32_t Cout, int32_t Cin, int32_t K, int32_t groups);
int set_gconv1d_fwd(const float *x, const float *wp, const float *bias, float *out, int32_t R, int32_t Cin, int32_t Cout, int32_t groups,
                    int32_t H_in, int32_t K, int32_t s, int32_t pad, int32_t act, float slope, void *stream);
int set_gconv1d_dgrad(const float *dz_out, const float *wtp, const float *f_in, const float *add, float *dz_in, int32_t R, int32_t Cin,
                      int32_t Cout, int32_t groups, int32_t H_in, int32_t K, int32_t s, int32_t pad, float slope, void *stream);
int set_wave_conv_fwd(const float *y, const float *y_hat, const float *w, const float *bias, float *out, int32_t B, int32_t T, int32_t C,
                      int32_t K, int32_t pad, int32_t act, float slope, void *stream);
int set_wave_conv_bwd(const float *dz, const float *w, float *g_wav, int32_t B, int32_t T, int32_t C, int32_t K, int32_t pad,
                      void *stream);
int32_t set_avgpool4s2_out_len(int32_t T);
int set_avgpool4s2_fwd(const float *x, float *out, int32_t B, int32_t T, void *stream);
int set_avgpool4s2_bwd(const float *g_out, const float *add, float *g_in, int32_t B, int32_t T, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The discriminator step (tasks/vocoder/hifigan.py:51-61): gradients with respect to the discriminators' own weights.
 * csrc/disc_wgrad.hip.  Activations are the [R][C][H] rows above, over ALL rows (real and generated).  fp32 operands; no atomics; every
 * result is bit-identical from run to run.  `accumulate` 1: the result is ADDED to the output (one fp32 add per element), 0: stored.
 *
 * set_gconv1d_wgrad:  dW[co][ci][k] (+)= sum_r sum_h dz[r][co][h] x[r][g Cin/G + ci][s h + k - pad], x = 0 outside [0, H_in), g = co /
 *   (Cout / G);  dW [Cout][Cin / G][K];  the ranges of set_gconv1d_fwd (G = 1: the dense layers of both discriminators).  db (optional)
 *   [Cout]: db[co] (+)= sum_r sum_h dz[r][co][h].  dw or db may be NULL (not wanted), not both.
 *   The reduction index j = r H_out + h runs over the frames of every row, in chunks of SET_GCONV_WGRAD_CHUNK; `slices` consecutive
 *   runs of ceil(chunks / slices) chunks each (the last ones may be short or empty).  On v_mfma_f32_32x32x2_f32, a block being 32 rows
 *   of one group by SET_GCONV_WGRAD_COLS flattened (ci, k) columns.  Order of an element's sum: per slice one fp32 fma chain from 0 over
 *   j ascending, products unrounded (indices past the end and taps outside the row add an exact 0);  then t = ((p_0 + p_1) + p_2) + ..
 *   over the slices ascending;  then dW = t, or dW_old + t.  With one slice and accumulate = 0 the chain is stored directly.
 *   db: thread t of 256 adds the terms j = t, t + 256, .. ascending in double; the thread sums are halved (red[t] += red[t + st], st =
 *   128, 64, .. 1); rounded to fp32 once; then stored or added.
 *   slices: 0 = set_gconv1d_wgrad_plan on the current device's CU count, 1 .. SET_GCONV_WGRAD_MAX_SLICES forces it.  scratch:
 *   set_gconv1d_wgrad_scratch_floats(.., slices) floats (slices Cout Cin/G K), reusable by the next call on the stream; not read when
 *   slices == 1 and accumulate == 0 (may then be NULL).
 * set_gconv1d_wgrad_plan: the slice count, a pure function of the shapes and n_cu (0: the current device's): with tiles = G
 *   ceil((Cout/G) / 32) ceil((Cin/G) K / COLS) and chunks = ceil(R H_out / CHUNK): min(ceil(4 n_cu / tiles), chunks / 8, MAX_SLICES),
 *   at least 1.
 * set_mpd_fold_conv_wgrad / set_wave_conv_wgrad: the first layers (one input channel), from the waveforms y, y_hat [B][T] and dz over
 *   all rows ([2 B p][C][H_out] / [2 B][C][T]; set_wave_conv_wgrad with y_hat NULL: the B rows of y alone):
 *   dW[c][k] (+)= sum_r sum_h dz[r][c][h] X(r, s h + k - pad), db[c] (+)= sum dz, X as set_mpd_fold_conv_fwd's xpad[i p + w] (0 for i
 *   outside [0, H)) / set_wave_conv_fwd's wav[i]; dW [C][K] raw.  K <= SET_WAVE_CONV_KMAX.  Order: j = r H_out + h; slice z owns the
 *   j in [z per, (z + 1) per), per = ceil(J / slices); thread t adds the terms j = lo + t, lo + t + 256, .. ascending in double (products
 *   exact), halved as above -> part[z][c][k] (k = K: the bias); then the slices ascending in double, rounded to fp32 once, stored or
 *   added.  slices 0: min(ceil(4 n_cu / C), J / 4096, SET_FIRST_WGRAD_MAX_SLICES), at least 1.  part:
 *   set_first_conv_wgrad_part_doubles(C, K, slices) doubles.  dw or db may be NULL.
 * set_weight_norm_fold_bwd: w = g v / |v| per row (set_weight_norm_fold) -> dg[row] = <dW, v> / n, dv = (g / n) (dW - v <dW, v> / n^2),
 *   n = sqrt(sum v^2).  Per row, thread t adds v_i^2 and dW_i v_i of i = t, t + 256, .. in double, halved as above; the formulas in
 *   double, rounded once.  dg or dv may be NULL.
 * set_spectral_norm_fold_bwd: W = W_orig / sigma, sigma = u^T W_orig v with u, v constants (torch.nn.utils.spectral_norm) ->
 *   d W_orig = (dW - (<dW, W_orig> / sigma) u v^T) / sigma, W_orig [n0][inner], sigma a DEVICE float.  <dW, W_orig>: row sums as above
 *   -> part[row] (n0 doubles), then thread t adds rows t, t + 256, .. ascending, halved; the formula in double, rounded once. */
#define SET_GCONV_WGRAD_CHUNK 32
#define SET_GCONV_WGRAD_COLS 128
#define SET_GCONV_WGRAD_MAX_SLICES 64
#define SET_FIRST_WGRAD_MAX_SLICES 64
int32_t set_gconv1d_wgrad_plan(int32_t R, int32_t Cin, int32_t Cout, int32_t groups, int32_t H_in, int32_t K, int32_t s, int32_t pad,
                               int32_t n_cu);
int64_t set_gconv1d_wgrad_scratch_floats(int32_t R, int32_t Cin, int32_t Cout, int32_t groups, int32_t H_in, int32_t K, int32_t s,
                                         int32_t pad, int32_t slices);
int set_gconv1d_wgrad(const float *dz, const float *x, float *dw, float *db, int32_t R, int32_t Cin, int32_t Cout, int32_t groups,
                      int32_t H_in, int32_t K, int32_t s, int32_t pad, int32_t accumulate, int32_t slices, float *scratch,
                      int64_t scratch_floats, void *stream);
int64_t set_first_conv_wgrad_part_doubles(int32_t C, int32_t K, int32_t slices);
int set_mpd_fold_conv_wgrad(const float *dz, const float *y, const float *y_hat, float *dw, float *db, int32_t B, int32_t T, int32_t p,
                            int32_t C, int32_t K, int32_t s, int32_t pad, int32_t accumulate, int32_t slices, double *part,
                            int64_t part_doubles, void *stream);
int set_wave_conv_wgrad(const float *dz, const float *y, const float *y_hat, float *dw, float *db, int32_t B, int32_t T, int32_t C,
                        int32_t K, int32_t pad, int32_t accumulate, int32_t slices, double *part, int64_t part_doubles, void *stream);
int set_weight_norm_fold_bwd(const float *dw, const float *g, const float *v, float *dg, float *dv, int32_t n0, int64_t inner,
                             int32_t accumulate, void *stream);
int set_spectral_norm_fold_bwd(const float *dw, const float *w_orig, const float *u, const float *v, const float *sigma, float *dw_orig,
                               int32_t n0, int64_t inner, int32_t accumulate, double *part, void *stream);

/* MFMA fragment-layout self test: runs a 32x32xK product through v_mfma_f32_32x32x2_f32 with the layout
 * this library assumes and returns the max abs error vs an in-kernel scalar reference via *max_err (HOST).
 * Synchronises.  Used by tests to pin the hardware layout assumption. */
int set_selftest_mfma(float *max_err_host, void *stream);

/* sizeof() of the argument structs, so a foreign-language binding can verify its mirror of the layout */
int64_t set_sizeof_conv1d_args(void);
int64_t set_sizeof_diffnet_layer_args(void);
int64_t set_sizeof_diff_loop_args(void);

#ifdef __cplusplus
}
#endif
#endif /* SET_AMD_H */
