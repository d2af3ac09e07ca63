"""GPU branch sweep of the fp32 convolution family (csrc/conv1d.hip: naive, mfma v1, mfma2 v2, fewout) and of the fp32 weight
gradient (csrc/train.hip: conv1d_wgrad_mfma_kernel with its split-K slice plan, the naive kernel, the deterministic entry point):
every path the launch code picks by shape, stride or alignment, as ONE kernel call against the float64 reference of
tests/test_conv_reference.py (written from the comment above SetConv1dArgs), so that a failing model-level test can be pinned on
one kernel.  Each case names the branch it reaches and the C condition it satisfies.

Two assertions per case, as in tests/test_gpu_kernel_branches.py:
  exact    small-integer inputs (x in [-3, 3], w in [-2, 2], integer bias / res / previous out, 0/1 mask, power-of-two alpha /
           slopes / out_div): every partial sum is an integer multiple of a power of two below 2^24 times it in ANY order, so the
           kernel must equal the float64 result bit for bit -- an indexing, chunk-walk or tap-offset error of any size shows.
  bounded  Gaussian inputs within the DERIVED per-element bar conv_bound() (gamma(Cin K + 4) S |alpha| Lip(act) + 4 u (...)).
The output lives inside a larger buffer pre-filled with a sentinel (or the integer previous output); the WHOLE buffer is
compared: the reference's written set against the reference, every other element -- skipped polyphase frames, frames >= T_iter,
the neighbours of a channel or frame slice -- against what was there before.  Kernels that admit the same case must agree bit
for bit on the integer inputs."""
import ctypes as C

import pytest
import torch

from test_conv_reference import (WGRAD_CASES, conv_bound, conv_ref, gamma, ints, polyphase_calls, weight_view, wgrad_plan,
                                 wgrad_ref)

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
E_UNSUPPORTED, E_INVALID = -2, -1


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_ALIVE = []  # device tensors whose raw address went to a launch: a temporary freed before its kernel ran could be handed out again


@pytest.fixture(autouse=True)
def _keep_launch_operands():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _p(t):
    from set_amd.ops import _p as p
    if t is not None:
        _ALIVE.append(t)
    return p(t)


def _L():
    from set_amd import _lib
    return _lib.lib()


def _s():
    from set_amd.ops import _stream
    return _stream()


# ------------------------------------------------------------------------------------------------------------------------
# forward cases
# ------------------------------------------------------------------------------------------------------------------------
NMV = ("naive", "mfma", "mfma2")
NM = ("naive", "mfma")


def _case(name, impls, B, Cin, Cout, K, dil, T, **kw):
    """pad defaults to "same" (dil (K - 1) / 2), T_in = T_iter = T_out = T.  emb / res_emb / x_emb: (batch stride, channel stride,
    offset) of the out / res / in view inside its buffer (default: contiguous, offset 0; ops.conv1d takes contiguous inputs only, so a
    case with x_emb goes through the raw ABI).  wview: 'plain' [Cout][Cin][K], 'transposed' (the
    input-gradient operand: storage [Cin][Cout][K], sco <-> sci) or ('phase', k, u, p) (one polyphase branch of a ConvTranspose1d
    weight [Cin][Cout][k]: base p, sco k, sci Cout k, stap u)."""
    c = dict(name=name, impls=impls, B=B, Cin=Cin, Cout=Cout, K=K, dil=dil, T_in=T, pad=abs(dil) * (K - 1) // 2, out_stride=1, out_off=0,
             pro="none", act="none", alpha=False, bias=True, res=False, mask=False, add=False, accumulate=False, out_div=False,
             emb=None, res_emb=None, x_emb=None, wview="plain", modes=("exact", "bounded"))
    c.update(kw)
    c.setdefault("T_out", c["T_in"])
    c.setdefault("T_iter", c["T_out"])
    if c["act"] in ("gelu", "tanh", "softplus", "mish"):
        c["modes"] = ("bounded",)  # no exact form of a transcendental epilogue
    return c


FWD = [
    # ---- mfma v1: tile shape by RBn = ceil(Cout / 32); staging loop by halo = (K - 1) |dil| (piped: nj = ceil((64 WN + halo) / 64)
    #      <= WN + 1, i.e. halo <= 64, LDS sized * 2; else the single-buffered loop over column-block groups, LDS sized * 1) ----
    # RBn = 5 >= 4 -> <4, 1>; grid.y = 2: the second block's rb 5..7 >= RBn (rb_valid == false still stages); halo 2: piped; Cin 40 is
    # not a multiple of 16 (CinP 48); Cout 160: full row blocks -> batched epilogue with bias, res, mask; T_iter 129 = 2 * 64 + 1
    _case("v1_4x1_piped_rows_past_RBn", NMV, 2, 40, 160, 3, 1, 129, res=True, mask=True, act="relu"),
    # RBn = 4 -> <4, 1>; halo 80 in 65..128: unpiped, W = 144, nj = 3 > NJP = 2: two column-block groups (jj0 = 0, 2); T_iter 192 = 3 * 64
    _case("v1_4x1_unpiped_halo80", NM, 1, 24, 128, 3, 40, 192, res=True),
    # RBn = 5 -> <4, 1>, Cout 130: ragged last row block (rb 4: rb * 32 + 32 > Cout -> per-element epilogue, co >= Cout skipped);
    # halo 512 (the largest admitted): W = 576, nj = 9: five groups, the last one odd (`j < W` guard); T_iter 703 = 11 * 64 - 1 >= halo +
    # 64: interior tiles read data through every tap offset 0 / 128 / 256 / 384 / 512
    _case("v1_4x1_unpiped_halo512_ragged_rows", NM, 1, 16, 130, 5, 128, 703, pro="lrelu"),
    # RBn = 3 -> <2, 2>; grid.y = 2: rb 3 >= RBn; halo 18: piped (nj = 3 <= NJP = 3); Cin 20 -> CinP 32 (two chunks: both LDS buffers);
    # full blocks + lrelu + accumulate: batched epilogue with the previous-output batch; T_iter 256 = 2 * 128
    _case("v1_2x2_piped", NMV, 2, 20, 96, 7, 3, 256, act="lrelu", accumulate=True, res=True),
    # RBn = 2 -> <2, 2>; halo 128: unpiped, W = 256, nj = 4 > NJP = 3: groups jj0 = 0, 3; T_iter 257
    _case("v1_2x2_unpiped_halo128", NM, 1, 16, 64, 3, 64, 257, mask=True),
    # RBn = 2 (Cout 40: ragged) -> <2, 2>; halo 504 near 512: W = 632, nj = 10: groups 0, 3, 6, 9; T_iter 767 = 6 * 128 - 1
    _case("v1_2x2_unpiped_halo504_ragged_rows", NM, 1, 16, 40, 9, 63, 767, alpha=True),
    # RBn = 1 -> <1, 4>; halo 50: piped (W = 306, nj = 5 <= NJP = 5); three chunks; T_iter 513 = 2 * 256 + 1
    _case("v1_1x4_piped", NMV, 1, 48, 32, 11, 5, 513, pro="lrelu", res=True),
    # RBn = 1, Cout 7 (ragged: per-element epilogue) -> <1, 4>; halo 66 in 65..128: unpiped, W = 322, nj = 6 > NJP = 5; T_iter 512
    _case("v1_1x4_unpiped_halo66_ragged_rows", NM, 2, 16, 7, 3, 33, 512, add=True),
    # RBn = 1 -> <1, 4>; halo 510 near 512: W = 766, nj = 12: groups 0, 5, 10; T_iter 1023 = 4 * 256 - 1
    _case("v1_1x4_unpiped_halo510", NM, 1, 16, 32, 11, 51, 1023, act="relu"),
    # transcendental activation on FULL row blocks: !act_simple -> the per-element epilogue although rb * 32 + 32 <= Cout
    _case("v1_gelu_on_full_blocks", NMV, 2, 32, 64, 3, 1, 130, act="gelu", alpha=True, res=True, mask=True),
    _case("v1_tanh_one_row", NMV, 1, 32, 1, 7, 1, 300, act="tanh", pro="lrelu"),
    _case("v1_mish_softplus_rows", NMV, 1, 16, 128, 1, 1, 70, act="mish"),
    _case("v1_softplus_mask", NMV, 1, 24, 33, 1, 1, 70, act="softplus", mask=True),
    # ---- mfma2 v2: RB by Cout (>= 384: 4, >= 192: 2, else 1), LDS chunk ch_max = 128 if (64 + halo) * 256 * 4 > 96 KiB (halo > 32)
    #      else 256, chunks = ceil(CinP / ch_max) ----
    # RB 1, Cout 128 (one full 128-row block); ch_max 256, CinP 64: one chunk; two full 64-frame tiles: vec4 epilogue throughout
    _case("v2_rb1_ch256_one_chunk", NMV, 2, 64, 128, 3, 1, 128, res=True, mask=True, act="relu"),
    # RB 2, Cout 200 (ragged: rows 200..255 of the 256-row block are padding); halo 4: ch_max 256, CinP 304: chunks 256 + 48
    _case("v2_rb2_ch256_two_chunks_ragged", NMV, 2, 300, 200, 3, 2, 132, res=True),
    # RB 4, Cout 400 (ragged: 512-row block); halo 4: ch_max 256, one chunk (CinP 48); one tile
    _case("v2_rb4_ch256_one_chunk_ragged", NMV, 1, 48, 400, 5, 1, 64),
    # RB 1, Cout 130 (two row blocks, the second ragged); halo 34 > 32: ch_max 128, CinP 112: one chunk
    _case("v2_rb1_ch128_one_chunk_ragged", NMV, 1, 100, 130, 3, 17, 100, pro="lrelu"),
    # RB 2, Cout 192; halo 50: ch_max 128, Cin 256: two 128-channel chunks (the decode loop of the big-tile image, img_f32_big_index, and the
    # kernel's walk with CH = 128)
    _case("v2_rb2_ch128_two_chunks", NMV, 1, 256, 192, 11, 5, 96, res=True),
    # RB 4, Cout 384; halo 64 exactly (the largest admitted): ch_max 128, CinP 304: chunks 128 + 128 + 48 (ragged third chunk)
    _case("v2_rb4_ch128_three_chunks_halo64", NMV, 1, 300, 384, 5, 16, 72, add=True),
    # ---- v2 epilogue: vec4 = act_simple && out_stride == 1 && out_off == 0 && !accumulate && T_out % 4 == 0 && out_cs % 4 == 0 &&
    #      out_bs % 4 == 0 && (!res || (res_cs % 4 == 0 && res_bs % 4 == 0)) && t0 + 64 <= T_iter && T_iter <= T_out; the base case
    #      v2_rb1_ch256_one_chunk satisfies every term; each case below fails exactly ONE ----
    _case("v2_vec4_T_out_mod4", NMV, 2, 32, 128, 3, 1, 130, res=True, mask=True, emb=(128 * 132, 132, 0),  # T_out & 3 = 2 under
          res_emb=(128 * 132, 132, 0)),                                                               # 16-byte strides (cs 132)
    _case("v2_vec4_out_cs_mod4", NMV, 2, 32, 128, 3, 1, 128, res=True, emb=(128 * 129, 129, 0)),      # out_cs 129, out_bs 16512 (% 4 == 0)
    _case("v2_vec4_out_bs_mod4", NMV, 2, 32, 128, 3, 1, 128, res=True, emb=(128 * 128 + 2, 128, 0)),  # out_bs 16386
    _case("v2_vec4_res_cs", NMV, 2, 32, 128, 3, 1, 128, res=True, res_emb=(16768, 131, 0)),          # res_cs 131, res_bs 16768 (% 4 == 0)
    _case("v2_vec4_res_bs", NMV, 2, 32, 128, 3, 1, 128, res=True, res_emb=(128 * 128 + 6, 128, 0)),   # res_cs 128, res_bs 16390
    _case("v2_vec4_last_tile", NMV, 2, 32, 128, 3, 1, 100, res=True, mask=True),                      # tile 1: t0 + 64 = 128 > T_iter
    _case("v2_vec4_accumulate", NMV, 2, 32, 128, 3, 1, 128, res=True, accumulate=True),
    _case("v2_vec4_act_gelu", NMV, 2, 32, 128, 3, 1, 128, res=True, act="gelu"),
    _case("v2_vec4_out_stride", NMV, 2, 32, 128, 3, 1, 128, T_iter=128, T_out=256, out_stride=2),
    _case("v2_vec4_out_off", NMV, 2, 32, 128, 3, 1, 128, T_iter=128, T_out=132, out_off=4),
    _case("v2_vec4_T_iter_gt_T_out", NMV, 2, 32, 128, 3, 1, 128, T_iter=128, T_out=124),                        # frames 124..127 are skipped
    # vec4 taken with strided, 16-byte aligned views (out_cs 136, res_cs 132) and lrelu; Cout 120: the 16-row group 112..127 is partial
    _case("v2_vec4_strided_views", NMV, 2, 32, 120, 3, 1, 128, res=True, mask=True, act="lrelu", emb=(130 * 136, 136, 4 * 136),
          res_emb=(125 * 132, 132, 132)),
    # ---- operand forms of production calls ----
    # out = a channel slice of a larger tensor (diffnet.py: condproj[:, l*2C:(l+1)*2C]): out_bs = 3 Cout T != Cout T_out
    _case("form_out_channel_slice", NMV, 2, 48, 64, 1, 1, 96, emb=(3 * 64 * 96, 96, 64 * 96)),
    _case("form_out_channel_slice_ragged", NMV, 2, 48, 200, 3, 1, 70, emb=(3 * 200 * 70, 70, 200 * 70), act="relu"),
    # out = a frame slice (frames 3..3+T_out of rows of T + 8): a 4-byte-aligned base under 16-byte strides
    _case("form_out_frame_slice", NMV, 2, 48, 128, 3, 1, 128, emb=(128 * 136, 136, 3), res=True),
    _case("form_out_frame_slice_ragged", NMV, 1, 20, 40, 3, 2, 75, emb=(40 * 83, 83, 5)),
    # res with strides of its own (a slice of a wider, longer tensor)
    _case("form_res_strides", NMV, 2, 32, 96, 3, 1, 128, res=True, res_emb=(200 * 140, 140, 7 * 140 + 4), act="relu"),
    _case("form_res_strides_ragged", NMV, 2, 32, 70, 5, 1, 90, res=True, res_emb=(99 * 93, 93, 11), mask=True),
    # in = a channel slice / a frame slice of a larger tensor (in_bs != Cin T_in, in_cs != T_in): raw ABI
    _case("form_in_channel_slice", NMV, 2, 40, 96, 3, 1, 100, x_emb=(3 * 40 * 100, 100, 40 * 100), res=True),
    _case("form_in_frame_slice", NMV, 2, 40, 200, 5, 2, 100, x_emb=(40 * 111 + 3, 111, 5), pro="lrelu", add=True),
    _case("form_in_slice_fewout", ("naive", "fewout"), 2, 12, 2, 7, 1, 1100, x_emb=(3 * 12 * 1104, 1104, 12 * 1104 + 4), pro="lrelu"),
    # T_out > T_iter (preln_ffn T_out=): frames T_iter.. keep their content; T_out < T_in: the unpadded conv
    _case("form_T_out_gt_T_iter", NMV, 2, 32, 96, 3, 1, 64, T_iter=50, T_out=80),
    _case("form_T_out_gt_T_iter_v2_rows", NMV, 1, 32, 192, 5, 1, 96, T_iter=70, T_out=100, res=True),
    _case("form_unpadded", NMV, 2, 32, 64, 5, 1, 100, pad=0, T_out=96),
    _case("form_unpadded_dilated", NMV, 1, 32, 130, 3, 8, 100, pad=0, T_out=84, act="relu"),
    _case("form_overpadded", NMV, 1, 16, 32, 3, 1, 60, pad=3, T_out=64),
    # accumulate with and without out_div (the MRF sum / mean of hifigan.py folded into a ResBlock's last conv)
    _case("form_accumulate", NMV, 2, 32, 64, 3, 1, 200, accumulate=True, pro="lrelu", res=True),
    _case("form_accumulate_out_div", NMV, 2, 32, 64, 3, 1, 200, accumulate=True, out_div=True, pro="lrelu", res=True),
    _case("form_accumulate_out_div_ragged", NMV, 1, 32, 200, 7, 1, 100, accumulate=True, out_div=True, pro="lrelu", res=True),
    _case("form_accumulate_out_div_one_row_block", NMV, 1, 16, 32, 11, 1, 300, accumulate=True, out_div=True, act="lrelu", mask=True),
    # alpha, act_param and PRO_DIV on every kernel
    _case("form_alpha_lrelu_div", NMV, 2, 32, 128, 3, 1, 128, alpha=True, act="lrelu", pro="div", add=True),
    _case("form_alpha_lrelu_div_ragged", NMV, 1, 20, 50, 5, 1, 77, alpha=True, act="lrelu", pro="div", add=True, mask=True),
    _case("form_no_bias", NMV, 1, 32, 96, 3, 1, 128, bias=False),
    # the T_iter < 16 path of `auto`: naive
    _case("auto_T_iter_15_is_naive", ("auto",) + NMV, 2, 256, 1024, 1, 1, 15, act="mish"),
    _case("auto_T_iter_1", ("auto",) + NMV, 3, 256, 192, 1, 1, 1),
    # ---- real shapes ----
    # HiFi-GAN v1 ResBlock1 c1 (k 11, dil 5, halo 50: v1 piped, v2 ch_max 128 with 4 / 2 / 1 chunks), lrelu prologue; Cin K = 5632
    _case("real_resblock_C512_k11_d5", ("mfma", "mfma2"), 1, 512, 512, 11, 5, 2048, pro="lrelu"),
    _case("real_resblock_C256_k11_d5", ("mfma", "mfma2"), 1, 256, 256, 11, 5, 2048, pro="lrelu", res=True),
    _case("real_resblock_C128_k11_d5", NMV, 1, 128, 128, 11, 5, 2112, pro="lrelu", accumulate=True, out_div=True, res=True),
    # DiffNet input-gradient convs: dilated conv (512 -> 256, k 3, dil = the yaml's dilation 1: dilation_cycle_length 1) and the
    # decoder FFN conv (384 -> 192, k 5), in gradient form (transposed weights, dil < 0, pad < 0)
    _case("real_diffnet_dilated_dx", NMV, 1, 512, 256, 3, -1, 800, pad=-1, wview="transposed"),
    _case("real_ffn_k5_dx", NMV, 2, 384, 192, 5, -1, 200, pad=-2, wview="transposed", mask=True),
]
# input-gradient form: dil < 0 with pad = -|dil| (K - 1) / 2 for K 3 / 5 / 9 and |dil| 1 / 2 / 8 (halo 64 for K 9, dil 8: still v2)
FWD += [_case("form_grad_k%d_d%d" % (K, d), NMV, 2, 48, 40, K, -d, 90, pad=-d * (K - 1) // 2, wview="transposed", res=K == 5)
        for K in (3, 5, 9) for d in (1, 2, 8)]
# polyphase transposed conv: out_stride u, out_off = p - P for every phase p (out_off in -P .. u - 1 - P; frames n < 0 and n >= T_out
# are skipped), dil -1, T_iter = T_in + J - 1, the strided weight view through set_pack_conv_weight and set_pack_conv_weight_v2.
# u 8: the first HiFi-GAN v1 upsampler (512 -> 256, k 16, P 4); u 2: the third (128 -> 64, k 4, P 1)
for _Cin, _Cout, _k, _u, _P, _T in ((512, 256, 16, 8, 4, 40), (128, 64, 4, 2, 1, 100), (24, 200, 7, 3, 2, 70)):
    for _p_, _J, _kw in polyphase_calls(_T, _k, _u, _P):
        FWD.append(_case("phase_%dto%d_k%d_u%d_p%d" % (_Cin, _Cout, _k, _u, _p_), NMV, 2, _Cin, _Cout, _J, _kw["dil"], _T, pro="lrelu",
                         wview=("phase", _k, _u, _p_), **{k_: v_ for k_, v_ in _kw.items() if k_ != "dil"}))

# exact / bounded parameter values
PARAMS = {"exact": dict(pro_lrelu=0.25, pro_div=2.0, act_lrelu=0.125, alpha=0.5, out_div=4.0),
          "bounded": dict(pro_lrelu=0.1, pro_div=20 ** 0.5, act_lrelu=0.2, alpha=5 ** -0.5, out_div=3.0)}


def _embed(view_shape, emb, fill, g, guard=64):
    """A flat buffer and the (bs, cs, off) view of `view_shape` inside it.  fill: a constant, or 'ints' / 'randn'."""
    B, Cc, T = view_shape
    bs, cs, off = emb if emb is not None else (Cc * T, T, 0)
    assert cs >= T and bs >= (Cc - 1) * cs + T  # no overlap
    n = off + (B - 1) * bs + (Cc - 1) * cs + T + (guard if emb is not None else 0)
    if fill == "ints":
        buf = ints(g, (n,), -4, 4)
    elif fill == "randn":
        buf = torch.randn(n, generator=g)
    else:
        buf = torch.full((n,), float(fill))
    return buf, (lambda b: b.as_strided((B, Cc, T), (bs, cs, 1), off))


def _make(c, mode):
    """CPU operands of a case (fp32), the reference's image of the whole out buffer and the per-element bar of every buffer element."""
    pv = PARAMS[mode]
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]) * 7 + (mode == "exact"))
    B, Cin, Cout, K = c["B"], c["Cin"], c["Cout"], c["K"]
    exact = mode == "exact"
    rnd = (lambda shape, lo, hi, sc=1.0: ints(g, shape, lo, hi)) if exact else (lambda shape, lo, hi, sc=1.0: torch.randn(shape, generator=g) * sc)
    o = dict(c)
    o["x"] = rnd((B, Cin, c["T_in"]), -3, 3)
    wv = c["wview"]
    wsc = (Cin * K) ** -0.5
    if wv == "plain":
        o["wstore"], o["waddr"] = rnd((Cout, Cin, K), -2, 2, wsc), dict(base=0, sco=Cin * K, sci=K, stap=1)
    elif wv == "transposed":
        o["wstore"], o["waddr"] = rnd((Cin, Cout, K), -2, 2, wsc), dict(base=0, sco=K, sci=Cout * K, stap=1)
    else:
        _, k, u, p = wv
        o["wstore"], o["waddr"] = rnd((Cin, Cout, k), -2, 2, wsc), dict(base=p, sco=k, sci=Cout * k, stap=u)
    W = weight_view(o["wstore"], Cout, Cin, K, **o["waddr"])
    o["bias_t"] = rnd((Cout,), -4, 4, 0.1) if c["bias"] else None
    o["mask_t"] = (torch.rand(B, c["T_out"], generator=g) > 0.3).float() if c["mask"] else None
    o["add_t"] = rnd((B, Cin), -2, 2) if c["add"] else None
    shape = (B, Cout, c["T_out"])
    o["res_buf"], o["res_view"] = (None, None)
    if c["res"]:
        o["res_buf"], o["res_view"] = _embed(shape, c["res_emb"], "ints" if exact else "randn", g)
    # the out buffer: the previous output where the call accumulates, the sentinel otherwise -- guards included
    o["out_buf"], o["out_view"] = _embed(shape, c["emb"], ("ints" if exact else "randn") if c["accumulate"] else SENTINEL, g)
    kw = dict(dil=c["dil"], pad=c["pad"], T_iter=c["T_iter"], T_out=c["T_out"], out_stride=c["out_stride"], out_off=c["out_off"],
              pro=c["pro"], pro_param={"lrelu": pv["pro_lrelu"], "div": pv["pro_div"], "none": 0.0}[c["pro"]], act=c["act"],
              act_param=pv["act_lrelu"] if c["act"] == "lrelu" else 0.0, alpha=pv["alpha"] if c["alpha"] else 1.0,
              accumulate=c["accumulate"], out_div=pv["out_div"] if c["out_div"] else 0.0)
    o["kw"] = kw
    res = o["res_view"](o["res_buf"]) if c["res"] else None
    prev = o["out_view"](o["out_buf"]).clone()
    r = conv_ref(o["x"], W, bias=o["bias_t"], res=res, mask=o["mask_t"], in_chan_add=o["add_t"], prev=prev, **kw)
    if exact:
        # every intermediate is a multiple of q and below 2^24 q in magnitude, in any summation order
        q = {"lrelu": pv["pro_lrelu"], "div": 1.0 / pv["pro_div"], "none": 1.0}[c["pro"]] * min(1.0, kw["alpha"]) * \
            (pv["act_lrelu"] if c["act"] == "lrelu" else 1.0) * (1.0 / pv["out_div"] if c["out_div"] else 1.0)
        top = float(r["S"].max()) * max(1.0, kw["alpha"]) + 16.0
        assert top / q < 2 ** 24, (top, q)
    want = o["out_buf"].double().clone()
    o["out_view"](want).copy_(r["y"])
    bar = torch.zeros_like(want)
    if not exact:
        b = conv_bound(r, Cin * K, act=c["act"], act_param=kw["act_param"], alpha=kw["alpha"], res=res, prev=prev if c["accumulate"] else None)
        o["out_view"](bar).copy_(b * r["written"].double())
    o["want"], o["bar"], o["written"] = want, bar, int(r["written"].sum())
    return o


def _run(o, impl, dev):
    """One ops.conv1d call on fresh device copies; returns the whole out buffer."""
    from set_amd import ops
    wd = o["wstore"].to(dev)
    cw = ops.ConvWeight(lambda: wd, o["Cout"], o["Cin"], o["K"], **o["waddr"])
    out_buf = o["out_buf"].to(dev)
    res_buf = o["res_buf"].to(dev) if o["res_buf"] is not None else None
    t = lambda v: None if v is None else v.to(dev)
    kw = o["kw"]
    if impl == "auto":
        assert ops._pick_impl("auto", o["T_iter"], o["Cout"], o["Cin"], o["K"], o["dil"]) == "naive"
    if o["x_emb"] is not None:
        return _run_raw(o, impl, cw, out_buf, res_buf, dev)
    y = ops.conv1d(o["x"].to(dev), cw, t(o["bias_t"]), res=None if res_buf is None else o["res_view"](res_buf), mask=t(o["mask_t"]),
                   in_chan_add=t(o["add_t"]), out=o["out_view"](out_buf), impl=impl, **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == o["out_view"](out_buf).data_ptr()
    if res_buf is not None:
        assert torch.equal(res_buf.cpu(), o["res_buf"])  # operands are read-only
    return out_buf.cpu()


def _run_raw(o, impl, cw, out_buf, res_buf, dev):
    """The same call with `in` as a strided view: SetConv1dArgs filled by hand (ops.conv1d has no input strides)."""
    from set_amd import _lib
    B, Cin, T_in = o["x"].shape
    x_buf, x_view = _embed((B, Cin, T_in), o["x_emb"], 99.0, None)  # 99 around the slice: a read outside it shows in the sums
    x_view(x_buf).copy_(o["x"])
    xd = x_buf.to(dev)
    kw = o["kw"]
    t = lambda v: None if v is None else v.to(dev)
    bias, mask, add = t(o["bias_t"]), t(o["mask_t"]), t(o["add_t"])
    out, res = o["out_view"](out_buf), None if res_buf is None else o["res_view"](res_buf)
    a = _lib.SetConv1dArgs()
    a.inp = _p(xd) + 4 * o["x_emb"][2]
    a.w = _p({"mfma": cw.packed, "mfma2": lambda: cw.packed_v2(o["dil"])}.get(impl, cw.raw)())
    a.bias, a.mask, a.in_chan_add = _p(bias), _p(mask), _p(add)
    a.res = None if res is None else res.data_ptr()
    a.out = out.data_ptr()
    _ALIVE.extend([out_buf, res_buf])
    a.in_bs, a.in_cs = o["x_emb"][0], o["x_emb"][1]
    a.out_bs, a.out_cs = out.stride(0), out.stride(1)
    if res is not None:
        a.res_bs, a.res_cs = res.stride(0), res.stride(1)
    a.w_base, a.w_sco, a.w_sci, a.w_stap = cw.base, cw.sco, cw.sci, cw.stap
    a.B, a.Cin, a.Cout, a.K, a.dil, a.pad = B, Cin, o["Cout"], o["K"], kw["dil"], kw["pad"]
    a.T_in, a.T_iter, a.T_out, a.out_stride, a.out_off = T_in, kw["T_iter"], kw["T_out"], kw["out_stride"], kw["out_off"]
    a.pro, a.act, a.accumulate = _lib.PRO[kw["pro"]], _lib.ACT[kw["act"]], int(kw["accumulate"])
    a.impl = {"naive": _lib.IMPL_NAIVE, "mfma": _lib.IMPL_MFMA, "mfma2": _lib.IMPL_MFMA2, "fewout": _lib.IMPL_FEWOUT}[impl]
    a.pro_param, a.act_param, a.alpha, a.out_div = kw["pro_param"], kw["act_param"], kw["alpha"], kw["out_div"]
    _lib.check(_L().set_conv1d(C.byref(a), _s()), "set_conv1d")
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x_buf)
    return out_buf.cpu()


def _admits(c, impl):
    halo = (c["K"] - 1) * abs(c["dil"])
    return halo <= (64 if impl == "mfma2" else 512) if impl in ("mfma", "mfma2") else True


def _report(name, impl, got, want, bar):
    d = (got.double() - want).abs()
    bad = (~(d <= bar)).nonzero().flatten()  # (a NaN is outside any bar)
    over = float((d / (bar + 1e-300)).max()) if bool((bar > 0).any()) else 0.0
    print("%s[%s]: max |d| %.3e, max |d| / bar %.3f, %d of %d buffer elements outside" % (name, impl, float(d.max()), over, bad.numel(), d.numel()))
    return bad


FWD_RUNS = [(c, mode) for c in FWD for mode in c["modes"]]


@pytest.mark.parametrize("c,mode", FWD_RUNS, ids=["%s-%s" % (c["name"], mode) for c, mode in FWD_RUNS])
def test_conv_forward_branch(dev, c, mode):
    o = _make(c, mode)
    assert 0 < o["written"] <= c["B"] * c["Cout"] * c["T_out"]
    got = {}
    for impl in c["impls"]:
        assert _admits(c, impl)
        got[impl] = _run(o, impl, dev)
        bad = _report(c["name"], impl, got[impl], o["want"], o["bar"])
        # exact: the bar is zero everywhere; bounded: zero outside the reference's written set
        assert bad.numel() == 0, (impl, bad[:8].tolist(), got[impl][bad[:8]].tolist(), o["want"][bad[:8]].tolist())
        assert bool(torch.isfinite(got[impl]).all())
    if mode == "exact":
        first = got[c["impls"][0]]
        for impl in c["impls"][1:]:
            assert torch.equal(got[impl], first), impl  # kernels against each other


def test_forward_inventory_is_complete():
    """Every row of the branch inventory is a named case (the C conditions are in the comments of FWD)."""
    halo = lambda c: (c["K"] - 1) * abs(c["dil"])
    v1 = [c for c in FWD if "mfma" in c["impls"]]
    for lo, hi in ((4, 99), (2, 3), (1, 1)):  # RBn -> tile shape
        rows = [c for c in v1 if lo <= -(-c["Cout"] // 32) <= hi]
        assert any(halo(c) <= 64 for c in rows) and any(65 <= halo(c) <= 128 for c in rows) and any(500 <= halo(c) <= 512 for c in rows)
    for WN, lo, hi in ((1, 4, 99), (2, 2, 3), (4, 1, 1)):
        rem = {c["T_iter"] % (64 * WN) for c in v1 if lo <= -(-c["Cout"] // 32) <= hi}
        assert {64 * WN - 1, 0, 1} <= rem, (WN, rem)
    for c in FWD:  # every tap of every case reads in-range data for some frame
        for tap in range(c["K"]):
            lo_t, hi_t = tap * c["dil"] - c["pad"], c["T_iter"] - 1 + tap * c["dil"] - c["pad"]
            assert hi_t >= 0 and lo_t < c["T_in"], (c["name"], tap)
    for c in v1:   # wide halos: an interior tile whose whole staging window [t0 + lo, t0 + lo + 64 WN + halo) holds data
        WN = 1 if c["Cout"] > 96 else (2 if c["Cout"] > 32 else 4)
        assert halo(c) <= 64 or c["T_in"] >= halo(c) + 64 * WN, c["name"]
    v2 = [c for c in FWD if "mfma2" in c["impls"]]
    chunks = lambda c: (128 if halo(c) > 32 else 256, -(-(-(-c["Cin"] // 16) * 16) // (128 if halo(c) > 32 else 256)))
    assert {(256, 1), (256, 2), (128, 1), (128, 2), (128, 3)} <= {chunks(c) for c in v2}
    assert {200, 130, 400, 128, 192, 384} <= {c["Cout"] for c in v2} and 64 in {halo(c) for c in v2}
    assert {(K, d) for K in (3, 5, 9) for d in (1, 2, 8)} <= {(c["K"], -c["dil"]) for c in FWD if c["wview"] == "transposed"}
    offs = {(c["out_stride"], c["out_off"]) for c in FWD if c["out_stride"] > 1}
    assert {(8, o) for o in range(-4, 4)} | {(2, -1), (2, 0)} <= offs
    assert len({c["name"] for c in FWD}) == len(FWD)


# ------------------------------------------------------------------------------------------------------------------------
# the one-launch re-pack of the optimizer (set_pack_conv_weights_batch: the pack kernel over a descriptor table on the device): same bits as
# set_pack_conv_weight / set_pack_conv_weight_v2 (the same kernel, one descriptor by value) for the layouts the forward cases above validate
# ------------------------------------------------------------------------------------------------------------------------
REPACK = [
    # Cout, Cin, K, dil, wview
    (384, 300, 5, 16, "plain"),           # v2: RB 4, ch_max 128, chunks 128 + 128 + 48
    (192, 256, 11, 5, "plain"),           # v2: RB 2, ch_max 128, two chunks
    (200, 300, 3, 2, "plain"),            # v2: RB 2 ragged, ch_max 256, chunks 256 + 48
    (130, 100, 3, -17, "transposed"),     # v2: RB 1 ragged, ch_max 128, one chunk; transposed addressing
    (256, 512, 2, -1, ("phase", 16, 8, 5)),  # polyphase view: base 5, sco 16, sci 256 * 16, stap 8
    (7, 20, 3, 1, "plain"),               # one ragged row block, Cin not a multiple of 16
]


def test_batched_repack_equals_the_per_image_packers_for_every_layout(dev):
    from set_amd import ops
    ops.repack_f32_images()  # images other modules used so far: not this test's business
    g = torch.Generator().manual_seed(5)
    cws, keep = [], []
    for Cout, Cin, K, dil, wv in REPACK:
        if wv == "plain":
            w, addr = torch.randn(Cout, Cin, K, generator=g), {}
        elif wv == "transposed":
            w, addr = torch.randn(Cin, Cout, K, generator=g), dict(sco=K, sci=Cout * K)
        else:
            _, k, u, p = wv
            w, addr = torch.randn(Cin, Cout, k, generator=g), dict(base=p, sco=k, sci=Cout * k, stap=u)
        wd = w.to(dev)
        keep.append(wd)
        cws.append((ops.ConvWeight(wd, Cout, Cin, K, **addr), dil))
    images = [(cw.packed(), cw.packed_v2(dil)) for cw, dil in cws]
    want = [(a.clone(), b.clone()) for a, b in images]
    for a, b in images:  # poison in place: whatever the batch launch does not write shows
        a.fill_(float("nan"))
        b.fill_(float("nan"))
    assert ops.repack_f32_images() >= 2 * len(cws)
    torch.cuda.synchronize()
    for (a, b), (wa, wb), case in zip(images, want, REPACK):
        assert torch.equal(a, wa) and torch.equal(b, wb), case
        assert bool(torch.isfinite(wa).all()) and bool(torch.isfinite(wb).all())


# ------------------------------------------------------------------------------------------------------------------------
# refused forms through the raw ABI: SET_E_UNSUPPORTED, `out` untouched
# ------------------------------------------------------------------------------------------------------------------------
def _raw_args(dev, impl, *, B=2, Cin=8, Cout=1, K=7, dil=1, pad=3, T_in=64, T_iter=None, T_out=None, out_stride=1, out_off=0, res=False,
              mask=False, add=False, accumulate=False, in_bs=None, in_cs=None, out_bs=None, out_cs=None, in_shift=0, out_shift=0):
    from set_amd import _lib
    T_out = T_in if T_out is None else T_out
    T_iter = T_out if T_iter is None else T_iter
    slack = 4096  # every buffer is large enough for any of the forms, should one be launched after all
    x = torch.ones(B * Cin * T_in + slack, device=dev)
    w = torch.ones(max(_L().set_packed_conv_weight_v2_size(Cout, Cin, K), _L().set_packed_conv_weight_size(Cout, Cin, K)), device=dev)
    out = torch.full((B * max(Cout, 2) * max(T_out, T_in) * 2 + slack,), SENTINEL, device=dev)
    other = torch.ones(out.numel(), device=dev)
    a = _lib.SetConv1dArgs()
    a.inp, a.w, a.out = _p(x) + 4 * in_shift, _p(w), _p(out) + 4 * out_shift
    a.bias = _p(other)
    a.res = _p(other) if res else None
    a.mask = _p(other) if mask else None
    a.in_chan_add = _p(other) if add else None
    a.in_bs, a.in_cs = (Cin * T_in if in_bs is None else in_bs), (T_in if in_cs is None else in_cs)
    a.out_bs, a.out_cs = (Cout * T_out if out_bs is None else out_bs), (T_out if out_cs is None else out_cs)
    a.res_bs, a.res_cs = Cout * T_out, T_out
    a.w_base, a.w_sco, a.w_sci, a.w_stap = 0, Cin * K, K, 1
    a.B, a.Cin, a.Cout, a.K, a.dil, a.pad = B, Cin, Cout, K, dil, pad
    a.T_in, a.T_iter, a.T_out, a.out_stride, a.out_off = T_in, T_iter, T_out, out_stride, out_off
    a.pro, a.act, a.accumulate, a.impl = 0, 0, int(accumulate), impl
    a.pro_param, a.act_param, a.alpha, a.out_div = 0.0, 0.0, 1.0, 0.0
    return a, out


FEWOUT_REFUSED = [
    ("Cout 3", dict(Cout=3)), ("K 11", dict(K=11, pad=4)), ("dil 2", dict(K=3, dil=2, pad=2)), ("pad -1", dict(K=3, pad=-1)),
    ("pad 5", dict(K=9, pad=5)), ("K - pad 6", dict(K=7, pad=1)), ("out_stride 2", dict(out_stride=2, T_out=128, T_iter=128)),
    ("out_off 4", dict(out_off=4)), ("T_in != T_out", dict(T_out=60)), ("T_iter != T_out", dict(T_iter=60)), ("T % 4", dict(T_in=66, in_cs=68, in_bs=8 * 68, out_cs=68, out_bs=68)),
    ("res", dict(res=True)), ("mask", dict(mask=True)), ("in_chan_add", dict(add=True)), ("accumulate", dict(accumulate=True)),
    ("in_bs % 4", dict(in_bs=8 * 64 + 2)), ("in_cs % 4", dict(in_cs=65, in_bs=8 * 65)), ("out_bs % 4", dict(out_bs=66)),
    ("out_cs % 4", dict(Cout=2, out_cs=65, out_bs=132)), ("in not 16-byte aligned", dict(in_shift=1)),
    ("out not 16-byte aligned", dict(out_shift=2)),
]


@pytest.mark.parametrize("why,kw", FEWOUT_REFUSED, ids=[w.replace(" ", "_") for w, _ in FEWOUT_REFUSED])
def test_fewout_refuses_what_it_cannot_run_and_leaves_out_alone(dev, why, kw):
    """launch_conv_fewout: each term of its `ok` condition in turn."""
    from set_amd import _lib
    a, out = _raw_args(dev, _lib.IMPL_FEWOUT, **kw)
    assert _L().set_conv1d(C.byref(a), _s()) == E_UNSUPPORTED, why
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_fewout_runs_the_call_the_refusals_are_variations_of(dev):
    from set_amd import _lib
    a, out = _raw_args(dev, _lib.IMPL_FEWOUT)
    assert _L().set_conv1d(C.byref(a), _s()) == 0
    torch.cuda.synchronize()
    assert bool((out[:2 * 64] != SENTINEL).all()) and bool((out[2 * 64:] == SENTINEL).all())


@pytest.mark.parametrize("impl,K,dil,ok", [("mfma2", 5, 16, True), ("mfma2", 6, 13, False), ("mfma2", 2, 65, False), ("mfma2", 2, -65, False),
                                           ("mfma", 3, 256, True), ("mfma", 3, 257, False), ("mfma", 2, -513, False)])
def test_receptive_field_limits_are_refused_cleanly(dev, impl, K, dil, ok):
    """launch_conv_v2: halo > 64, set_conv1d(mfma): halo > 512 -> SET_E_UNSUPPORTED before any launch."""
    from set_amd import _lib
    a, out = _raw_args(dev, {"mfma": _lib.IMPL_MFMA, "mfma2": _lib.IMPL_MFMA2}[impl], Cin=16, Cout=32, K=K, dil=dil,
                       pad=abs(dil) * (K - 1) // 2, T_in=128)
    rc = _L().set_conv1d(C.byref(a), _s())
    torch.cuda.synchronize()
    assert rc == (0 if ok else E_UNSUPPORTED)
    assert bool((out[:2 * 32 * 128] != SENTINEL).all()) == ok and bool((out[2 * 32 * 128:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------
# fewout: Cout 1 / 2, K 1 / 7 / 9 with every admissible pad (0 <= pad <= 4, K - pad <= 5), T a multiple of 4 but not of the 1024
# frames of a block (the last block is partial), against the reference and the naive kernel
# ------------------------------------------------------------------------------------------------------------------------
FEWOUT = [(Cout, K, pad) for Cout in (1, 2) for K in (1, 7, 9) for pad in range(5) if K - pad <= 5]


@pytest.mark.parametrize("Cout,K,pad", FEWOUT)
def test_fewout_every_admissible_tap_window(dev, Cout, K, pad):
    assert len(FEWOUT) == 2 * (5 + 3 + 1)
    T = 1036 + 4 * K  # two blocks, the second one partial; T % 1024 != 0
    for mode in ("exact", "bounded"):
        for pro, act in (("lrelu", "none"), ("div", "tanh" if mode == "bounded" else "relu")):
            c = _case("fewout_C%d_k%d_p%d_%s" % (Cout, K, pad, pro), ("naive", "fewout"), 2, 12, Cout, K, 1, T, pad=pad, pro=pro, act=act,
                      alpha=pro == "div")
            o = _make(c, mode)
            assert o["written"] == 2 * Cout * T
            got = [_run(o, impl, dev) for impl in c["impls"]]
            for impl, gt in zip(c["impls"], got):
                assert _report(c["name"] + "/" + mode, impl, gt, o["want"], o["bar"]).numel() == 0, impl
                assert bool(torch.isfinite(gt).all())
            if mode == "exact":
                assert torch.equal(got[0], got[1])


def test_auto_takes_fewout_for_conv_post_and_matches(dev, monkeypatch):
    """hifigan conv_post through impl=None: plain, Cout 1, K 7, pad 3, T_iter 4096 -> fewout (pinned on the CPU by
    test_auto_picks_the_expected_kernel); the result equals the explicit kernel's."""
    from set_amd import ops
    c = _case("conv_post", ("fewout", None), 1, 32, 1, 7, 1, 4096, pro="lrelu")
    o = _make(c, "exact")
    monkeypatch.setattr(ops, "_DEFAULT_IMPL", "auto")  # whatever SET_AMD_CONV_IMPL said
    assert ops.compute_dtype() == "f32" and ops._pick_impl(None, 4096, 1, 32, 7, 1, plain=True, pad=3) == "fewout"
    a, b = _run(o, "fewout", dev), _run(o, None, dev)
    assert torch.equal(a.double(), o["want"]) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------
# weight gradient: conv1d_wgrad_mfma_kernel (atomic and deterministic), the naive kernel; cases and their slice plans:
# WGRAD_CASES in tests/test_conv_reference.py
# ------------------------------------------------------------------------------------------------------------------------
PRO_CODE = {"none": 0, "lrelu": 1, "div": 2}


def _wgrad_operands(case, mode):
    name, B, Cin, Cout, K, dil, T, with_add, pro, _ = case
    g = torch.Generator().manual_seed(B * 1000 + Cin + Cout + K + T)
    pad = dil * (K - 1) // 2
    exact = mode == "exact"
    pp = {"none": 0.0, "lrelu": 0.25 if exact else 0.1, "div": 2.0 if exact else 20 ** 0.5}[pro]
    if exact:
        # |g| <= 2, |x + add| <= 3: B T <= 25600 frames -> |sum| <= 153600 < 2^24 (times the power-of-two prologue quantum)
        gy, x = ints(g, (B, Cout, T), -2, 2), ints(g, (B, Cin, T), -2, 2)
        add = ints(g, (B, Cin), -1, 1) if with_add else None
        dw0 = ints(g, (Cout, Cin, K), -4, 4)
    else:
        gy, x = torch.randn(B, Cout, T, generator=g), torch.randn(B, Cin, T, generator=g)
        add = torch.randn(B, Cin, generator=g) if with_add else None
        dw0 = torch.randn(Cout, Cin, K, generator=g)
    dw, A = wgrad_ref(gy, x, K, dil, pad, in_chan_add=add, pro=pro, pro_param=pp)
    return gy, x, add, dw0, pad, pp, dw, A


def _wgrad_paths(dev, case, gy, x, add, dw0, pad, pp):
    """dW (pre-filled with dw0: accumulate semantics) through every fp32 path."""
    from set_amd import _lib, autograd_ops as A_, ops
    _, B, Cin, Cout, K, dil, T, _, pro, (_, _, gz) = case
    L = _L()
    gd, xd, ad = gy.to(dev), x.to(dev), None if add is None else add.to(dev)
    outs = {}
    for path in ("atomic", "naive", "det", "conv_wgrad"):
        dw = dw0.to(dev)
        if path in ("atomic", "naive"):
            rc = L.set_conv1d_wgrad(_p(gd), _p(xd), _p(ad), _p(dw), B, Cin, Cout, K, dil, pad, T, T, PRO_CODE[pro], pp,
                                    _lib.IMPL_MFMA if path == "atomic" else _lib.IMPL_NAIVE, _s())
        elif path == "det":
            need = L.set_conv1d_wgrad_scratch_floats(B, Cin, Cout, K, T, _lib.DTYPE_F32)
            assert need == gz * Cout * Cin * K
            scratch = torch.full((need,), float("nan"), device=dev)  # poisoned: an empty slice must store zeros, not leave garbage
            rc = L.set_conv1d_wgrad_det(_p(gd), _p(xd), _p(ad), _p(dw), B, Cin, Cout, K, dil, pad, T, T, PRO_CODE[pro], pp, _lib.DTYPE_F32,
                                        _p(scratch), need, _s())
        else:  # the production wrapper: deterministic entry point for T >= 16 (compute dtype f32)
            assert T >= 16 and ops.compute_dtype() == "f32"
            A_.conv_wgrad(gd, xd, ad, dw, B, Cin, Cout, K, dil, pad, T, T, PRO_CODE[pro], pp)
            rc = 0
        assert rc == 0, path
        torch.cuda.synchronize()
        outs[path] = dw.cpu()
    return outs


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_wgrad_slice_plans(dev, case, mode):
    _, B, Cin, Cout, K, dil, T, _, _, (slices, cps, gz) = case
    plan = wgrad_plan(B, Cin, Cout, K, T)
    assert plan[:3] == (slices, cps, gz)
    gy, x, add, dw0, pad, pp, dw, A = _wgrad_operands(case, mode)
    want = dw0.double() + dw
    outs = _wgrad_paths(dev, case, gy, x, add, dw0, pad, pp)
    if mode == "exact":
        assert float(A.max()) * 4 + 8 < 2 ** 24
        for path, got in outs.items():
            bad = (got.double() != want).nonzero()
            print("%s[%s]: %d of %d weights differ" % (case[0], path, bad.shape[0], want.numel()))
            assert bad.shape[0] == 0, (path, bad[:6].tolist())
        return
    # a frame sum of B T products in any order, then <= slices partial sums (slice order, or atomics in any order; gz <= slices) and the
    # add onto the previous dW, which the "+ 4" covers (|dW0| << sum |g| |P(x)| here): gamma(B T + slices + 4) sum |g| |P(x)|
    assert gz <= slices and float(dw0.abs().max()) < float(A.min())
    bar = gamma(B * T + slices + 4) * A
    for path, got in outs.items():
        d = (got.double() - want).abs()
        print("%s[%s]: max |d| %.3e, max |d| / bar %.3f" % (case[0], path, float(d.max()), float((d / bar).max())))
        assert bool((d <= bar).all()), path
    assert torch.equal(outs["det"], outs["conv_wgrad"])  # the same kernel and slice order: bit-identical


def test_grouped_wgrad_entry_point_has_no_fp32_form(dev):
    """set_conv1d_wgrad_det_grouped takes bf16 operand types only (include/set_amd.h); SET_DTYPE_F32 is refused as an invalid argument
    and dW is left alone (the bf16 kernels have their own bit-level tests in tests/test_gpu_bf16.py)."""
    from set_amd import _lib
    B, Cin, Cout, K, T, G = 2, 64, 128, 3, 64, 2
    gy, x = torch.ones(G * B * Cout * T, device=dev), torch.ones(G * B * Cin * T, device=dev)
    dw = torch.full((G * Cout * Cin * K,), SENTINEL, device=dev)
    need = _L().set_conv1d_wgrad_grouped_scratch_floats(G, B, Cin, Cout, K, T)
    scratch = torch.zeros(need, device=dev)
    rc = _L().set_conv1d_wgrad_det_grouped(_p(gy), _p(x), None, _p(dw), G, B * Cout * T, B * Cin * T, 0, Cout * Cin * K, B, Cin, Cout, K, 1, 1, T,
                                           T, _lib.DTYPE_F32, _p(scratch), need, _s())
    torch.cuda.synchronize()
    assert rc == E_INVALID and bool((dw == SENTINEL).all())
