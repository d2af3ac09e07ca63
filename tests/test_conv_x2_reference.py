"""Piece model of the two-piece fp16 convolution family -- conv1d_x2_kernel (SET_IMPL_F16X2), its all-phase ConvTranspose1d form
(set_conv_transpose1d_x2) and the fused ResBlock pair (set_resblock_pair_x2) -- written from the header comments of
csrc/conv_x2.hip / csrc/resblock_x2.hip and the comment above SetConv1dArgs (include/set_amd.h), not from the kernel bodies, on top
of conv_ref of tests/test_conv_reference.py; the case tables of the GPU sweep tests/test_gpu_x2conv_branches.py; and the CPU
checks of both.

The model: the weights are multiplied by 2^k (ops._x2_exponent) and split into a0 = fp16(w), a1 = fp16(w - a0); the prologue's
fp32 output is split the same way into b0, b1; the kernel forms a1 b0 + a0 b1 + a0 b0 (never a1 b1) in fp32, multiplies the
accumulator by 2^-k and runs the fp32 epilogue ((acc / s + bias) * alpha -> act) + res) * mask + prev, / out_div.

Exactness (what the GPU sweep's `exact` mode rests on).  Inputs on the two-piece grid  v = a + sign(a) b 2^-12,  a a small integer,
b in {0, 1}:  fp16(v) and fp16(v - fp16(v)) reproduce v exactly with a non-zero, normal low piece wherever b = 1 and no rounding tie
(also after a power-of-two leaky-ReLU slope / divisor and after the pack-time scale).  Every piece product is then a multiple of a
granule q, and if  sum |piece products| < 2^24 q  for an output, every partial sum in ANY order is an fp32 number: the kernel must
equal the float64 sum of the three products bit for bit.  The budget is asserted per case (test_exact_cases_meet_their_budget),
never assumed; per case the integer ranges (and, for the deepest reductions, a sparsity) are picked from LADDER so that it holds.
Two assumptions about the hardware go into `exact`, both checked by the first GPU run of the sweep (outcome: DESIGN.md, "two-piece
grid"):
  1. v_mfma_f32_32x32x16_f16 adds its 16 exact products and the fp32 accumulator without losing a bit when every partial result is
     representable in fp32;
  2. the fp32 -> fp16 conversions of split2_f16 / cx_f2h round to nearest even and keep fp16 subnormals (what torch's .half() does).
     The grid itself needs neither a tie rule nor subnormals; the intermediate of a ResBlock pair (an arbitrary 24-bit value that is
     split again) needs the tie rule.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_reference import ACTS, U, conv_bound, conv_ref, f32, gamma, ints, polyphase_calls, prologue, shifted, weight_view
from test_gpu_conv_branches import PARAMS, SENTINEL, _case, _embed
from test_split_operand_numerics import F16X2, gemm_split, split_f16x2

BUDGET_BITS = 24.0  # sum |piece products| / granule < 2^24 (assumption 1 held on the MI355X: not lowered)
LOW_SHARE = 0.15    # least share of non-zero low pieces among the in-view activations and among the weights of an exact case


def x2_exponent(w):
    """The power of two of a two-piece image: ops._x2_exponent of the WHOLE raw weight tensor (one definition)."""
    import set_amd  # noqa: F401
    from set_amd import ops
    return ops._x2_exponent(w)


def split2(v):
    """(hi, lo) of fp32 values: hi = fp16(v), lo = fp16(v - hi), round to nearest even, subnormals kept; float64 tensors."""
    v = v.float()
    hi = v.half().float()
    lo = (v - hi).half().float()
    return hi.double(), lo.double()


def lowbit(v):
    """Elementwise: the largest power of two that divides v (v a multiple of 2^-40 below 2^22), 0 where v == 0."""
    n = (v.double().abs() * 2.0 ** 40).round().long()
    return (n & -n).double() * 2.0 ** -40


def granule(v):
    lb = lowbit(v)
    return float(lb[lb > 0].min()) if bool((lb > 0).any()) else math.inf


GEOM = ("dil", "pad", "T_iter", "T_out", "out_stride", "out_off")


def conv_x2_ref(x, W, k, *, bias=None, res=None, mask=None, prev=None, pro="none", pro_param=0.0, **kw):
    """conv_ref's arguments (no in_chan_add: the kernel refuses it) plus the scale exponent k.  Returns conv_ref's dict with y, z, f
    from the three piece products, S = sum |piece products| / s + |bias|, and
      S3       sum |piece products| / s per output (0 where nothing is written)
      q        the granule of the piece products / s;  bits = log2(max S3 / q)
      dropped  sum a1 b1 / s per output (the product the kernel leaves out);  D3 = sum |a1| |b1| / s
      lo_x, lo_w   share of non-zero low pieces among the activations of the view / the weights
      amax     max |prologue output| (what the range flag sees)."""
    geom = {n: kw[n] for n in GEOM if n in kw}
    P = prologue(x, None, pro, pro_param).float()  # the prologue is fp32: one rounding of the exact product / quotient
    b0, b1 = split2(P)
    s = 2.0 ** k
    Ws = W.double() * s
    assert bool((Ws.float().double() == Ws).all())
    a0, a1 = split2(Ws)
    r = conv_ref(torch.cat([b0, b1, b0], 1), torch.cat([a1, a0, a0], 1) / s, bias=bias, res=res, mask=mask, prev=prev, **kw)
    wr = r["written"].double()
    r["S3"] = r["S"] * wr - (0.0 if bias is None else bias.double().abs()[None, :, None] * wr)
    r["dropped"] = conv_ref(b1, a1 / s, **geom)["y"]
    r["D3"] = conv_ref(b1.abs(), a1.abs() / s, **geom)["y"]
    ga0, ga1, gb0, gb1 = granule(a0), granule(a1), granule(b0), granule(b1)
    q = min(v for v in (ga1 * gb0, ga0 * gb1, ga0 * gb0) if math.isfinite(v)) / s if math.isfinite(ga0 * gb0) else math.inf
    r["q"] = q
    r["bits"] = math.log2(max(float(r["S3"].max()), 1e-300) / q) if math.isfinite(q) else -math.inf
    r["lo_x"], r["lo_w"] = float((b1 != 0).double().mean()), float((a1 != 0).double().mean())
    r["amax"] = float(P.abs().max())
    r["split_exact"] = bool((b0 + b1 == P.double()).all()) and bool((a0 + a1 == Ws).all())
    return r


def phase_rows(wt, u, p):
    """Rows (co, p) of the all-phase image of a ConvTranspose1d weight [Cin][Cout][k]: W[co][ci][j] = wt[ci][co][u j + p], 0 beyond k."""
    Cin, Cout, k = wt.shape
    J = (k + u - 1) // u
    W = torch.zeros(Cout, Cin, J, dtype=wt.dtype)
    for j in range(J):
        if u * j + p < k:
            W[:, :, j] = wt[:, :, u * j + p].t()
    return W


def conv_transpose_x2_ref(x, wt, bias, k_exp, u, P, *, pro="none", pro_param=0.0):
    """set_conv_transpose1d_x2: rows (co, p), taps u j + p (zero beyond k), sample t of row (co, p) is output n = t u + p - P,
    T_iter = T_in + J - 1.  Returns the whole [B][Cout][T_out] image of y, S, S3, dropped, D3, written, and q / bits / lo_* / amax."""
    B, Cin, T_in = x.shape
    _, Cout, k = wt.shape
    J = (k + u - 1) // u
    T_out = (T_in - 1) * u - 2 * P + k
    out = {n: torch.zeros(B, Cout, T_out, dtype=torch.float64) for n in ("y", "S", "S3", "dropped", "D3")}
    out["written"] = torch.zeros(B, Cout, T_out, dtype=torch.bool)
    qs, lo_w, exact = [], [], True
    for p in range(u):
        r = conv_x2_ref(x, phase_rows(wt, u, p), k_exp, bias=bias, pro=pro, pro_param=pro_param, dil=-1, pad=0, T_iter=T_in + J - 1,
                        T_out=T_out, out_stride=u, out_off=p - P)
        assert not bool((out["written"] & r["written"]).any())
        for n in ("y", "S", "S3", "dropped", "D3"):
            out[n] += r[n] * r["written"].double()
        out["written"] |= r["written"]
        qs.append(r["q"])
        lo_w.append(r["lo_w"])
        exact = exact and r["split_exact"]
    out.update(q=min(qs), lo_x=r["lo_x"], lo_w=sum(lo_w) / u * (u * J / k), amax=r["amax"], split_exact=exact)  # (share among the k real taps)
    out["bits"] = math.log2(max(float(out["S3"].max()), 1e-300) / out["q"]) if math.isfinite(out["q"]) else -math.inf
    return out


def resblock_pair_x2_ref(x, W1, b1, W2, b2, k1, k2, dil, slope, *, prev=None, accumulate=False, out_div=0.0):
    """set_resblock_pair_x2: conv 1 (K taps, dilation dil, "same") by the piece model on lrelu(x) for the frames [0, T) only, the fp32
    intermediate, leaky ReLU, ZERO outside [0, T) (conv 2 pads with zeros), split again, conv 2 (K taps, dilation 1) by the piece
    model, + x, (+ prev, / out_div).  Returns (r1, r2): the two conv_x2_ref dicts; r2["y"] is the result."""
    K = W1.shape[-1]
    h2 = (K - 1) // 2
    r1 = conv_x2_ref(x, W1, k1, bias=b1, pro="lrelu", pro_param=slope, dil=dil, pad=dil * h2)
    t = r1["y"].float()  # the kernel's intermediate is fp32 (exact cases: no rounding here, asserted by the budget of GEMM 1)
    r2 = conv_x2_ref(t, W2, k2, bias=b2, res=x, prev=prev, pro="lrelu", pro_param=slope, dil=1, pad=h2, accumulate=accumulate, out_div=out_div)
    return r1, r2


def epilogue_exact(r, *, res=None, mask=None, prev=None, alpha=1.0, accumulate=False, out_div=0.0):
    """True if every intermediate of the fp32 epilogue is an fp32 number for this (exact-mode) result: acc / s + bias, f + res, the sum
    with the previous output (power-of-two alpha, slopes and out_div change no bits)."""
    w = r["written"]
    steps = [r["z"] / f32(alpha)]
    v = r["f"] + (0.0 if res is None else res.double())
    steps.append(v)
    if mask is not None:
        v = v * mask.double()[:, None]
    if accumulate:
        v = v + prev.double()
        steps.append(v)
        if out_div:
            steps.append(v / f32(out_div))
    return all(bool((s_.float().double() == s_)[w].all()) for s_ in steps)


def conv_x2_bound(r, m, ones, Wsum, k, *, Cin, K, act="none", act_param=0.0, alpha=1.0, res=None, prev=None):
    """Per-element bar of the two-piece kernel against the TRUE float64 convolution r = conv_ref(x, W, ...), for Gaussian inputs.
    m = conv_x2_ref of the same call (its S3, D3: functions of the inputs alone), ones = conv_ref(x, |W| -> 1, same prologue and
    geometry)["S"] = sum |P(x)| over the receptive field, Wsum[co] = sum |W[co]|, k the scale exponent.  With u = 2^-24, s = 2^k, P the exact prologue output:
      * the prologue rounds once in fp32: P~ = P (1 + d), |d| <= u                                     -> u sum |W| |P|
      * a two-piece split keeps 22 bits, or stops at the fp16 subnormal floor (tests/test_split_operand_numerics.py:
        |v - hi - lo| <= max(2^-22 |v|, 2^-25)); for the weights that floor is 2^-25 / s (the scale keeps max |w s| in [8, 16), but a
        weight 2^7 below the largest still has a subnormal low piece); (W + eW)(P + eP) - W P, second order dropped into the factor
        1 + 2^-10                                                  -> (1 + 2^-10) (2^-21 sum |W| |P| + 2^-25 (sum |W| + sum |P| / s))
      * the product the kernel leaves out                                                              -> D3 = sum |a1| |b1| / s
      * fp32 accumulation of the 3 Cin_P K exact piece products (zero padding adds nothing) in ANY order, whatever the association
        inside an MFMA                                                                                 -> gamma(3 Cin_P K) S3
    all of which the activation amplifies by |alpha| Lip(act); the epilogue terms are conv_bound's with no products left:
    gamma(4) S |alpha| Lip(act) + 4 u (|y| + |res| + |prev|) (+ 64 u (|f| + |z|) for a transcendental activation).  No constant is
    fitted to GPU output."""
    CinP = -(-Cin // 32) * 32
    wr = r["written"].double()
    SWP = r["S"]  # sum |W| |P| + |bias| >= sum |W| |P|
    e_acc = U * SWP + (1 + 2.0 ** -10) * (2.0 ** -21 * SWP + 2.0 ** -25 * (Wsum.double()[None, :, None] * wr + ones * 2.0 ** -k)) + m["D3"] + \
        gamma(3 * CinP * K) * m["S3"]
    return e_acc * abs(f32(alpha)) * ACTS[act][1](f32(act_param)) + conv_bound(r, 0, act=act, act_param=act_param, alpha=alpha, res=res, prev=prev)


# ------------------------------------------------------------------------------------------------------------------------
# the two-piece grid and the operands of a case
# ------------------------------------------------------------------------------------------------------------------------
LADDER = ((3, 2, 1.0), (1, 2, 1.0), (1, 1, 1.0), (1, 1, 0.5))  # (|a| of x, |a| of w, density of x): the first rung whose budget holds


def grid(g, shape, amax, density=1.0):
    a = torch.randint(-amax, amax + 1, shape, generator=g).double()
    b = torch.randint(0, 2, shape, generator=g).double()
    v = a + a.sign() * b * 2.0 ** -12
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).double()
    return v.float()


def _seed(name, mode, rung=0):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 7 + (mode == "exact") + 1000003 * rung


X2 = ("f16x2",)


def _halo(c):
    return (c["K"] - 1) * abs(c["dil"])


def _nb(c):
    return 128 if c["Cout"] > 64 else 256


# Generic conv.  launch_conv_x2 by Cout: <= 32 -> <1, 4, 1, 2> (MB 32, NB 256), 33..64 -> <2, 2, 1, 4> (MB 64, NB 256), > 64 ->
# <4, 1, 1, 4> (MB 128, NB 128); staging passes npass = ceil((NB + halo) / 128) (the last one partial unless (NB + halo) % 128 == 0);
# nchunks = ceil(Cin / 32).  x_emb / emb / res_emb: (batch stride, channel stride, offset) as in tests/test_gpu_conv_branches.py
CONV = [
    # ---- Cout <= 32: 32 x 256 ----
    # T_iter 255 = NB - 1; halo 2: npass 3, the last partial (258 rows); one chunk; Cout 32 = MB
    _case("s32_T255_halo2", X2, 2, 32, 32, 3, 1, 255),
    # T_iter 256 = NB; K 1: halo 0, npass 2; Cout 20 % 32 != 0; Cin 33: two chunks, Cin % 32 == 1 (31 padded channels zeroed)
    _case("s32_T256_k1_ragged", X2, 1, 33, 20, 1, 1, 256, act="relu"),
    # T_iter 257 = NB + 1 (grid.x 2); K 9, dil 16: halo 128 exactly, npass 3 full; Cin 48: % 32 == 16 (second 16-channel group padded)
    _case("s32_T257_halo128_k9", X2, 1, 48, 32, 9, 16, 257, pro="lrelu"),
    # one tile, T_iter 100 < NB; Cout 7; Cin 49: % 32 == 17
    _case("s32_T100_cin49", X2, 2, 49, 7, 5, 2, 100, act="relu", res=True),
    # ---- Cout 33..64: 64 x 256 ----
    _case("s64_T511_halo18", X2, 1, 64, 64, 7, 3, 511, pro="lrelu", res=True),               # T_iter 2 NB - 1; two chunks; Cout 64 = MB
    _case("s64_T512_k1_five_chunks", X2, 1, 160, 33, 1, 1, 512, mask=True),                  # T_iter 2 NB; halo 0; five chunks; Cout 33
    _case("s64_T513_halo128_k2", X2, 1, 32, 48, 2, 128, 513),                                # T_iter 2 NB + 1; K 2, dil 128: halo 128
    _case("s64_T70_grad_form", X2, 2, 17, 64, 3, -1, 70, pad=-1, wview="transposed"),        # one tile; dil < 0; Cin 17 -> one chunk
    # ---- Cout > 64: 128 x 128 ----
    _case("s128_T127_cout65", X2, 1, 32, 65, 3, 1, 127),                                     # T_iter NB - 1; Cout 65: rows 64..95 ragged
    # Cout 130: CoutP 160, grid.y 2; the second block's waves 1..3 (rows 160..255) lie wholly past CoutP: a_off clamps rb to 4
    _case("s128_T128_rows_past_CoutP", X2, 2, 64, 130, 5, 1, 128, act="lrelu"),
    _case("s128_T129_halo128_div", X2, 1, 80, 160, 9, 16, 129, pro="div"),                   # T_iter NB + 1; halo 128: npass 2 full; three chunks
    _case("s128_T100_k1", X2, 1, 32, 128, 1, 1, 100),                                        # one tile; halo 0: npass 1
    # ---- operand forms ----
    _case("form_unpadded", X2, 2, 32, 64, 5, 1, 100, pad=0, T_out=96),                       # T_out != T_in
    _case("form_overpadded_dilated", X2, 1, 32, 96, 3, 8, 92, pad=10, T_out=96),
    _case("form_gelu", X2, 2, 32, 64, 3, 1, 130, act="gelu", alpha=True, res=True, mask=True),
    _case("form_tanh", X2, 1, 64, 32, 7, 1, 300, act="tanh", pro="lrelu"),
    _case("form_no_bias", X2, 1, 32, 96, 3, 1, 128, bias=False),
    _case("form_res_strides", X2, 2, 32, 96, 3, 1, 128, res=True, res_emb=(200 * 140, 140, 7 * 140 + 4), act="relu"),
    _case("form_out_channel_slice", X2, 2, 48, 64, 3, 1, 96, emb=(3 * 64 * 96, 96, 64 * 96), res=True, res_emb=(64 * 99, 99, 1)),
    _case("form_accumulate", X2, 2, 32, 64, 3, 1, 200, accumulate=True, pro="lrelu", res=True),
    _case("form_accumulate_out_div", X2, 2, 32, 40, 3, 1, 200, accumulate=True, out_div=True, pro="lrelu", res=True, mask=True),
    _case("form_alpha_lrelu_div", X2, 2, 32, 128, 3, 1, 128, alpha=True, act="lrelu", pro="div"),
    # B 3, in / out / res batch strides that are not C T, every view at a 4-byte offset; x sits in a buffer whose surroundings hold 5e4
    _case("form_B3_all_strided", X2, 3, 40, 96, 3, 1, 100, x_emb=(40 * 111 + 3, 111, 5), emb=(96 * 107 + 5, 107, 3), res=True,
          res_emb=(96 * 103 + 1, 103, 1), pro="lrelu"),
    _case("form_in_channel_slice", X2, 2, 40, 33, 5, 2, 100, x_emb=(3 * 40 * 100, 100, 40 * 100), mask=True),
    # weight views through ConvWeight(..., base, sco, sci, stap)
    _case("view_transposed_k5", X2, 2, 48, 40, 5, -2, 90, pad=-4, wview="transposed", res=True),
    _case("view_phase_k16_u8_p5", X2, 1, 64, 32, 2, -1, 64, pad=0, T_iter=65, T_out=512, out_stride=8, out_off=1, wview=("phase", 16, 8, 5)),
    # ---- HiFi-GAN V1 shapes at a short T ----
    _case("v1_conv_pre_80to512_k7", X2, 1, 80, 512, 7, 1, 200),
]
CONV += [_case("v1_resblock_C%d_k%d_d%d" % (C_, k_, d_), X2, 1, C_, C_, k_, d_, 200 + C_ // 8, pro="lrelu", res=(k_ == 7), accumulate=(k_ == 11),
               out_div=(k_ == 11 and C_ == 64)) for C_ in (256, 128, 64, 32) for k_, d_ in ((3, 1), (7, 3), (11, 5))]
# the polyphase calls of one ConvTranspose1d (128 -> 64, k 4, u 2, P 1: the third V1 upsampler; and k 7, u 3, P 2) on impl="f16x2",
# which _pick_impl hands out inside split_convs() (the `bf16 out_stride 2` row of test_conv_reference.py): out_stride u, every out_off
POLY = ((128, 64, 4, 2, 1, 100), (32, 40, 7, 3, 2, 70))
for _Cin, _Cout, _k, _u, _P, _T in POLY:
    for _p_, _J, _kw in polyphase_calls(_T, _k, _u, _P):
        CONV.append(_case("phase_%dto%d_k%d_u%d_p%d" % (_Cin, _Cout, _k, _u, _p_), X2, 2, _Cin, _Cout, _J, _kw["dil"], _T, pro="lrelu",
                          wview=("phase", _k, _u, _p_), **{k_: v_ for k_, v_ in _kw.items() if k_ != "dil"}))

# All-phase transposed conv: rows = u Cout; <= 64 -> <2, 2, 1, 4, true> (NB 256), > 64 -> <4, 1, 1, 4, true> (NB 128); T_iter = T_in + J - 1;
# store form: 16-byte if u % 4 == 0 && P % 4 == 0 && T_out % 4 == 0, else the 8-byte form if u == 2, else per element
#   name, B, Cin, Cout, k, u, P, T_in, bias, pro
CONVT = [
    ("u8_vec_rows128_T127", 2, 32, 16, 16, 8, 4, 126, True, "lrelu"),          # 16-byte form; rows 128 > 64; T_iter 127 = NB - 1
    ("u4_vec_rows32_T256", 1, 64, 8, 8, 4, 4, 255, True, "none"),              # 16-byte form; rows 32; T_out 4 T - 4; T_iter 256 = NB
    ("u4_P2_refused_by_P", 1, 32, 20, 8, 4, 2, 128, True, "lrelu"),            # P % 4 != 0 -> per element; rows 80 (% 32 != 0); T_iter 129
    ("u4_k10_refused_by_T_out", 2, 64, 8, 10, 4, 4, 100, True, "none"),        # T_out 4 T - 2; J 3 with zero taps (k % u != 0)
    ("u8_k18_refused_by_T_out", 1, 32, 4, 18, 8, 4, 70, True, "none"),         # T_out 8 T + 2; rows 32
    ("u2_P1_edges_T128", 1, 128, 64, 4, 2, 1, 127, True, "lrelu"),             # 8-byte form, P odd: edge lanes at n = -1 and T_out; T_iter 128
    ("u2_P2_even_T257", 1, 32, 16, 4, 2, 2, 256, True, "none"),                # P even: the frames at the ends lie wholly outside; T_iter 257
    ("u2_k2_no_edge", 2, 32, 40, 2, 2, 0, 90, False, "lrelu"),                 # k 2, P 0: J 1, every pair inside; rows 80; no bias
    ("u3_k7_per_element_T255", 1, 96, 11, 7, 3, 2, 253, True, "lrelu"),        # rows 33 (% 32 != 0, <= 64); zero taps; T_iter 255 = NB - 1
    ("u1_k3", 3, 32, 48, 3, 1, 1, 100, True, "none"),                          # u 1: an ordinary "same" conv in transposed form; B 3
    ("u5_k5_k_equals_u", 1, 64, 13, 5, 5, 0, 80, False, "none"),               # k = u: J 1; rows 65 > 64
    # the four V1 upsamplers (hifigan.py:114-115) at a short T
    ("v1_ups0_512to256", 1, 512, 256, 16, 8, 4, 70, True, "lrelu"),
    ("v1_ups1_256to128", 2, 256, 128, 16, 8, 4, 70, True, "lrelu"),
    ("v1_ups2_128to64", 1, 128, 64, 4, 2, 1, 70, True, "lrelu"),
    ("v1_ups3_64to32", 2, 64, 32, 4, 2, 1, 70, True, "lrelu"),
]

# ResBlock pair.  launch_pair by C: <= 32 -> NB 256, 33..64 -> NB 256, 65..128 -> NB 128, 129..256 (K <= 5) -> NB 64; NV = NB - (K - 1)
# stored columns per block.  x_emb / emb: strided x / out through the raw ABI
#   name, B, C, K, dil, T, accumulate, out_div, x_emb, emb
PAIR = [
    ("c16_T64", 2, 16, 3, 1, 64, False, False, None, None),                          # C 16 (the least), T 64 (the least) < NV 254
    ("c32_T253", 1, 32, 3, 1, 253, False, False, None, None),                        # T % NV = NV - 1
    ("c24_k5_T252", 1, 24, 5, 2, 252, True, False, None, None),                      # C % 32 != 0; NV 252: T % NV = 0
    ("c64_k7_T251", 1, 64, 7, 3, 251, True, False, None, None),                      # 33..64; NV 250: T % NV = 1
    ("c48_halo128", 1, 48, 3, 64, 300, False, False, None, None),                    # dil (K - 1) = 128 (the most); C % 32 != 0
    ("c128_k15_T228", 1, 128, 15, 1, 228, True, True, None, None),                   # 65..128; K 15 (the most): NV 114, T = 2 NV
    ("c100_T125", 2, 100, 3, 5, 125, False, False, None, None),                      # NV 126: T = NV - 1 < NV; C % 32 != 0
    ("c96_k5_T125", 1, 96, 5, 1, 125, False, False, None, None),                     # NV 124: T % NV = 1
    ("c256_k3_T124", 3, 256, 3, 1, 124, True, True, None, None),                     # 129..256; NV 62: T = 2 NV; B 3
    ("c160_k5_T121", 1, 160, 5, 1, 121, False, False, None, None),                   # K 5, NV 60: T % NV = 1; C % 32 != 0
    ("c129_T185", 1, 129, 3, 2, 185, True, False, None, None),                       # C 129: 31 padded rows; NV 62: T % NV = NV - 1
    ("c64_B3_strided", 3, 64, 3, 1, 200, True, True, (64 * 211 + 3, 211, 5), (64 * 207 + 5, 207, 3)),
    ("c40_strided_out", 2, 40, 5, 1, 90, False, False, (3 * 40 * 90, 90, 40 * 90), (40 * 97, 97, 1)),
]
# the twelve pairs of a V1 generator the fused kernel takes (ResBlock1: k in 3 / 7 / 11, dilations 1 / 3 / 5; 256 channels: 3 taps only)
PAIR += [("v1_C%d_k%d_d%d" % (C_, k_, d_), 1, C_, k_, d_, 150, d_ == 5, d_ == 5 and k_ == 3, None, None)
         for C_, kd in ((256, ((3, 1), (3, 3), (3, 5))), (128, ((3, 1), (7, 3), (11, 5))), (64, ((3, 3), (7, 5), (11, 1))),
                        (32, ((3, 5), (7, 1), (11, 3)))) for k_, d_ in kd]


def _weights(c, g, mode, rung):
    """wstore, waddr (the ConvWeight addressing) and the [Cout][Cin][K] view of a conv case."""
    Cin, Cout, K, wv = c["Cin"], c["Cout"], c["K"], c["wview"]
    gen = (lambda shape: grid(g, shape, LADDER[rung][1])) if mode == "exact" else (lambda shape: torch.randn(shape, generator=g) * (Cin * K) ** -0.5)
    if wv == "plain":
        ws, addr = gen((Cout, Cin, K)), dict(base=0, sco=Cin * K, sci=K, stap=1)
    elif wv == "transposed":
        ws, addr = gen((Cin, Cout, K)), dict(base=0, sco=K, sci=Cout * K, stap=1)
    else:
        _, k, u, p = wv
        ws, addr = gen((Cin, Cout, k)), dict(base=p, sco=k, sci=Cout * k, stap=u)
    return ws, addr, weight_view(ws, Cout, Cin, K, **addr)


def make_conv(c, mode, rung=None):
    """CPU operands of a conv case, the model's image of the WHOLE out buffer and the bar of every buffer element.  exact: the first rung
    of LADDER whose budget holds (o["rung"]; an assertion if none does)."""
    if mode == "exact" and rung is None:
        for rung in range(len(LADDER)):
            o = make_conv(c, mode, rung)
            if o["ok"]:
                return o
        raise AssertionError("%s: no rung of LADDER meets the budget (last: %.2f bits)" % (c["name"], o["m"]["bits"]))
    rung = rung or 0
    pv = PARAMS[mode]
    exact = mode == "exact"
    g = torch.Generator().manual_seed(_seed(c["name"], mode, rung))
    B, Cin, Cout = c["B"], c["Cin"], c["Cout"]
    o = dict(c)
    o["rung"] = rung
    o["x"] = grid(g, (B, Cin, c["T_in"]), LADDER[rung][0], LADDER[rung][2]) if exact else torch.randn(B, Cin, c["T_in"], generator=g)
    o["wstore"], o["waddr"], W = _weights(c, g, mode, rung)
    rnd = (lambda shape, lo, hi, sc: ints(g, shape, lo, hi)) if exact else (lambda shape, lo, hi, sc: torch.randn(shape, generator=g) * sc)
    o["bias_t"] = rnd((Cout,), -4, 4, 0.1) if c["bias"] else None
    o["mask_t"] = (torch.rand(B, c["T_out"], generator=g) > 0.3).float() if c["mask"] else None
    o["add_t"] = None
    shape = (B, Cout, c["T_out"])
    fill = "ints" if exact else "randn"
    o["res_buf"], o["res_view"] = _embed(shape, c["res_emb"], fill, g) if c["res"] else (None, None)
    o["out_buf"], o["out_view"] = _embed(shape, c["emb"], fill if c["accumulate"] else SENTINEL, g)
    kw = dict(dil=c["dil"], pad=c["pad"], T_iter=c["T_iter"], T_out=c["T_out"], out_stride=c["out_stride"], out_off=c["out_off"],
              pro=c["pro"], pro_param={"lrelu": pv["pro_lrelu"], "div": pv["pro_div"], "none": 0.0}[c["pro"]], act=c["act"],
              act_param=pv["act_lrelu"] if c["act"] == "lrelu" else 0.0, alpha=pv["alpha"] if c["alpha"] else 1.0,
              accumulate=c["accumulate"], out_div=pv["out_div"] if c["out_div"] else 0.0)
    o["kw"] = kw
    res = o["res_view"](o["res_buf"]) if c["res"] else None
    prev = o["out_view"](o["out_buf"]).clone()
    o["k"] = x2_exponent(o["wstore"])
    m = conv_x2_ref(o["x"], W, o["k"], bias=o["bias_t"], res=res, mask=o["mask_t"], prev=prev, **kw)
    o["m"] = m
    want = o["out_buf"].double().clone()
    bar = torch.zeros_like(want)
    if exact:
        o["ok"] = m["split_exact"] and m["bits"] < BUDGET_BITS and \
            epilogue_exact(m, res=res, mask=o["mask_t"], prev=prev, alpha=kw["alpha"], accumulate=c["accumulate"], out_div=kw["out_div"])
        o["out_view"](want).copy_(m["y"])
        o["r"] = m
    else:
        r = conv_ref(o["x"], W, bias=o["bias_t"], res=res, mask=o["mask_t"], prev=prev, **kw)
        geom = {n: kw[n] for n in GEOM}
        ones = conv_ref(o["x"], torch.ones_like(W), pro=kw["pro"], pro_param=kw["pro_param"], **geom)["S"]
        b = conv_x2_bound(r, m, ones, W.double().abs().sum((1, 2)), o["k"], Cin=Cin, K=c["K"], act=c["act"], act_param=kw["act_param"], alpha=kw["alpha"], res=res,
                          prev=prev if c["accumulate"] else None)
        o["out_view"](want).copy_(r["y"])
        o["out_view"](bar).copy_(b * r["written"].double())
        o["r"], o["W"] = r, W
    o["want"], o["bar"], o["written"] = want, bar, int(m["written"].sum())
    return o


def make_convt(case, mode, rung=None):
    name, B, Cin, Cout, k, u, P, T_in, with_bias, pro = case
    if mode == "exact" and rung is None:
        for rung in range(len(LADDER)):
            o = make_convt(case, mode, rung)
            if o["ok"]:
                return o
        raise AssertionError("%s: no rung of LADDER meets the budget (last: %.2f bits)" % (name, o["m"]["bits"]))
    rung = rung or 0
    exact = mode == "exact"
    g = torch.Generator().manual_seed(_seed(name, mode, rung))
    T_out = (T_in - 1) * u - 2 * P + k
    o = dict(name=name, B=B, Cin=Cin, Cout=Cout, k=k, u=u, P=P, T_in=T_in, T_out=T_out, pro=pro, rung=rung)
    o["pro_param"] = PARAMS[mode]["pro_lrelu"] if pro == "lrelu" else 0.0
    if exact:
        o["x"], o["wt"] = grid(g, (B, Cin, T_in), LADDER[rung][0], LADDER[rung][2]), grid(g, (Cin, Cout, k), LADDER[rung][1])
        o["bias_t"] = ints(g, (Cout,), -4, 4) if with_bias else None
    else:
        o["x"], o["wt"] = torch.randn(B, Cin, T_in, generator=g), torch.randn(Cin, Cout, k, generator=g) * (Cin * k / u) ** -0.5
        o["bias_t"] = torch.randn(Cout, generator=g) * 0.1 if with_bias else None
    o["k_exp"] = x2_exponent(o["wt"])
    m = conv_transpose_x2_ref(o["x"], o["wt"], o["bias_t"], o["k_exp"], u, P, pro=pro, pro_param=o["pro_param"])
    assert bool(m["written"].all())  # every sample of a ConvTranspose1d output belongs to exactly one (frame, phase)
    o["m"] = m
    n = B * Cout * T_out
    want = torch.full((n + 64,), SENTINEL, dtype=torch.float64)  # the contiguous out the entry point takes, and a guard behind it
    bar = torch.zeros_like(want)
    if exact:
        o["ok"] = m["split_exact"] and m["bits"] < BUDGET_BITS and bool(((m["y"]).float().double() == m["y"]).all())
        want[:n] = m["y"].reshape(-1)
    else:
        yd = F.conv_transpose1d(prologue(o["x"], None, pro, o["pro_param"]), o["wt"].double(), None if o["bias_t"] is None else o["bias_t"].double(),
                                stride=u, padding=P)
        J = (k + u - 1) // u
        CinP = -(-Cin // 32) * 32
        SWP = F.conv_transpose1d(prologue(o["x"], None, pro, o["pro_param"]).abs(), o["wt"].double().abs(), stride=u, padding=P)
        ones = F.conv_transpose1d(prologue(o["x"], None, pro, o["pro_param"]).abs(), torch.ones_like(o["wt"]).double(), stride=u, padding=P)[:, :1]
        Wsum = o["wt"].double().abs().sum((0, 2))[None, :, None]
        bias_abs = 0.0 if o["bias_t"] is None else o["bias_t"].double().abs()[None, :, None]
        # conv_x2_bound, term by term, for the epilogue acc / s + bias (one rounding: u (|y| + ...) <= 4 u |y| + gamma(4) S)
        b = U * SWP + (1 + 2.0 ** -10) * (2.0 ** -21 * SWP + 2.0 ** -25 * (Wsum + ones * 2.0 ** -o["k_exp"])) + m["D3"] + gamma(3 * CinP * J) * m["S3"] + \
            gamma(4) * (SWP + bias_abs) + 4 * U * yd.abs()
        want[:n] = yd.reshape(-1)
        bar[:n] = b.reshape(-1)
        o["yd"] = yd
    o["want"], o["bar"] = want, bar
    return o


def _selection_weight(g, C, K, nnz):
    """A one-piece W2 [C][C][K] with nnz entries +-1 per row at distinct channels and random taps, and its sparse form."""
    ci = torch.stack([torch.randperm(C, generator=g)[:nnz] for _ in range(C)])
    tap = torch.randint(0, K, (C, nnz), generator=g)
    sgn = torch.randint(0, 2, (C, nnz), generator=g) * 2 - 1
    W = torch.zeros(C, C, K)
    W[torch.arange(C)[:, None], ci, tap] = sgn.float()
    return W, (ci, tap)


def _gemm2_bits(t_act, sparse, K, S3):
    """Budget of a pair's second GEMM in exact mode, per output: sum |piece products| over the SMALLEST low bit among the products that
    meet in that output (W2 holds +-1 only, so a product is +- a piece of the intermediate and a1 = 0)."""
    b0, b1 = split2(t_act)
    lb = torch.where(b1 != 0, lowbit(b1), lowbit(b0))
    inv = torch.where(lb > 0, 1.0 / lb.clamp(min=1e-300), torch.zeros_like(lb))
    ci, tap = sparse
    B, C, T = t_act.shape
    h2 = (K - 1) // 2
    worst = torch.zeros(B, C, T, dtype=torch.float64)
    for kk in range(K):
        sh = shifted(inv, kk - h2, T)
        for j in range(ci.shape[1]):
            rows = (tap[:, j] == kk).nonzero().flatten()
            if rows.numel():
                worst[:, rows] = torch.maximum(worst[:, rows], sh[:, ci[rows, j]])
    ratio = float((S3 * worst).max())
    return math.log2(max(ratio, 1e-300))


def make_pair(case, mode, rung=None):
    """exact: GEMM 1 runs on the two-piece grid (budget asserted like a conv's); its output is an arbitrary fp32 value of fine granule, so
    GEMM 2 gets a one-piece selection weight (+-1, two entries per row) whose per-output budget _gemm2_bits asserts -- every tap and
    channel offset of GEMM 2 still moves a value, and the dense GEMM 2 is carried by the bit-identity with two conv launches, whose
    kernel the conv sweep pins on the piece model.  bounded: Gaussian, dense, as tests/test_gpu_x2conv.py."""
    name, B, C, K, dil, T, accumulate, out_div, x_emb, emb = case
    if mode == "exact" and rung is None:
        for rung in range(len(LADDER)):
            o = make_pair(case, mode, rung)
            if o["ok"]:
                return o
        raise AssertionError("%s: no rung of LADDER meets the budget (last: %.2f / %.2f bits)" % (name, o["r1"]["bits"], o["bits2"]))
    rung = rung or 0
    exact = mode == "exact"
    pv = PARAMS[mode]
    g = torch.Generator().manual_seed(_seed(name, mode, rung))
    o = dict(name=name, B=B, C=C, K=K, dil=dil, T=T, accumulate=accumulate, out_div=pv["out_div"] if out_div else 0.0, slope=pv["pro_lrelu"],
             x_emb=x_emb, emb=emb, rung=rung)
    if exact:
        o["x"], o["w1"] = grid(g, (B, C, T), LADDER[rung][0], LADDER[rung][2]), grid(g, (C, C, K), LADDER[rung][1])
        o["w2"], sparse = _selection_weight(g, C, K, 2)
        o["b1"], o["b2"] = ints(g, (C,), -4, 4), ints(g, (C,), -4, 4)
    else:
        o["x"] = torch.randn(B, C, T, generator=g)
        o["w1"], o["w2"] = (torch.randn(C, C, K, generator=g) * (C * K) ** -0.5 for _ in range(2))
        o["b1"], o["b2"] = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    o["out_buf"], o["out_view"] = _embed((B, C, T), emb, ("ints" if exact else "randn") if accumulate else SENTINEL, g)
    prev = o["out_view"](o["out_buf"]).clone()
    o["k1"], o["k2"] = x2_exponent(o["w1"]), x2_exponent(o["w2"])
    want = o["out_buf"].double().clone()
    if exact:
        r1, r2 = resblock_pair_x2_ref(o["x"], o["w1"], o["b1"], o["w2"], o["b2"], o["k1"], o["k2"], dil, o["slope"], prev=prev,
                                      accumulate=accumulate, out_div=o["out_div"])
        t_act = prologue(r1["y"].float(), None, "lrelu", o["slope"]).float()
        o["bits2"] = _gemm2_bits(t_act, sparse, K, r2["S3"])
        o["ok"] = r1["split_exact"] and r1["bits"] < BUDGET_BITS and epilogue_exact(r1) and o["bits2"] < BUDGET_BITS and \
            epilogue_exact(r2, res=o["x"], prev=prev, accumulate=accumulate, out_div=o["out_div"])
        o["r1"], o["r2"] = r1, r2
        o["out_view"](want).copy_(r2["y"])
    else:
        xd = o["x"].double()
        td = F.conv1d(F.leaky_relu(xd, f32(o["slope"])), o["w1"].double(), o["b1"].double(), dilation=dil, padding=dil * (K - 1) // 2)
        yd = F.conv1d(F.leaky_relu(td, f32(o["slope"])), o["w2"].double(), o["b2"].double(), padding=(K - 1) // 2) + xd
        if accumulate:
            yd = yd + prev.double()
        if o["out_div"]:
            yd = yd / f32(o["out_div"])
        o["out_view"](want).copy_(yd)
        o["yd"] = yd
    o["want"] = want
    return o


# ------------------------------------------------------------------------------------------------------------------------
# the piece model against conv_ref and against torch in float64
# ------------------------------------------------------------------------------------------------------------------------
SMALL = [(2, 6, 4, 3, 1, 1, 33), (1, 4, 9, 5, 2, 4, 40), (1, 7, 3, 9, 1, 0, 30), (1, 3, 4, 11, 5, 25, 64), (2, 5, 7, 1, 1, 0, 19)]


@pytest.mark.parametrize("case", SMALL)
def test_piece_model_equals_conv_ref_on_integers_and_misses_it_by_the_dropped_product_on_the_grid(case):
    B, Cin, Cout, K, dil, pad, T = case
    g = torch.Generator().manual_seed(sum(case))
    kw = dict(dil=dil, pad=pad, pro="lrelu", pro_param=0.25, act="lrelu", act_param=0.125, alpha=0.5)
    xi, Wi, bi = ints(g, (B, Cin, T), -3, 3), ints(g, (Cout, Cin, K), -2, 2), ints(g, (Cout,), -4, 4)
    m, r = conv_x2_ref(xi, Wi, x2_exponent(Wi), bias=bi, **kw), conv_ref(xi, Wi, bias=bi, **kw)
    assert torch.equal(m["y"], r["y"]) and torch.equal(m["written"], r["written"]) and m["lo_x"] == 0.0 and m["lo_w"] == 0.0
    assert float(m["dropped"].abs().max()) == 0.0
    xg, Wg = grid(g, (B, Cin, T), 3), grid(g, (Cout, Cin, K), 2)
    m = conv_x2_ref(xg, Wg, x2_exponent(Wg), dil=dil, pad=pad, pro="lrelu", pro_param=0.25)
    r = conv_ref(xg, Wg, dil=dil, pad=pad, pro="lrelu", pro_param=0.25)
    assert m["split_exact"] and m["lo_x"] > 0.3 and m["lo_w"] > 0.3
    assert torch.equal(m["y"] + m["dropped"], r["y"]) and float(m["dropped"].abs().max()) > 0.0  # exactly the a1 b1 product, and it is there
    assert bool((m["D3"] >= m["dropped"].abs()).all()) and float(m["D3"].max()) < 2.0 ** -20 * float(r["S"].max())
    assert m["amax"] == float(prologue(xg, None, "lrelu", 0.25).abs().max())


@pytest.mark.parametrize("case", SMALL)
def test_piece_model_follows_torch_conv1d_in_float64_on_the_grid(case):
    B, Cin, Cout, K, dil, pad, T = case
    g = torch.Generator().manual_seed(sum(case) + 3)
    x, W, b = grid(g, (B, Cin, T), 3), grid(g, (Cout, Cin, K), 2), ints(g, (Cout,), -4, 4)
    m = conv_x2_ref(x, W, x2_exponent(W), bias=b, dil=dil, pad=pad, pro="div", pro_param=2.0)
    want = F.conv1d(F.pad(x.double() / 2.0, (pad, pad)), W.double(), b.double(), dilation=dil)
    assert torch.equal(m["y"] + m["dropped"], want)


@pytest.mark.parametrize("cfg", [(2, 6, 5, 8, 4, 2, 13), (1, 4, 3, 4, 2, 1, 9), (1, 3, 2, 16, 8, 4, 7), (2, 5, 4, 7, 3, 2, 10), (1, 2, 3, 8, 8, 0, 5),
                                 (1, 3, 2, 3, 1, 1, 9), (1, 4, 3, 10, 4, 4, 6)])
def test_transposed_piece_model_follows_torch_conv_transpose1d(cfg):
    B, Cin, Cout, k, u, P, T = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x, wt, b = grid(g, (B, Cin, T), 3), grid(g, (Cin, Cout, k), 2), ints(g, (Cout,), -4, 4)
    m = conv_transpose_x2_ref(x, wt, b, x2_exponent(wt), u, P, pro="lrelu", pro_param=0.25)
    want = F.conv_transpose1d(F.leaky_relu(x.double(), 0.25), wt.double(), b.double(), stride=u, padding=P)
    assert bool(m["written"].all()) and m["y"].shape == want.shape and m["split_exact"]
    assert torch.equal(m["y"] + m["dropped"], want)
    # the rows of the image are the polyphase branches ops.conv_transpose1d issues, padded with zero taps
    for p, J, _ in polyphase_calls(T, k, u, P):
        assert torch.equal(phase_rows(wt, u, p)[:, :, :J], weight_view(wt, Cout, Cin, J, base=p, sco=k, sci=Cout * k, stap=u))
        assert float(phase_rows(wt, u, p)[:, :, J:].abs().sum()) == 0.0


@pytest.mark.parametrize("cfg", [(2, 6, 3, 1, 40), (1, 5, 5, 2, 33), (1, 4, 7, 3, 64)])
def test_pair_model_follows_the_two_conv_composition(cfg):
    B, C, K, dil, T = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x, W1, b1, b2 = ints(g, (B, C, T), -3, 3), ints(g, (C, C, K), -2, 2), ints(g, (C,), -4, 4), ints(g, (C,), -4, 4)
    W2, _ = _selection_weight(g, C, K, 2)
    prev = ints(g, (B, C, T), -4, 4)
    r1, r2 = resblock_pair_x2_ref(x, W1, b1, W2, b2, x2_exponent(W1), x2_exponent(W2), dil, 0.25, prev=prev, accumulate=True, out_div=4.0)
    td = F.conv1d(F.leaky_relu(x.double(), 0.25), W1.double(), b1.double(), dilation=dil, padding=dil * (K - 1) // 2)
    yd = (F.conv1d(F.leaky_relu(td, 0.25), W2.double(), b2.double(), padding=(K - 1) // 2) + x.double() + prev.double()) / 4.0
    assert torch.equal(r2["y"], yd)  # integers: one piece everywhere, nothing dropped, nothing rounded
    # Gaussian: the model keeps 22 bits per operand; conv 1 evaluated OUTSIDE [0, T) would feed conv 2's edge taps (it must not)
    x, W1, W2 = torch.randn(B, C, T, generator=g), torch.randn(C, C, K, generator=g) * 0.3, torch.randn(C, C, K, generator=g) * 0.3
    r1, r2 = resblock_pair_x2_ref(x, W1, b1, W2, b2, x2_exponent(W1), x2_exponent(W2), dil, 0.1)
    td = F.conv1d(F.leaky_relu(x.double(), f32(0.1)), W1.double(), b1.double(), dilation=dil, padding=dil * (K - 1) // 2)
    yd = F.conv1d(F.leaky_relu(td, f32(0.1)), W2.double(), b2.double(), padding=(K - 1) // 2) + x.double()
    assert float((r2["y"] - yd).abs().max()) < 1e-5 * float(yd.abs().max())
    assert r1["y"].shape[-1] == T and float((r1["y"] - td).abs().max()) < 1e-5 * float(td.abs().max())


# ------------------------------------------------------------------------------------------------------------------------
# every exact case of the sweep: pieces exact, budget, low-piece shares
# ------------------------------------------------------------------------------------------------------------------------
def _exact(c):
    return "exact" in c["modes"]


@pytest.mark.parametrize("c", [c for c in CONV if _exact(c)], ids=[c["name"] for c in CONV if _exact(c)])
def test_exact_conv_cases_meet_their_budget(c):
    o = make_conv(c, "exact")
    m = o["m"]
    print("%s: rung %s, scale 2^%d, bits needed %.2f, low pieces non-zero x %.2f / w %.2f, dropped / max|y| %.1e" % (
        c["name"], LADDER[o["rung"]], o["k"], m["bits"], m["lo_x"], m["lo_w"], float(m["dropped"].abs().max()) / float(m["y"].abs().max())))
    assert o["ok"] and m["split_exact"] and m["bits"] < BUDGET_BITS
    assert m["lo_x"] >= LOW_SHARE and m["lo_w"] >= LOW_SHARE
    assert m["amax"] < 32768.0 and 0 < o["written"] <= c["B"] * c["Cout"] * c["T_out"]


@pytest.mark.parametrize("case", CONVT, ids=[c[0] for c in CONVT])
def test_exact_transposed_cases_meet_their_budget(case):
    o = make_convt(case, "exact")
    m = o["m"]
    print("%s: rung %s, scale 2^%d, bits needed %.2f, low pieces non-zero x %.2f / w %.2f" % (case[0], LADDER[o["rung"]], o["k_exp"], m["bits"],
                                                                                           m["lo_x"], m["lo_w"]))
    assert o["ok"] and m["bits"] < BUDGET_BITS and m["lo_x"] >= LOW_SHARE and m["lo_w"] >= LOW_SHARE and m["amax"] < 32768.0


@pytest.mark.parametrize("case", PAIR, ids=[c[0] for c in PAIR])
def test_exact_pair_cases_meet_both_budgets(case):
    """(GEMM 2 is exempt from the low-piece floor: its activations are the split intermediate, its weights one piece by design.)"""
    o = make_pair(case, "exact")
    r1, r2 = o["r1"], o["r2"]
    print("%s: rung %s, bits needed GEMM 1 %.2f / GEMM 2 %.2f, low pieces non-zero x %.2f / w1 %.2f / intermediate %.2f" % (
        case[0], LADDER[o["rung"]], r1["bits"], o["bits2"], r1["lo_x"], r1["lo_w"], r2["lo_x"]))
    assert o["ok"] and r1["bits"] < BUDGET_BITS and o["bits2"] < BUDGET_BITS
    assert r1["lo_x"] >= LOW_SHARE and r1["lo_w"] >= LOW_SHARE and r2["lo_x"] >= LOW_SHARE
    assert max(r1["amax"], r2["amax"]) < 32768.0


# ------------------------------------------------------------------------------------------------------------------------
# bounded cases: an emulation of the kernel's order on the sweep's own Gaussian inputs stays inside conv_x2_bound
# ------------------------------------------------------------------------------------------------------------------------
EMULATED = [c for c in CONV if c["out_stride"] == 1 and c["Cout"] * c["Cin"] * c["K"] * c["B"] * c["T_iter"] <= 6e8]


@pytest.mark.parametrize("c", EMULATED, ids=[c["name"] for c in EMULATED])
def test_emulated_kernel_order_stays_inside_the_bound(c):
    """gemm_split of tests/test_split_operand_numerics.py (pieces exact, 16 products per step, small terms first, fp32 accumulator) in the
    kernel's k order (32-channel chunk, tap, 16-channel half), then the epilogue of conv_ref: the reference alone meets the bar.  Run on
    the stride-1 cases of at most 6e8 multiply-adds (all but the widest V1 shapes)."""
    o = make_conv(c, "bounded")
    kw, W, x = o["kw"], o["W"], o["x"]
    B, Cin, Cout, K, T_iter = c["B"], c["Cin"], c["Cout"], c["K"], c["T_iter"]
    CinP = -(-Cin // 32) * 32
    P = prologue(x, None, kw["pro"], kw["pro_param"]).float().double()
    order = [(ci, tap) for c0 in range(0, CinP, 32) for tap in range(K) for h in range(2) for ci in range(c0 + 16 * h, c0 + 16 * h + 16)]
    ci_idx = torch.tensor([min(ci, Cin - 1) for ci, _ in order])
    live = torch.tensor([float(ci < Cin) for ci, _ in order], dtype=torch.float64)
    A = (W.double() * 2.0 ** o["k"])[:, ci_idx, torch.tensor([t for _, t in order])] * live
    cols = torch.stack([shifted(P, tap * kw["dil"] - kw["pad"], T_iter) for tap in range(K)], 0)  # [K][B][Cin][T_iter]
    Bm = cols[torch.tensor([t for _, t in order]), :, ci_idx] * live[:, None, None]              # [k][B][T_iter]
    acc = gemm_split(split_f16x2(A.numpy().astype(np.float32)), split_f16x2(Bm.reshape(len(order), -1).numpy().astype(np.float32)), F16X2)
    acc = torch.from_numpy(acc.astype(np.float64) * 2.0 ** -o["k"]).reshape(Cout, B, T_iter).permute(1, 0, 2).float()
    res = o["res_view"](o["res_buf"]) if c["res"] else None
    prev = o["out_view"](o["out_buf"]).clone()
    epi = {n: v for n, v in kw.items() if n not in ("dil", "pad", "pro", "pro_param")}
    e = conv_ref(acc, torch.eye(Cout)[:, :, None], bias=o["bias_t"], res=res, mask=o["mask_t"], prev=prev, dil=1, pad=0, **epi)
    got = o["out_buf"].double().clone()
    o["out_view"](got).copy_(e["y"])
    d = (got - o["want"]).abs()
    ratio = float((d / (o["bar"] + 1e-300))[o["bar"] > 0].max())
    print("%s: emulated max |d| %.3e, max |d| / bar %.3f" % (c["name"], float(d.max()), ratio))
    assert ratio <= 1.0 and bool((d[o["bar"] == 0] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# the branch inventory
# ------------------------------------------------------------------------------------------------------------------------
def test_conv_inventory_is_complete():
    names = [c["name"] for c in CONV]
    assert len(set(names)) == len(names) and all(c["impls"] == X2 for c in CONV)
    plain = [c for c in CONV if c["out_stride"] == 1]
    shapes = {"s32": [c for c in plain if c["Cout"] <= 32], "s64": [c for c in plain if 33 <= c["Cout"] <= 64], "s128": [c for c in plain if c["Cout"] > 64]}
    for key, rows in shapes.items():
        NB = _nb(rows[0])
        assert {NB - 1, 0, 1} <= {c["T_iter"] % NB for c in rows if c["T_iter"] >= NB - 1}, key
        assert any(c["T_iter"] < NB - 1 for c in rows), key
        passes = {(-(-(NB + _halo(c)) // 128), (NB + _halo(c)) % 128 != 0) for c in rows}
        want = {(2, False), (3, True), (3, False)} if NB == 256 else {(1, False), (2, True), (2, False)}
        assert want <= passes, (key, passes)
    assert {0, 128} <= {_halo(c) for c in CONV}
    assert {(2, 128), (9, 16)} <= {(c["K"], c["dil"]) for c in CONV if _halo(c) == 128}
    assert any(c["dil"] < 0 for c in plain) and any(c["T_out"] < c["T_in"] for c in plain) and any(c["T_out"] > c["T_in"] for c in plain)
    assert any(c["Cout"] % 32 for c in CONV) and {32, 64, 65} <= {c["Cout"] for c in CONV}
    assert any(c["Cout"] > 128 and -(-c["Cout"] // 32) * 32 <= -(-c["Cout"] // 128) * 128 - 32 for c in CONV)  # a wave wholly past CoutP
    assert {1, 2, 5} <= {-(-c["Cin"] // 32) for c in CONV} and {1, 16, 17} <= {c["Cin"] % 32 for c in CONV}
    assert {"none", "lrelu", "div"} <= {c["pro"] for c in CONV} and {"none", "relu", "lrelu", "gelu", "tanh"} <= {c["act"] for c in CONV}
    assert any(not c["bias"] for c in CONV) and any(c["mask"] for c in CONV) and any(c["alpha"] for c in CONV)
    assert any(c["res"] and c["res_emb"] and c["emb"] and c["res_emb"][1] != c["emb"][1] for c in CONV)       # res_cs != out_cs
    assert any(c["res"] and c["res_emb"] and not c["emb"] for c in CONV)
    assert any(c["accumulate"] and c["out_div"] for c in CONV) and any(c["accumulate"] and not c["out_div"] for c in CONV)
    assert any(c["B"] == 3 and c["x_emb"] and c["emb"] and c["res_emb"] and c["x_emb"][0] != c["Cin"] * c["T_in"] and
               c["emb"][0] != c["Cout"] * c["T_out"] and c["x_emb"][2] % 4 and c["emb"][2] % 4 and c["res_emb"][2] % 4 for c in CONV)
    assert any(c["wview"] == "transposed" for c in CONV) and any(isinstance(c["wview"], tuple) for c in CONV)
    offs = {(c["out_stride"], c["out_off"]) for c in CONV if c["out_stride"] > 1}
    assert {(2, -1), (2, 0), (3, -2), (3, -1), (3, 0)} <= offs
    assert any((c["Cin"], c["Cout"], c["K"]) == (80, 512, 7) for c in CONV)
    assert {(C_, k_, d_) for C_ in (256, 128, 64, 32) for k_, d_ in ((3, 1), (7, 3), (11, 5))} <= {(c["Cin"], c["K"], c["dil"]) for c in CONV if c["Cin"] == c["Cout"]}
    for c in CONV:
        assert set(c["modes"]) == ({"bounded"} if c["act"] in ("gelu", "tanh") else {"exact", "bounded"}), c["name"]
        assert _halo(c) <= 128 and c["T_in"] <= 1100 and c["B"] <= 3
        for tap in range(c["K"]):  # every tap reads in-range data for some frame
            lo_t, hi_t = tap * c["dil"] - c["pad"], c["T_iter"] - 1 + tap * c["dil"] - c["pad"]
            assert hi_t >= 0 and lo_t < c["T_in"], (c["name"], tap)


def test_transposed_inventory_is_complete():
    names = [c[0] for c in CONVT]
    assert len(set(names)) == len(names)
    form = lambda c: "vec" if c[5] % 4 == 0 and c[6] % 4 == 0 and ((c[7] - 1) * c[5] - 2 * c[6] + c[4]) % 4 == 0 else ("pair" if c[5] == 2 else "elem")
    rows = lambda c: c[3] * c[5]
    assert {(8, "vec"), (4, "vec"), (4, "elem"), (8, "elem")} <= {(c[5], form(c)) for c in CONVT}
    assert any(c[5] == 4 and c[6] % 4 for c in CONVT) and any(c[5] % 4 == 0 and c[6] % 4 == 0 and form(c) == "elem" for c in CONVT)  # refused by P / by T_out
    u2 = [c for c in CONVT if c[5] == 2]
    assert any(c[6] % 2 == 1 for c in u2) and any(c[6] % 2 == 0 and c[6] > 0 for c in u2) and any(c[4] == 2 and c[6] == 0 for c in u2)
    assert {3, 1, 5} <= {c[5] for c in CONVT if form(c) == "elem"} and any(c[4] % c[5] for c in CONVT) and any(c[4] == c[5] for c in CONVT)
    assert any(rows(c) <= 64 for c in CONVT) and any(rows(c) > 64 for c in CONVT) and any(rows(c) % 32 for c in CONVT)
    assert any(not c[8] for c in CONVT) and any(c[1] == 3 for c in CONVT)
    for lo, hi, NB in ((1, 64, 256), (65, 10 ** 6, 128)):
        t_iter = lambda c: c[7] + (c[4] + c[5] - 1) // c[5] - 1
        rem = {t_iter(c) % NB for c in CONVT if lo <= rows(c) <= hi and t_iter(c) >= NB - 1}
        assert {NB - 1, 0, 1} <= rem, (NB, rem)
    assert {(512, 256, 16, 8, 4), (256, 128, 16, 8, 4), (128, 64, 4, 2, 1), (64, 32, 4, 2, 1)} <= {c[2:7] for c in CONVT}
    assert all(c[7] <= 1100 and c[1] <= 3 for c in CONVT)


def test_pair_inventory_is_complete():
    names = [c[0] for c in PAIR]
    assert len(set(names)) == len(names)
    nb = lambda C_: 64 if C_ > 128 else (128 if C_ > 64 else 256)
    for lo, hi in ((16, 32), (33, 64), (65, 128), (129, 256)):
        rows = [c for c in PAIR if lo <= c[2] <= hi]
        assert rows and any(c[2] % 32 for c in rows), (lo, hi)
        assert {3, 5} <= {c[3] for c in rows} or hi != 256
    assert any(c[2] == 16 for c in PAIR) and any(c[5] == 64 for c in PAIR)
    rem = {}
    for c in PAIR:
        NV = nb(c[2]) - (c[3] - 1)
        rem.setdefault(nb(c[2]), set()).update({c[5] % NV} | ({"short"} if c[5] < NV else set()))
    assert all({0, 1} <= v for v in rem.values()) and "short" in rem[256] and "short" in rem[128], rem
    assert all(any(c[5] % (nb(c[2]) - c[3] + 1) == nb(c[2]) - c[3] and nb(c[2]) == n for c in PAIR) for n in (256, 128, 64))  # T % NV = NV - 1
    assert any(c[4] * (c[3] - 1) == 128 for c in PAIR) and any(c[3] == 15 for c in PAIR)
    assert any(c[6] and c[7] for c in PAIR) and any(c[6] and not c[7] for c in PAIR) and any(c[1] == 3 for c in PAIR)
    assert any(c[8] and c[9] and c[8][1] != c[5] and c[9][1] != c[5] and c[8][0] != c[2] * c[8][1] for c in PAIR)
    assert sum(c[0].startswith("v1_") for c in PAIR) == 12
    import set_amd  # noqa: F401
    from set_amd import _lib
    _lib.build()
    assert all(_lib.lib().set_resblock_pair_x2_supported(c[2], c[3], c[4], c[5]) == 0 and c[5] <= 1100 for c in PAIR)


# ------------------------------------------------------------------------------------------------------------------------
# host-only entry points of the built library
# ------------------------------------------------------------------------------------------------------------------------
PAIR_SUPPORT = [  # C, K, dil, T, taken
    (15, 3, 1, 64, False), (16, 3, 1, 64, True), (128, 5, 1, 64, True), (129, 5, 1, 64, True), (128, 7, 1, 64, True), (129, 7, 1, 64, False),
    (256, 3, 1, 64, True), (257, 3, 1, 64, False), (64, 4, 1, 64, False), (64, 2, 1, 64, False), (64, 1, 1, 64, False), (64, 15, 1, 64, True),
    (64, 17, 1, 64, False), (64, 3, 64, 64, True), (64, 3, 65, 64, False), (64, 5, 32, 64, True), (64, 5, 33, 64, False), (64, 3, 0, 64, False),
    (64, 3, 1, 63, False), (64, 3, 1, 64, True), (256, 5, 1, 64, True),
]


@pytest.mark.parametrize("C_,K,dil,T,taken", PAIR_SUPPORT)
def test_pair_supported_on_both_sides_of_every_threshold(built_lib, C_, K, dil, T, taken):
    """set_resblock_pair_x2_supported: C 15 / 16, 128 / 129 with K 5 and 7, 256 / 257, even K, K 15 / 17, dil (K - 1) 128 / 130 (and 132),
    T 63 / 64; ops.resblock_pair_eligible adds the split scope, the default impl and SET_AMD_RESBLOCK_FUSED."""
    from set_amd import ops
    assert (built_lib.set_resblock_pair_x2_supported(C_, K, dil, T) == 0) == taken
    assert not ops.resblock_pair_eligible(C_, K, dil, T)  # outside split_convs()
    with ops.split_convs():
        assert ops.resblock_pair_eligible(C_, K, dil, T) == (taken and ops._DEFAULT_IMPL == "auto" and os.environ.get("SET_AMD_RESBLOCK_FUSED", "1") != "0")


def test_pair_eligibility_follows_the_environment_switch(built_lib, monkeypatch):
    from set_amd import ops
    monkeypatch.setattr(ops, "_DEFAULT_IMPL", "auto")
    with ops.split_convs():
        monkeypatch.setenv("SET_AMD_RESBLOCK_FUSED", "1")
        assert ops.resblock_pair_eligible(64, 3, 1, 64)
        monkeypatch.setenv("SET_AMD_RESBLOCK_FUSED", "0")
        assert not ops.resblock_pair_eligible(64, 3, 1, 64)
        monkeypatch.delenv("SET_AMD_RESBLOCK_FUSED")
        monkeypatch.setattr(ops, "_DEFAULT_IMPL", "mfma")
        assert not ops.resblock_pair_eligible(64, 3, 1, 64)
    with ops.split_convs(False):
        assert not ops.resblock_pair_eligible(64, 3, 1, 64)


@pytest.mark.parametrize("Cout", [1, 31, 32, 33, 127, 128, 130, 191, 192, 200, 383, 384, 400, 512, 513])
@pytest.mark.parametrize("Cin", [1, 15, 16, 17, 200, 256, 300])
def test_x2_image_sizes_follow_their_formula(built_lib, Cout, Cin):
    """fp16 elements: two pieces x 32-row blocks x 16-channel groups of the 32-channel padded Cin x K x 512, + 8 (four fp32 tail words);
    the transposed image is the plain one of u Cout rows and ceil(k / u) taps."""
    up = lambda v, m: -(-v // m) * m
    size = lambda rows, K: 2 * (up(rows, 32) // 32) * (up(Cin, 32) // 16) * K * 512 + 8
    for K in (1, 3, 11):
        assert built_lib.set_packed_conv_weight_x2_size(Cout, Cin, K) == size(Cout, K)
    for k, u in ((16, 8), (4, 2), (7, 3), (3, 1), (10, 4), (5, 5)):
        assert built_lib.set_packed_conv_transpose_x2_size(Cout, Cin, k, u) == size(Cout * u, -(-k // u))
