"""float64 / integer model of the bf16-operand conv family (csrc/bf16.hip), and the CPU checks of that model.
tests/test_gpu_bf16_branches.py compares every branch of the forward / input-gradient kernels, of the weight-gradient kernels and of
the pack kernels with it.

The contract modelled (csrc/bf16.hip, head comment): P(x) = pro(x + in_chan_add) in fp32, ONE round-to-nearest-even to bf16; weights
rounded once at pack time; products and sums in fp32; the epilogue of SetConv1dArgs in fp32.  So
    conv_bf16_ref  = conv_ref  (tests/test_conv_reference.py) on rne_bf16(P32) and rne_bf16(W),
    wgrad_bf16_ref = wgrad_ref on rne_bf16(G) and rne_bf16(P32),
with P32 computed in numpy float32, one IEEE operation per step in the kernel's order (the library is built with -ffp-contract=off
and correctly rounded division: P32 is the kernel's value bit for bit).  rne_bf16 is written from the definition on the fp32 bit
pattern and checked against torch on every fp32 value of five binades.

The module also holds what the GPU sweep shares and what can be checked without a GPU: the case tables, Python mirrors of the launch
code (which kernel instance and slice count a case reaches; the tables name them by hand, the mirrors must agree), the operand
generators of the exact mode ("rounding probes": values with 10 significant bits, so that every rounding rule -- down, up, tie to
even of both parities -- is exercised while every partial sum stays an fp32 number), their budgets and tie shares."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_reference import conv_bound, conv_ref, f32, gamma, ints, prologue, weight_view, wgrad_ref  # noqa: F401

# ------------------------------------------------------------------------------------------------------------------------
# round-to-nearest-even to 8 significant bits, on the fp32 bit pattern
# ------------------------------------------------------------------------------------------------------------------------
def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32)


def rne_bf16_bits(t):
    """uint16 bf16 bits of the finite fp32 values `t`: keep the upper 16 bits; the dropped 16 bits above half a granule round the kept
    integer up, exactly half rounds it to even.  The kept integer is sign | exponent | 7 mantissa bits, so a mantissa carry moves
    into the exponent (the next binade; past the largest finite value: infinity), which is what rounding means there."""
    a = _np32(t)
    assert np.isfinite(a).all()
    u = a.view(np.uint32).astype(np.uint64)
    low, hi = u & 0xFFFF, u >> 16
    up = (low > 0x8000) | ((low == 0x8000) & ((hi & 1) == 1))
    return (hi + up.astype(np.uint64)).astype(np.uint16)


def bf16_value(bits):
    """float64 values of uint16 bf16 bits (numpy array or integer tensor), as a torch tensor of the same shape."""
    b = np.ascontiguousarray(bits.cpu().numpy() if torch.is_tensor(bits) else bits).astype(np.int64).astype(np.uint32) & 0xFFFF
    return torch.from_numpy((b << 16).astype(np.uint32).view(np.float32).astype(np.float64))


def rne_bf16(t):
    """The bf16 number nearest to each fp32 value, ties to even, as float64."""
    return bf16_value(rne_bf16_bits(t))


def rounding_kinds(t):
    """Per fp32 element: 0 already a bf16 number, 1 rounds down, 2 rounds up (both not ties), 3 tie with an even kept bit (stays), 4
    tie with an odd kept bit (goes up)."""
    u = _np32(t).view(np.uint32)
    low, odd = u & 0xFFFF, (u >> 16) & 1
    return np.where(low == 0, 0, np.where(low == 0x8000, 3 + odd, np.where(low < 0x8000, 1, 2)))


BINADES = [0, 1, 120, 127, 254]  # biased exponents: the denormals, the smallest normals, 2^-7, [1, 2), the top (rounds to infinity)


@pytest.mark.parametrize("e", BINADES)
@pytest.mark.parametrize("sign", [0, 1])
def test_rne_bf16_equals_torch_on_every_fp32_value_of_a_binade(e, sign):
    u = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(e << 23) | np.uint32(sign << 31))
    x = u.view(np.float32)
    got = rne_bf16_bits(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    kinds = rounding_kinds(x)
    assert [(kinds == k).sum() for k in range(5)] == [128, 128 * 32767, 128 * 32767, 64, 64]  # ties of both parities included
    if e < 254:
        v = bf16_value(got).numpy()
        assert (np.abs(v - x.astype(np.float64)) <= np.abs(bf16_value(got ^ np.uint16(1)).numpy() - x.astype(np.float64))).all()


def test_rne_bf16_on_hand_values():
    # 1 + 2^-8 is a tie between 1 (even) and 1 + 2^-7: stays; 1 + 3 2^-8 ties between 1 + 2^-7 (odd) and 1 + 2^-6: goes up
    x = torch.tensor([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, -(1 + 2.0 ** -8), 255.5, 255.75, 0.0, -0.0])
    assert rne_bf16(x).tolist() == [1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, 256.0, 256.0, 0.0, -0.0]
    assert rounding_kinds(x).tolist() == [0, 3, 4, 2, 3, 4, 2, 0, 0]


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def prologue32(x, in_chan_add=None, pro="none", pro_param=0.0):
    """P(x) in fp32 as the kernels compute it: one IEEE add, then the select-and-multiply of lrelu or one IEEE division."""
    P = _np32(x)
    if in_chan_add is not None:
        P = P + _np32(in_chan_add)[:, :, None]
    if pro == "lrelu":
        P = np.where(P > 0, P, P * np.float32(pro_param))
    elif pro == "div":
        P = P / np.float32(pro_param)
    else:
        assert pro == "none"
    assert P.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(P))


def conv_bf16_ref(x, W, *, in_chan_add=None, pro="none", pro_param=0.0, **kw):
    """conv_ref on the rounded operands; the epilogue (bias, alpha, act, res, mask, accumulate, out_div) stays conv_ref's."""
    return conv_ref(rne_bf16(prologue32(x, in_chan_add, pro, pro_param)), rne_bf16(W), **kw)


def wgrad_bf16_ref(g, x, K, dil, pad, *, in_chan_add=None, pro="none", pro_param=0.0, dtype="bf16"):
    """wgrad_ref on the rounded operands.  dtype 'bf16': g, x fp32; 'g16': g given as bf16 bits (an integer array [B][Cout][T]), not
    rounded again; 'gx16': x too (such an x takes no per-channel add and no prologue)."""
    gr = rne_bf16(g) if dtype == "bf16" else bf16_value(g)
    if dtype == "gx16":
        assert in_chan_add is None and pro == "none"
        xr = bf16_value(x)
    else:
        xr = rne_bf16(prologue32(x, in_chan_add, pro, pro_param))
    return wgrad_ref(gr, xr, K, dil, pad)


def q4(bits):
    """Storage of a bf16 operand [B][C][T] handed over by the fused layer kernels, channel-quad interleaved (comment above q4_row in
    csrc/bf16.hip): element (c, t) of a batch slice at byte ((c >> 2) T + t) 8 + (c & 3) 2.  Returns the flat uint16 array."""
    bits = np.asarray(bits, dtype=np.uint16)
    B, Cc, T = bits.shape
    assert Cc % 4 == 0
    out = np.zeros(B * Cc * T, dtype=np.uint16)
    b, c, t = np.meshgrid(np.arange(B), np.arange(Cc), np.arange(T), indexing="ij")
    byte = ((c >> 2) * T + t) * 8 + (c & 3) * 2
    assert (byte % 2 == 0).all()
    out[b * (Cc * T) + byte // 2] = bits
    return out


def up(x, m):
    return -(-x // m) * m


def pack_bf16_image(W_view, Cout, Cin, K, size=None):
    """The image SET_IMPL_BF16 reads (include/set_amd.h above set_packed_conv_weight_bf16_size): wp[tap][chunk][row][32] bf16 with row <
    Cout rounded up to 128 and chunk < ceil(Cin / 32), zero padded; W_view [Cout][Cin][K] fp32.  Flat uint16."""
    CoutP, nchunk = up(Cout, 128), up(Cin, 32) // 32
    img = np.zeros((K, nchunk, CoutP, 32), dtype=np.uint16)
    bits = rne_bf16_bits(W_view).reshape(Cout, Cin, K)
    co, ci, tap = np.meshgrid(np.arange(Cout), np.arange(Cin), np.arange(K), indexing="ij")
    img[tap, ci // 32, co, ci % 32] = bits
    if size is not None:
        assert img.size == size
    return img.reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------
# exact mode: rounding probes
# ------------------------------------------------------------------------------------------------------------------------
F_WEIGHTS = torch.tensor([0.10, 0.25, 0.40, 0.25])  # share of f = 0 (a bf16 number), 1 (down), 2 (tie), 3 (up)


def probe_grid(g, shape, s, p_neg=0.5):
    """+-(128 + k + f / 4) 2^s with k in 0..127 and f in 0..3: 10 significant bits, 8 are kept.  f = 2 is a tie whose kept bit is the
    parity of k; f = 1 rounds down, f = 3 up."""
    n = int(np.prod(shape))
    k = torch.randint(0, 128, (n,), generator=g)
    f = torch.multinomial(F_WEIGHTS, n, replacement=True, generator=g)
    sign = torch.where(torch.rand(n, generator=g) < p_neg, -1.0, 1.0)
    v = sign * (128.0 + k + f / 4.0) * 2.0 ** s
    return v.float().reshape(shape)


def probe_split(g, shape_x, s, p_neg=0.5):
    """The same grid as x + in_chan_add: x = +-(128 + k) 2^s per element, the per-(b, channel) add carries the fraction f / 4 2^s (a
    negative x lands on -(127 + k + (4 - f) / 4)); the fp32 sum is exact."""
    B, Cc, T = shape_x
    k = torch.randint(1, 128, shape_x, generator=g)
    sign = torch.where(torch.rand(shape_x, generator=g) < p_neg, -1.0, 1.0)
    f = torch.multinomial(F_WEIGHTS, B * Cc, replacement=True, generator=g).reshape(B, Cc)
    return (sign * (128.0 + k) * 2.0 ** s).float(), (f / 4.0 * 2.0 ** s).float()


def granule(*tensors):
    """The largest power of two that divides every non-zero value of the tensors (float64)."""
    e_min = None
    for t in tensors:
        if t is None:
            continue
        v = t.double().reshape(-1).numpy()
        v = v[v != 0]
        if v.size == 0:
            continue
        m, e = np.frexp(np.abs(v))
        mi = (m * 2.0 ** 53).astype(np.int64)
        low = mi & -mi
        lsb = e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)
        e_min = int(lsb.min()) if e_min is None else min(e_min, int(lsb.min()))
    return math.inf if e_min is None else 2.0 ** e_min


def tie_shares(P32):
    """(share of ties, both parities present, share of non-tie roundings) of the probed fp32 elements."""
    k = rounding_kinds(P32).reshape(-1)
    return float((k >= 3).mean()), bool((k == 3).any() and (k == 4).any()), float(((k == 1) | (k == 2)).mean())


def assert_probe_shares(P32, what):
    ties, both, moved = tie_shares(P32)
    assert ties >= 0.20 and both and moved >= 0.40, (what, ties, both, moved)


PARAMS = {"exact": dict(pro_lrelu=0.375, pro_div=2.0, act_lrelu=0.125, alpha=0.5, out_div=4.0),
          "bounded": dict(pro_lrelu=0.1, pro_div=20 ** 0.5, act_lrelu=0.2, alpha=5 ** -0.5, out_div=3.0)}
SCALES = ((1.0, 1.0), (2.0 ** -9 * 3, 37.0))  # bounded mode: (input scale, weight scale) of the two Gaussian draws
S_TINY = -110  # the case near the bottom of the normal range: granules down to 2^-112, every non-zero result still a normal number


# ------------------------------------------------------------------------------------------------------------------------
# forward cases.  branch: ("oneshot", CINP) | ("staged", "2x2" | "1x4", KCH, TGM, VEC) -- named by hand; conv_bf16_branch() must agree
# ------------------------------------------------------------------------------------------------------------------------
def _fc(name, branch, B, Cin, Cout, K, dil, T, **kw):
    """pad defaults to "same" for dil > 0; T_in = T_out = T_iter = T unless given.  emb / res_emb / x_emb: (batch stride, channel stride,
    offset) of the out / res / in view inside its buffer; add_off: element offset of in_chan_add inside its buffer; units: the value of
    SET_AMD_CONV_BF16_UNITS (None: unset); probe: which operand carries the rounding probes in exact mode; s: their power of two."""
    c = dict(name=name, branch=branch, B=B, Cin=Cin, Cout=Cout, K=K, dil=dil, T_in=T, pad=dil * (K - 1) // 2, pro="none", act="none",
             alpha=False, bias=True, res=False, mask=False, add=False, accumulate=False, out_div=False, emb=None, res_emb=None,
             x_emb=None, add_off=0, units=None, wview="plain", probe=None, s=None, modes=("exact", "bounded"))
    c.update(kw)
    c.setdefault("T_out", c["T_in"])
    c.setdefault("T_iter", c["T_out"])
    if c["act"] == "gelu":
        c["modes"] = ("bounded",)
    return c


W22, N14, OS = "2x2", "1x4", "oneshot"
_ST = lambda shape, KCH, TGM, VEC: ("staged", shape, KCH, TGM, VEC)

FWD = [
    # ---- one-shot 1x1: K == 1 && Cin > 32 && Cout > 64 && halo == 0 && !in_chan_add && pad == 0; CINP by cp = up32(Cin) ----
    # cp 64 -> <64>; Cout 72: ragged 128-row block (rows 72..95 of the third 32-row block masked, the fourth skipped); T 130: two
    # frames in the second 128-frame tile
    _fc("os64_ragged_rows_two_frames", (OS, 64), 2, 40, 72, 1, 1, 130, pro="lrelu", res=True, mask=True),
    _fc("os64_plain", (OS, 64), 1, 33, 65, 1, 1, 127, bias=False),
    _fc("os128", (OS, 128), 2, 100, 130, 1, 1, 70, act="relu"),                       # cp 128; two row blocks, the second ragged
    _fc("os192", (OS, 192), 2, 164, 96, 1, 1, 129, pro="div", res=True),              # cp 192
    _fc("os256_one_chunk", (OS, 256), 1, 256, 72, 1, 1, 100, mask=True),              # cp 256: nchunks 1
    _fc("os256_two_chunks", (OS, 256), 2, 512, 130, 1, 1, 130, pro="lrelu", res=True, mask=True),  # nchunks 2, both full
    # Cin 300: the second chunk has 44 channels: k-steps 3.. of it lie beyond the image's last 32-channel chunk (a_off clamps, B rows zero)
    _fc("os256_ragged_second_chunk", (OS, 256), 2, 300, 72, 1, 1, 130, res=True),
    _fc("os256_cin_260", (OS, 256), 1, 260, 200, 1, 1, 64, act="lrelu", alpha=True),
    # ---- staged KCH = 64: K == 1 && Cin > 32 && halo == 0 && !in_chan_add, and (pad != 0 -> wide) or (Cout <= 64 -> narrow) ----
    # Cin 96 = 3 chunks of 32: the second 64-channel stage has an odd chunk, zeroed in commit_a
    _fc("k64_wide_pad1", _ST(W22, 64, 1, False), 2, 96, 130, 1, 1, 130, pad=1, res=True),
    _fc("k64_narrow_two_tiles", _ST(N14, 64, 1, False), 2, 96, 40, 1, 1, 300, pro="lrelu", mask=True),
    _fc("k64_narrow_cin64", _ST(N14, 64, 1, False), 1, 64, 64, 1, 1, 257, act="relu"),
    # ---- K == 1 falling through to the 4-tap stage: Cin <= 32, or in_chan_add ----
    _fc("k1_cin20_falls_through", _ST(W22, 32, 4, True), 2, 20, 72, 1, 1, 132, probe="both"),
    _fc("k1_cin20_narrow", _ST(N14, 32, 4, False), 2, 20, 40, 1, 1, 130, pro="div"),
    _fc("k1_cin64_chan_add", _ST(W22, 32, 4, True), 2, 64, 130, 1, 1, 132, add=True, res=True),
]
# ---- TGM = 5: K == 5 || K > 8 (K 5: one tap group, 9: 5 + 4, 11: 5 + 5 + 1); TGM = 4 otherwise (3, 7: 4 + 3, 8: 4 + 4, 2) ----
# narrow = Cout <= 64 || (128 < Cout <= 192 && K > 1): Cout 40, 160 and 130 (wide only for K == 1); wide: Cout 100 and 200.  T 133: per-frame staging (T_in % 4), T 132:
# 16-byte units.  Cin 40: CinP 64, the second chunk has 8 channels
_VAR = [dict(pro="lrelu", res=True), dict(mask=True, act="relu"), dict(add=True), dict(act="lrelu", alpha=True), dict(pro="div", accumulate=True),
        dict(bias=False, res=True, mask=True)]
for _i, (_K, _Cout) in enumerate([(K, Co) for K in (5, 9, 11, 3, 7, 8, 2) for Co in (40, 160, 130, 100, 200)]):
    _T, _tgm = (133, 132)[_i % 2], 5 if _K in (5, 9, 11) else 4
    _nar = _Cout in (40, 160, 130)
    FWD.append(_fc("tg%d_k%d_cout%d" % (_tgm, _K, _Cout), _ST(N14 if _nar else W22, 32, _tgm, _T % 4 == 0), 2 if _Cout < 200 else 1, 40, _Cout, _K, 1,
                   _T, pad=(_K - 1) // 2, **_VAR[_i % len(_VAR)]))
FWD += [
    _fc("tg5_k5_both_rounded", _ST(N14, 32, 5, True), 1, 40, 40, 5, 1, 64, probe="both"),
    _fc("tg4_k3_tiny_scale", _ST(W22, 32, 4, True), 2, 64, 100, 3, 1, 132, pro="lrelu", res=True, act="lrelu", alpha=True, s=S_TINY),
    # ---- VEC = env && al && halo <= 16, al = in % 16 bytes == 0 && T_in % 4 == 0 && T_in >= 4 && in_cs % 4 == 0 && in_bs % 4 == 0 &&
    #      Cin % 4 == 0 && (!in_chan_add || in_chan_add % 16 bytes == 0).  The base case satisfies every term; each case below fails ONE
    #      (T_in < 4 cannot hold with T_in % 4 == 0: that case fails both) and must reach the per-frame form ----
    _fc("vec_base", _ST(W22, 32, 4, True), 2, 64, 100, 3, 1, 132, add=True, res=True, pro="lrelu"),
    _fc("vec_off_base_address", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 132, add=True, res=True, pro="lrelu", x_emb=(64 * 132 + 4, 132, 1)),
    _fc("vec_off_T_in_mod4", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 130, add=True, res=True, pro="lrelu", x_emb=(64 * 132, 132, 0)),
    _fc("vec_off_T_in_lt4", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 3, add=True, pro="lrelu", x_emb=(64 * 4, 4, 0), T_out=20),
    _fc("vec_off_in_cs_mod4", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 132, add=True, res=True, pro="lrelu", x_emb=(64 * 133, 133, 0)),
    _fc("vec_off_in_bs_mod4", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 132, add=True, res=True, pro="lrelu", x_emb=(64 * 132 + 2, 132, 0)),
    _fc("vec_off_Cin_mod4", _ST(W22, 32, 4, False), 2, 66, 100, 3, 1, 132, add=True, res=True, pro="lrelu"),
    _fc("vec_off_chan_add_address", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 132, add=True, res=True, pro="lrelu", add_off=1),
    _fc("vec_off_halo17", _ST(W22, 32, 4, False), 2, 64, 100, 2, 17, 132, pad=8, add=True, res=True, pro="lrelu"),
    _fc("vec_off_env", _ST(W22, 32, 4, False), 2, 64, 100, 3, 1, 132, add=True, res=True, pro="lrelu", units="0"),
    _fc("vec_strided_aligned_view", _ST(W22, 32, 4, True), 2, 64, 100, 3, 1, 132, add=True, x_emb=(70 * 136, 136, 2 * 136 + 4), add_off=4),
    # the sizing limit of the unit staging: halo 16 with the tile start 3 off a quad ((t0 + lo) & 3 == 3 for lo = -9): vNQ == VQMAX
    _fc("vec_limit_halo16_start3_wide", _ST(W22, 32, 5, True), 2, 40, 100, 9, 2, 260, pad=9),
    _fc("vec_limit_halo16_start3_narrow", _ST(N14, 32, 5, True), 1, 40, 40, 9, 2, 516, pad=9, pro="lrelu"),
    _fc("vec_start1", _ST(W22, 32, 4, True), 2, 40, 100, 3, 1, 132, pad=3),   # lo = -3: (t0 + lo) & 3 == 1
    _fc("vec_start2", _ST(N14, 32, 4, True), 2, 40, 40, 3, 1, 260, pad=2),    # lo = -2
    _fc("vec_last_quad_past_T_iter", _ST(W22, 32, 4, True), 2, 40, 100, 3, 1, 132, T_iter=130, T_out=131, res=True),
    # ---- halo 17 .. 128 (per-frame staging; the halo pass of 128 rows), both tile shapes ----
    _fc("halo64_wide", _ST(W22, 32, 4, False), 1, 40, 100, 3, 32, 300, mask=True),
    _fc("halo128_wide", _ST(W22, 32, 4, False), 1, 40, 100, 3, 64, 300, pro="lrelu"),   # the largest admitted
    _fc("halo128_narrow", _ST(N14, 32, 4, False), 1, 36, 40, 3, 64, 600, res=True),
    _fc("halo120_k9_narrow", _ST(N14, 32, 5, False), 1, 36, 160, 9, 15, 400),
    # ---- epilogue ----
    _fc("epi_T_iter_lt_T_out", _ST(W22, 32, 4, False), 2, 40, 72, 3, 1, 130, T_iter=100, res=True, mask=True),
    _fc("epi_res_cs_ne_out_cs_offsets", _ST(W22, 32, 4, True), 2, 40, 72, 3, 1, 132, res=True, emb=(80 * 140, 140, 3 * 140 + 5),
        res_emb=(75 * 133, 133, 133 + 2), act="relu"),
    _fc("epi_os_views", (OS, 64), 2, 40, 72, 1, 1, 130, res=True, mask=True, emb=(3 * 72 * 130, 130, 72 * 130), res_emb=(99 * 131, 131, 7)),
    _fc("epi_accumulate", _ST(N14, 32, 4, True), 2, 40, 40, 3, 1, 132, accumulate=True, res=True),
    _fc("epi_accumulate_out_div", _ST(W22, 32, 4, True), 2, 40, 100, 3, 1, 132, accumulate=True, out_div=True, mask=True, pro="lrelu"),
    _fc("epi_os_accumulate_out_div", (OS, 64), 2, 40, 72, 1, 1, 130, accumulate=True, out_div=True, act="lrelu"),
    _fc("epi_alpha_no_bias", _ST(W22, 32, 5, False), 1, 40, 100, 5, 1, 77, alpha=True, bias=False),
    _fc("epi_gelu", _ST(W22, 32, 4, True), 2, 40, 72, 3, 1, 132, act="gelu", alpha=True, res=True, mask=True),
    _fc("epi_os_gelu", (OS, 64), 1, 40, 72, 1, 1, 130, act="gelu"),
]
# ---- input-gradient form: dil = -d, pad = -d (K - 1) / 2, transposed weight view; T_iter = T_out = the forward's T_in ----
for _K in (1, 3, 9):
    for _d in (1, 4):
        _br = (OS, 128) if _K == 1 else _ST(W22, 32, 5 if _K == 9 else 4, (_K - 1) * _d <= 16)
        FWD.append(_fc("dgrad_k%d_d%d" % (_K, _d), _br, 2, 72, 100, _K, -_d, 92, pad=-_d * (_K - 1) // 2, wview="transposed", res=_K == 3, bias=False))
FWD.append(_fc("dgrad_k3_d4_narrow", _ST(N14, 32, 4, True), 2, 72, 40, 3, -4, 92, pad=-4, wview="transposed", mask=True, bias=False))

REFUSED = [
    # name, kwargs of the raw call, the C condition
    ("halo129", dict(K=2, dil=129, pad=64)),               # halo > 128
    ("halo129_negative_dil", dict(K=2, dil=-129, pad=-64)),
    ("out_stride2", dict(K=2, dil=-1, pad=0, out_stride=2)),  # out_stride != 1
    ("out_off1", dict(K=1, dil=1, pad=0, out_off=1)),         # out_off != 0
]


def conv_bf16_branch(c):
    """set_conv1d_bf16_dispatch and launch_conv_bf16 (csrc/bf16.hip), predicate by predicate.  The buffers of the sweep are allocations of
    their own (16-byte aligned), so the alignment of a base address is that of its element offset."""
    K, Cin, Cout, dil, pad = c["K"], c["Cin"], c["Cout"], c["dil"], c["pad"]
    if c.get("out_stride", 1) != 1 or c.get("out_off", 0) != 0:
        return ("refused", "strided")
    o_first, o_last = -pad, (K - 1) * dil - pad
    lo, halo = min(o_first, o_last), abs(o_last - o_first)
    if halo > 128:
        return ("refused", "halo")
    narrow = Cout <= 64 or (128 < Cout <= 192 and K > 1)
    if K == 1 and Cin > 32 and Cout > 64 and halo == 0 and not c["add"] and pad == 0:
        cp = up(Cin, 32)
        return (OS, 64 if cp <= 64 else 128 if cp <= 128 else 192 if cp <= 192 else 256)
    if K == 1 and Cin > 32 and halo == 0 and not c["add"]:
        return _ST(N14 if narrow else W22, 64, 1, False)
    bs, cs, off = c["x_emb"] if c["x_emb"] is not None else (Cin * c["T_in"], c["T_in"], 0)
    al = off % 4 == 0 and c["T_in"] % 4 == 0 and c["T_in"] >= 4 and cs % 4 == 0 and bs % 4 == 0 and Cin % 4 == 0 and \
        (not c["add"] or c["add_off"] % 4 == 0)
    env = not (c["units"] is not None and int(c["units"]) == 0)
    return _ST(N14 if narrow else W22, 32, 5 if (K == 5 or K > 8) else 4, bool(env and al and halo <= 16))


def fwd_tiles(c):
    """(frame tile NB, lo, halo, tile starts) of a staged case."""
    lo = min(-c["pad"], (c["K"] - 1) * c["dil"] - c["pad"])
    NB = 256 if c["branch"][1] == N14 else 128
    return NB, lo, (c["K"] - 1) * abs(c["dil"]), list(range(0, c["T_iter"], NB))


@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_forward_case_reaches_the_branch_it_names(c):
    assert conv_bf16_branch(c) == c["branch"]
    for tap in range(c["K"]):  # every tap of every case reads in-range data for some frame
        assert c["T_iter"] - 1 + tap * c["dil"] - c["pad"] >= 0 and tap * c["dil"] - c["pad"] < c["T_in"]


def test_refused_forms_are_refused_by_the_mirror_too():
    for name, kw in REFUSED:
        c = _fc(name, None, 1, 64, 64, kw["K"], kw["dil"], 300, pad=kw["pad"])
        c.update({k: v for k, v in kw.items() if k.startswith("out_")})
        assert conv_bf16_branch(c)[0] == "refused", name


def test_forward_inventory_is_complete():
    by = {}
    for c in FWD:
        by.setdefault(c["branch"], []).append(c)
    assert len({c["name"] for c in FWD}) == len(FWD)
    assert {(OS, n) for n in (64, 128, 192, 256)} <= set(by)
    os256 = {-(-c["Cin"] // 256): c for c in by[(OS, 256)]}
    assert {1, 2} <= set(os256) and any(c["Cin"] > 256 and c["Cin"] % 256 and up(c["Cin"], 32) % 256 < 256 - 32 for c in by[(OS, 256)])
    assert any(c["pro"] != "none" for c in FWD if c["branch"][0] == OS) and any(c["res"] and c["mask"] for c in FWD if c["branch"][0] == OS)
    assert any(not c["res"] and not c["mask"] and c["pro"] == "none" for c in FWD if c["branch"][0] == OS)
    for shape in (W22, N14):  # both KCH = 64 shapes, over an odd number of 32-channel chunks
        assert any(up(c["Cin"], 32) // 32 % 2 == 1 for c in by[_ST(shape, 64, 1, False)])
    assert any(c["pad"] != 0 for c in by[_ST(W22, 64, 1, False)]) and all(c["Cout"] <= 64 for c in by[_ST(N14, 64, 1, False)])
    k1 = [c for c in FWD if c["K"] == 1 and c["branch"][0] == "staged" and c["branch"][2] == 32]
    assert any(c["Cin"] <= 32 for c in k1) and any(c["add"] and c["Cin"] > 32 for c in k1)
    for tgm, Ks in ((5, (5, 9, 11)), (4, (3, 7, 8, 2))):
        for shape, couts in ((N14, (40, 160, 130)), (W22, (100, 200))):
            seen = {(c["K"], c["Cout"]) for vec in (False, True) for c in by.get(_ST(shape, 32, tgm, vec), [])}
            assert {(K, Co) for K in Ks for Co in couts} <= seen, (tgm, shape)
    for shape in (W22, N14):
        for tgm in (4, 5):
            assert _ST(shape, 32, tgm, True) in by and _ST(shape, 32, tgm, False) in by, (shape, tgm)
    names = {c["name"] for c in FWD}
    base = next(c for c in FWD if c["name"] == "vec_base")
    offs = [c for c in FWD if c["name"].startswith("vec_off_")]
    assert len(offs) == 9 and all(not c["branch"][4] for c in offs) and base["branch"][4]
    for c in offs:  # each differs from the base case in what its name says, and in nothing the epilogue sees (but T / K where it must)
        assert (c["Cout"], c["B"], c["pro"], c["add"]) == (base["Cout"], base["B"], base["pro"], base["add"])
    # unit staging: the limit vNQ == VQMAX for both tile widths, tile starts 0 .. 3 off a quad, a last quad partly past T_iter
    vec = [c for c in FWD if c["branch"][0] == "staged" and c["branch"][4]]
    lim = set()
    for c in vec:
        NB, lo, halo, starts = fwd_tiles(c)
        for t0 in starts:
            vsh = (t0 + lo) & 3
            if (NB + halo + vsh + 3) >> 2 == (NB + 16 + 3) // 4 + 1:
                lim.add(NB)
    assert lim == {128, 256}
    assert {(fwd_tiles(c)[1]) & 3 for c in vec} == {0, 1, 2, 3}
    assert any(c["T_iter"] % 4 for c in vec)
    halos = {fwd_tiles(c)[2] for c in FWD if c["branch"][0] == "staged"}
    assert {17, 64, 128} <= halos and any(17 < h < 128 and h not in (64,) for h in halos)
    assert {n for n, _ in REFUSED} >= {"halo129", "out_stride2", "out_off1"}
    for c in FWD:  # a wide halo: some tile's whole staging window [t0 + lo, t0 + lo + NB + halo) starts inside the data
        if c["branch"][0] == "staged" and fwd_tiles(c)[2] >= 64:
            assert c["T_in"] >= fwd_tiles(c)[2] + 128, c["name"]
    dg = {(c["K"], -c["dil"]) for c in FWD if c["wview"] == "transposed" and c["dil"] < 0 and c["pad"] <= 0}
    assert {(K, d) for K in (1, 3, 9) for d in (1, 4)} <= dg
    # epilogue
    assert any(c["Cout"] % 32 and c["Cout"] % 128 <= 96 for c in FWD)  # a partly masked 32-row block AND a skipped one
    assert any(c["T_iter"] < c["T_out"] for c in FWD)
    assert any(c["res"] and c["res_emb"] and c["emb"] and c["res_emb"][1] != c["emb"][1] and c["emb"][2] % c["emb"][1] and c["res_emb"][2] for c in FWD)
    assert any(not c["bias"] for c in FWD) and any(c["mask"] for c in FWD) and any(c["alpha"] for c in FWD)
    assert any(c["accumulate"] and not c["out_div"] for c in FWD) and any(c["accumulate"] and c["out_div"] for c in FWD)
    assert {"none", "relu", "lrelu", "gelu"} <= {c["act"] for c in FWD} and {"none", "lrelu", "div"} <= {c["pro"] for c in FWD}
    assert {"tg4_k3_tiny_scale", "tg5_k5_both_rounded"} <= names
    # frame tiles: more than one block, ragged last tile
    assert any(c["T_iter"] > 256 for c in by[_ST(N14, 64, 1, False)])


def fwd_probe(c, i):
    """Which operand carries the probes (the input under a prologue, where "round, then prologue" must differ from the contract; else
    alternating over the table) and their power of two (0 / -7 alternating, or the case's own)."""
    probe = c["probe"] or ("x" if c["pro"] != "none" else ("x", "w")[i % 2])
    s = c["s"] if c["s"] is not None else (0, -7)[(i // 2) % 2]
    return probe, s


def make_forward(c, mode, scale=0, case_index=0, sentinel=-7777.0, guard=64):
    """CPU operands of a forward case, the model's image of the whole out buffer and the bar of every buffer element.  exact: bar 0."""
    pv = PARAMS[mode]
    exact = mode == "exact"
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]) * 7 + (mode == "exact") + 1000 * scale)
    B, Cin, Cout, K = c["B"], c["Cin"], c["Cout"], c["K"]
    o = dict(c)
    probe, s = fwd_probe(c, case_index)
    o["probe"], o["s"] = probe, s
    pro_param = {"lrelu": pv["pro_lrelu"], "div": pv["pro_div"], "none": 0.0}[c["pro"]]
    wshape = (Cout, Cin, K) if c["wview"] == "plain" else (Cin, Cout, K)
    o["waddr"] = dict(base=0, sco=Cin * K, sci=K, stap=1) if c["wview"] == "plain" else dict(base=0, sco=K, sci=Cout * K, stap=1)
    add = None
    if exact:
        es = 2.0 ** s if s < -7 else 1.0  # bias / res / prev: integers (times the power of two of the tiny case)
        p_neg = 0.3 if c["pro"] == "lrelu" else 0.5  # (a negative value times 0.375 is a tie far less often: keep the tie share)
        if probe in ("x", "both"):
            if c["add"]:
                x, add = probe_split(g, (B, Cin, c["T_in"]), s, p_neg)
            else:
                x = probe_grid(g, (B, Cin, c["T_in"]), s, p_neg)
        else:
            x = ints(g, (B, Cin, c["T_in"]), -3, 3)
            add = ints(g, (B, Cin), -2, 2) if c["add"] else None
        wstore = probe_grid(g, wshape, s if probe == "w" else 0) if probe in ("w", "both") else ints(g, wshape, -2, 2)
        rnd = lambda shape, lo, hi, sc=1.0: ints(g, shape, lo, hi) * es
    else:
        xs, ws = SCALES[scale]
        x = torch.randn(B, Cin, c["T_in"], generator=g) * xs
        add = torch.randn(B, Cin, generator=g) * xs if c["add"] else None
        wstore = torch.randn(wshape, generator=g) * ((Cin * K) ** -0.5 * ws)
        es = xs * ws
        rnd = lambda shape, lo, hi, sc=1.0: torch.randn(shape, generator=g) * (sc * es)
    o["x"], o["add_t"], o["wstore"] = x, add, wstore
    W = weight_view(wstore, Cout, Cin, K, **o["waddr"])
    o["W"] = W
    o["bias_t"] = rnd((Cout,), -4, 4, 0.1) if c["bias"] else None
    o["mask_t"] = (torch.rand(B, c["T_out"], generator=g) > 0.3).float() if c["mask"] else None
    shape = (B, Cout, c["T_out"])

    def embed(emb, fill):
        bs, cs, off = emb if emb is not None else (Cout * c["T_out"], c["T_out"], 0)
        assert cs >= c["T_out"] and bs >= (Cout - 1) * cs + c["T_out"]
        n = guard + off + (B - 1) * bs + (Cout - 1) * cs + c["T_out"] + guard
        buf = torch.full((n,), sentinel) if fill is None else rnd((n,), -4, 4)
        return buf, (lambda b: b.as_strided(shape, (bs, cs, 1), guard + off))

    o["res_buf"], o["res_view"] = embed(c["res_emb"], True) if c["res"] else (None, None)
    o["out_buf"], o["out_view"] = embed(c["emb"], True if c["accumulate"] else None)
    kw = dict(dil=c["dil"], pad=c["pad"], T_iter=c["T_iter"], T_out=c["T_out"], act=c["act"],
              act_param=pv["act_lrelu"] if c["act"] == "lrelu" else 0.0, alpha=pv["alpha"] if c["alpha"] else 1.0,
              accumulate=c["accumulate"], out_div=pv["out_div"] if c["out_div"] else 0.0)
    o["kw"], o["pro_param"] = kw, pro_param
    res = o["res_view"](o["res_buf"]) if c["res"] else None
    prev = o["out_view"](o["out_buf"]).clone()
    o["P32"] = prologue32(x, add, c["pro"], pro_param)
    r = conv_bf16_ref(x, W, in_chan_add=add, pro=c["pro"], pro_param=pro_param, bias=o["bias_t"], res=res, mask=o["mask_t"], prev=prev, **kw)
    if exact:
        # every operand of the sums is a multiple of q; sum |products| + |bias| + |res| + |prev| < 2^24 q for every output: any partial sum
        # in any order is an fp32 number
        xr, Wr = rne_bf16(o["P32"]), rne_bf16(W)
        q_acc = granule(xr) * granule(Wr)
        assert granule(o["bias_t"], res, prev if c["accumulate"] else None) >= q_acc
        q = q_acc * min(1.0, kw["alpha"]) * (pv["act_lrelu"] if c["act"] == "lrelu" else 1.0) * (1.0 / pv["out_div"] if c["out_div"] else 1.0)
        top = float(r["S"].max()) * max(1.0, kw["alpha"]) + (float(res.abs().max()) if c["res"] else 0.0) + \
            (float(prev.abs().max()) if c["accumulate"] else 0.0)
        o["budget"] = top / q
        assert o["budget"] < 2 ** 24, (c["name"], top, q)
        assert q > 2.0 ** -126 and float(xr.abs().max()) * float(Wr.abs().max()) < 2.0 ** 100
    want = o["out_buf"].double().clone()
    o["out_view"](want).copy_(r["y"])
    bar = torch.zeros_like(want)
    if not exact:
        b = conv_bound(r, Cin * K, act=c["act"], act_param=kw["act_param"], alpha=kw["alpha"], res=res, prev=prev if c["accumulate"] else None)
        o["out_view"](bar).copy_(b * r["written"].double())
    o["want"], o["bar"], o["written"] = want, bar, int(r["written"].sum())
    return o


FWD_EXACT = [(i, c) for i, c in enumerate(FWD) if "exact" in c["modes"]]


@pytest.mark.parametrize("i,c", FWD_EXACT, ids=[c["name"] for _, c in FWD_EXACT])
def test_forward_exact_case_fits_fp32_and_probes_every_rounding(i, c):
    """The budget (asserted inside make_forward) and the tie shares of the probed operand."""
    o = make_forward(c, "exact", case_index=i)
    assert 0 < o["written"] <= c["B"] * c["Cout"] * c["T_out"]
    if o["probe"] in ("x", "both"):
        assert_probe_shares(o["P32"], c["name"] + " x")
    if o["probe"] in ("w", "both"):
        assert_probe_shares(o["W"], c["name"] + " w")
    if o["probe"] == "both":
        assert o["budget"] < 2 ** 24


def test_exact_budget_by_hand_at_the_deepest_reduction():
    """256 channels x 3 taps x |x| <= 256 x |w| <= 2 (in granules): 2^18.6; with the lrelu prologue the granule is a quarter: 2^20.6."""
    assert 256 * 3 * 256 * 2 * 4 + 64 < 2 ** 24
    assert {fwd_probe(c, i)[1] for i, c in enumerate(FWD)} == {0, -7, S_TINY}
    assert {fwd_probe(c, i)[0] for i, c in enumerate(FWD)} == {"x", "w", "both"}


def mfma_exactness_case():
    """One product of one granule against 2^24 - 2 granules held in the accumulator, either sign: 2^24 - 2 = 255 2^16 + 255 2^8 + 254 (three
    products of bf16 numbers).  Row 2 i + j of a K = 3, Cin = 64 conv (weights on the centre tap only) adds (+1, -1)[j] in channel (3, 16,
    32)[i]: inside the first MFMA of the stage, in its second MFMA, in the next 32-channel stage.  Returns x [1][64][T], W [8][64][3] and
    the exact outputs per row."""
    T = 8
    x = torch.zeros(1, 64, T)
    x[0, 0], x[0, 1], x[0, 2] = 2.0 ** 16, 2.0 ** 8, 1.0
    x[0, 3] = x[0, 16] = x[0, 32] = 1.0
    W = torch.zeros(8, 64, 3)
    W[:, 0, 1], W[:, 1, 1], W[:, 2, 1] = 255.0, 255.0, 254.0
    want = []
    for i, ch in enumerate((3, 16, 32)):
        for j, sg in enumerate((1.0, -1.0)):
            W[2 * i + j, ch, 1] = sg
            want.append(2.0 ** 24 - 2 + sg)
    want += [2.0 ** 24 - 2] * 2
    return x, W, torch.tensor(want, dtype=torch.float64)


def test_mfma_exactness_case_is_what_it_says():
    x, W, want = mfma_exactness_case()
    assert torch.equal(rne_bf16(x), x.double()) and torch.equal(rne_bf16(W), W.double())
    r = conv_bf16_ref(x, W, dil=1, pad=1)
    assert torch.equal(r["y"][0, :, 3], want) and want.tolist()[:2] == [16777215.0, 16777213.0]
    assert float(r["S"].max()) < 2 ** 24  # every partial sum of every order is an integer below 2^24


# ------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------------
def _wc(name, branch, dtype, B, Cin, Cout, K, dil, T, **kw):
    """branch: (kernel family, template arguments); S: the slice count, named by hand where the case is about the slice plan."""
    c = dict(name=name, branch=branch, dtype=dtype, B=B, Cin=Cin, Cout=Cout, K=K, dil=dil, T=T, pad=dil * (K - 1) // 2, T_in=None,
             pro="none", add=False, S=None, probe=None, units3=None, heavy=False)
    c.update(kw)
    if c["T_in"] is None:
        c["T_in"] = T
    return c


WG, WG3, WG3U, WGT = "wgrad", "wgrad3", "wgrad3u", "taps"
WGRAD = [
    # ---- conv1d_wgrad_bf16_kernel<GB16, XB16, GU, XU>: three dtypes x {element-wise: T % 8 != 0; GU: T % 8 == 0 && T >= 8; XU: GU && K == 1
    #      && pad == 0 && T_in == T}.  K = 3 with a prologue keeps bf16 / g16 off the 3-tap kernels (wgrad3_applies needs pro == NONE);
    #      gx16 never takes them ----
    _wc("w_bf16_elementwise_T77", (WG, (False, False, False, False)), "bf16", 2, 100, 200, 1, 1, 77, add=True, pro="lrelu"),
    _wc("w_bf16_gu", (WG, (False, False, True, False)), "bf16", 2, 40, 72, 3, 1, 72, pro="lrelu"),
    _wc("w_bf16_xu", (WG, (False, False, True, True)), "bf16", 2, 100, 200, 1, 1, 136, add=True, pro="div"),
    _wc("w_g16_elementwise_T77", (WG, (True, False, False, False)), "g16", 3, 100, 200, 1, 1, 77, add=True),
    _wc("w_g16_gu", (WG, (True, False, True, False)), "g16", 2, 40, 72, 3, 2, 72, pro="div", T_in=70),
    _wc("w_g16_xu", (WG, (True, False, True, True)), "g16", 2, 100, 200, 1, 1, 64),
    _wc("w_gx16_elementwise_T77", (WG, (True, True, False, False)), "gx16", 3, 100, 200, 1, 1, 77),
    _wc("w_gx16_gu", (WG, (True, True, True, False)), "gx16", 2, 40, 72, 3, 1, 72),
    _wc("w_gx16_xu", (WG, (True, True, True, True)), "gx16", 2, 100, 200, 1, 1, 136),
    # frame counts: one partial chunk, exactly one chunk, one frame into the second; both operands rounded at a depth the budget allows
    _wc("w_bf16_T40_both", (WG, (False, False, True, True)), "bf16", 2, 40, 72, 1, 1, 40, probe="both"),
    _wc("w_bf16_T64", (WG, (False, False, True, False)), "bf16", 2, 40, 72, 2, 1, 64, pad=1),
    _wc("w_bf16_T65", (WG, (False, False, False, False)), "bf16", 2, 40, 72, 1, 1, 65, T_in=70),
    _wc("w_bf16_k9_dil2_tiny_scale", (WG, (False, False, True, False)), "bf16", 1, 36, 40, 9, 2, 128, s=S_TINY),
    # ---- conv1d_wgrad3_bf16_kernel<GB16, GU>: K == 3 && dil > 0 && 2 dil <= 64 && pad >= 0 && pro == NONE && dtype in (bf16, g16) ----
    _wc("w3_f32g_dil1", (WG3, (False,)), "bf16", 2, 100, 200, 3, 1, 77, pad=0, T_in=79, add=True),
    _wc("w3_f32g_dil3", (WG3, (False,)), "bf16", 2, 40, 72, 3, 3, 72, pad=1, T_in=76),
    _wc("w3_f32g_dil32", (WG3, (False,)), "bf16", 2, 40, 130, 3, 32, 130, pad=30, T_in=134, add=True),
    _wc("w3_g16_elementwise", (WG3, (True,)), "g16", 2, 100, 200, 3, 3, 77, pad=1, T_in=81, add=True),
    _wc("w3_g16_units_dil32", (WG3, (True, True)), "g16", 2, 40, 72, 3, 32, 136, pad=32),
    _wc("w3_g16_units_pad_ne_dil", (WG3, (True, True)), "g16", 2, 40, 72, 3, 1, 72, pad=0, T_in=74, add=True),
    _wc("w3_g16_units_T_in_ne_T", (WG3, (True, True)), "g16", 2, 40, 72, 3, 2, 72, T_in=76),
    _wc("w3_g16_units_env_off", (WG3, (True, True)), "g16", 2, 40, 72, 3, 1, 72, units3="0"),
    _wc("w3_dil33_is_not_admitted", (WG, (False, False, True, False)), "bf16", 1, 40, 72, 3, 33, 136),  # 2 dil > 64: one tap per block
    # ---- conv1d_wgrad3u_bf16_kernel<DIL>: g16 && T % 8 == 0 && pad == dil in (1, 2, 4, 8) && T_in == T ----
    _wc("w3u_dil1", (WG3U, (1,)), "g16", 2, 100, 200, 3, 1, 136, add=True),
    _wc("w3u_dil2", (WG3U, (2,)), "g16", 2, 40, 72, 3, 2, 72),
    _wc("w3u_dil4", (WG3U, (4,)), "g16", 3, 40, 72, 3, 4, 128, add=True),
    _wc("w3u_dil8_one_chunk", (WG3U, (8,)), "g16", 1, 64, 128, 3, 8, 64),  # exactly one chunk: every halo frame is padding
    # ---- conv1d_wgrad_taps_bf16_kernel<K, PAD>: bf16 && !chan_add && K in (5, 7, 9) && dil == 1 && pad in ((K - 1) / 2, K - 1); 64-row tiles:
    #      Cout 72 and Cin 100 are ragged ----
    _wc("wt_k9_same", (WGT, (9, 4)), "bf16", 2, 100, 72, 9, 1, 77, pro="lrelu", T_in=80),
    _wc("wt_k9_causal", (WGT, (9, 8)), "bf16", 2, 40, 72, 9, 1, 65, pad=8, pro="div", T_in=60),
    _wc("wt_k7_same", (WGT, (7, 3)), "bf16", 2, 100, 72, 7, 1, 64, pro="div", T_in=66),
    _wc("wt_k7_causal", (WGT, (7, 6)), "bf16", 2, 40, 130, 7, 1, 40, pad=6, pro="lrelu", T_in=44),
    _wc("wt_k5_same", (WGT, (5, 2)), "bf16", 3, 100, 72, 5, 1, 130, T_in=128),
    _wc("wt_k5_causal", (WGT, (5, 4)), "bf16", 2, 40, 72, 5, 1, 77, pad=4, pro="lrelu", T_in=79),
    _wc("wt_chan_add_is_not_admitted", (WG, (False, False, False, False)), "bf16", 2, 40, 72, 5, 1, 77, add=True),
    # ---- slice plans.  plain: tiles = K ceil(Cin / 128) ceil(Cout / 128), S = min(ceil(640 / tiles), total, 64); 3 taps: tiles =
    #      ceil(Cin / 64) ceil(Cout / 128), cap 32; all taps: tiles = ceil(Cin / 64) ceil(Cout / 64), ceil(512 / tiles), cap 16;
    #      then cps = ceil(total / S), S = ceil(total / cps) ----
    # total 16 * 8 = 128, tiles 1: S 640 -> 128 -> cap 64; cps 2
    _wc("plan_plain_cap64", (WG, (False, False, True, True)), "bf16", 16, 32, 32, 1, 1, 512, S=64),
    # total 8 * 8 = 64, tiles 1: S 640 -> 64 -> cap 32; cps 2
    _wc("plan_taps3_cap32", (WG3, (False,)), "bf16", 8, 32, 32, 3, 1, 512, S=32, probe="g"),
    # total 15 * 5 = 75, tiles 1: cap 64; cps 2, S 38: the last slice has ONE chunk (chunks_per_slice rounds UP: rounded down, 37 chunks are lost)
    _wc("plan_plain_cap64_uneven_last", (WG, (False, False, True, True)), "bf16", 15, 32, 32, 1, 1, 320, S=38),
    # total 7 * 5 = 35, tiles 1: cap 32; cps 2, S 18, the last slice has one chunk
    _wc("plan_taps3_cap32_uneven_last", (WG3U, (1,)), "g16", 7, 32, 32, 3, 1, 320, S=18),
    # total 3 * 7 = 21, tiles 1: S 512 -> 21 -> cap 16; cps 2, S 11: the last slice has ONE chunk; slice 3 = chunks 6 (utterance 0), 7 (utterance 1)
    _wc("plan_taps_cap16_uneven_last", (WGT, (5, 2)), "bf16", 3, 32, 32, 5, 1, 448, S=11),
    # total 3 * 2 = 6, tiles 16 * 16 = 256: S = 2; cps 3: slice 0 = utterance 0 and the first chunk of utterance 1
    _wc("plan_slice_crosses_utterance", (WGT, (5, 2)), "bf16", 3, 1024, 1024, 5, 1, 128, S=2, heavy=True),
    # total 2 * 2 = 4 limits S (tiles 3 * 1 * 2 = 6: 107)
    _wc("plan_total_limits", (WG, (True, False, True, False)), "g16", 2, 100, 200, 3, 1, 128, pro="lrelu", S=4),
    # total 5 * 3 = 15, tiles 1 * 3 * 4 = 12: S 54 -> 15
    _wc("plan_taps3_ragged", (WG3U, (1,)), "g16", 5, 132, 400, 3, 1, 136, S=15, add=True),
]

GROUPED = [
    # the three production forms of the grouped launch (one launch over the residual layers): name, groups, dtype, B, Cin, Cout, K, dil, T,
    # x shared, add; the branch of each group's GEMM and S (target 1280 blocks: S = min(ceil(1280 / (groups tiles)), total, cap))
    dict(name="grp2_gx16_k1", groups=2, dtype="gx16", B=2, Cin=40, Cout=72, K=1, dil=1, T=136, x_shared=False, add=False, branch=(WG, (True, True, True, True)), S=6),
    dict(name="grp3_gx16_k1_ragged_T", groups=3, dtype="gx16", B=2, Cin=100, Cout=200, K=1, dil=1, T=77, x_shared=False, add=False, branch=(WG, (True, True, False, False)), S=4),
    dict(name="grp2_g16_k1_shared_x", groups=2, dtype="g16", B=3, Cin=100, Cout=200, K=1, dil=1, T=72, x_shared=True, add=False, branch=(WG, (True, False, True, True)), S=6),
    dict(name="grp3_g16_k1_shared_x", groups=3, dtype="g16", B=2, Cin=40, Cout=72, K=1, dil=1, T=77, x_shared=True, add=False, branch=(WG, (True, False, False, False)), S=4),
    dict(name="grp2_g16_k3_add", groups=2, dtype="g16", B=2, Cin=100, Cout=200, K=3, dil=1, T=136, x_shared=False, add=True, branch=(WG3U, (1,)), S=6),
    dict(name="grp3_g16_k3_add_dil2", groups=3, dtype="g16", B=3, Cin=40, Cout=72, K=3, dil=2, T=72, x_shared=False, add=True, branch=(WG3U, (2,)), S=6),
    dict(name="grp3_g16_k3_add_ragged_T", groups=3, dtype="g16", B=2, Cin=40, Cout=72, K=3, dil=1, T=77, x_shared=False, add=True, branch=(WG3, (True,)), S=4),
]
for _c in GROUPED:
    _c.update(pad=_c["dil"] * (_c["K"] - 1) // 2, T_in=_c["T"], pro="none", probe=None, units3=None, heavy=False, s=None)


def _slices(total, tiles, target, cap):
    S = max(1, min(-(-target // tiles), total, cap))
    cps = -(-total // S)
    return -(-total // cps)


def wgrad_bf16_plans(c, groups=1):
    """(S of the one-tap-per-block kernel, S of the 3-tap kernels, S of the all-taps kernel, total chunks)."""
    total = c["B"] * -(-c["T"] // 64)
    ci128, ci64, co128, co64 = -(-c["Cin"] // 128), -(-c["Cin"] // 64), -(-c["Cout"] // 128), -(-c["Cout"] // 64)
    target = 640 if groups == 1 else 1280
    return (_slices(total, groups * c["K"] * ci128 * co128, target, 64), _slices(total, groups * ci64 * co128, target, 32),
            _slices(total, ci64 * co64, 512, 16), total)


def wgrad_bf16_branch(c, groups=1):
    """wgrad_bf16_launch (csrc/bf16.hip): ((family, template arguments), S)."""
    K, dil, pad, T, T_in, dt = c["K"], c["dil"], c["pad"], c["T"], c["T_in"], c["dtype"]
    S1, S3, St, _ = wgrad_bf16_plans(c, groups)
    gu = T % 8 == 0 and T >= 8
    if groups == 1 and dt == "bf16" and not c["add"] and K in (5, 7, 9) and dil == 1 and pad in ((K - 1) // 2, K - 1):
        return (WGT, (K, pad)), St
    if K == 3 and dil > 0 and 2 * dil <= 64 and pad >= 0 and c["pro"] == "none" and dt in ("bf16", "g16"):
        env = not (c["units3"] is not None and int(c["units3"]) == 0)
        if env and dt == "g16" and gu and pad == dil and T_in == T and dil in (1, 2, 4, 8):
            return (WG3U, (dil,)), S3
        return (WG3, (False,) if dt == "bf16" else ((True, True) if gu else (True,))), S3
    return (WG, (dt != "bf16", dt == "gx16", gu, gu and K == 1 and pad == 0 and T_in == T)), S1


def wgrad_scratch_mirror(c):
    """set_conv1d_wgrad_scratch_floats for a bf16 dtype: the largest S over the variants the dtype could take."""
    S1, S3, St, _ = wgrad_bf16_plans(c)
    S = S1
    if c["K"] == 3:
        S = max(S, S3)
    if c["dtype"] == "bf16" and c["K"] in (5, 7, 9):
        S = max(S, St)
    return S * c["Cout"] * c["Cin"] * c["K"]


DTYPE_CODE = {"bf16": 1, "g16": 2, "gx16": 3}


@pytest.mark.parametrize("c", WGRAD, ids=[c["name"] for c in WGRAD])
def test_wgrad_case_reaches_the_branch_and_slice_plan_it_names(built_lib, c):
    branch, S = wgrad_bf16_branch(c)
    assert branch == c["branch"]
    if c["S"] is not None:
        assert S == c["S"]
    n = c["Cout"] * c["Cin"] * c["K"]
    lib = built_lib.set_conv1d_wgrad_scratch_floats(c["B"], c["Cin"], c["Cout"], c["K"], c["T"], DTYPE_CODE[c["dtype"]])
    assert lib == wgrad_scratch_mirror(c) and S * n <= lib
    if c["K"] not in (3, 5, 7, 9):
        assert S * n == lib  # one variant only: an exact count, not an upper bound
    assert 1 <= S <= wgrad_bf16_plans(c)[3]


@pytest.mark.parametrize("c", GROUPED, ids=[c["name"] for c in GROUPED])
def test_grouped_case_reaches_the_branch_and_slice_plan_it_names(built_lib, c):
    branch, S = wgrad_bf16_branch(c, c["groups"])
    assert branch == c["branch"] and S == c["S"]
    S1, S3, _, _ = wgrad_bf16_plans(c, c["groups"])
    n = c["Cout"] * c["Cin"] * c["K"]
    lib = built_lib.set_conv1d_wgrad_grouped_scratch_floats(c["groups"], c["B"], c["Cin"], c["Cout"], c["K"], c["T"])
    assert lib == c["groups"] * (max(S1, S3) if c["K"] == 3 else S1) * n and c["groups"] * S * n <= lib
    if c["K"] != 3:
        assert c["groups"] * S * n == lib


def test_wgrad_inventory_is_complete():
    got = {c["branch"] for c in WGRAD}
    want = {(WG, (g, x, gu, xu)) for g, x in ((False, False), (True, False), (True, True)) for gu, xu in ((False, False), (True, False), (True, True))}
    want |= {(WG3, (False,)), (WG3, (True,)), (WG3, (True, True))} | {(WG3U, (d,)) for d in (1, 2, 4, 8)}
    want |= {(WGT, kp) for kp in ((9, 4), (9, 8), (7, 3), (7, 6), (5, 2), (5, 4))}
    assert got == want and len({c["name"] for c in WGRAD}) == len(WGRAD)
    w3 = [c for c in WGRAD if c["branch"][0] == WG3]
    assert {1, 3, 32} <= {c["dil"] for c in w3} and any(c["pad"] != c["dil"] for c in w3) and any(c["T_in"] != c["T"] for c in w3) and any(c["add"] for c in w3)
    taps = [c for c in WGRAD if c["branch"][0] == WGT]
    assert {"lrelu", "div"} <= {c["pro"] for c in taps} and any(c["T_in"] != c["T"] for c in taps) and any(c["Cout"] == 72 for c in taps)
    Ts = {c["T"] for c in WGRAD}
    assert any(t < 64 for t in Ts) and {64, 65} <= Ts
    assert any(c["branch"][0] == WG3U and c["T"] == 64 and c["B"] == 1 for c in WGRAD)
    assert any(c["Cin"] == 100 and c["Cout"] == 200 for c in WGRAD)
    plans = {c["name"]: (wgrad_bf16_branch(c)[1], wgrad_bf16_plans(c)[3]) for c in WGRAD}
    assert plans["plan_plain_cap64"][0] == 64 and plans["plan_taps3_cap32"][0] == 32  # S at each cap (the all-taps cap: below)
    c = next(c for c in WGRAD if c["name"] == "plan_taps_cap16_uneven_last")
    assert min(-(-512 // 1), 21) > 16 and plans[c["name"]] == (11, 21) and 21 % 2 == 1
    assert plans["plan_total_limits"] == (4, 4)
    for fam in ((WG,), (WG3, WG3U), (WGT,)):  # every launch path computes chunks_per_slice itself: an uneven last slice in each
        assert any(c["branch"][0] in fam and plans[c["name"]][1] % -(-plans[c["name"]][1] // plans[c["name"]][0]) for c in WGRAD), fam
    S, total = plans["plan_slice_crosses_utterance"]
    assert (S, total) == (2, 6) and -(-total // S) == 3  # B = 3 with two chunks per utterance: a slice of three chunks
    forms = {(c["dtype"], c["K"], c["x_shared"], c["add"]) for c in GROUPED}
    assert forms == {("gx16", 1, False, False), ("g16", 1, True, False), ("g16", 3, False, True)}
    for form in forms:
        assert {2, 3} <= {c["groups"] for c in GROUPED if (c["dtype"], c["K"], c["x_shared"], c["add"]) == form}


def wgrad_probe(c, i):
    probe = c["probe"] or ("x" if c["pro"] != "none" or c["add"] else ("g", "x")[i % 2])
    if c["dtype"] == "gx16" and probe == "x":
        probe = "g"
    s = c.get("s")
    return probe, (s if s is not None else (0, -7)[(i // 2) % 2])


def make_wgrad(c, mode, scale=0, case_index=0, groups=1):
    """CPU operands of a weight-gradient case (per group), dW0 and the model.  Operands of a bf16 dtype are returned as bits [B][C][T]
    (the caller stores them through q4()); values the kernel rounds itself as fp32."""
    exact = mode == "exact"
    pv = PARAMS[mode]
    g_ = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]) * 11 + exact + 1000 * scale)
    B, Cin, Cout, K, T, T_in, dt = c["B"], c["Cin"], c["Cout"], c["K"], c["T"], c["T_in"], c["dtype"]
    probe, s = wgrad_probe(c, case_index)
    pp = {"lrelu": pv["pro_lrelu"], "div": pv["pro_div"], "none": 0.0}[c["pro"]]
    out = dict(c, probe=probe, s=s, pp=pp, groups=groups, g=[], x=[], adds=[], dw=[], A=[], P32=[])
    es = 2.0 ** s if (exact and s < -7) else 1.0
    for q in range(groups):
        add = None
        if exact:
            p_neg = 0.3 if c["pro"] == "lrelu" else 0.5
            gy = probe_grid(g_, (B, Cout, T), s) if probe in ("g", "both") else ints(g_, (B, Cout, T), -2, 2)
            if probe in ("x", "both"):
                sx = s if probe == "x" else 0
                if c["add"]:
                    x, add = probe_split(g_, (B, Cin, T_in), sx, p_neg)
                else:
                    x = probe_grid(g_, (B, Cin, T_in), sx, p_neg)
            else:
                x = ints(g_, (B, Cin, T_in), -3, 3)
                add = ints(g_, (B, Cin), -2, 2) if c["add"] else None
        else:
            xs, ws = SCALES[scale]
            gy, x = torch.randn(B, Cout, T, generator=g_) * ws, torch.randn(B, Cin, T_in, generator=g_) * xs
            add = torch.randn(B, Cin, generator=g_) * xs if c["add"] else None
        if c.get("x_shared") and q > 0:
            x = out["x_f32"]
        out["x_f32"] = x
        gop = gy if dt == "bf16" else torch.from_numpy(rne_bf16_bits(gy).astype(np.int32))
        xop = torch.from_numpy(rne_bf16_bits(x).astype(np.int32)) if dt == "gx16" else x
        dw, A = wgrad_bf16_ref(gop, xop, K, c["dil"], c["pad"], in_chan_add=add, pro=c["pro"], pro_param=pp, dtype=dt)
        out["g"].append(gop)
        out["x"].append(xop)
        out["adds"].append(add)
        out["dw"].append(dw)
        out["A"].append(A)
        out["P32"].append((gy, prologue32(x, add, c["pro"], pp) if dt != "gx16" else x))
    if exact:
        dw0 = ints(g_, (groups, Cout, Cin, K), -4, 4) * es
        # every product is a multiple of q; sum |products| + |dW0| < 2^24 q for every weight
        gr = [rne_bf16(p[0]) for p in out["P32"]]
        xr = [rne_bf16(p[1]) for p in out["P32"]]
        q_ = granule(*gr) * granule(*xr)
        assert granule(dw0) >= q_
        out["budget"] = (max(float(A.max()) for A in out["A"]) + float(dw0.abs().max())) / q_
        assert out["budget"] < 2 ** 24, (c["name"], out["budget"])
        assert q_ > 2.0 ** -126
    else:
        dw0 = torch.randn(groups, Cout, Cin, K, generator=g_) * (SCALES[scale][0] * SCALES[scale][1])
    out["dw0"] = dw0
    return out


def slice_frames(c, S):
    """Per slice: the list of (utterance, first frame, end frame) it sums, from the chunk walk of the kernels."""
    n_t = -(-c["T"] // 64)
    total = c["B"] * n_t
    cps = -(-total // S)
    out = []
    for z in range(S):
        out.append([(ch // n_t, (ch % n_t) * 64, min((ch % n_t) * 64 + 64, c["T"])) for ch in range(z * cps, min((z + 1) * cps, total))])
    return out


def wgrad_slice_models(o, q=0):
    """The model of every slice's partial tile (exact mode): wgrad_bf16_ref with the output gradient zeroed outside the slice's frames."""
    c = o
    _, S = wgrad_bf16_branch(c, o["groups"])
    parts = []
    for frames in slice_frames(c, S):
        keep = torch.zeros(c["B"], 1, c["T"], dtype=torch.bool)
        for b, t0, t1 in frames:
            keep[b, 0, t0:t1] = True
        gm = torch.where(keep, o["g"][q], torch.zeros_like(o["g"][q]))
        parts.append(wgrad_bf16_ref(gm, o["x"][q], c["K"], c["dil"], c["pad"], in_chan_add=o["adds"][q], pro=c["pro"], pro_param=o["pp"],
                                    dtype=c["dtype"])[0])
    return torch.stack(parts)


WGRAD_LIGHT = [(i, c) for i, c in enumerate(WGRAD)]


@pytest.mark.parametrize("i,c", WGRAD_LIGHT, ids=[c["name"] for _, c in WGRAD_LIGHT])
def test_wgrad_exact_case_fits_fp32_and_probes_every_rounding(i, c):
    o = make_wgrad(c, "exact", case_index=i)
    gy, P = o["P32"][0]
    if o["probe"] in ("g", "both"):
        assert_probe_shares(gy, c["name"] + " g")
    if o["probe"] in ("x", "both"):
        assert_probe_shares(P, c["name"] + " x")
    if not c["heavy"]:
        parts = wgrad_slice_models(o)
        assert torch.equal(parts.sum(0), o["dw"][0])  # the slices partition the frames


def test_wgrad_budget_by_hand_at_the_deepest_reduction():
    """16 x 512 frames x |g| <= 256 granules x |x| <= 3: 2^22.6."""
    assert 16 * 512 * 256 * 3 + 4 < 2 ** 24
    assert {wgrad_probe(c, i)[0] for i, c in enumerate(WGRAD)} == {"g", "x", "both"}
    assert {wgrad_probe(c, i)[1] for i, c in enumerate(WGRAD)} == {0, -7, S_TINY}


# ------------------------------------------------------------------------------------------------------------------------
# pack cases
# ------------------------------------------------------------------------------------------------------------------------
PACK = [
    # Cout, Cin, K, view: 'plain' [Cout][Cin][K], 'transposed' (storage [Cin][Cout][K]), ('phase', k, u, p) (one polyphase branch of a
    # ConvTranspose1d weight [Cin][Cout][k]: base p, sco k, sci Cout k, stap u)
    (72, 40, 3, "plain"), (72, 40, 3, "transposed"), (72, 40, 2, ("phase", 7, 3, 1)),
    (256, 256, 3, "plain"), (256, 256, 3, "transposed"), (256, 256, 2, ("phase", 16, 8, 5)), (130, 33, 1, "plain"),
]


def pack_operands(case, seed=0):
    Cout, Cin, K, view = case
    g = torch.Generator().manual_seed(Cout + Cin + K + seed)
    if view == "plain":
        store, addr = probe_grid(g, (Cout, Cin, K), -7), dict(base=0, sco=Cin * K, sci=K, stap=1)
    elif view == "transposed":
        store, addr = probe_grid(g, (Cin, Cout, K), 0), dict(base=0, sco=K, sci=Cout * K, stap=1)
    else:
        _, k, u, p = view
        store, addr = probe_grid(g, (Cin, Cout, k), -7), dict(base=p, sco=k, sci=Cout * k, stap=u)
    return store, addr


@pytest.mark.parametrize("case", PACK, ids=["%d_%d_%d_%s" % (c[0], c[1], c[2], c[3] if isinstance(c[3], str) else "phase") for c in PACK])
def test_pack_image_equals_a_direct_gather(built_lib, case):
    """pack_bf16_image against the decode of every image index (idx -> kk, row, chunk, tap) and the strided weight address."""
    Cout, Cin, K, _ = case
    store, addr = pack_operands(case)
    W = weight_view(store, Cout, Cin, K, **addr)
    assert_probe_shares(W, "pack")
    size = built_lib.set_packed_conv_weight_bf16_size(Cout, Cin, K)
    img = pack_bf16_image(W, Cout, Cin, K, size)
    CoutP, CinP = up(Cout, 128), up(Cin, 32)
    assert size == CoutP * K * CinP
    idx = np.arange(size)
    kk, r = idx & 31, idx >> 5
    row, r = r % CoutP, r // CoutP
    chunk, tap = r % (CinP // 32), r // (CinP // 32)
    ci = chunk * 32 + kk
    ok = (row < Cout) & (ci < Cin)
    flat = store.reshape(-1).numpy()
    src = addr["base"] + row * addr["sco"] + ci * addr["sci"] + tap * addr["stap"]
    vals = np.where(ok, flat[np.where(ok, src, 0)], np.float32(0))
    want = torch.from_numpy(vals.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(img, want) and int(ok.sum()) == Cout * Cin * K


# ------------------------------------------------------------------------------------------------------------------------
# the model against torch in float64
# ------------------------------------------------------------------------------------------------------------------------
PLAIN = [(2, 5, 7, 1, 1, 0, 19), (2, 6, 4, 3, 1, 1, 33), (1, 4, 9, 5, 2, 4, 40), (1, 7, 3, 9, 1, 0, 30), (1, 3, 4, 11, 5, 25, 64)]


@pytest.mark.parametrize("case", PLAIN)
def test_bf16_model_equals_torch_conv1d_in_float64_on_operands_rounded_by_torch(case):
    B, Cin, Cout, K, dil, pad, T = case
    g = torch.Generator().manual_seed(sum(case))
    x, W, b = torch.randn(B, Cin, T, generator=g), torch.randn(Cout, Cin, K, generator=g), torch.randn(Cout, generator=g)
    add = torch.randn(B, Cin, generator=g)
    r = conv_bf16_ref(x, W, in_chan_add=add, pro="lrelu", pro_param=0.1, bias=b, dil=dil, pad=pad, alpha=0.5, act="relu")
    xin = F.leaky_relu(x + add[:, :, None], f32(0.1)).to(torch.bfloat16).double()  # fp32 add, fp32 lrelu, torch's rounding
    want = torch.relu(F.conv1d(F.pad(xin, (pad, pad)), W.to(torch.bfloat16).double(), b.double(), dilation=dil) * 0.5)
    assert float((r["y"] - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    xd = torch.randn(B, Cin, T, generator=g)
    assert torch.equal(prologue32(xd, None, "div", 20 ** 0.5), xd / torch.tensor(20 ** 0.5, dtype=torch.float32))
    # probes: exact in float64 in either order
    xi, Wi = probe_grid(g, (B, Cin, T), -7), ints(g, (Cout, Cin, K), -2, 2)
    ri = conv_bf16_ref(xi, Wi, dil=dil, pad=pad)
    assert torch.equal(ri["y"], F.conv1d(F.pad(xi.to(torch.bfloat16).double(), (pad, pad)), Wi.double(), dilation=dil))


@pytest.mark.parametrize("case", PLAIN)
def test_bf16_model_in_gradient_form_equals_autograd_on_rounded_operands(case):
    B, Cin, Cout, K, dil, pad, T = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    x32, W32 = probe_grid(g, (B, Cin, T), 0), probe_grid(g, (Cout, Cin, K), -7)
    x = x32.to(torch.bfloat16).double().requires_grad_(True)
    W = W32.to(torch.bfloat16).double().requires_grad_(True)
    with torch.enable_grad():
        y = F.conv1d(F.pad(x, (pad, pad)), W, dilation=dil)
        gy32 = probe_grid(g, tuple(y.shape), -7)
        y.backward(gy32.to(torch.bfloat16).double())
    Wt_ = weight_view(W32, Cin, Cout, K, sco=K, sci=Cin * K)  # the transposed view of the fp32 master weights
    r = conv_bf16_ref(gy32, Wt_, dil=-dil, pad=-pad, T_out=T, T_iter=T)
    assert bool(r["written"].all()) and torch.equal(r["y"], x.grad)
    dw, A = wgrad_bf16_ref(gy32, x32, K, dil, pad)
    assert torch.equal(dw, W.grad) and bool((A >= dw.abs()).all())
    bits = torch.from_numpy(rne_bf16_bits(gy32).astype(np.int32))  # operands handed over as bits are not rounded again
    assert torch.equal(wgrad_bf16_ref(bits, x32, K, dil, pad, dtype="g16")[0], dw)
    xb = torch.from_numpy(rne_bf16_bits(x32).astype(np.int32))
    assert torch.equal(wgrad_bf16_ref(bits, xb, K, dil, pad, dtype="gx16")[0], dw)


def test_q4_is_the_layout_of_the_fused_layer_kernels():
    """Against the reshape the existing bf16 tests use ([B][C / 4][T][4]) and on hand values."""
    bits = np.arange(2 * 8 * 5, dtype=np.uint16).reshape(2, 8, 5)
    flat = q4(bits)
    assert np.array_equal(flat.reshape(2, 2, 5, 4), bits.reshape(2, 2, 4, 5).transpose(0, 1, 3, 2))
    # element (c = 6, t = 3) of utterance 1: byte ((6 >> 2) 5 + 3) 8 + (6 & 3) 2 = 68 -> uint16 index 34 of the slice
    assert flat[40 + 34] == bits[1, 6, 3]
