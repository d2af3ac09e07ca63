"""float64 reference of set_conv1d and of the conv weight gradient, written from the comment above SetConv1dArgs in
include/set_amd.h (not from the kernels), and the CPU checks of that reference: against F.conv1d, against F.conv_transpose1d
through the polyphase calls ops.conv_transpose1d issues, and against autograd for the input-gradient and weight-gradient forms.
tests/test_gpu_conv_branches.py compares every fp32 conv / wgrad kernel branch with it.

The module also pins what no kernel test can see: which kernel `auto` picks for every conv shape of the shipped configs
(ops._pick_impl), the host-only image size functions, and the split-K slice plan of the fp32 weight gradient for the cases the
GPU sweep runs (the hand-computed numbers of WGRAD_CASES against the library's own scratch size)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, base_hparams
from oracle import weights as Wt
from test_gpu_kernel_branches import U, _gamma as gamma  # u = 2^-24, gamma(k) = k u / (1 - k u): one definition for both sweeps


def f32(v):
    """The value a C `float` parameter holds (pro_param, act_param, alpha and out_div cross the ABI as fp32)."""
    return float(np.float32(v))


def _mish(z):
    return z * torch.tanh(F.softplus(z))


# name -> (float64 function of (z, act_param), Lipschitz constant).  gelu' peaks at 1.1290 (z = 1.4142), mish' at 1.0885
# (z = 1.4906); the others have slope <= 1 (leaky ReLU: max(1, |slope|)).
ACTS = {
    "none": (lambda z, p: z, lambda p: 1.0),
    "relu": (lambda z, p: torch.relu(z), lambda p: 1.0),
    "gelu": (lambda z, p: 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))), lambda p: 1.13),
    "tanh": (lambda z, p: torch.tanh(z), lambda p: 1.0),
    "softplus": (lambda z, p: torch.where(z > 20.0, z, torch.log1p(torch.exp(torch.clamp(z, max=20.0)))), lambda p: 1.0),
    "mish": (lambda z, p: _mish(z), lambda p: 1.09),
    "lrelu": (lambda z, p: torch.where(z > 0, z, z * p), lambda p: max(1.0, abs(p))),
}
TRANSCENDENTAL = ("gelu", "tanh", "softplus", "mish")


def weight_view(wflat, Cout, Cin, K, base=0, sco=None, sci=None, stap=1):
    """W[co][ci][tap] = wflat[base + co*sco + ci*sci + tap*stap] (the NAIVE weight addressing of SetConv1dArgs)."""
    sco = Cin * K if sco is None else sco
    sci = K if sci is None else sci
    co, ci, tap = torch.meshgrid(torch.arange(Cout), torch.arange(Cin), torch.arange(K), indexing="ij")
    return wflat.reshape(-1)[base + co * sco + ci * sci + tap * stap]


def prologue(x, in_chan_add=None, pro="none", pro_param=0.0):
    """P(x) = pro(x + in_chan_add[b][ci]) in float64."""
    P = x.double()
    if in_chan_add is not None:
        P = P + in_chan_add.double()[:, :, None]
    if pro == "lrelu":
        P = torch.where(P > 0, P, P * f32(pro_param))
    elif pro == "div":
        P = P / f32(pro_param)
    else:
        assert pro == "none"
    return P


def shifted(P, shift, T_iter):
    """[B][Cin][T_iter]: P[..., t + shift], 0 outside [0, T_in)."""
    T_in = P.shape[-1]
    idx = torch.arange(T_iter) + shift
    ok = (idx >= 0) & (idx < T_in)
    return P[..., idx.clamp(0, T_in - 1)] * ok.double()


def conv_ref(x, W, *, bias=None, res=None, mask=None, in_chan_add=None, prev=None, dil=1, pad=0, T_iter=None, T_out=None,
             out_stride=1, out_off=0, pro="none", pro_param=0.0, act="none", act_param=0.0, alpha=1.0, accumulate=False,
             out_div=0.0):
    """SetConv1dArgs, literally, in float64.  x [B][Cin][T_in], W [Cout][Cin][K], res / prev [B][Cout][T_out], mask [B][T_out]: the
    fp32 tensors the kernel gets.  Returns a dict of [B][Cout][T_out] tensors:
      y        the result (`prev` -- zeros when there is none -- wherever the call writes nothing)
      written  bool: the elements the call writes (t in [0, T_iter), n = t*out_stride + out_off inside [0, T_out))
      S        sum |W| |P(x)| + |bias|, the magnitude an fp32 summation error is proportional to
      z, f     (acc + bias) * alpha and act(z): what the bar of a transcendental activation is written in
    """
    B, Cin, T_in = x.shape
    Cout, Cin_w, K = W.shape
    assert Cin_w == Cin
    if T_out is None:
        T_out = T_in + 2 * pad - dil * (K - 1) if dil > 0 else T_in
    if T_iter is None:
        T_iter = T_out
    P = prologue(x, in_chan_add, pro, pro_param)
    Wd = W.double()
    acc = torch.zeros(B, Cout, T_iter, dtype=torch.float64)
    S = torch.zeros(B, Cout, T_iter, dtype=torch.float64)
    for tap in range(K):
        Pt = shifted(P, tap * dil - pad, T_iter)
        acc += torch.einsum("oc,bct->bot", Wd[:, :, tap], Pt)
        S += torch.einsum("oc,bct->bot", Wd[:, :, tap].abs(), Pt.abs())
    if bias is not None:
        acc = acc + bias.double()[None, :, None]
        S = S + bias.double().abs()[None, :, None]
    z = acc * f32(alpha)
    f = ACTS[act][0](z, f32(act_param))
    n = torch.arange(T_iter) * out_stride + out_off
    keep = (n >= 0) & (n < T_out)
    t_ok, n_ok = torch.arange(T_iter)[keep], n[keep]
    assert n_ok.unique().numel() == n_ok.numel()
    y = torch.zeros(B, Cout, T_out, dtype=torch.float64) if prev is None else prev.double().clone()
    v = f[:, :, t_ok]
    if res is not None:
        v = v + res.double()[:, :, n_ok]
    if mask is not None:
        v = v * mask.double()[:, None, n_ok]
    if accumulate:
        assert prev is not None
        v = y[:, :, n_ok] + v
        if out_div != 0.0:
            v = v / f32(out_div)
    else:
        assert out_div == 0.0
    y[:, :, n_ok] = v
    out = {"y": y, "written": torch.zeros(B, Cout, T_out, dtype=torch.bool)}
    out["written"][:, :, n_ok] = True
    for name, src in (("S", S), ("z", z), ("f", f)):
        full = torch.zeros(B, Cout, T_out, dtype=torch.float64)
        full[:, :, n_ok] = src[:, :, t_ok]
        out[name] = full
    return out


def conv_bound(r, CinK, *, act="none", act_param=0.0, alpha=1.0, res=None, prev=None):
    """Per-element bar of an fp32 kernel against conv_ref, for ANY accumulation order of fp32 FMA / MFMA chains: the Cin*K products and
    the roundings of the per-channel add, the prologue, the bias add and the alpha product are within gamma(Cin*K + 4) S of the exact
    sum, the activation amplifies that by at most its Lipschitz constant, and the activation's own rounding, the residual add, the mask
    product and the accumulate add cost one u each of a partial result no larger than |y| + |res| + |prev| (4 u covers them; a mean
    divisor >= 1 only shrinks every term).  gelu / tanh / softplus / mish add the forward bar of
    test_activation_forward_backward_paths (tests/test_gpu_kernel_branches.py), 64 u (|f| + |z|)."""
    b = gamma(CinK + 4) * r["S"] * abs(f32(alpha)) * ACTS[act][1](f32(act_param))
    mag = r["y"].abs()
    if res is not None:
        mag = mag + res.double().abs()
    if prev is not None:
        mag = mag + prev.double().abs()
    b = b + 4 * U * mag
    if act in TRANSCENDENTAL:
        b = b + 64 * U * (r["f"].abs() + r["z"].abs())
    return b


def wgrad_ref(g, x, K, dil, pad, *, in_chan_add=None, pro="none", pro_param=0.0):
    """dW[co][ci][tap] = sum_{b,t} G[b][co][t] P(X[b][ci][t + tap*dil - pad]) in float64 (the gradient of conv_ref's `acc` with
    respect to W), and A = sum |G| |P(X)| for the error bar."""
    T = g.shape[-1]
    P = prologue(x, in_chan_add, pro, pro_param)
    gd = g.double()
    dw, A = [], []
    for tap in range(K):
        Pt = shifted(P, tap * dil - pad, T)
        dw.append(torch.einsum("bot,bct->oc", gd, Pt))
        A.append(torch.einsum("bot,bct->oc", gd.abs(), Pt.abs()))
    return torch.stack(dw, -1), torch.stack(A, -1)


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------------------------------
# the reference against torch in float64
# ------------------------------------------------------------------------------------------------------------------------
PLAIN = [
    # B, Cin, Cout, K, dil, pad, T
    (2, 5, 7, 1, 1, 0, 19),
    (2, 6, 4, 3, 1, 1, 33),
    (1, 4, 9, 5, 2, 4, 40),
    (2, 3, 5, 3, 8, 8, 50),
    (1, 7, 3, 9, 1, 0, 30),    # unpadded: T_out = T - 8
    (1, 2, 2, 3, 3, 5, 21),    # more padding than "same": T_out = T + 4
    (1, 3, 4, 11, 5, 25, 64),
]


@pytest.mark.parametrize("case", PLAIN)
def test_reference_equals_torch_conv1d_in_float64(case):
    B, Cin, Cout, K, dil, pad, T = case
    g = torch.Generator().manual_seed(sum(case))
    x, W, b = torch.randn(B, Cin, T, generator=g), torch.randn(Cout, Cin, K, generator=g), torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, T + 2 * pad - dil * (K - 1), generator=g)
    mask = (torch.rand(B, res.shape[-1], generator=g) > 0.3).float()
    add = torch.randn(B, Cin, generator=g)
    r = conv_ref(x, W, bias=b, res=res, mask=mask, in_chan_add=add, dil=dil, pad=pad, pro="lrelu", pro_param=0.1, act="gelu", alpha=0.5)
    xin = F.leaky_relu(x.double() + add.double()[:, :, None], f32(0.1))
    want = F.conv1d(F.pad(xin, (pad, pad)), W.double(), b.double(), dilation=dil)
    want = (F.gelu(want * 0.5) + res.double()) * mask.double()[:, None]
    assert r["y"].shape == want.shape and bool(r["written"].all())
    assert float((r["y"] - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    # integers: float64 sums are exact in either order
    xi, Wi = ints(g, (B, Cin, T), -3, 3), ints(g, (Cout, Cin, K), -2, 2)
    ri = conv_ref(xi, Wi, dil=dil, pad=pad)
    assert torch.equal(ri["y"], F.conv1d(F.pad(xi.double(), (pad, pad)), Wi.double(), dilation=dil))
    assert torch.equal(ri["S"], F.conv1d(F.pad(xi.double().abs(), (pad, pad)), Wi.double().abs(), dilation=dil))


def polyphase_calls(T_in, k, u, P):
    """The set_conv1d calls ops.conv_transpose1d issues for nn.ConvTranspose1d(k, stride u, padding P): one per output phase."""
    T_out = (T_in - 1) * u - 2 * P + k
    for p in range(u):
        J = (k - p + u - 1) // u
        if J > 0:
            yield p, J, dict(dil=-1, pad=0, T_iter=T_in + J - 1, T_out=T_out, out_stride=u, out_off=p - P)


@pytest.mark.parametrize("cfg", [(2, 6, 5, 8, 4, 2, 13), (1, 4, 3, 4, 2, 1, 9), (1, 3, 2, 16, 8, 4, 7), (2, 5, 4, 7, 3, 2, 10),
                                 (1, 2, 3, 8, 8, 0, 5)])
def test_reference_equals_torch_conv_transpose1d_through_the_polyphase_calls(cfg):
    B, Cin, Cout, k, u, P, T = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x, wt, b = ints(g, (B, Cin, T), -3, 3), ints(g, (Cin, Cout, k), -2, 2), ints(g, (Cout,), -4, 4)
    want = F.conv_transpose1d(F.leaky_relu(x.double(), 0.25), wt.double(), b.double(), stride=u, padding=P)
    out = torch.full(want.shape, float("nan"), dtype=torch.float64)
    hits = torch.zeros(want.shape, dtype=torch.int32)
    for p, J, kw in polyphase_calls(T, k, u, P):
        W = weight_view(wt, Cout, Cin, J, base=p, sco=k, sci=Cout * k, stap=u)
        r = conv_ref(x, W, bias=b, pro="lrelu", pro_param=0.25, **kw)
        out[r["written"]] = r["y"][r["written"]]
        hits += r["written"].int()
    assert bool((hits == 1).all())  # every output sample belongs to exactly one phase
    assert torch.equal(out, want)


@pytest.mark.parametrize("case", PLAIN)
def test_reference_in_gradient_form_equals_autograd(case):
    """dx of a convolution = the same call on the output gradient with transposed weight addressing and negated dil / pad
    (ConvWeight.transposed(); include/set_amd.h, training section), T_out = the forward's T_in; dW = wgrad_ref."""
    B, Cin, Cout, K, dil, pad, T = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    x = ints(g, (B, Cin, T), -3, 3).double().requires_grad_(True)
    W = ints(g, (Cout, Cin, K), -2, 2).double().requires_grad_(True)
    with torch.enable_grad():  # (another module of the suite may have switched the tape off for the process)
        y = F.conv1d(F.pad(x, (pad, pad)), W, dilation=dil)
        gy = ints(g, tuple(y.shape), -3, 3)
        y.backward(gy.double())
    Wt_ = weight_view(W.detach().float(), Cin, Cout, K, sco=K, sci=Cin * K)  # transposed(): sco <-> sci
    r = conv_ref(gy, Wt_, dil=-dil, pad=-pad, T_out=T, T_iter=T)
    assert bool(r["written"].all()) and torch.equal(r["y"], x.grad)
    dw, A = wgrad_ref(gy, x.detach().float(), K, dil, pad)
    assert torch.equal(dw, W.grad) and bool((A >= dw.abs()).all())


def test_reference_marks_exactly_the_frames_the_header_says():
    x, W = torch.ones(1, 1, 6), torch.ones(1, 1, 1)
    prev = torch.full((1, 1, 10), 7.0)
    r = conv_ref(x, W, prev=prev, T_iter=5, T_out=10, out_stride=3, out_off=-4)  # n = -4, -1, 2, 5, 8
    assert r["written"][0, 0].nonzero().flatten().tolist() == [2, 5, 8]
    assert r["y"][0, 0].tolist() == [7, 7, 1, 7, 7, 1, 7, 7, 1, 7]
    r = conv_ref(x, W, prev=prev, T_iter=4, T_out=10, accumulate=True, out_div=2.0)  # frames >= T_iter stay
    assert r["y"][0, 0].tolist() == [4, 4, 4, 4, 7, 7, 7, 7, 7, 7]
    r = conv_ref(x, W, T_iter=9, T_out=9)  # frames past T_in read zeros, and are written
    assert r["y"][0, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0] and bool(r["written"].all())


def test_integer_sums_of_the_exact_cases_fit_fp32():
    """The bit-exact GPU checks need every partial sum below 2^24 in any order: x in [-3, 3], w in [-2, 2] up to Cin*K = 5632."""
    assert 5632 * 3 * 2 == 33792 and 33792 + 4 < 2 ** 24


# ------------------------------------------------------------------------------------------------------------------------
# which kernel `auto` picks for the conv shapes of the shipped configs (ops._pick_impl)
# ------------------------------------------------------------------------------------------------------------------------
def _hifigan_rows():
    h = Wt.HIFIGAN_V1
    T = 32  # mel frames: 32 * prod(upsample_rates) = 8192 samples at conv_post
    ch = h["upsample_initial_channel"]
    # conv_pre: T_iter 32 < 64 keeps it off the two-piece kernel
    rows = [("hifigan conv_pre", dict(T_iter=T, Cout=ch, Cin=80, K=7, pad=3, plain=True), ("mfma", "mfma", "bf16", "bf16"))]
    # T_iter < 64 keeps the first upsampler's phases off the two-piece kernel; out_stride > 1 keeps every phase off the bf16 one
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cin, cout = ch >> i, ch >> (i + 1)
        J = k // u
        first = i == 0
        rows.append(("hifigan ups.%d phase" % i, dict(T_iter=T + J - 1, Cout=cout, Cin=cin, K=J, dil=-1, out_stride=u, out_off=-(k - u) // 2),
                     ("mfma", "mfma" if first else "f16x2", "mfma", "mfma" if first else "f16x2")))
        T *= u
        for k_rb in h["resblock_kernel_sizes"]:
            for d in h["resblock_dilation_sizes"][0]:
                # Cin * K >= 96 holds for every ResBlock conv (32 * 3); halo (k - 1) d <= 50
                rows.append(("hifigan resblock C%d k%d d%d" % (cout, k_rb, d),
                             dict(T_iter=T, Cout=cout, Cin=cout, K=k_rb, dil=d, pad=(k_rb * d - d) // 2), ("mfma", "f16x2", "bf16", "f16x2")))
    assert T == 8192 and cout == 32
    rows.append(("hifigan conv_post", dict(T_iter=T, Cout=1, Cin=cout, K=7, pad=3, plain=True), ("fewout", "fewout", "mfma", "mfma")))
    return rows


def _model_rows():
    hp = base_hparams()
    H, C, k = hp["hidden_size"], hp["residual_channels"], hp["enc_kernel_size"]
    assert (H, C, k, hp["dec_kernel_size"], hp["audio_num_mel_bins"]) == (192, 256, 5, 5, 80)
    dmax = 2 ** ((hp["residual_layers"] - 1) % hp["dilation_cycle_length"])
    assert dmax == 1
    T, Tt = 800, 200  # mel frames / text tokens of the benchmark utterances
    rows = [
        # text encoder / decoder FFN (fs.ResidualBlock): conv k (H -> 2H), conv 1x1 (2H -> H)
        ("text ffn conv k5", dict(T_iter=Tt, Cout=2 * H, Cin=H, K=k, pad=2), ("mfma", "f16x2", "bf16", "f16x2")),
        ("text ffn conv 1x1", dict(T_iter=Tt, Cout=H, Cin=2 * H, K=1), ("mfma", "mfma", "bf16", "bf16")),
        ("decoder ffn conv k5", dict(T_iter=T, Cout=2 * H, Cin=H, K=k, pad=2), ("mfma", "f16x2", "bf16", "f16x2")),
        # their input gradients: transposed weights, dil = -1, pad = -2
        ("text ffn conv k5 dx", dict(T_iter=Tt, Cout=H, Cin=2 * H, K=k, dil=-1, pad=-2), ("mfma2", "f16x2", "bf16", "f16x2")),
        ("decoder ffn conv k5 dx", dict(T_iter=T, Cout=H, Cin=2 * H, K=k, dil=-1, pad=-2), ("mfma2", "f16x2", "bf16", "f16x2")),
        # mel encoder (fs.MelEncoder): three linears
        ("mel encoder 80 -> H", dict(T_iter=T, Cout=H, Cin=80, K=1), ("mfma", "mfma", "bf16", "bf16")),
        ("mel encoder H -> H", dict(T_iter=T, Cout=H, Cin=H, K=1), ("mfma", "mfma", "bf16", "bf16")),
        # DiffNet
        ("diffnet input projection", dict(T_iter=T, Cout=C, Cin=80, K=1), ("mfma", "mfma", "bf16", "bf16")),
        ("diffnet conditioner projection", dict(T_iter=T, Cout=2 * C, Cin=H, K=1), ("mfma", "mfma", "bf16", "bf16")),
        ("diffnet step mlp.0 (one column)", dict(T_iter=1, Cout=4 * C, Cin=C, K=1), ("naive", "naive", "naive", "naive")),
        ("diffnet output projection 1x1", dict(T_iter=T, Cout=2 * C, Cin=C, K=1), ("mfma", "mfma", "bf16", "bf16")),
        ("diffnet dilated conv", dict(T_iter=T, Cout=2 * C, Cin=C, K=3, dil=dmax, pad=dmax, chan_add=True), ("mfma", "mfma", "bf16", "bf16")),
        ("diffnet dilated conv, no step add", dict(T_iter=T, Cout=2 * C, Cin=C, K=3, dil=dmax, pad=dmax), ("mfma", "f16x2", "bf16", "f16x2")),
        ("diffnet dilated conv dx", dict(T_iter=T, Cout=C, Cin=2 * C, K=3, dil=-dmax, pad=-dmax), ("mfma2", "f16x2", "bf16", "f16x2")),
        ("diffnet output projection dx", dict(T_iter=T, Cout=C, Cin=2 * C, K=1), ("mfma", "mfma", "bf16", "bf16")),
        ("diffnet final projection", dict(T_iter=T, Cout=80, Cin=C, K=1), ("mfma", "mfma", "bf16", "bf16")),
    ]
    return rows


_DX = dict(Cout=256, Cin=512, K=3, dil=-1, pad=-1)        # the mfma2 rule: Cout >= 192, Cin >= 384, K >= 3, 32 <= T_iter <= 2048, halo <= 16
_POST = dict(Cout=1, Cin=32, K=7, pad=3, plain=True)      # the fewout rule
THRESHOLDS = [
    ("T_iter 15", dict(T_iter=15, Cout=256, Cin=256, K=3, pad=1), ("naive", "naive", "naive", "naive")),
    ("T_iter 16", dict(T_iter=16, Cout=256, Cin=256, K=3, pad=1), ("mfma", "mfma", "mfma", "mfma")),
    ("mfma2 T_iter 31", dict(_DX, T_iter=31), ("mfma", "mfma", "mfma", "mfma")),
    ("mfma2 T_iter 32", dict(_DX, T_iter=32), ("mfma2", "mfma2", "bf16", "bf16")),
    ("f16x2 T_iter 63", dict(_DX, T_iter=63), ("mfma2", "mfma2", "bf16", "bf16")),
    ("f16x2 T_iter 64", dict(_DX, T_iter=64), ("mfma2", "f16x2", "bf16", "f16x2")),
    ("mfma2 T_iter 2048", dict(_DX, T_iter=2048), ("mfma2", "f16x2", "bf16", "f16x2")),
    ("mfma2 T_iter 2049", dict(_DX, T_iter=2049), ("mfma", "f16x2", "bf16", "f16x2")),
    ("mfma2 Cout 191", dict(_DX, T_iter=800, Cout=191), ("mfma", "f16x2", "bf16", "f16x2")),
    ("mfma2 Cout 192", dict(_DX, T_iter=800, Cout=192), ("mfma2", "f16x2", "bf16", "f16x2")),
    ("mfma2 Cin 383", dict(_DX, T_iter=800, Cin=383), ("mfma", "f16x2", "bf16", "f16x2")),
    ("mfma2 Cin 384", dict(_DX, T_iter=800, Cin=384), ("mfma2", "f16x2", "bf16", "f16x2")),
    ("mfma2 K 2", dict(_DX, T_iter=800, K=2), ("mfma", "f16x2", "bf16", "f16x2")),
    ("mfma2 halo 16", dict(_DX, T_iter=800, dil=-8, pad=-8), ("mfma2", "f16x2", "bf16", "f16x2")),
    ("mfma2 halo 18", dict(_DX, T_iter=800, dil=-9, pad=-9), ("mfma", "f16x2", "bf16", "f16x2")),
    ("f16x2 / bf16 halo 128", dict(T_iter=800, Cout=64, Cin=64, K=3, dil=64, pad=64), ("mfma", "f16x2", "bf16", "f16x2")),
    ("f16x2 / bf16 halo 130", dict(T_iter=800, Cout=64, Cin=64, K=3, dil=65, pad=65), ("mfma", "mfma", "mfma", "mfma")),
    ("f16x2 Cout 31", dict(T_iter=800, Cout=31, Cin=64, K=3, pad=1), ("mfma", "mfma", "mfma", "mfma")),
    ("f16x2 Cout 32", dict(T_iter=800, Cout=32, Cin=64, K=3, pad=1), ("mfma", "f16x2", "bf16", "f16x2")),
    ("f16x2 Cin 31", dict(T_iter=800, Cout=64, Cin=31, K=4, pad=1), ("mfma", "mfma", "bf16", "bf16")),
    ("f16x2 Cin*K 94", dict(T_iter=800, Cout=64, Cin=47, K=2, pad=1), ("mfma", "mfma", "bf16", "bf16")),
    ("f16x2 Cin*K 96", dict(T_iter=800, Cout=64, Cin=48, K=2, pad=1), ("mfma", "f16x2", "bf16", "f16x2")),
    ("f16x2 K 1", dict(T_iter=800, Cout=64, Cin=128, K=1), ("mfma", "mfma", "bf16", "bf16")),
    ("bf16 Cin*K 63", dict(T_iter=800, Cout=64, Cin=21, K=3, pad=1), ("mfma", "mfma", "mfma", "mfma")),
    ("bf16 Cin*K 64", dict(T_iter=800, Cout=64, Cin=64, K=1), ("mfma", "mfma", "bf16", "bf16")),
    ("bf16 out_stride 2", dict(T_iter=800, Cout=64, Cin=64, K=2, dil=-1, out_stride=2), ("mfma", "f16x2", "mfma", "f16x2")),
    ("bf16 out_off 1", dict(T_iter=800, Cout=64, Cin=64, K=1, out_off=1), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout T_iter 4092", dict(_POST, T_iter=4092), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout T_iter 4096", dict(_POST, T_iter=4096), ("fewout", "fewout", "mfma", "mfma")),
    ("fewout T_iter 4098", dict(_POST, T_iter=4098), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout Cout 2", dict(_POST, T_iter=8192, Cout=2), ("fewout", "fewout", "mfma", "mfma")),
    ("fewout Cout 3", dict(_POST, T_iter=8192, Cout=3), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout K 9 pad 4", dict(_POST, T_iter=8192, K=9, pad=4), ("fewout", "fewout", "mfma", "mfma")),
    ("fewout K 11", dict(_POST, T_iter=8192, K=11, pad=5), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout pad 5", dict(_POST, T_iter=8192, K=9, pad=5), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout K - pad 6", dict(_POST, T_iter=8192, K=7, pad=1), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout pad -1", dict(_POST, T_iter=8192, K=3, pad=-1), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout dil 2", dict(_POST, T_iter=8192, K=3, dil=2, pad=2), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout not plain", dict(_POST, T_iter=8192, plain=False), ("mfma", "mfma", "mfma", "mfma")),
    ("fewout out_stride 2", dict(_POST, T_iter=8192, out_stride=2), ("mfma", "mfma", "mfma", "mfma")),
]

PICK_ROWS = _model_rows() + _hifigan_rows() + THRESHOLDS


@pytest.mark.parametrize("row", PICK_ROWS, ids=[r[0].replace(" ", "_") for r in PICK_ROWS])
def test_auto_picks_the_expected_kernel(row):
    """Expected names in the order (f32, f32 inside split_convs(), bf16, bf16 inside split_convs())."""
    import set_amd  # noqa: F401
    from set_amd import ops
    _, kw, want = row
    got = []
    try:
        for dtype in ("f32", "bf16"):
            ops.set_compute_dtype(dtype)
            got.append(ops._pick_impl("auto", **kw))
            with ops.split_convs():
                got.append(ops._pick_impl("auto", **kw))
    finally:
        ops.set_compute_dtype("f32")
    assert tuple(got) == want
    for impl in ("naive", "mfma", "mfma2", "fewout"):  # an explicit choice is never overridden
        assert ops._pick_impl(impl, **kw) == impl


def test_pick_table_covers_the_shipped_configs():
    names = [r[0] for r in PICK_ROWS]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("hifigan resblock") for n in names) == 4 * 3 * 3
    assert sum(n.startswith("hifigan ups") for n in names) == 4
    for cfg in ("spec_denoiser.yaml", "spec_denoiser_libritts.yaml"):
        assert os.path.exists(os.path.join(ROOT, "speech-editing-toolkit_amd", "egs", cfg))


# ------------------------------------------------------------------------------------------------------------------------
# host-only size functions
# ------------------------------------------------------------------------------------------------------------------------
def _up(x, m):
    return -(-x // m) * m


@pytest.mark.parametrize("Cout", [1, 31, 32, 33, 127, 128, 130, 191, 192, 200, 383, 384, 400, 512, 513])
@pytest.mark.parametrize("Cin", [1, 15, 16, 17, 200, 256, 300])
def test_packed_image_sizes_follow_their_formula(built_lib, Cout, Cin):
    from set_amd import _lib
    for K in (1, 3, 11):
        # v1: 32-row blocks x K x channels padded to the 16-channel LDS chunk
        assert built_lib.set_packed_conv_weight_size(Cout, Cin, K) == _up(Cout, 32) * K * _up(Cin, 16)
        # v2: 128 * RB rows per block, RB = 4 / 2 / 1 for Cout >= 384 / >= 192 / else
        RB = 4 if Cout >= 384 else (2 if Cout >= 192 else 1)
        assert built_lib.set_packed_conv_weight_v2_size(Cout, Cin, K) == _up(Cout, 128 * RB) * K * _up(Cin, 16)
        # set_fill_pack_desc holds the same rules: the element counts of the _size entries, the bf16 image's 128 / 32 roundings, and below
        # the big-tile image's channels per LDS chunk as ConvWeight.packed_v2 picks its slot
        d = _lib.SetPackDesc(Cout=Cout, Cin=Cin, K=K)
        assert built_lib.set_fill_pack_desc(C.byref(d), _lib.IMG_F32, 0) == built_lib.set_packed_conv_weight_size(Cout, Cin, K)
        assert (d.kind, d.CoutP, d.CinP, d.RB) == (_lib.IMG_F32, _up(Cout, 32), _up(Cin, 16), 1)
        assert built_lib.set_fill_pack_desc(C.byref(d), _lib.IMG_BF16, 0) == built_lib.set_packed_conv_weight_bf16_size(Cout, Cin, K)
        assert (d.kind, d.CoutP, d.CinP) == (_lib.IMG_BF16, _up(Cout, 128), _up(Cin, 32))
    for K, dils in ((2, range(-64, 65)), (3, (1, -32)), (11, (-6, 7))):  # K = 2: every halo 0 .. 64 the big-tile kernel takes, both signs
        for dil in dils:
            halo = (K - 1) * abs(dil)
            d = _lib.SetPackDesc(Cout=Cout, Cin=Cin, K=K)
            assert built_lib.set_fill_pack_desc(C.byref(d), _lib.IMG_F32_BIG, dil) == built_lib.set_packed_conv_weight_v2_size(Cout, Cin, K)
            assert (d.kind, d.CoutP, d.CinP, d.RB) == (_lib.IMG_F32_BIG, _up(Cout, 128 * RB), _up(Cin, 16), RB)
            assert d.ch_max == (128 if (64 + halo) * 256 * 4 > 96 * 1024 else 256), (K, dil)  # ConvWeight.packed_v2's slot
    d = _lib.SetPackDesc(Cout=Cout, Cin=Cin, K=0)
    assert built_lib.set_fill_pack_desc(C.byref(d), _lib.IMG_F32, 0) == -1 and built_lib.set_fill_pack_desc(None, 0, 0) == -1
    d.K = 1
    assert built_lib.set_fill_pack_desc(C.byref(d), 3, 0) == -1 and built_lib.set_fill_pack_desc(C.byref(d), -1, 0) == -1


# ------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases of the GPU sweep and their split-K slice plan (wgrad_f32_plan in csrc/train.hip), computed by hand:
#   total = B * ceil(T / 32) frame chunks;  tiles = K * ceil(Cin / 64) * ceil(Cout / 128);  slices = min(ceil(640 / tiles), total)
#   xcd_map = slices >= 8, then slices -> up8(slices) if that is <= total, else down8(slices)
#   cps = ceil(total / slices);  real = ceil(total / cps);  gz = up8(real) if xcd_map else real
# Slices real .. gz - 1 are padding (empty); slice real - 1 is short when total % cps != 0.
# ------------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [
    # name, B, Cin, Cout, K, dil, T, chan_add, pro, (slices, chunks_per_slice, gz)
    # total 2*3 = 6, tiles 3*1*1 = 3: slices min(214, 6) = 6 < 8 -> no xcd_map; cps 1
    ("no_xcd_map", 2, 48, 96, 3, 1, 70, False, "none", (6, 1, 6)),
    # total 3*4 = 12, tiles 1: slices min(640, 12) = 12, xcd_map; up8 = 16 > 12 -> rounds DOWN to 8; cps 2, real 6, gz 8: slices 6, 7 empty
    ("rounds_down_then_pads", 3, 64, 128, 1, 1, 97, True, "none", (8, 2, 8)),
    # total 1*13 = 13, tiles 3*1*1 = 3: slices min(214, 13) = 13; up8 = 16 > 13 -> 8; cps 2, real 7 (last slice 1 chunk: short), gz 8
    ("rounds_down_short_last", 1, 64, 96, 3, 2, 416, False, "none", (8, 2, 8)),
    # total 4*25 = 100, tiles 9*4*3 = 108: slices 6 < 8 -> no xcd_map; cps 17, real 6 (last slice 15 chunks: short)
    ("ragged_tiles_k9", 4, 200, 300, 9, 1, 800, False, "lrelu", (6, 17, 6)),
    # total 8*4 = 32, tiles 3*1*3 = 9: slices 72 -> 32 (total); up8 = 32 <= 32; cps 1, real 32, gz 32; T % 32 == 1
    ("one_chunk_per_slice_T_mod32_1", 8, 48, 300, 3, 8, 97, True, "none", (32, 1, 32)),
    # total 2*32 = 64, tiles 1*4*1 = 4: slices 160 -> 64; cps 1, gz 64; T % 32 == 31 (last chunk of each utterance has one dead frame)
    ("T_mod32_31", 2, 200, 128, 1, 1, 1023, False, "div", (64, 1, 64)),
    # total 5*7 = 35, tiles 3*1*1 = 3: slices min(214, 35) = 35; up8 = 40 > 35 -> 32; cps 2, real 18 (last slice 1 chunk), gz 24: 6 padding slices
    ("round_up_adds_padding", 5, 64, 128, 3, 2, 224, True, "none", (32, 2, 24)),
    # total 3*10 = 30, tiles 9*1*1 = 9: slices 72 -> 30; up8 = 32 > 30 -> 24; cps 2, real 15, gz 16: one padding slice; dil 8
    ("k9_dil8", 3, 64, 96, 9, 8, 320, False, "none", (24, 2, 16)),
    # the bench shape of a DiffNet dilated conv: total 32*25 = 800, tiles 3*4*4 = 48: slices 14 -> up8 16 <= 800; cps 50, real 16, gz 16
    ("diffnet_dilated_bench", 32, 256, 512, 3, 1, 800, True, "none", (16, 50, 16)),
]


def wgrad_plan(B, Cin, Cout, K, T):
    up8 = lambda v: (v + 7) // 8 * 8
    total = B * -(-T // 32)
    tiles = K * -(-Cin // 64) * -(-Cout // 128)
    slices = max(1, min(-(-640 // tiles), total))
    xcd = slices >= 8
    if xcd:
        slices = up8(slices) if up8(slices) <= total else slices // 8 * 8
    cps = -(-total // slices)
    real = -(-total // cps)
    return slices, cps, up8(real) if xcd else real, real, total, xcd


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_slice_plan_of_the_sweep_cases(built_lib, case):
    _, B, Cin, Cout, K, dil, T, _, _, (slices, cps, gz) = case
    assert wgrad_plan(B, Cin, Cout, K, T)[:3] == (slices, cps, gz)
    # the library's own plan: the deterministic entry point sizes its scratch as gz tiles of dW
    assert built_lib.set_conv1d_wgrad_scratch_floats(B, Cin, Cout, K, T, 0) == gz * Cout * Cin * K


def test_wgrad_sweep_reaches_every_plan_branch():
    plans = {c[0]: wgrad_plan(*c[1:5], c[6]) for c in WGRAD_CASES}
    up8 = lambda v: (v + 7) // 8 * 8
    assert not plans["no_xcd_map"][5]
    first = {n: min(-(-640 // (c[4] * -(-c[2] // 64) * -(-c[3] // 128))), p[4]) for (n, p), c in zip(plans.items(), WGRAD_CASES)}
    assert any(p[5] and up8(first[n]) > p[4] for n, p in plans.items())       # the multiple-of-8 round-up would exceed total: rounds down
    assert any(p[5] and up8(first[n]) <= p[4] and up8(first[n]) != first[n] for n, p in plans.items())  # ... fits: rounds up
    assert any(p[2] > p[3] for p in plans.values())                           # padding slices
    assert any(p[4] % p[1] != 0 for p in plans.values())                      # a short last slice
    assert {c[6] % 32 for c in WGRAD_CASES} >= {0, 1, 31}
    assert {c[2] for c in WGRAD_CASES} >= {48, 64, 200} and {c[3] for c in WGRAD_CASES} >= {96, 128, 300}
    assert {(c[4], c[5]) for c in WGRAD_CASES} >= {(1, 1), (3, 1), (3, 2), (3, 8), (9, 1), (9, 8)}
