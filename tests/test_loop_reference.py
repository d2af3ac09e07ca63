"""float64 model of one reverse diffusion step and of the reverse loop (set_diffusion_loop, csrc/diffusion_loop.hip) with its two fused
step-boundary kernels (csrc/boundary.hip), written from the formulas in the header comment of csrc/boundary.hip and the Python lines it
cites (diffnet.py:118-131, spec_denoiser.py:86-101, 181), not from the kernels; the case tables of the GPU sweep
tests/test_gpu_loop_branches.py (each row names the branch it reaches and the C condition it meets); and the CPU checks of both.

  in_proj    xin = ReLU(W_in x + b_in)                                              (diffnet.py:118-120)
  layers     the L residual layers: (x_L, skip sum)                                 (diffnet.py:60-81, 123-127)
  head       x0 = W_out ReLU(W_skip (skip / f32(sqrt L)) + b_skip) + b_out          (diffnet.py:128-131; the division as `pro = div` does it)
  posterior  x' = c1 x0 + c2 x_t + nonzero exp(logvar / 2) eps                      (spec_denoiser.py:86-101)
  loop       steps x (in_proj, layers, head, posterior); step k runs diffusion step sid = steps-1-k: column sid of dstep, row sid of coef4,
             noise slice k                                                          (spec_denoiser.py:181)
The GEMMs are conv_ref / conv_x2_ref of the conv reference modules with K = 1, so every function also returns the magnitude sums its
error bar needs, and the bars are conv_bound / conv_x2_bound composed:
  bar_h   = conv_bound(K = 256, relu, pro = div)
  bar_x0  = gamma(256 + 4) S_out + |W_out| @ bar_h + 4 u |x0|
  bar_x'  = |c1| bar_x0 + 4 u (|c1 x0| + |c2 x_t| + |sigma eps|) + 64 u (1 + |logvar / 2|) |sigma eps|   (the last term: expf, as the
            transcendental term of conv_bound)
  bar_xin = gamma(MP + 4) S_in + 4 u |xin|     on the fp32 x' actually used (teacher forcing: the GPU test feeds the model what the kernel read)
and the same with conv_x2_bound for the two-piece fp16 kernel.

Exact mode (make_exact): operands on the grid of integers / 128, chosen so that every phase of both boundary kernels is exact: L = 4
(div = 2) or L = 1, small-integer W_skip / W_out / W_in and biases, c1 / c2 powers of two, logvar = 0, integer eps.  The skip sum is made
exact by saturating the gate: condproj = +40 on the sigmoid half and +-40 (a random sign per (b, layer, channel, t)) on the tanh half,
zero dilated-conv weights, so z is +-1 and the skip sum is sum_l (Wo_l z_l + bo_l), an integer / 128 (L = 1) or / 64 (L = 4) the model predicts.  The fractions
give s, h and x' non-zero low fp16 pieces.  test_exact_inputs_meet_their_budget asserts the budget, never assumes it."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_conv_reference import U, conv_bound, conv_ref, gamma, ints
from test_conv_x2_reference import BUDGET_BITS, conv_x2_bound, conv_x2_ref, split2  # noqa: F401 (split2: re-exported for the GPU sweep)

torch.set_grad_enabled(False)
DC = 256
RSQRT2 = float(np.float32(0.70710678118654752440))  # the layer kernels scale the residual by this fp32 constant (one rounding)
Q = 2.0 ** -7  # granule of every exact-mode intermediate (layer biases are integers / 64 with div = 2, integers / 128 with div = 1)


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def _ones_S(x, **pro):
    return conv_ref(x, torch.ones(1, x.shape[1], 1), **pro)["S"]


def _gemm(x, W, b, x2k, *, act="none", **pro):
    """One 1x1 conv of the boundary: conv_ref's dict plus `bar` (fp32 kernel: conv_bound with K = Cin rounded up to 16; two-piece fp16
    kernel, x2k = the image's scale exponent: conv_x2_bound) and, for the two-piece kernel, `x2` = conv_x2_ref's dict."""
    Cin = W.shape[1]
    r = conv_ref(x, W, bias=b, act=act, **pro)
    if x2k is None:
        r["bar"] = conv_bound(r, -(-Cin // 16) * 16, act=act)
    else:
        r["x2"] = conv_x2_ref(x.float(), W, x2k, bias=b, act=act, **pro)
        r["bar"] = conv_x2_bound(r, r["x2"], _ones_S(x, **pro), W.abs().sum((1, 2)), x2k, Cin=Cin, K=1, act=act)
    return r


def in_proj(x, W_in, b_in, x2k=None):
    """xin = ReLU(W_in x + b_in): dict y, S, bar (bar_xin)."""
    return _gemm(x, W_in, b_in, x2k, act="relu")


def layers(xin, cp, dcol, Wd, bd, Wo, bo, dcl):
    """(x_L, skip): the fp64 layer evaluation (diffnet.py:60-81): y = dilated_conv(x + d) + cond; z = sigmoid(y[:256]) tanh(y[256:]);
    o = W_o z + b_o; x <- (x + o[:256]) / sqrt 2; skip += o[256:].  cp [B][L*512][T], dcol [L*256], dilation 2^(l mod dcl)."""
    x, skip = xin.double(), torch.zeros_like(xin, dtype=torch.float64)
    for l in range(len(Wd)):
        d = 1 << (l % dcl)
        dv = dcol[l * DC:(l + 1) * DC].double()[None, :, None]
        y = F.conv1d(x + dv, Wd[l].double(), bd[l].double(), padding=d, dilation=d) + cp[:, l * 512:(l + 1) * 512].double()
        z = torch.sigmoid(y[:, :DC]) * torch.tanh(y[:, DC:])
        o = F.conv1d(z, Wo[l].double(), bo[l].double())
        x, skip = (x + o[:, :DC]) / 2 ** 0.5, skip + o[:, DC:]
    return x, skip


def head(skip, L, W_skip, b_skip, W_out, b_out, x2k=None):
    """x0 of the output head from the skip sum.  x2k = (k of the W_skip image, k of the W_out image) for the two-piece kernel.
    dict: h, x0, S_h, S_out, bar_h, prop = |W_out| @ bar_h, bar_x0."""
    ks, ko = (None, None) if x2k is None else x2k
    rh = _gemm(skip, W_skip, b_skip, ks, act="relu", pro="div", pro_param=math.sqrt(L))
    ro = _gemm(rh["y"], W_out, b_out, ko)
    prop = torch.einsum("oc,bct->bot", W_out[:, :, 0].double().abs(), rh["bar"])
    return dict(h=rh["y"], x0=ro["y"], S_h=rh["S"], S_out=ro["S"], bar_h=rh["bar"], prop=prop, bar_x0=ro["bar"] + prop, rh=rh, ro=ro)


def posterior(x0, x_t, coef4, eps, bar_x0=None):
    """x' = c1 x0 + c2 x_t + sigma eps, sigma = nonzero exp(logvar / 2); coef4 = the fp32 {c1, c2, logvar, nonzero}.  dict y, sigma, bar."""
    c1, c2, lv, nz = (float(v) for v in coef4.double())
    sigma = nz * math.exp(0.5 * lv)
    a, b, c = c1 * x0.double(), c2 * x_t.double(), sigma * eps.double()
    bar = 4 * U * (a.abs() + b.abs() + c.abs()) + 64 * U * (1 + abs(0.5 * lv)) * c.abs()
    if bar_x0 is not None:
        bar = bar + abs(c1) * bar_x0
    return dict(y=a + b + c, sigma=sigma, bar=bar)


def loop(o, steps=None, noise=None):
    """The reverse loop on the operands `o` (make_exact / make_gauss): (x after the last step, per-step trace of xin, skip, x0, x)."""
    steps = o["steps"] if steps is None else steps
    noise = o["noise"] if noise is None else noise
    x, trace = o["x_T"].double(), []
    for k in range(steps):
        sid = steps - 1 - k  # spec_denoiser.py:181: reversed(range(steps))
        xin = in_proj(x, o["W_in"], o["b_in"])["y"]
        xL, skip = layers(xin, o["cp"], o["dstep"][:, sid], o["Wd"], o["bd"], o["Wo"], o["bo"], o["dcl"])
        x0 = head(skip, o["L"], o["W_skip"], o["b_skip"], o["W_out"], o["b_out"])["x0"]
        x = posterior(x0, x, o["coef4"][sid], noise[k].reshape(x.shape))["y"]
        trace.append(dict(xin=xin, xL=xL, skip=skip, x0=x0, x=x))
    return x, trace


# ------------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------------
def fusable(M, T):
    """boundary_fusable (csrc/boundary.hip) without its environment switch."""
    return T % 4 == 0 and 2 <= M <= 96


def _row(B, M, T, fused, why, **kw):
    return dict(name="B%d_M%d_T%d" % (B, M, T), B=B, M=M, T=T, fused=fused, why=why, **kw)


# steps = 1 (the last-step branch: xin_next == NULL).  rbn = ceil(M / 32) waves run GEMM 3, MP = ceil16(M) rows of the x' tile,
# T % 64 = frames of the last tile.  `small`: 4 B ceil(T / 32) blocks fit the row-split kernel on any chip this runs on.
BOUNDARY = [
    _row(1, 2, 4, True, "rbn 1 (waves 1-2 idle), MP 16 with 14 padding rows, M % 16 != 0; T < 64 with ONE quad: every clamped load reads t = 3", small=True),
    _row(3, 2, 68, True, "rbn 1; T % 64 = 4: second tile holds one quad, grid.y = 3", small=True),
    _row(1, 16, 36, True, "rbn 1, MP 16 = M (no padding row); T < 64, T % 64 = 36: second column block holds one quad", small=True),
    _row(1, 16, 96, True, "rbn 1; T % 64 = 32: second column block of the last tile entirely past T", small=True),
    _row(3, 17, 60, True, "rbn 1, MP 32, M % 16 = 1 (15 padding rows, bias clamp min(row, 16)); T % 64 = 60: one quad missing", small=True),
    _row(1, 17, 64, True, "rbn 1, MP 32; T % 64 = 0, one full tile", small=True),
    _row(1, 32, 100, True, "rbn 1 at its last M, MP 32 = M; T % 64 = 36 in the second tile", small=True),
    _row(3, 32, 4, True, "rbn 1; T = 4, grid.y = 3", small=True),
    _row(1, 33, 128, True, "rbn 2 (wave 2 idle) at its first M, MP 48, M % 16 = 1, ngin 4; T % 64 = 0, two full tiles", small=True),
    _row(1, 33, 36, True, "rbn 2, MP 48; T < 64", small=True),
    _row(1, 64, 132, True, "rbn 2 at its last M, MP 64 = M; T % 64 = 4 in the third tile", small=True),
    _row(3, 64, 96, True, "rbn 2; T % 64 = 32, grid.y = 3", small=True),
    _row(1, 80, 64, True, "rbn 3, MP 80 (the shipped mel_bins); T % 64 = 0", small=True),
    _row(3, 80, 100, True, "rbn 3; T % 64 = 36, grid.y = 3", small=True),
    _row(1, 95, 68, True, "rbn 3, MP 96, M % 16 = 15 (ONE padding row, bias clamp min(95, 94)); T % 64 = 4", small=True),
    _row(1, 95, 60, True, "rbn 3, MP 96; T % 64 = 60", small=True),
    _row(1, 96, 96, True, "rbn 3, MP 96 = M: the last fusable M, no padding row in either kernel; T % 64 = 32", small=True),
    _row(3, 96, 132, True, "rbn 3, MP 96; T % 64 = 4 in the third tile, grid.y = 3", small=True),
    _row(1, 96, 4, True, "rbn 3; T = 4", small=True),
    _row(1, 2, 128, True, "rbn 1, 94 zero rows of the x2 kernel's 96-row tile; two full tiles", small=True),
    _row(1, 17, 132, True, "MP 32, M % 16 != 0 with three tiles", small=True),
    # unfused: boundary_fusable is false, the three conv launches and set_posterior_step run
    _row(1, 1, 64, False, "M = 1 < 2: unfused"),
    _row(1, 97, 64, False, "M = 97 > 96: unfused"),
    _row(1, 80, 5, False, "T % 4 = 1: unfused"),
    _row(3, 33, 66, False, "T % 4 = 2, M T % 4 = 2: unfused, Philox quads straddle utterances"),
]
# steps = 2 (the non-last branch: phase 5 runs at the first boundary): every MP / ngin, M % 16 != 0, every T % 64 class
PHASE5 = [r for r in BOUNDARY if r["name"] in ("B1_M2_T4", "B1_M16_T36", "B3_M17_T60", "B1_M17_T64", "B1_M32_T100", "B1_M33_T128",
                                                "B1_M64_T132", "B3_M64_T96", "B3_M80_T100", "B1_M95_T68", "B1_M96_T96", "B3_M96_T132")]
# end to end against loop(): (name, B, M, T, L, steps, dcl)
LOOP = [
    dict(name="s1_L2_d1", B=2, M=80, T=68, L=2, steps=1, dcl=1, why="steps == 1: no non-last boundary at all"),
    dict(name="s2_L3_d2", B=2, M=33, T=100, L=3, steps=2, dcl=2, why="sid 1, 0; dilations 1, 2, 1; L odd: x_L in ws_x1"),
    dict(name="s3_L2_d2", B=3, M=80, T=132, L=2, steps=3, dcl=2, why="sid 2, 1, 0: dstep + sid with d_cs = 3, coef4 + 4 sid, noise slice k"),
    dict(name="s3_L3_d1_unfused", B=2, M=97, T=66, L=3, steps=3, dcl=1, why="the unfused boundary over three steps"),
]
# utterance groups: b0 = floor(B g / G); n_groups 8 is clamped to B; per_batch % 4 != 0 forces G = 1
GROUPS = [
    dict(name="B3", B=3, M=80, T=68, L=2, steps=2, dcl=1, groups=(1, 2, 3, 8), why="B 3: groups of 1 + 2, 1 + 1 + 1, 8 -> 3"),
    dict(name="B5", B=5, M=17, T=36, L=2, steps=2, dcl=1, groups=(1, 2, 3, 8), why="B 5: groups of 2 + 3, 1 + 2 + 2, 8 -> 5 (uneven splits)"),
    dict(name="B3_odd", B=3, M=33, T=66, L=2, steps=2, dcl=1, groups=(1, 3), why="M T % 4 = 2: one group whatever n_groups says, unfused"),
]


def _seed(name, tag):
    return zlib.crc32(("%s/%s" % (name, tag)).encode()) & 0x7FFFFFFF


def step_tables(g, L, steps, exact):
    """dstep [L*256][steps] and coef4 [steps][4] whose columns / rows differ strongly from step to step, so that a wrong sid moves the
    result by orders of magnitude more than any bar."""
    if exact:
        dstep = ints(g, (L * DC, steps), -2, 2)
        # row 0 (the last step) takes x' of the step before it as x_t: c2 = 2 keeps c2 x' on the 2^-7 grid
        rows = [(1.0, 2.0, 0.0, 1.0), (1.0, 2.0 ** -4, 0.0, 1.0), (0.5, 2.0 ** -6, 0.0, 0.0)]
    else:
        dstep = torch.randn(L * DC, steps, generator=g) * (1.0 + torch.arange(steps).float())[None, :]
        rows = [(0.3, 0.9, -2.5, 0.0), (1.7, -0.4, -0.7, 1.0), (-0.6, 1.3, 0.4, 1.0)]
    return dstep, torch.tensor([rows[s % 3] for s in range(steps)], dtype=torch.float32)


def make_exact(c, steps=1, L=4, tag="exact"):
    """Operands of an exact-mode case (see the module docstring) and `skip_want`, the skip sum the model predicts for every step."""
    g = torch.Generator().manual_seed(_seed(c["name"], tag))
    B, M, T = c["B"], c["M"], c["T"]
    sparse = lambda shape, lo, hi, p: ints(g, shape, lo, hi) * (torch.rand(shape, generator=g) < p).float()
    o = dict(B=B, M=M, T=T, L=L, steps=steps, dcl=1, mode="exact")
    o["W_in"], o["b_in"] = ints(g, (DC, M, 1), -1, 1), ints(g, (DC,), -4, 4)
    o["W_skip"], o["b_skip"] = sparse((DC, DC, 1), -1, 1, 0.25), ints(g, (DC,), -8, 8)
    o["W_out"], o["b_out"] = sparse((M, DC, 1), -1, 1, 0.25), ints(g, (M,), -8, 8)
    o["Wd"], o["bd"] = torch.zeros(L, 512, DC, 3), torch.zeros(L, 512)
    den = 128 // math.isqrt(L)  # the skip sum / sqrt(L) lands on the grid of integers / 128 (L is 1 or 4)
    o["Wo"], o["bo"] = ints(g, (L, 512, DC, 1), -1, 1), ints(g, (L, 512), -3 * den, 3 * den) / den
    sign = (torch.randint(0, 2, (B, L, DC, T), generator=g) * 2 - 1).float()
    cp = torch.full((B, L, 512, T), 40.0)
    cp[:, :, DC:] = 40.0 * sign
    o["cp"] = cp.reshape(B, L * 512, T).contiguous()
    o["dstep"], o["coef4"] = step_tables(g, L, steps, True)
    o["x_T"], o["noise"] = ints(g, (B, M, T), -3, 3), ints(g, (steps, B, M, T), -3, 3)
    o["skip_want"] = sum(torch.einsum("oc,bct->bot", o["Wo"][l, DC:, :, 0].double(), sign[:, l].double()) +
                         o["bo"][l, DC:].double()[None, :, None] for l in range(L))
    return o


def make_gauss(c, scale, steps=1, L=1, dcl=1, tag="gauss"):
    """Gaussian operands (the _random_stack recipe for the layers); scale 1: unit activations, scale 8: the skip side 8 x larger."""
    g = torch.Generator().manual_seed(_seed(c["name"], "%s%g" % (tag, scale)))
    B, M, T = c["B"], c["M"], c["T"]
    rn = lambda *s: torch.randn(*s, generator=g)
    o = dict(B=B, M=M, T=T, L=L, steps=steps, dcl=dcl, mode="bounded")
    o["W_in"], o["b_in"] = rn(DC, M, 1) / math.sqrt(M), rn(DC) * 0.1
    o["W_skip"], o["b_skip"] = rn(DC, DC, 1) / 16, rn(DC) * 0.1
    o["W_out"], o["b_out"] = rn(M, DC, 1) / 16, rn(M) * 0.1
    o["Wd"], o["bd"] = rn(L, 512, DC, 3) / 27.7, rn(L, 512) * 0.1
    o["Wo"], o["bo"] = rn(L, 512, DC, 1) / 16 * scale, rn(L, 512) * 0.1
    o["cp"] = rn(B, L * 512, T) * 0.5
    o["dstep"], o["coef4"] = step_tables(g, L, steps, False)
    o["x_T"], o["noise"] = rn(B, M, T) * math.sqrt(scale), rn(steps, B, M, T)
    return o


def one_step_of(o, sid, k):
    """The companion steps = 1 operands of a longer loop: column sid of its tables, noise slice k."""
    c = dict(o)
    c.update(steps=1, dstep=o["dstep"][:, sid:sid + 1].contiguous(), coef4=o["coef4"][sid:sid + 1].contiguous(), noise=o["noise"][k:k + 1].contiguous())
    if "skip_want" in o:
        c["skip_want"] = o["skip_want"]
    return c


def phase5_form(o):
    """Zero the residual half of the single layer's output conv: the stack then returns x_L = xin * RSQRT2 with one rounding."""
    assert o["L"] == 1
    o["Wo"][:, :DC] = 0
    o["bo"][:, :DC] = 0
    return o


def x2_exponent(w):
    """ops._x2_exponent without the package: max |w| 2^k lands in [8, 16)."""
    m = float(w.abs().max())
    return max(-60, min(60, 4 - math.frexp(m)[1])) if m > 0 and math.isfinite(m) else 0


def x2_exponents(o):
    return (x2_exponent(o["W_skip"]), x2_exponent(o["W_out"])), x2_exponent(o["W_in"])


# ------------------------------------------------------------------------------------------------------------------------
# CPU checks
# ------------------------------------------------------------------------------------------------------------------------
def test_posterior_equals_the_python_formula_in_float64():
    """spec_denoiser.py:86-101 evaluated in float64 (oracle.q_posterior_sample on float64 tables), nonzero = 0 (t == 0) included."""
    from oracle import oracle as O
    g = torch.Generator().manual_seed(5)
    steps = 4
    tab = {k: torch.randn(steps, generator=g, dtype=torch.float64) for k in ("posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped")}
    x0, xt, eps = (torch.randn(2, 1, 7, 9, generator=g, dtype=torch.float64) for _ in range(3))
    for t in range(steps):
        coef4 = torch.stack([tab["posterior_mean_coef1"][t], tab["posterior_mean_coef2"][t], tab["posterior_log_variance_clipped"][t],
                             torch.tensor(float(t != 0), dtype=torch.float64)])
        want = O.q_posterior_sample(tab, x0, xt, torch.full((2,), t, dtype=torch.long), eps)
        r = posterior(x0, xt, coef4, eps)
        assert float((r["y"] - want).abs().max()) <= 1e-14 * float(want.abs().max())
        assert (r["sigma"] == 0.0) == (t == 0)
        if t == 0:
            assert torch.equal(r["y"], coef4[0] * x0 + coef4[1] * xt)


def test_model_equals_the_oracle_reverse_loop_in_float64():
    """loop() on the infer_tiny golden inputs against oracle.p_sample_loop, both in float64 on the same conditioner output."""
    from oracle import oracle as O
    from oracle import weights as Wt
    m = load_golden("infer_tiny")["meta"]
    W = Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), m["wseed"])
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=m["pad_tail"])
    noises = Wt.synthetic_noises(m["B"], m["T"], m["steps"], seed=m["iseed"] + 1)
    _, cond = O.conditioner(W, inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"],
                            **m["flags"])
    steps, dcl = m["steps"], m["overrides"].get("dilation_cycle_length", 1)
    W64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    tab = {k: v.double() for k, v in O.diffusion_tables(steps)[0].items()}
    n64 = [n.double() for n in noises]
    want = O.p_sample_loop(W64, tab, cond.double(), n64, steps, dcl)[:, 0]
    p = "denoise_fn."
    L = 0
    while (p + "residual_layers.%d.dilated_conv.weight" % L) in W:
        L += 1
    lw = lambda l, n: W64[p + "residual_layers.%d.%s" % (l, n)]
    emb = O.step_embedding(W64, torch.arange(steps), p)  # [steps][C]
    o = dict(L=L, steps=steps, dcl=dcl, x_T=n64[0][:, 0], noise=torch.stack([n[:, 0] for n in n64[1:]]),
             W_in=W64[p + "input_projection.weight"], b_in=W64[p + "input_projection.bias"],
             W_skip=W64[p + "skip_projection.weight"], b_skip=W64[p + "skip_projection.bias"],
             W_out=W64[p + "output_projection.weight"], b_out=W64[p + "output_projection.bias"],
             Wd=[lw(l, "dilated_conv.weight") for l in range(L)], bd=[lw(l, "dilated_conv.bias") for l in range(L)],
             Wo=[lw(l, "output_projection.weight") for l in range(L)], bo=[lw(l, "output_projection.bias") for l in range(L)],
             cp=torch.cat([F.conv1d(cond.double(), lw(l, "conditioner_projection.weight"), lw(l, "conditioner_projection.bias")) for l in range(L)], 1),
             dstep=torch.cat([F.linear(emb, lw(l, "diffusion_projection.weight"), lw(l, "diffusion_projection.bias")).t() for l in range(L)], 0),
             coef4=torch.stack([tab["posterior_mean_coef1"][:steps], tab["posterior_mean_coef2"][:steps], tab["posterior_log_variance_clipped"][:steps],
                                (torch.arange(steps) != 0).double()], -1))
    got, trace = loop(o)
    assert len(trace) == steps and got.shape == want.shape
    # float64 on both sides; the model divides by the fp32 sqrt(L) as the kernels do (relative 3e-8 of the head's input)
    assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max())), float((got - want).abs().max())


def _classes(c):
    M, T = c["M"], c["T"]
    return dict(rbn=-(-M // 32), MP=-(-M // 16) * 16, ragged=M % 16 != 0, tail=T % 64, short=T < 64, ngin=2 * -(-M // 32))


def test_inventory_is_complete():
    """Every branch value the sweep claims is reached by a fused row of BOUNDARY and of PHASE5 (both boundary kernels run every fused row,
    with explicit eps and with Philox, see the GPU module), and the fusable predicate is false for exactly the rows marked unfused."""
    for c in BOUNDARY:
        assert fusable(c["M"], c["T"]) == c["fused"], c["name"]
    assert {c["M"] for c in BOUNDARY if not c["fused"]} >= {1, 97} and {c["T"] % 4 for c in BOUNDARY if not c["fused"] and 2 <= c["M"] <= 96} >= {1, 2}
    assert len({c["name"] for c in BOUNDARY}) == len(BOUNDARY) and all(c["why"] for c in BOUNDARY + LOOP + GROUPS)
    for table, name in ((BOUNDARY, "BOUNDARY"), (PHASE5, "PHASE5")):
        fused = [_classes(c) for c in table if c["fused"]]
        assert {k["rbn"] for k in fused} == {1, 2, 3}, name
        assert {k["MP"] for k in fused} == {16, 32, 48, 64, 80, 96}, name
        assert {k["ngin"] for k in fused} == {2, 4, 6}, name
        assert {k["ragged"] for k in fused} == {False, True}, name
        assert {k["tail"] for k in fused} >= {0, 4, 32, 36, 60}, name
        assert {k["short"] for k in fused} == {False, True}, name
        assert {c["B"] for c in table if c["fused"]} >= {1, 3}, name
        # the padding-row extremes: one padding row and fifteen, and the last fusable M
        assert {c["M"] % 16 for c in table if c["fused"]} >= {0, 1, 15} and 96 in {c["M"] for c in table}, name
    assert {c["M"] for c in BOUNDARY if c["fused"]} == {2, 16, 17, 32, 33, 64, 80, 95, 96}
    assert {c["T"] for c in BOUNDARY if c["fused"]} == {4, 36, 60, 64, 68, 96, 100, 128, 132}
    assert {c["steps"] for c in LOOP} == {1, 2, 3} and {c["L"] for c in LOOP} == {2, 3} and {c["dcl"] for c in LOOP} == {1, 2}
    assert {fusable(c["M"], c["T"]) for c in LOOP} == {False, True}
    assert {c["B"] for c in GROUPS} == {3, 5} and any((c["M"] * c["T"]) % 4 for c in GROUPS)
    for c in GROUPS:  # uneven splits: some G gives groups of different sizes
        sizes = {tuple((c["B"] * (g + 1)) // min(G, c["B"]) - (c["B"] * g) // min(G, c["B"]) for g in range(min(G, c["B"]))) for G in c["groups"]}
        assert c["name"] == "B3_odd" or any(len(set(s)) > 1 for s in sizes), c["name"]
    assert all(max(c["B"] for c in t) <= 5 and max(c["T"] for c in t) <= 132 for t in (BOUNDARY, LOOP, GROUPS))


def _on_grid(v):
    return bool(((v.double() / Q).round() * Q == v.double()).all()) and bool((v.double().float().double() == v.double()).all())


def _fp32(v):
    return bool((v.double().float().double() == v.double()).all())


@pytest.mark.parametrize("c", [c for c in BOUNDARY if c["fused"]], ids=lambda c: c["name"])
def test_exact_inputs_meet_their_budget(c):
    """The exact-mode operands fed forward as the loop feeds them (step k: row sid = steps-1-k, noise slice k, x_t = x' of the step
    before): s, h, x0, every x' and the xin of every non-last boundary are multiples of 2^-7 and fp32 numbers; every product and partial
    sum of the posterior (c1 x0, c2 x_t, their sum, + eps) is an fp32 number; every sum of magnitudes is below 2^24 granules (fp32 kernel:
    any order is exact); the piece products of the two-piece kernel are within BUDGET_BITS with exact splits and nothing in the dropped
    product; every split operand stays below 32768; the low pieces are not all zero."""
    for o in (make_exact(c), phase5_form(make_exact(c, steps=2, L=1, tag="exact5"))):
        kh, kin = x2_exponents(o)
        skip, steps = o["skip_want"], o["steps"]
        assert _on_grid(skip / math.sqrt(o["L"]))
        hd = head(skip.float(), o["L"], o["W_skip"], o["b_skip"], o["W_out"], o["b_out"], kh)  # the same at every step: Wd = 0
        for name, v, S, r in (("h", hd["h"], hd["S_h"], hd["rh"]), ("x0", hd["x0"], hd["S_out"], hd["ro"])):
            assert _on_grid(v) and float(S.max()) < 2.0 ** 24 * Q, (c["name"], name, float(S.max()))
        x = o["x_T"].double()
        for k in range(steps):
            sid = steps - 1 - k
            c1, c2 = float(o["coef4"][sid][0]), float(o["coef4"][sid][1])
            p = posterior(hd["x0"], x, o["coef4"][sid], o["noise"][k])
            a, b = c1 * hd["x0"], c2 * x
            assert _fp32(a) and _fp32(b) and _fp32(a + b) and _fp32(p["y"]) and p["sigma"] == 1.0, (c["name"], k)
            assert _on_grid(p["y"]), (c["name"], k)
            assert float((a.abs() + b.abs() + o["noise"][k].double().abs()).max()) < 2.0 ** 24 * Q, (c["name"], k)
            gemms = [("h", hd["rh"]), ("x0", hd["ro"])]
            if k + 1 < steps:  # phase 5 runs: the next step's input projection, then split by the next step's stack
                xi = in_proj(p["y"].float(), o["W_in"], o["b_in"], kin)
                assert _on_grid(xi["y"]) and float(xi["S"].max()) < 2.0 ** 24 * Q, (c["name"], k, float(xi["S"].max()))
                assert float(xi["y"].abs().max()) < 32768.0 and xi["x2"]["lo_x"] > 0.02, c["name"]
                gemms.append(("xin", xi))
            for name, r in gemms:
                m = r["x2"]
                assert m["bits"] < BUDGET_BITS and m["split_exact"] and not bool(m["dropped"].any()), (c["name"], name, m["bits"])
                assert torch.equal(m["y"], r["y"]), (c["name"], name)
                assert m["amax"] < 32768.0, (c["name"], name, m["amax"])
            x = p["y"]
        assert hd["rh"]["x2"]["lo_x"] > 0.02 and hd["ro"]["x2"]["lo_x"] > 0.02, c["name"]
        assert float(skip.std()) > 4.0 and skip.unique().numel() > 100  # varies with (b, channel, t)
