"""GPU branch sweep of the two-piece fp16 conv family: conv1d_x2_kernel (SET_IMPL_F16X2, csrc/conv_x2.hip), its PHASES
instantiation behind set_conv_transpose1d_x2 with pack_conv_x2_kernel's phase addressing, and resblock_pair_x2_kernel
(csrc/resblock_x2.hip) -- every path the launch code picks by shape, stride or alignment, as ONE kernel call against the piece model
of tests/test_conv_x2_reference.py (where the case tables live, each case naming the branch it reaches and the C condition it meets,
and where the CPU half of the argument runs).  Same shape as tests/test_gpu_conv_branches.py: the output view lives inside a larger
buffer filled with a sentinel (or the previous output when accumulating) and the WHOLE buffer is compared; operands are checked
unchanged after the call.  Two modes per case:
  exact    inputs on the two-piece grid a + sign(a) b 2^-12 (non-trivial low pieces in a third of the operands, no rounding in either
           split), per-case budget sum |piece products| < 2^24 granules asserted on the CPU: the kernel must equal the float64 sum of
           the products a1 b0 + a0 b1 + a0 b0 BIT FOR BIT -- a lost cross product, a low piece paired with the wrong tap or channel, a
           piece taken before the prologue or a wrong 2^-k shows in the last bit, a misplaced store in the buffer around the view.
  bounded  Gaussian inputs, every element within the derived bar conv_x2_bound of the TRUE float64 convolution, zero outside the
           written set, and beside it the criterion of tests/test_gpu_x2conv.py: largest error against float64 at most 1.5 x that of
           the fp32 MFMA path on the same call + 1e-7.
Transcendental activations run `bounded` only.  A ResBlock pair is in addition bit-identical to the two f16x2 conv launches it
replaces on the whole buffer in both modes; in `exact` mode its first GEMM runs on the grid and its second on a one-piece selection
weight (make_pair says why), in `bounded` mode the float64 bar is the 1e-5 max |y| of test_fused_resblock_pair_equals_two_convs.

The two hardware assumptions of `exact` (test_conv_x2_reference.py) both HELD on the MI355X: every exact case whose budget is below
2^24 granules is bit-identical to the piece model, test_mfma_adds_without_losing_a_bit places one granule against an accumulator just
below 2^24 granules inside one MFMA and across two, and the pair's re-split intermediate (fp16 rounding ties included) follows
round-to-nearest-even.  The budget is therefore the full 24 bits.

Not swept, on purpose: the 2 GiB guards of the three entry points.  A refusal test must stay harmless if the refusal fails to trigger,
and no operand of that size is valid here; they are left to a reading of the code."""
import ctypes as C

import pytest
import torch

from test_conv_x2_reference import CONV, CONVT, PAIR, POLY, conv_x2_ref, make_conv, make_convt, make_pair, x2_exponent
from test_gpu_conv_branches import (E_INVALID, E_UNSUPPORTED, SENTINEL, _ALIVE, _L, _embed, _keep_launch_operands, _p, _report, _run,  # noqa: F401
                                    _s, dev)

pytestmark = pytest.mark.gpu

BIG = 5.0e4  # what surrounds a strided x: outside the fp16 range of the splitting -- it may neither change a result nor raise the flag


def _flag(reset=True):
    from set_amd import ops
    return ops.conv_x2_range_flag(reset=reset)


# ------------------------------------------------------------------------------------------------------------------------
# generic conv
# ------------------------------------------------------------------------------------------------------------------------
def _run_raw(o, impl, dev):
    """The call with `in` as a strided view (ops.conv1d has no input strides): SetConv1dArgs filled by hand."""
    from set_amd import _lib, ops
    B, Cin, T_in = o["x"].shape
    x_buf, x_view = _embed((B, Cin, T_in), o["x_emb"], BIG, None)
    x_view(x_buf).copy_(o["x"])
    xd, wd = x_buf.to(dev), o["wstore"].to(dev)
    cw = ops.ConvWeight(wd, o["Cout"], Cin, o["K"], **o["waddr"])
    out_buf = o["out_buf"].to(dev)
    res_buf = o["res_buf"].to(dev) if o["res_buf"] is not None else None
    kw = o["kw"]
    t = lambda v: None if v is None else v.to(dev)
    bias, mask = t(o["bias_t"]), t(o["mask_t"])
    out, res = o["out_view"](out_buf), None if res_buf is None else o["res_view"](res_buf)
    img = cw.packed_x2() if impl == "f16x2" else cw.packed()
    a = _lib.SetConv1dArgs()
    a.inp = _p(xd) + 4 * o["x_emb"][2]
    a.w, a.bias, a.mask = _p(img), _p(bias), _p(mask)
    a.res = None if res is None else res.data_ptr()
    a.out = out.data_ptr()
    _ALIVE.extend([out_buf, res_buf, wd])
    a.in_bs, a.in_cs = o["x_emb"][0], o["x_emb"][1]
    a.out_bs, a.out_cs = out.stride(0), out.stride(1)
    if res is not None:
        a.res_bs, a.res_cs = res.stride(0), res.stride(1)
    a.w_base, a.w_sco, a.w_sci, a.w_stap = cw.base, cw.sco, cw.sci, cw.stap
    a.B, a.Cin, a.Cout, a.K, a.dil, a.pad = B, Cin, o["Cout"], o["K"], kw["dil"], kw["pad"]
    a.T_in, a.T_iter, a.T_out, a.out_stride, a.out_off = T_in, kw["T_iter"], kw["T_out"], kw["out_stride"], kw["out_off"]
    a.pro, a.act, a.accumulate = _lib.PRO[kw["pro"]], _lib.ACT[kw["act"]], int(kw["accumulate"])
    a.impl = _lib.IMPL_F16X2 if impl == "f16x2" else _lib.IMPL_MFMA
    a.pro_param, a.act_param, a.alpha, a.out_div = kw["pro_param"], kw["act_param"], kw["alpha"], kw["out_div"]
    _lib.check(_L().set_conv1d(C.byref(a), _s()), "set_conv1d")
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x_buf)  # operands are read-only
    if res_buf is not None:
        assert torch.equal(res_buf.cpu(), o["res_buf"])
    return out_buf.cpu()


def _conv(o, impl, dev):
    return _run_raw(o, impl, dev) if o["x_emb"] is not None else _run(o, impl, dev)


def _worst(got, o):
    return float((got.double() - o["want"]).abs().max())


CONV_RUNS = [(c, mode) for c in CONV for mode in c["modes"]]


@pytest.mark.parametrize("c,mode", CONV_RUNS, ids=["%s-%s" % (c["name"], mode) for c, mode in CONV_RUNS])
def test_x2_conv_branch(dev, c, mode):
    o = make_conv(c, mode)
    assert 0 < o["written"] <= c["B"] * c["Cout"] * c["T_out"]
    _flag()
    got = _conv(o, "f16x2", dev)
    assert not _flag()  # nothing in the view leaves the fp16 range (and the 5e4 around a strided x is not in the view)
    bad = _report(c["name"], "f16x2", got, o["want"], o["bar"])
    # exact: the bar is zero everywhere; bounded: zero outside the reference's written set
    assert bad.numel() == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), o["want"][bad[:8]].tolist())
    assert bool(torch.isfinite(got).all())
    if mode == "bounded":
        e2, e32 = _worst(got, o), _worst(_conv(o, "mfma", dev), o)
        print("%s: max err vs float64: fp32 MFMA kernel %.3e, f16x2 kernel %.3e" % (c["name"], e32, e2))
        assert e2 <= 1.5 * e32 + 1e-7


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("cfg", POLY, ids=["%dto%d_k%d_u%d" % c[:4] for c in POLY])
def test_polyphase_calls_on_f16x2_fill_one_buffer(dev, cfg, mode):
    """The calls ops.conv_transpose1d issues for one ConvTranspose1d with impl="f16x2" (out_stride u, every out_off), all phases into
    ONE sentinel-filled buffer: together they are the transposed convolution, and no phase touches another's samples or the guard."""
    from set_amd import ops
    Cin, Cout, k, u, P, T = cfg
    o = make_convt(("poly_%dto%d_k%d_u%d" % cfg[:4], 2, Cin, Cout, k, u, P, T, True, "lrelu"), mode)
    buf = torch.full((o["want"].numel(),), SENTINEL, device=dev)
    out = buf[:2 * Cout * o["T_out"]].view(2, Cout, o["T_out"])
    xd, wd, bd = o["x"].to(dev), o["wt"].to(dev), o["bias_t"].to(dev)
    _flag()
    got = {}
    for impl in ("f16x2", "mfma") if mode == "bounded" else ("f16x2",):
        buf.fill_(SENTINEL)
        y = ops.conv_transpose1d(xd, wd, bd, Cin, Cout, k, u, P, pro="lrelu", pro_param=o["pro_param"], impl=impl, cache={})
        assert y.shape == out.shape
        for p in range(u):  # the same calls, into the guarded buffer
            J = (k - p + u - 1) // u
            cw = ops.ConvWeight(wd, Cout, Cin, J, base=p, sco=k, sci=Cout * k, stap=u)
            ops.conv1d(xd, cw, bd, dil=-1, pad=0, pro="lrelu", pro_param=o["pro_param"], out=out, impl=impl, T_iter=T + J - 1, T_out=o["T_out"],
                       out_stride=u, out_off=p - P)
        torch.cuda.synchronize()
        got[impl] = buf.cpu()
        assert torch.equal(got[impl][:y.numel()], y.cpu().reshape(-1))
    assert not _flag()
    bad = _report(o["name"], "f16x2", got["f16x2"], o["want"], o["bar"])
    assert bad.numel() == 0, (bad[:8].tolist(), got["f16x2"][bad[:8]].tolist(), o["want"][bad[:8]].tolist())
    if mode == "bounded":
        assert _worst(got["f16x2"], o) <= 1.5 * _worst(got["mfma"], o) + 1e-7


# ------------------------------------------------------------------------------------------------------------------------
# all-phase transposed conv
# ------------------------------------------------------------------------------------------------------------------------
def _convt_raw(o, dev):
    """set_pack_conv_transpose_x2 + set_conv_transpose1d_x2 through the raw ABI; `out` is contiguous (the entry point takes no strides)
    and sits at the head of a sentinel-filled buffer with a guard behind it.  Returns the whole buffer."""
    from set_amd import _lib
    B, Cin, Cout, k, u, P, T_in = (o[n] for n in ("B", "Cin", "Cout", "k", "u", "P", "T_in"))
    xd, wd = o["x"].to(dev), o["wt"].to(dev)
    bd = None if o["bias_t"] is None else o["bias_t"].to(dev)
    wp = torch.empty(_L().set_packed_conv_transpose_x2_size(Cout, Cin, k, u), dtype=torch.float16, device=dev)
    _lib.check(_L().set_pack_conv_transpose_x2(_p(wd), _p(wp), Cout, Cin, k, u, o["k_exp"], _s()), "set_pack_conv_transpose_x2")
    buf = torch.full((o["want"].numel(),), SENTINEL, device=dev)
    assert buf.numel() >= B * Cout * o["T_out"] + 64
    _lib.check(_L().set_conv_transpose1d_x2(_p(xd), _p(wp), _p(bd), _p(buf), B, Cin, Cout, k, u, P, T_in, _lib.PRO[o["pro"]], float(o["pro_param"]),
                                            _s()), "set_conv_transpose1d_x2")
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), o["x"]) and torch.equal(wd.cpu(), o["wt"])
    return buf.cpu()


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("case", CONVT, ids=[c[0] for c in CONVT])
def test_x2_transposed_conv_branch(dev, case, mode):
    from set_amd import ops
    o = make_convt(case, mode)
    _flag()
    got = _convt_raw(o, dev)
    assert not _flag()
    bad = _report(case[0], "convT f16x2", got, o["want"], o["bar"])
    assert bad.numel() == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), o["want"][bad[:8]].tolist())
    if mode == "bounded":  # the fp32 path: one strided-output conv per phase
        name, B, Cin, Cout, k, u, P, T_in, _, pro = case
        bd = None if o["bias_t"] is None else o["bias_t"].to(dev)
        y32 = ops.conv_transpose1d(o["x"].to(dev), o["wt"].to(dev), bd, Cin, Cout, k, u, P, pro=pro, pro_param=o["pro_param"], impl="mfma", cache={})
        e2, e32 = _worst(got, o), float((y32.double().cpu() - o["yd"]).abs().max())
        print("%s: max err vs float64: fp32 polyphase %.3e, all-phase f16x2 %.3e" % (name, e32, e2))
        assert e2 <= 1.5 * e32 + 1e-7


def test_split_scope_sends_a_transposed_conv_to_the_all_phase_kernel(dev):
    """ops.conv_transpose1d inside split_convs() (Cin >= 32, u Cout >= 32, T_in >= 64, k >= u): the all-phase launch, bit for bit the raw
    call above; outside the scope, and for T_in 63 inside it, the polyphase calls."""
    from set_amd import ops
    case = next(c for c in CONVT if c[0] == "u2_P1_edges_T128")
    o = make_convt(case, "exact")
    name, B, Cin, Cout, k, u, P, T_in, _, pro = case
    xd, wd, bd = o["x"].to(dev), o["wt"].to(dev), o["bias_t"].to(dev)
    cache = {}
    with ops.split_convs():
        y = ops.conv_transpose1d(xd, wd, bd, Cin, Cout, k, u, P, pro=pro, pro_param=o["pro_param"], cache=cache)
    assert "x2" in cache and not [p for p in cache if p != "x2"]
    n = B * Cout * o["T_out"]
    assert torch.equal(y.cpu().reshape(-1).double(), o["want"][:n])
    cache = {}
    ops.conv_transpose1d(xd, wd, bd, Cin, Cout, k, u, P, pro=pro, pro_param=o["pro_param"], cache=cache)
    assert "x2" not in cache and sorted(cache) == list(range(u))
    cache = {}
    with ops.split_convs():
        ops.conv_transpose1d(xd[:, :, :63].contiguous(), wd, bd, Cin, Cout, k, u, P, pro=pro, pro_param=o["pro_param"], cache=cache)
    assert "x2" not in cache
    assert not _flag()


# ------------------------------------------------------------------------------------------------------------------------
# ResBlock pair
# ------------------------------------------------------------------------------------------------------------------------
def _pair_fused(o, dev, cw1, cw2, b1, b2):
    """ops.resblock_pair, or the raw ABI when x is a strided view.  Returns the whole out buffer."""
    from set_amd import _lib, ops
    B, Cc, T = o["x"].shape
    out_buf = o["out_buf"].to(dev)
    out = o["out_view"](out_buf)
    if o["x_emb"] is None:
        xd = o["x"].to(dev)
        ops.resblock_pair(xd, cw1, b1, cw2, b2, o["dil"], slope=o["slope"], out=out, accumulate=o["accumulate"], out_div=o["out_div"])
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu(), o["x"])
        return out_buf.cpu()
    x_buf, x_view = _embed((B, Cc, T), o["x_emb"], BIG, None)
    x_view(x_buf).copy_(o["x"])
    xd = x_buf.to(dev)
    a = _lib.SetResblockPairArgs()
    a.x, a.out = _p(xd) + 4 * o["x_emb"][2], out.data_ptr()
    a.w1, a.w2 = _p(cw1.packed_x2()), _p(cw2.packed_x2())
    a.b1, a.b2 = _p(b1), _p(b2)
    _ALIVE.append(out_buf)
    a.x_bs, a.x_cs, a.out_bs, a.out_cs = o["x_emb"][0], o["x_emb"][1], out.stride(0), out.stride(1)
    a.B, a.C, a.K, a.dil, a.T = B, Cc, o["K"], o["dil"], T
    a.accumulate, a.slope, a.out_div = int(o["accumulate"]), o["slope"], o["out_div"]
    _lib.check(_L().set_resblock_pair_x2(C.byref(a), _s()), "set_resblock_pair_x2")
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x_buf)
    return out_buf.cpu()


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("case", PAIR, ids=[c[0] for c in PAIR])
def test_x2_resblock_pair_branch(dev, case, mode):
    from set_amd import ops
    o = make_pair(case, mode)
    K, dil = o["K"], o["dil"]
    w1, w2, b1, b2, xd = (o[n].to(dev) for n in ("w1", "w2", "b1", "b2", "x"))
    cw1, cw2 = ops.ConvWeight(w1, o["C"], o["C"], K), ops.ConvWeight(w2, o["C"], o["C"], K)
    _flag()
    got = _pair_fused(o, dev, cw1, cw2, b1, b2)
    # the two launches it replaces, the second one into a copy of the same buffer
    two_buf = o["out_buf"].to(dev)
    t = ops.conv1d(xd, cw1, b1, dil=dil, pad=dil * (K - 1) // 2, pro="lrelu", pro_param=o["slope"], impl="f16x2")
    ops.conv1d(t, cw2, b2, dil=1, pad=(K - 1) // 2, pro="lrelu", pro_param=o["slope"], res=xd, out=o["out_view"](two_buf), accumulate=o["accumulate"],
               out_div=o["out_div"], impl="f16x2")
    torch.cuda.synchronize()
    assert not _flag()
    two = two_buf.cpu()
    d = (got.double() - o["want"]).abs()
    if mode == "exact":
        bar = torch.zeros_like(d)
    else:  # 1e-5 of the output's size inside the view, nothing outside it
        bar = torch.zeros_like(d)
        o["out_view"](bar).fill_(1e-5 * max(1.0, float(o["yd"].abs().max())))
    assert _report(case[0], "two f16x2 convs", two, o["want"], bar).numel() == 0
    bad = _report(case[0], "pair", got, o["want"], bar)
    assert bad.numel() == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), o["want"][bad[:8]].tolist())
    assert torch.equal(got, two), float((got - two).abs().max())  # the same products in the same order: BIT-identical, guards included
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------------------------------
# assumption 1: the f16 MFMA adds without losing a bit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["one_mfma", "two_mfmas", "two_chunks"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_mfma_adds_without_losing_a_bit(dev, where, sign):
    """One product of ONE granule against products that sum to (2^24 - 2) granules: the exact result, (2^24 - 1) q or (2^24 - 3) q, needs
    all 24 bits, so a lost low bit, or a small product flushed inside the MFMA, changes it.  K = 1, every operand one exact fp16 piece.
    Weights m / 2048 (scale 2^4: m 2^-7), activations n 2^-13: a product is m n granules of q = 2^-20 (2^-24 after the 2^-4).  Channels
    0..7 hold 2047 x 1024 each (2^24 - 8192 together), channels 9 and 10 hold 2040 x 4 and 1 x 30 (8190), and the +-1 x 1 product sits in
    channel 8 (the same 16-product MFMA), 16 (the next MFMA of the chunk: the big sum arrives as the accumulator) or 32 (the next chunk,
    after a barrier and a new LDS tile)."""
    from set_amd import ops
    Cin, Cout, T = 64, 32, 64
    x, w = torch.zeros(1, Cin, T), torch.zeros(Cout, Cin, 1)
    terms = {ch: (2047.0, 1024.0) for ch in range(8)}
    terms.update({9: (2040.0, 4.0), 10: (1.0, 30.0), {"one_mfma": 8, "two_mfmas": 16, "two_chunks": 32}[where]: (sign, 1.0)})
    assert sum(m_ * n_ for m_, n_ in terms.values()) == 2.0 ** 24 - 2 + sign
    for ch, (m_, n_) in terms.items():
        w[:, ch, 0], x[0, ch, :] = m_ / 2048.0, n_ * 2.0 ** -13
    k = x2_exponent(w)
    m = conv_x2_ref(x, w, k)
    assert m["split_exact"] and m["lo_x"] == 0.0 and m["lo_w"] == 0.0
    units = m["y"] / m["q"]
    assert float(units.max()) == 2.0 ** 24 - 2 + sign and bool((m["y"].float().double() == m["y"]).all())
    got = ops.conv1d(x.to(dev), ops.ConvWeight(w.to(dev), Cout, Cin, 1), None, impl="f16x2")
    torch.cuda.synchronize()
    d = (got.cpu().double() - m["y"]).abs()
    print("mfma add, small term in %s, sign %+d: max |d| %.3e granules" % (where, sign, float(d.max()) / m["q"]))
    assert float(d.max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# the range flag
# ------------------------------------------------------------------------------------------------------------------------
def _flag_conv(dev, value, pro="none", pro_param=0.0, where=(0, 3, 50)):
    from set_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 32, 128, generator=g)
    x[where] = value
    w = torch.randn(32, 32, 3, generator=g) * 0.1
    ops.conv1d(x.to(dev), ops.ConvWeight(w.to(dev), 32, 32, 3), None, pad=1, pro=pro, pro_param=pro_param, impl="f16x2")
    torch.cuda.synchronize()


@pytest.mark.parametrize("value,pro,pro_param,raised", [
    (32767.99, "none", 0.0, False), (-32767.99, "none", 0.0, False), (32768.0, "none", 0.0, True), (-32768.0, "none", 0.0, True),
    (float("inf"), "none", 0.0, True), (-4.0e4, "lrelu", 0.1, False), (4.0e4, "lrelu", 0.1, True), (4.0e4, "div", 2.0, False),
    (7.0e4, "div", 2.0, True),
    # a NaN input does not raise the flag: fmaxf(amax, |NaN|) keeps amax.  It is not a range matter either -- the fp32 kernels turn the
    # same NaN into the same NaN outputs, so the caller's repeat on them would change nothing; pinned here so that it stays a decision
    (float("nan"), "none", 0.0, False),
])
def test_range_flag_is_judged_after_the_prologue(dev, value, pro, pro_param, raised):
    assert not _flag()
    _flag_conv(dev, value, pro, pro_param)
    assert _flag(reset=False) == raised
    assert _flag() == raised and not _flag()  # sticky until reset, then clear


def test_range_flag_words_of_both_kernels_and_the_pair_intermediate(dev):
    """g_x2_range_flag (conv_x2.hip) and g_rp_range_flag (resblock_x2.hip) are two device words behind one entry point: each is read,
    and each is cleared, through set_conv_x2_range_flag; the pair raises its word for x and for its intermediate alone."""
    from set_amd import ops
    g = torch.Generator().manual_seed(4)
    Cc, K, T = 32, 3, 128
    w1, w2 = (ops.ConvWeight((torch.randn(Cc, Cc, K, generator=g) * 0.1).to(dev), Cc, Cc, K) for _ in range(2))
    zero = torch.zeros(Cc, device=dev)
    x = torch.randn(1, Cc, T, generator=g).to(dev)
    v = C.c_int32(7)

    def read(reset):
        assert _L().set_conv_x2_range_flag(C.byref(v), int(reset)) == 0
        return v.value

    assert read(True) in (0, 1) and read(False) == 0
    ops.resblock_pair(x, w1, zero, w2, zero, 1)
    assert read(False) == 0
    xb = x.clone()
    xb[0, 3, 50] = 4.0e4
    ops.resblock_pair(xb, w1, zero, w2, zero, 1)              # the pair's word alone
    assert read(False) == 1 and read(True) == 1 and read(False) == 0
    big = torch.full((Cc,), 5.0e4, device=dev)                # conv 1's bias alone leaves the range: only the intermediate does
    ops.resblock_pair(x, w1, big, w2, zero, 1)
    assert read(True) == 1 and read(False) == 0
    _flag_conv(dev, 4.0e4)                                     # the conv's word alone
    assert read(False) == 1 and read(True) == 1 and read(False) == 0
    _flag_conv(dev, 4.0e4)                                     # both, cleared by one call
    ops.resblock_pair(xb, w1, zero, w2, zero, 1)
    assert read(True) == 1 and read(False) == 0
    assert _L().set_conv_x2_range_flag(None, 0) == 0            # a null flag pointer is allowed


# ------------------------------------------------------------------------------------------------------------------------
# refusals: the documented code, `out` untouched.  Every operand is valid and large enough for the call as if it were run
# ------------------------------------------------------------------------------------------------------------------------
def test_conv_x2_refuses_in_chan_add_and_a_halo_of_129(dev):
    from set_amd import _lib, ops
    B, Cin, Cout, T = 2, 32, 32, 300
    x = torch.ones(B, Cin, T, device=dev)
    add = torch.ones(B, Cin, device=dev)
    out = torch.full((B * Cout * T + 64,), SENTINEL, device=dev)
    view = out[:B * Cout * T].view(B, Cout, T)
    for K, dil, with_add, ok in ((3, 1, True, False), (2, 129, False, False), (2, -129, False, False), (4, 43, False, False), (2, 128, False, True)):
        cw = ops.ConvWeight(torch.ones(Cout, Cin, K, device=dev), Cout, Cin, K)
        halo = (K - 1) * abs(dil)
        kw = dict(dil=dil, pad=halo // 2 if dil > 0 else -(halo // 2), T_out=T, T_iter=T, in_chan_add=add if with_add else None, out=view, impl="f16x2")
        if ok:
            ops.conv1d(x, cw, None, **kw)
            torch.cuda.synchronize()
            assert bool((out[:B * Cout * T] != SENTINEL).all()) and bool((out[B * Cout * T:] == SENTINEL).all())
            continue
        with pytest.raises(_lib.SetAmdError) as e:
            ops.conv1d(x, cw, None, **kw)
        assert "rc=%d" % E_UNSUPPORTED in str(e.value)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    with pytest.raises(AssertionError):  # out_div without accumulate never reaches the library
        ops.conv1d(x, cw, None, dil=128, pad=64, out=view, impl="f16x2", out_div=2.0)
    assert not _flag()


def _pair_args(dev, Cc, K, dil, T, *, B=2, alias=False, accumulate=0, out_div=0.0):
    from set_amd import _lib
    x = torch.ones(B * Cc * T + 64, device=dev)
    out = torch.full((B * Cc * T + 64,), SENTINEL, device=dev)
    w = torch.zeros(_L().set_packed_conv_weight_x2_size(Cc, Cc, K), dtype=torch.float16, device=dev)
    bias = torch.zeros(max(Cc, 32), device=dev)
    a = _lib.SetResblockPairArgs()
    a.x, a.out = _p(x), _p(x) if alias else _p(out)
    a.w1, a.w2, a.b1, a.b2 = _p(w), _p(w), _p(bias), _p(bias)
    a.x_bs, a.x_cs, a.out_bs, a.out_cs = Cc * T, T, Cc * T, T
    a.B, a.C, a.K, a.dil, a.T = B, Cc, K, dil, T
    a.accumulate, a.slope, a.out_div = accumulate, 0.1, out_div
    return a, x, out


PAIR_REFUSED = [  # why, C, K, dil, T, extra, code
    ("C 15", 15, 3, 1, 64, {}, E_UNSUPPORTED), ("C 257", 257, 3, 1, 64, {}, E_UNSUPPORTED), ("C 129 with K 7", 129, 7, 1, 64, {}, E_UNSUPPORTED),
    ("K 4", 64, 4, 1, 64, {}, E_UNSUPPORTED), ("K 1", 64, 1, 1, 64, {}, E_UNSUPPORTED), ("K 17", 64, 17, 1, 64, {}, E_UNSUPPORTED),
    ("dil 0", 64, 3, 0, 64, {}, E_UNSUPPORTED), ("dil (K - 1) 130", 64, 3, 65, 200, {}, E_UNSUPPORTED), ("T 63", 64, 3, 1, 63, {}, E_UNSUPPORTED),
    ("out == x", 64, 3, 1, 64, dict(alias=True), E_INVALID), ("out_div without accumulate", 64, 3, 1, 64, dict(out_div=2.0), E_INVALID),
]


@pytest.mark.parametrize("why,Cc,K,dil,T,extra,code", PAIR_REFUSED, ids=[r[0].replace(" ", "_") for r in PAIR_REFUSED])
def test_pair_refuses_what_it_cannot_run_and_leaves_out_alone(dev, why, Cc, K, dil, T, extra, code):
    a, x, out = _pair_args(dev, Cc, K, dil, T, **extra)
    assert _L().set_resblock_pair_x2(C.byref(a), _s()) == code, why
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((x == 1.0).all())
    assert not _flag()


def test_pair_runs_the_call_the_refusals_are_variations_of(dev):
    a, x, out = _pair_args(dev, 64, 3, 1, 64)
    assert _L().set_resblock_pair_x2(C.byref(a), _s()) == 0
    torch.cuda.synchronize()
    # zero weights and biases: out = x = 1 on the view, the guard behind it untouched
    assert bool((out[:2 * 64 * 64] == 1.0).all()) and bool((out[2 * 64 * 64:] == SENTINEL).all())
