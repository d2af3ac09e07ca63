"""GPU sweep of the two opt-in bf16 step bodies of the reverse loop (set_diffusion_loop with SetDiffLoopArgs.img16_all set: STEP_BF16_GROUPS
and STEP_BF16_LAYERS of csrc/diffusion_loop.hip) against the float64 model of tests/bf16_loop_models.py, where the case table lives (each
row names the branch it reaches; tests/test_bf16_loop_reference.py pins every row's plan and runs the CPU half of the argument).  What is
under test is the HOST code that composes the loop -- plan_steps, step_bf16_groups, step_bf16_layers: the kernels it launches are held
to float64 by their own sweeps (test_gpu_diffnet_bf16_branches.py, test_gpu_conv_branches.py, test_gpu_loop_branches.py).

Plumbing as in test_gpu_loop_branches.py: SetDiffLoopArgs is filled by hand; x, the five workspaces AND bf16_ws are views at offset G
inside sentinel-filled buffers compared whole; every operand (cond, the layer images, the three bias arrays, dstep, coef4, noise, the
conv images) is checked unchanged.  condproj, w1p_all, w2p_all and sync_ws are NULL: the entry point promises the bf16 form needs none.

  a  composition (steps = 1): the test makes the launches itself -- set_conv1d for the in-projection on the same image, then L calls of
     set_diffnet_layer_fwd_bf16 with its own bookkeeping (diffnet.py:118-127) -- and keeps every x_l.  ws_skip must equal its skip sum and
     ws_x0 / ws_x1 the two x_l the plan's ping-pong leaves there, bit for bit: this is also the WITNESS of the body that ran (one layer per
     launch leaves x_{L-1} and x_L, a stride of fuse other layers).  On forced 128-frame tiles the scratch is written exactly where
     layers_scratch_written says, per utterance group; every other plan leaves it sentinel.
  d  the same run, teacher-forced: x = posterior(head(ws_skip read back)) within the boundary's derived bar (explicit eps and Philox);
     fused fp32 == unfused bit for bit; the two-piece boundary differs from the fp32 one in bits and leaves err_flag 0.
  b  GROUPS == LAYERS bit for bit over the row's 2 - 3 steps (the rule of test_fused_layer_groups_equal_one_launch_per_layer, through the loop).
  c  exact mode: ws_skip == skip_want bit for bit (blames the layers), then x bit for bit the model's (Philox: within the bar); over two
     steps teacher-forced from a companion one-step run, and with L = 1 xin_next in ws_x0 bit for bit.
  e  end to end against float64: max |x - loop64| <= 4 max |mirror - loop64| + 1e-4 max(1, |x|max), the same form for the last skip sum;
     the ratios are printed (profiles/bf16_loop_gpu_accuracy.log).
  f  refusals launch nothing;  g  ops.diffusion_loop(bf16=...) gives the bits of the raw call;  h  the model takes the bf16 loop from
     T = 32 on;  ws_q4 and the timing outputs change no bit.
Timing values are not compared with each other; offsets beyond 2 GiB are out of reach of shapes a test can afford."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bf16_loop_models as Mo
import test_diffnet_bf16_reference as D
import test_loop_reference as R
from conftest import base_hparams
from test_gpu_conv_branches import _ALIVE, _L, _p, _s, dev  # noqa: F401
from test_gpu_loop_branches import G, SENTINEL, _check_last_step, _flat, _guards_intact, _philox, _same, _view, _witness

pytestmark = pytest.mark.gpu

DC = 256
E_INVALID = -1
SWITCHES = ("SET_AMD_BF16_FUSE", "SET_AMD_BF16_FUSE_TILE", "SET_AMD_BOUNDARY_X2", "SET_AMD_FUSED_BOUNDARY", "SET_AMD_WS_Q4")
BUFS = ("x", "ws_x0", "ws_x1", "ws_skip", "ws_h", "ws_x0pred")
RATIOS = {}  # (row, noise) -> observed error / bar of section e


@pytest.fixture(autouse=True)
def _keep_launch_operands():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more is started on this GPU
        pytest.exit("device error after a sweep case, the session ends here: %s" % e, returncode=3)
    _ALIVE.clear()


def _setenv(monkeypatch, env):
    for n in SWITCHES:
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)


def _operands16(dev, o):
    """Device copies of a case's operands, the bf16 layer images (ONE set_pack_diffnet_layers_bf16 launch) and the conv images."""
    from set_amd import ops
    d = {n: o[n].float().contiguous().to(dev) for n in ("W_in", "b_in", "W_skip", "b_skip", "W_out", "b_out", "dstep", "coef4", "noise", "bd", "bo", "cond", "bc")}
    L, M = o["L"], o["M"]
    w = [o[k].float().contiguous().to(dev) for k in ("Wd", "Wc", "Wo")]
    d["imgs"] = torch.zeros(L * D.N_IMG, dtype=torch.int16, device=dev)
    assert _L().set_pack_diffnet_layers_bf16(_p(w[0]), _p(w[1]), _p(w[2]), 512 * DC * 3, 512 * Mo.FH, 512 * DC, d["imgs"].data_ptr(), L, _s()) == 0
    torch.cuda.synchronize()
    d["cw"] = dict(W_in=ops.ConvWeight(d["W_in"], DC, M, 1), W_skip=ops.ConvWeight(d["W_skip"], DC, DC, 1), W_out=ops.ConvWeight(d["W_out"], M, DC, 1))
    d["img"] = {n: cw.packed() for n, cw in d["cw"].items()}
    if R.fusable(M, o["T"]):
        d["img_x2"] = {n: cw.packed_x2() for n, cw in d["cw"].items()}
    return d


def _readonly(d):
    return [d[n] for n in ("b_in", "b_skip", "b_out", "dstep", "coef4", "noise", "bd", "bo", "cond", "bc", "imgs")] + list(d["img"].values()) + \
        list(d.get("img_x2", {}).values())


def _run16(dev, o, d, c, *, seed=None, ws_q4=0, timing=False, drop=(), dcl=None, expect_rc=0):
    """One set_diffusion_loop call in the bf16 form on the plan of row c (ws, n_groups, x2_images; the environment is the caller's).
    seed None: the explicit noise, else Philox.  drop: operands passed as NULL.  Returns the whole buffers (CPU), the error word, the
    timing outputs."""
    from set_amd import _lib
    B, M, T, L, steps = o["B"], o["M"], o["T"], o["L"], o["steps"]
    n = dict(x=B * M * T, ws_x0=B * DC * T, ws_x1=B * DC * T, ws_skip=B * DC * T, ws_h=B * DC * T, ws_x0pred=B * M * T)
    n_ws = Mo.ws_floats_of(c)
    if c["ws"] is not None:
        n["bf16_ws"] = n_ws
    cpu = {k: _flat(v) for k, v in n.items()}
    cpu["x"][G:-G] = o["x_T"].flatten()
    dbuf = {k: v.to(dev) for k, v in cpu.items()}
    ro = _readonly(d)
    before = [t.clone() for t in ro]
    a = _lib.SetDiffLoopArgs()
    a.B, a.T, a.M, a.L, a.steps, a.dilation_cycle_length = B, T, M, L, steps, o["dcl"] if dcl is None else dcl
    for k in BUFS:
        setattr(a, k, _p(dbuf[k]) + 4 * G)
    a.noise, a.seed = (_p(d["noise"]), 0) if seed is None else (None, int(seed))
    a.dstep, a.coef4 = _p(d["dstep"]), _p(d["coef4"])
    a.w_in_p, a.b_in = _p(d["img"]["W_in"]), _p(d["b_in"])
    a.w_skip_p, a.b_skip = _p(d["img"]["W_skip"]), _p(d["b_skip"])
    a.w_outp_p, a.b_outp = _p(d["img"]["W_out"]), _p(d["b_out"])
    if "img_x2" in d and c["x2_images"]:
        a.w_in_x2, a.w_skip_x2, a.w_outp_x2 = _p(d["img_x2"]["W_in"]), _p(d["img_x2"]["W_skip"]), _p(d["img_x2"]["W_out"])
    a.b_dil_all, a.b_out_all = _p(d["bd"]), _p(d["bo"])
    a.cond = None if "cond" in drop else _p(d["cond"])
    a.img16_all = d["imgs"].data_ptr()
    a.b_cond_all = None if "b_cond" in drop else _p(d["bc"])
    if c["ws"] is not None:
        a.bf16_ws, a.bf16_ws_floats = _p(dbuf["bf16_ws"]) + 4 * G, n_ws
    # condproj, w1p_all, w2p_all, sync_ws: NULL
    a.persistent, a.n_groups, a.ws_q4 = 1, int(c["n_groups"]), int(ws_q4)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a.err_flag = _p(err)
    spans, loop_ms = None, None
    if timing:
        spans = (C.c_float * steps)(*([-1.0] * steps))
        a.layer_span_ms = C.cast(spans, C.POINTER(C.c_float))
        loop_ms = C.c_float(-1.0)
        a.loop_ms = C.pointer(loop_ms)
    rc = _L().set_diffusion_loop(C.byref(a), _s())
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, expect_rc)
    for t, b in zip(ro, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "an operand changed"
    out = {k: v.cpu() for k, v in dbuf.items()}
    out["before"] = cpu
    out["err"] = int(err.item())
    if timing:
        out["spans"], out["loop_ms"] = list(spans), float(loop_ms.value)
    return out


def _bits(name, got, want):
    """Whole flat buffer `got` against the view `want` inside untouched guards, bit for bit."""
    w = torch.full(got.shape, SENTINEL)
    w[G:-G] = want.float().flatten()
    bad = (got.view(torch.int32) != w.view(torch.int32)).nonzero().flatten()
    assert bad.numel() == 0, (name, bad.numel(), bad[:6].tolist(), got[bad[:6]].tolist(), w[bad[:6]].tolist())


def _compose(dev, o, d):
    """The launches of one step by the test's own bookkeeping: (x_0 .. x_L, skip sum) on the CPU."""
    from set_amd import _lib
    B, M, T, L, steps, dcl = o["B"], o["M"], o["T"], o["L"], o["steps"], o["dcl"]
    assert steps == 1
    x = o["x_T"].float().contiguous().to(dev)
    xs = [torch.full((B, DC, T), SENTINEL, device=dev) for _ in range(L + 1)]
    skip = torch.full((B, DC, T), float("nan"), device=dev)  # first = 1 must not read it
    ca = _lib.SetConv1dArgs()  # xin = ReLU(W_in x + b_in) (diffnet.py:118-120)
    ca.inp, ca.w, ca.bias, ca.out = _p(x), _p(d["img"]["W_in"]), _p(d["b_in"]), _p(xs[0])
    ca.in_bs, ca.in_cs, ca.out_bs, ca.out_cs = M * T, T, DC * T, T
    ca.B, ca.Cin, ca.Cout, ca.K, ca.dil, ca.pad = B, M, DC, 1, 1, 0
    ca.T_in, ca.T_iter, ca.T_out, ca.out_stride, ca.out_off = T, T, T, 1, 0
    ca.alpha, ca.impl, ca.act = 1.0, _lib.IMPL_MFMA, _lib.ACT["relu"]
    assert _L().set_conv1d(C.byref(ca), _s()) == 0
    for l in range(L):  # diffnet.py:123-127: layer l on x_l with its own image, biases and step-embedding rows; dilation 2^(l mod dcl)
        la = _lib.SetDiffnetLayerBf16Args()
        la.x_in, la.x_out, la.skip, la.cond = _p(xs[l]), _p(xs[l + 1]), _p(skip), _p(d["cond"])
        la.dstep, la.d_bs, la.d_cs = _p(d["dstep"]) + 4 * l * DC, 0, 1
        la.img = d["imgs"].data_ptr() + 2 * l * D.N_IMG
        la.b_dil, la.b_cond, la.b_out = _p(d["bd"]) + 4 * 512 * l, _p(d["bc"]) + 4 * 512 * l, _p(d["bo"]) + 4 * 512 * l
        la.B, la.T, la.dil, la.first = B, T, 1 << (l % dcl), int(l == 0)
        assert _L().set_diffnet_layer_fwd_bf16(C.byref(la), _s()) == 0
    torch.cuda.synchronize()
    return [t.cpu() for t in xs], skip.cpu()


def _scratch_written(c, plan):
    return Mo.scratch_written(c, plan, torch.cuda.get_device_properties(0).multi_processor_count)


def _check_scratch(out, c, plan):
    if c["ws"] is None:
        return
    h = out["bf16_ws"]
    _guards_intact(out, ("bf16_ws",))
    used, m = h[G:-G].numpy(), _scratch_written(c, plan)
    assert not (used[~m] != SENTINEL).any(), ("scratch written outside the modelled set", np.nonzero((used != SENTINEL) & ~m)[0][:8].tolist())
    assert not (used[m] == SENTINEL).any() and np.isfinite(used[m]).all(), "scratch: a parked skip row is missing"


def _plan(c):
    return Mo.plan_mirror(c, torch.cuda.get_device_properties(0).multi_processor_count)


def _eps(dev, o, seed, k):
    return o["noise"][k] if seed is None else _philox(dev, o, seed, k)


# ------------------------------------------------------------------------------------------------------------------------
# a + d. composition and the boundary, steps = 1
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Mo.ROWS, ids=lambda c: c["name"])
def test_composition_and_last_boundary(dev, monkeypatch, c):
    plan = _plan(c)
    assert all((g["body"], g["fuse"], len(g["launches"])) == (c["body"], c["fuse"], c["n"]) for g in plan["groups"]) and plan["boundary"] == c["boundary"]
    o = Mo.make_gauss_c(c, steps=1)
    d = _operands16(dev, o)
    xs, skip = _compose(dev, o, d)
    held = Mo.final_x_layers(c["L"], c["fuse"])
    if c["body"] == "GROUPS":  # the witness tells the bodies apart
        assert held != Mo.final_x_layers(c["L"], 1) or _scratch_written(c, plan).any()
    fused, x2 = c["boundary"] != "unfused", c["boundary"] == "x2"
    for seed in (None, 81):
        _setenv(monkeypatch, c["env"])
        out = _run16(dev, o, d, c, seed=seed)
        tag = "%s %s" % (c["name"], "eps" if seed is None else "philox")
        assert out["err"] == 0, tag
        _bits(tag + " ws_skip", out["ws_skip"], skip)
        for k, l in held.items():
            _bits("%s %s = x_%d" % (tag, k, l), out[k], xs[l])
        _check_scratch(out, c, plan)
        if c["env"].get(Mo.TILE) == "128" and c["body"] == "GROUPS":
            assert _scratch_written(c, plan).any()
        _witness(out, o, fused)
        _check_last_step(dev, o, out, o["x_T"], _eps(dev, o, seed, 0), x2, "bounded", c["name"], tag)
        if c["boundary"] == "fused_f32":  # bit-identical to the four separate kernels
            _setenv(monkeypatch, dict(c["env"], SET_AMD_FUSED_BOUNDARY="0"))
            sep = _run16(dev, o, d, c, seed=seed)
            _witness(sep, o, False)
            _same(out, sep, ("x", "ws_x0", "ws_x1", "ws_skip"))
        if x2:  # the switch switches
            _setenv(monkeypatch, dict(c["env"], SET_AMD_BOUNDARY_X2="0"))
            f32 = _run16(dev, o, d, c, seed=seed)
            assert f32["err"] == 0
            _same(out, f32, ("ws_x0", "ws_x1", "ws_skip"))
            assert not torch.equal(out["x"], f32["x"]), "the two-piece boundary did not run: same bits as the fp32 boundary"
            _check_last_step(dev, o, f32, o["x_T"], _eps(dev, o, seed, 0), False, "bounded", c["name"], tag + " fp32 boundary")


# ------------------------------------------------------------------------------------------------------------------------
# b. GROUPS == LAYERS
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in Mo.ROWS if c["body"] == "GROUPS"], ids=lambda c: c["name"])
def test_groups_equal_one_launch_per_layer(dev, monkeypatch, c):
    o = Mo.make_gauss_c(c)
    d = _operands16(dev, o)
    assert o["steps"] in (2, 3)
    _setenv(monkeypatch, c["env"])
    for seed in (None, 82):
        grp = _run16(dev, o, d, c, seed=seed)
        lay = _run16(dev, o, d, dict(c, ws=None), seed=seed)
        assert grp["err"] == 0 and lay["err"] == 0
        _same(grp, lay, ("x", "ws_skip", "ws_h", "ws_x0pred"))
        hg, hl = Mo.final_x_layers(c["L"], c["fuse"]), Mo.final_x_layers(c["L"], 1)
        kg, kl = (next(k for k, l in h.items() if l == c["L"]) for h in (hg, hl))
        assert torch.equal(grp[kg].view(torch.int32), lay[kl].view(torch.int32)), "x_L differs between the bodies"
        _check_scratch(grp, c, _plan(c))
        # utterance groups: one group gives the same bits in every buffer
        if c["n_groups"] > 1:
            _same(grp, _run16(dev, o, d, dict(c, n_groups=1), seed=seed), BUFS)


# ------------------------------------------------------------------------------------------------------------------------
# c. exact mode
# ------------------------------------------------------------------------------------------------------------------------
def _precondition(out, o, tag):
    got, want = _view(out, "ws_skip", o), o["skip_want"].float()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        "the bf16 layers (%s), not the boundary: their skip sum differs from the integer model at %s" % (tag, (got != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("c", Mo.EXACT, ids=lambda c: c["name"])
def test_exact_mode(dev, monkeypatch, c):
    x2 = c["boundary"] == "x2"
    o2 = Mo.make_exact_c(c, steps=2, L=c["L"])
    o1 = R.one_step_of(o2, 1, 0)
    d2 = _operands16(dev, o2)
    d1 = dict(d2)
    d1.update({n: o1[n].float().contiguous().to(dev) for n in ("dstep", "coef4", "noise")})
    _setenv(monkeypatch, c["env"])
    for seed in (None, 83):
        mode = "exact" if seed is None else "bounded"
        tag = "%s %s" % (c["name"], "eps" if seed is None else "philox")
        one, two = _run16(dev, o1, d1, c, seed=seed), _run16(dev, o2, d2, c, seed=seed)
        assert one["err"] == 0 and two["err"] == 0, tag
        _precondition(one, o1, tag), _precondition(two, o2, tag)
        _check_last_step(dev, o1, one, o1["x_T"], _eps(dev, o1, seed, 0), x2, mode, c["name"], tag + " one step")
        xp = _view(one, "x", o1)  # the fp32 x' the first boundary of the two-step run handed on
        if c["L"] == 1:  # ws_x0 still holds xin_next of the first boundary: layer 0 of step 2 read it and wrote ws_x1
            xi = R.in_proj(xp, o2["W_in"], o2["b_in"], R.x2_exponents(o2)[1] if x2 else None)
            if mode == "exact":
                _bits(tag + " xin_next", two["ws_x0"], xi["y"])
            else:
                w = torch.full(two["ws_x0"].shape, SENTINEL, dtype=torch.float64)
                w[G:-G] = xi["y"].flatten()
                bar = torch.zeros_like(w)
                bar[G:-G] = (xi["bar"] + R.U * xi["y"].abs()).flatten()
                assert bool(((two["ws_x0"].double() - w).abs() <= bar).all()), tag
        _check_last_step(dev, o2, two, xp, _eps(dev, o2, seed, 1), x2, mode, c["name"], tag + " step 2")


# ------------------------------------------------------------------------------------------------------------------------
# e. end to end against float64
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Mo.E2E, ids=lambda c: c["name"])
def test_end_to_end_against_float64(dev, monkeypatch, c):
    """max |x - loop64| <= 4 max |mirror - loop64| + 1e-4 max(1, |x|max), and the same form for the skip sum of the last step.  Observed on
    the MI355X: profiles/bf16_loop_gpu_accuracy.log."""
    o = Mo.make_gauss_c(c)
    d = _operands16(dev, o)
    _setenv(monkeypatch, c["env"])
    for seed in (None, 84):
        noise = None if seed is None else torch.stack([_philox(dev, o, seed, k) for k in range(o["steps"])])
        (x, tr), (xm, trm) = Mo.loop_c(o, noise=noise), Mo.loop_c(o, mirror=True, noise=noise)
        out = _run16(dev, o, d, c, seed=seed)
        assert out["err"] == 0
        _guards_intact(out, BUFS)
        res = {}
        for k, want, mir in (("x", x, xm), ("ws_skip", tr[-1]["skip"], trm[-1]["skip"])):
            bar = Mo.e2e_bar(o, want, mir)
            e = float((_view(out, k, o).double() - want).abs().max())
            res[k] = (e, bar)
        key = (c["name"], "eps" if seed is None else "philox")
        RATIOS[key] = {k: e / bar for k, (e, bar) in res.items()}
        print("BF16LOOP e2e row=%-14s body=%s fuse=%d steps=%d L=%d noise=%s  x: err %.3e bar %.3e ratio %.3f   ws_skip: err %.3e bar %.3e ratio %.3f" % (
            c["name"], c["body"], c["fuse"], c["steps"], c["L"], key[1], res["x"][0], res["x"][1], res["x"][0] / res["x"][1],
            res["ws_skip"][0], res["ws_skip"][1], res["ws_skip"][0] / res["ws_skip"][1]))
        for k, (e, bar) in res.items():
            assert e <= bar, (key, k, e, bar)


def test_worst_end_to_end_ratios(dev):
    for k, v in sorted(RATIOS.items()):
        print("BF16LOOP worst error / bar  %-16s %-7s x %.4f ws_skip %.4f" % (k[0], k[1], v["x"], v["ws_skip"]))
    assert all(r <= 1.0 for v in RATIOS.values() for r in v.values())


# ------------------------------------------------------------------------------------------------------------------------
# f. refusals
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("no_cond", dict(drop=("cond",))), ("no_b_cond", dict(drop=("b_cond",))), ("dcl5", dict(dcl=5)), ("dcl0", dict(dcl=0))])
def test_refusals_launch_nothing(dev, monkeypatch, name, kw):
    """dcl 5 at L = 7: layers 0 - 3 run at dilations the kernel takes, so a check that comes only with layer 4 leaves the workspaces half written."""
    c = Mo.row("plan_L7_dcl1")
    o = Mo.make_gauss_c(c)
    d = _operands16(dev, o)
    _setenv(monkeypatch, {})
    for ws in ("exact", None):
        out = _run16(dev, o, d, dict(c, ws=ws), expect_rc=E_INVALID, **kw)
        for k, before in out["before"].items():
            assert torch.equal(out[k].view(torch.int32), before.view(torch.int32)), (name, k, "written by a refused call")
        assert out["err"] == 0


# ------------------------------------------------------------------------------------------------------------------------
# ws_q4 and the timing outputs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plan_L7_dcl1", "no_ws"])
def test_ws_q4_changes_no_bit(dev, monkeypatch, name):
    """The bf16 bodies never take the channel-quad layout (plan_steps: STEP_STACK only)."""
    c = Mo.row(name)
    o = Mo.make_gauss_c(c)
    d = _operands16(dev, o)
    _setenv(monkeypatch, c["env"])
    _same(_run16(dev, o, d, c, ws_q4=1), _run16(dev, o, d, c, ws_q4=0), BUFS)


@pytest.mark.parametrize("name", ["t128_ragged", "groups2", "no_ws"])
def test_timing_outputs_are_written_and_change_no_bit(dev, monkeypatch, name):
    c = Mo.row(name)
    o = Mo.make_gauss_c(c)
    d = _operands16(dev, o)
    _setenv(monkeypatch, c["env"])
    plain, timed = _run16(dev, o, d, c), _run16(dev, o, d, c, timing=True)
    _same(plain, timed, BUFS + (("bf16_ws",) if c["ws"] is not None else ()))
    assert len(timed["spans"]) == o["steps"] and all(math.isfinite(v) and v > 0 for v in timed["spans"]), timed["spans"]
    assert math.isfinite(timed["loop_ms"]) and timed["loop_ms"] > 0


# ------------------------------------------------------------------------------------------------------------------------
# g. the Python wrapper
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plan_L7_dcl1", "dcl3_T132"])
def test_python_wrapper_gives_the_bits_of_the_raw_call(dev, monkeypatch, name):
    """ops.diffusion_loop(bf16=...) allocates its own workspaces (a scratch for any group size at dcl <= 2, none above) and passes
    ws_q4 = 1: the plan is the row's, so x must carry the same bits."""
    from set_amd import ops
    c = Mo.row(name)
    o = Mo.make_gauss_c(c)
    d = _operands16(dev, o)
    _setenv(monkeypatch, c["env"])
    raw = _run16(dev, o, d, c)
    L = o["L"]
    packs = ops.StackImages(w1p=torch.zeros(L, 8, device=dev), w2p=torch.zeros(L, 8, device=dev), b_dil=d["bd"], b_out=d["bo"], w1w=None, w2w=None,
                            w1s=None, w2s=None, wx3=None)  # (the fp32 images are not read in the bf16 form)
    x = o["x_T"].float().contiguous().to(dev)
    ops.diffusion_loop(x=x, noise=d["noise"], seed=0, condproj=None, dstep=d["dstep"], coef4=d["coef4"], w_in=d["cw"]["W_in"], b_in=d["b_in"],
                       packs=packs, w_skip=d["cw"]["W_skip"], b_skip=d["b_skip"], w_outp=d["cw"]["W_out"], b_outp=d["b_out"], L=L, steps=o["steps"],
                       dilation_cycle_length=o["dcl"], n_groups=1, bf16=dict(cond=d["cond"], imgs=d["imgs"], b_cond=d["bc"]))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), _view(raw, "x", o).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------
# h. the model
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,takes_bf16", [(24, False), (64, True)])
def test_model_takes_the_bf16_loop_from_32_frames_on(dev, monkeypatch, T, takes_bf16):
    """spec_denoiser.py:177: below 32 frames set_compute_dtype("bf16") leaves the reverse loop (and every conv: bf16_eligible) on fp32, so
    the mel carries the same bits; from 32 frames on the loop is called with bf16 operands and the mel differs."""
    from oracle import weights as Wt
    from set_amd import ops
    from set_amd.diffnet import DiffNet
    from set_amd.spec_denoiser import GaussianDiffusion
    _setenv(monkeypatch, {})
    steps = 3
    hp = base_hparams(timesteps=steps)
    model = GaussianDiffusion(list(range(80)), 80, DiffNet(80, hp), timesteps=steps, time_scale=1, loss_type="l1", spec_min=[], spec_max=[], hp=hp)
    model.load_state_dict(Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), 11), strict=False)
    model.to(dev).eval()
    inp = {k: v.to(dev) for k, v in Wt.synthetic_inputs(2, T, 8, seed=101).items()}
    noises = torch.stack(Wt.synthetic_noises(2, T, steps, seed=102)).to(dev)
    seen = []
    real = ops.diffusion_loop

    def spy(**kw):
        seen.append(kw.get("bf16") is not None)
        return real(**kw)
    monkeypatch.setattr(ops, "diffusion_loop", spy)

    def run():
        with torch.no_grad():
            return model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"],
                         infer=True, noises=noises)["mel_out"].float().cpu()
    ref = run()
    ops.set_compute_dtype("bf16")
    try:
        got = run()
    finally:
        ops.set_compute_dtype("f32")
    assert seen == [False, takes_bf16], seen
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, ref) == (not takes_bf16)
