"""GPU branch sweep of the reverse loop (set_diffusion_loop, csrc/diffusion_loop.hip) and of its two fused step-boundary kernels
(diffnet_boundary_kernel / diffnet_boundary_x2_kernel, csrc/boundary.hip) against the float64 model of tests/test_loop_reference.py
(where the case tables live, each row naming the branch it reaches, and where the CPU half of the argument runs).  Same shape as
tests/test_gpu_conv_branches.py / test_gpu_attention_branches.py: SetDiffLoopArgs is filled by hand; x, ws_x0, ws_x1, ws_skip, ws_h and
ws_x0pred are views at offset G inside larger buffers filled with a sentinel and the WHOLE buffers are compared; every operand (weights,
images, condproj, dstep, coef4, noise) is checked unchanged after the call.  The layer images follow the _random_stack recipe of
tests/test_gpu_parity.py (pack_diffnet_layer, SplitOperandImages.pack, split_images) on the case's own weights, plus the Winograd images.

Branch witness: ws_h and ws_x0pred are written only by the unfused boundary -- a fused case finds them all sentinel, an unfused case
fully written.  The two-piece fp16 boundary: ops.stack_variant names a two-piece family and the result differs in at least one bit from
the same case under SET_AMD_BOUNDARY_X2=0.

  BOUNDARY  steps = 1 (last-step branch), teacher-forced: the reference is posterior(head(ws_skip read back), x_T, coef4[0], eps), so the
            stack's error is not in the comparison.  Explicit eps and Philox (reference noise: ops.randn at the loop's quad offset).
  PHASE5    steps = 2, L = 1 with the residual half of the output conv zeroed: ws_x1 after the loop is xin_next * fl32(2^-1/2) of the first
            boundary; its fp32 input x' comes from a companion steps = 1 run on column sid = 1 / noise slice 0.  The final x is checked
            teacher-forced from the second skip sum, which also pins x' of the two-step run to the companion's.
  two modes exact (integer grid, bit for bit after a precondition that blames the stack; with Philox noise, which is not on the grid,
            within the derived bar) and bounded (Gaussian, derived bars), as in test_loop_reference.py.  The worst |d| / bar per kernel and output goes to WORST, printed by the last test.
  LOOP / GROUPS  end to end against loop(): the project's comparative rules (fused == unfused bit for bit on the fp32 boundary; the fp32
            per-layer path within 1e-4 max(1, |x|max) of the model, its error e32 printed; two-piece fp16 paths within 1.5 e32 + 1e-7,
            bf16x3 within e32 + 1e-7); utterance groups bit-identical to one group in every buffer; the Philox seed delta.
  the range word of the two-piece boundary (err_flag = 2) raised through x', s and h.

Swept elsewhere: the two opt-in bf16 step bodies (SetDiffLoopArgs.img16_all: one layer or a group of layers per launch, the host code
that composes them, every boundary form behind them) in tests/test_gpu_bf16_loop_branches.py, which reuses this file's plumbing; that
file also checks that layer_span_ms and loop_ms are written (finite, > 0) and change no bit of any buffer.  Not swept, on purpose: the
VALUES of the timing outputs (no time is compared with another), the 2 GiB offset limits."""
import ctypes as C
import math

import pytest
import torch

import test_loop_reference as R
from test_conv_reference import U
from test_gpu_conv_branches import SENTINEL, _ALIVE, _L, _keep_launch_operands, _p, _report, _s, dev  # noqa: F401

pytestmark = pytest.mark.gpu

G = 64       # guard elements in front of and behind every view
DC = 256
WORST = {}   # (kernel, output) -> worst observed |d| / bar of bounded mode
E32 = {}     # LOOP case -> error of the fp32 per-layer path against the float64 model
SWITCHES = ("SET_AMD_X3", "SET_AMD_SPLIT", "SET_AMD_SPLIT_F32", "SET_AMD_WINO", "SET_AMD_BOUNDARY_X2", "SET_AMD_FUSED_BOUNDARY",
            "SET_AMD_X3_TILE", "SET_AMD_X3_WINO", "SET_AMD_STACK_NCB")
# how the L layers run: persistent flag, environment, x3 image mode, expected ops.stack_variant, whether the step boundary is the two-piece one
FAMILIES = {
    "f32_layers": dict(persistent=0, env={}, x3_mode=2, variant=None, x2=False),
    "direct": dict(persistent=1, env={"SET_AMD_WINO": "0"}, x3_mode=2, variant=(0, 1), x2=False),
    "wino": dict(persistent=1, env={"SET_AMD_WINO": "2"}, x3_mode=2, variant=(2,), x2=False),
    "f32_stack": dict(persistent=1, env={"SET_AMD_X3": "0", "SET_AMD_SPLIT": "0"}, x3_mode=2, variant=(0, 1, 2), x2=False),
    "split_f32": dict(persistent=1, env={"SET_AMD_SPLIT": "2", "SET_AMD_SPLIT_F32": "1"}, x3_mode=2, variant=(3,), x2=False),
    "split_x2": dict(persistent=1, env={"SET_AMD_SPLIT": "2"}, x3_mode=2, variant=(3,), x2=True),
    "x3_f16": dict(persistent=1, env={"SET_AMD_X3": "2", "SET_AMD_SPLIT": "0"}, x3_mode=2, variant=(5,), x2=True),
    "x3_bf16": dict(persistent=1, env={"SET_AMD_X3": "2", "SET_AMD_SPLIT": "0"}, x3_mode=3, variant=(4,), x2=False),
}


def _setenv(monkeypatch, env):
    for n in SWITCHES:
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)


def _operands(dev, o, x3_mode=2):
    """Device copies of a case's operands and every weight image the loop can use."""
    from set_amd import ops
    d = {n: o[n].to(dev).contiguous() for n in ("W_in", "b_in", "W_skip", "b_skip", "W_out", "b_out", "cp", "dstep", "coef4", "noise", "bd", "bo")}
    L = o["L"]
    w1, w2 = torch.empty(L, 512 * 768, device=dev), torch.empty(L, 512 * 256, device=dev)
    w1w, w2w = torch.empty(L, 512 * 256 * 4, device=dev), torch.empty(L, 512 * 256, device=dev)
    wx3 = ops.SplitOperandImages(L, x3_mode, dev)
    for l in range(L):
        wd, wo = o["Wd"][l].to(dev).contiguous(), o["Wo"][l].to(dev).contiguous()
        ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        ops.pack_diffnet_layer_wino(wd, wo, w1w[l], w2w[l])
        wx3.pack(l, wd, wo)
    w1s, w2s = ops.split_images(w1, w2)
    d["packs"] = ops.StackImages(w1p=w1, w2p=w2, b_dil=d["bd"], b_out=d["bo"], w1w=w1w, w2w=w2w, w1s=w1s, w2s=w2s, wx3=wx3)
    M = o["M"]
    d["cw"] = dict(W_in=ops.ConvWeight(d["W_in"], DC, M, 1), W_skip=ops.ConvWeight(d["W_skip"], DC, DC, 1), W_out=ops.ConvWeight(d["W_out"], M, DC, 1))
    d["img"] = {n: w.packed() for n, w in d["cw"].items()}
    if R.fusable(M, o["T"]):
        d["img_x2"] = {n: w.packed_x2() for n, w in d["cw"].items()}
    d["x3_mode"] = x3_mode
    return d


def _readonly(d):
    t = [d[n] for n in ("b_in", "b_skip", "b_out", "cp", "dstep", "coef4", "noise", "bd", "bo")]
    t += [v for v in d["packs"][:8] if v is not None] + [d["packs"].wx3.data] + list(d["img"].values()) + list(d.get("img_x2", {}).values())
    return t


def _flat(n):
    return torch.full((G + n + G,), SENTINEL)


def _run(dev, o, d, *, seed=None, persistent=1, n_groups=1, err=None):
    """One set_diffusion_loop call; seed = None: the explicit noise, else Philox.  Returns the whole buffers (CPU) and the error word."""
    from set_amd import _lib, ops
    B, M, T, L, steps = o["B"], o["M"], o["T"], o["L"], o["steps"]
    n = dict(x=B * M * T, ws_x0=B * DC * T, ws_x1=B * DC * T, ws_skip=B * DC * T, ws_h=B * DC * T, ws_x0pred=B * M * T)
    cpu = {k: _flat(v) for k, v in n.items()}
    cpu["x"][G:-G] = o["x_T"].flatten()
    dbuf = {k: v.to(dev) for k, v in cpu.items()}
    ro = _readonly(d)
    before = [t.clone() for t in ro]
    a = _lib.SetDiffLoopArgs()
    a.B, a.T, a.M, a.L, a.steps, a.dilation_cycle_length = B, T, M, L, steps, o["dcl"]
    for k in n:
        setattr(a, k, _p(dbuf[k]) + 4 * G)
    a.noise, a.seed = (_p(d["noise"]), 0) if seed is None else (None, int(seed))
    a.condproj, a.dstep, a.coef4 = _p(d["cp"]), _p(d["dstep"]), _p(d["coef4"])
    a.w_in_p, a.b_in = _p(d["img"]["W_in"]), _p(d["b_in"])
    a.w_skip_p, a.b_skip = _p(d["img"]["W_skip"]), _p(d["b_skip"])
    a.w_outp_p, a.b_outp = _p(d["img"]["W_out"]), _p(d["b_out"])
    if "img_x2" in d and d["x3_mode"] == 2:  # what ops.diffusion_loop passes whenever the stack images are two-piece fp16
        a.w_in_x2, a.w_skip_x2, a.w_outp_x2 = _p(d["img_x2"]["W_in"]), _p(d["img_x2"]["W_skip"]), _p(d["img_x2"]["W_out"])
    z_ws = ops._set_images(a, d["packs"], B, T, o["dcl"], dev)
    _ALIVE.append(z_ws)
    a.persistent, a.n_groups = int(persistent), int(n_groups)
    sync_ws = torch.zeros(ops.sync_ws_size(B, T), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev) if err is None else err
    a.sync_ws, a.err_flag = _p(sync_ws), _p(err)
    _lib.check(_L().set_diffusion_loop(C.byref(a), _s()), "set_diffusion_loop")
    torch.cuda.synchronize()
    for t, b in zip(ro, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "an operand changed"
    out = {k: v.cpu() for k, v in dbuf.items()}
    out["err"] = int(err.item())
    return out


def _view(out, k, o):
    return out[k][G:-G].view(o["B"], -1, o["T"])


def _cmp(name, tag, got, want, bar, key=None):
    """Whole-buffer comparison of a flat buffer: `want` / `bar` are the view's, everything else must still be the sentinel."""
    w = torch.full(got.shape, SENTINEL, dtype=torch.float64)
    b = torch.zeros(got.shape, dtype=torch.float64)
    w[G:-G] = want.double().flatten()
    b[G:-G] = bar.double().flatten() if torch.is_tensor(bar) else bar
    bad = _report(name, tag, got, w, b)
    assert bad.numel() == 0, (name, tag, bad[:8].tolist(), got[bad[:8]].tolist(), w[bad[:8]].tolist(), b[bad[:8]].tolist())
    if key is not None and bool((b > 0).any()):
        WORST[key] = max(WORST.get(key, 0.0), float(((got.double() - w).abs() / (b + 1e-300))[b > 0].max()))


def _guards_intact(out, names):
    for k in names:
        assert bool((out[k][:G] == SENTINEL).all()) and bool((out[k][-G:] == SENTINEL).all()), k


def _witness(out, o, fused):
    """ws_h / ws_x0pred: written only by the unfused boundary."""
    for k in ("ws_h", "ws_x0pred"):
        if fused:
            assert bool((out[k] == SENTINEL).all()), "%s was written: the fused boundary did not run" % k
        else:
            _guards_intact(out, (k,))
            assert not bool((out[k][G:-G] == SENTINEL).any()), "%s is not fully written: the unfused boundary did not run" % k


def _same(a, b, names=("x", "ws_x0", "ws_x1", "ws_skip", "ws_h", "ws_x0pred")):
    for k in names:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (k, float((a[k] - b[k]).abs().max()))


def _philox(dev, o, seed, k):
    """The noise of executed step k by the loop's numbering, from the independently callable kernel."""
    from set_amd import ops
    n = o["B"] * o["M"] * o["T"]
    return ops.randn((n,), dev, seed=seed, offset=(k + 1) * ((n + 3) // 4)).cpu().view(o["B"], o["M"], o["T"])


def _check_variant(o, fam):
    from set_amd import ops
    f = FAMILIES[fam]
    if f["variant"] is not None:
        v = ops.stack_variant(o["B"], o["T"], o["dcl"], have_wino=True, have_split=True, x3_mode=f["x3_mode"])
        assert v in f["variant"], (fam, v)


def _precondition(out, o, fam):
    got, want = _view(out, "ws_skip", o), o["skip_want"].float()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        "the layer stack (%s), not the boundary: its skip sum differs from the integer model at %s" % (
            fam, (got != want).nonzero()[:4].tolist())


def _check_last_step(dev, o, out, x_t, eps, x2, mode, name, tag):
    """x after the last boundary, teacher-forced from the skip sum the boundary read."""
    k = R.x2_exponents(o)[0] if x2 else None
    hd = R.head(_view(out, "ws_skip", o), o["L"], o["W_skip"], o["b_skip"], o["W_out"], o["b_out"], k)
    p = R.posterior(hd["x0"], x_t, o["coef4"][0], eps, hd["bar_x0"])
    if mode == "exact":
        _cmp(name + ".x", tag, out["x"], p["y"], 0.0)
    else:
        _cmp(name + ".x", tag, out["x"], p["y"], p["bar"], key=("boundary_x2" if x2 else "boundary", "x"))
    _guards_intact(out, ("ws_x0", "ws_x1", "ws_skip"))


def _cmp_mode(mode, seed):
    """Philox noise is not on the integer grid: an exact case drawn from it keeps its precondition (the skip sum, bit for bit) and is
    compared within the derived bar like a bounded one."""
    return mode if seed is None else "bounded"


def _families_of(c, fused):
    fams = ["f32_layers", "f32_stack"]
    if fused:
        fams += ["x3_f16"] + (["split_x2"] if c.get("small") else [])
    return fams


def _make(c, mode, steps, L):
    if mode == "exact":
        return R.make_exact(c, steps=steps, L=L, tag="exact" if steps == 1 else "exact5")
    o = R.make_gauss(c, 1 if mode == "bounded1" else 8, steps=steps, L=L)
    if steps == 1 and mode == "bounded8":
        o["coef4"] = torch.tensor([[1.7, -0.4, -0.7, 1.0]])  # nonzero = 1 with logvar != 0 (bounded1: nonzero = 0; exact: logvar = 0)
    return o


# ------------------------------------------------------------------------------------------------------------------------
# a. BOUNDARY: steps = 1
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.BOUNDARY, ids=lambda c: c["name"])
def test_last_step_boundary(dev, monkeypatch, c):
    fused = c["fused"]
    for mode in (("exact", "bounded1", "bounded8") if fused else ("bounded1", "bounded8")):
        o = _make(c, mode, 1, 4 if mode == "exact" else 1)
        d = _operands(dev, o)
        for fam in _families_of(c, fused):
            f = FAMILIES[fam]
            for seed in (None, 77):
                tag = "%s %s %s" % (mode, fam, "eps" if seed is None else "philox")
                _setenv(monkeypatch, f["env"])
                _check_variant(o, fam)
                out = _run(dev, o, d, seed=seed, persistent=f["persistent"])
                assert out["err"] == 0, tag
                _witness(out, o, fused)
                if mode == "exact":
                    _precondition(out, o, fam)
                eps = o["noise"][0] if seed is None else _philox(dev, o, seed, 0)
                _check_last_step(dev, o, out, o["x_T"], eps, f["x2"], _cmp_mode(mode, seed), c["name"], tag)
                if fused and not f["x2"]:  # the fp32 boundary is bit-identical to the four separate kernels, in every buffer it shares with them
                    _setenv(monkeypatch, dict(f["env"], SET_AMD_FUSED_BOUNDARY="0"))
                    sep = _run(dev, o, d, seed=seed, persistent=f["persistent"])
                    _witness(sep, o, False)
                    _same(out, sep, ("x", "ws_x0", "ws_x1", "ws_skip"))
                if f["x2"] and mode != "exact":  # (exact: both kernels give the same bits) the switch does switch kernels
                    _setenv(monkeypatch, dict(f["env"], SET_AMD_BOUNDARY_X2="0"))
                    f32 = _run(dev, o, d, seed=seed, persistent=f["persistent"])
                    _same(out, f32, ("ws_skip",))
                    assert not torch.equal(out["x"], f32["x"]), "the two-piece boundary did not run: same bits as the fp32 boundary"


# ------------------------------------------------------------------------------------------------------------------------
# b. PHASE5: steps = 2, the non-last branch
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.PHASE5, ids=lambda c: c["name"])
def test_non_last_boundary_input_projection(dev, monkeypatch, c):
    rs2 = torch.tensor(R.RSQRT2, dtype=torch.float32)
    for mode in ("exact", "bounded1", "bounded8"):
        o2 = R.phase5_form(_make(c, mode, 2, 1))
        o1 = R.one_step_of(o2, 1, 0)
        d2 = _operands(dev, o2)
        d1 = dict(d2)
        d1.update({n: o1[n].to(dev).contiguous() for n in ("dstep", "coef4", "noise")})
        for fam in _families_of(c, True):
            f = FAMILIES[fam]
            for seed in (None, 78):
                tag = "%s %s %s" % (mode, fam, "eps" if seed is None else "philox")
                _setenv(monkeypatch, f["env"])
                _check_variant(o2, fam)
                one = _run(dev, o1, d1, seed=seed, persistent=f["persistent"])
                two = _run(dev, o2, d2, seed=seed, persistent=f["persistent"])
                assert one["err"] == 0 and two["err"] == 0, tag
                _witness(one, o1, True), _witness(two, o2, True)
                if mode == "exact":
                    _precondition(one, o1, fam), _precondition(two, o2, fam)
                xp = _view(one, "x", o1)  # the fp32 x' the first boundary's phase 5 read
                xi = R.in_proj(xp, o2["W_in"], o2["b_in"], R.x2_exponents(o2)[1] if f["x2"] else None)
                if _cmp_mode(mode, seed) == "exact":
                    _cmp(c["name"] + ".xin", tag, two["ws_x1"], xi["y"].float() * rs2, 0.0)
                else:
                    want = xi["y"] * R.RSQRT2
                    _cmp(c["name"] + ".xin", tag, two["ws_x1"], want, xi["bar"] * R.RSQRT2 + U * want.abs(),
                         key=("boundary_x2" if f["x2"] else "boundary", "xin_next"))
                # the second (last) step from ITS skip sum and the companion's x': a different x' inside the two-step run shows here
                eps = o2["noise"][1] if seed is None else _philox(dev, o2, seed, 1)
                _check_last_step(dev, o2, two, xp, eps, f["x2"], _cmp_mode(mode, seed), c["name"], tag + " step 2")


# ------------------------------------------------------------------------------------------------------------------------
# c. LOOP: end to end
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.LOOP, ids=lambda c: c["name"])
def test_loop_end_to_end(dev, monkeypatch, c):
    o = R.make_gauss(c, 1, steps=c["steps"], L=c["L"], dcl=c["dcl"], tag="loop")
    want, trace = R.loop(o)
    # a wrong sid must move the result by orders of magnitude more than the bar: the model with the dstep columns / coef4 rows reversed
    scale = max(1.0, float(want.abs().max()))
    if c["steps"] > 1:
        wrong = dict(o, dstep=o["dstep"].flip(1), coef4=o["coef4"].flip(0))
        assert float((R.loop(wrong)[0] - want).abs().max()) > 1e3 * 1e-4 * scale
        assert float((R.loop(o, noise=o["noise"].flip(0))[0] - want).abs().max()) > 1e3 * 1e-4 * scale
    fused = R.fusable(c["M"], c["T"])
    d = {2: _operands(dev, o, 2), 3: _operands(dev, o, 3)}
    err, outs = {}, {}
    for fam, f in FAMILIES.items():
        if fam == "f32_stack":
            continue
        _setenv(monkeypatch, f["env"])
        _check_variant(o, fam)
        out = _run(dev, o, d[f["x3_mode"]], persistent=f["persistent"])
        assert out["err"] == 0, fam
        _witness(out, o, fused)
        _guards_intact(out, ("x", "ws_x0", "ws_x1", "ws_skip"))
        err[fam] = float((_view(out, "x", o).double() - want).abs().max())
        outs[fam] = out
        if fused and not f["x2"]:
            _setenv(monkeypatch, dict(f["env"], SET_AMD_FUSED_BOUNDARY="0"))
            sep = _run(dev, o, d[f["x3_mode"]], persistent=f["persistent"])
            _witness(sep, o, False)
            _same(out, sep, ("x", "ws_x0", "ws_x1", "ws_skip"))
        if fused and f["x2"]:
            _setenv(monkeypatch, dict(f["env"], SET_AMD_BOUNDARY_X2="0"))
            f32 = _run(dev, o, d[f["x3_mode"]], persistent=f["persistent"])
            assert not torch.equal(out["x"], f32["x"]), fam
            err[fam + "+f32_boundary"] = float((_view(f32, "x", o).double() - want).abs().max())
    e32 = err["f32_layers"]
    E32[c["name"]] = e32
    print("loop %s: e32 %.3e (bar %.3e); %s" % (c["name"], e32, 1e-4 * scale, ", ".join("%s %.3e" % kv for kv in sorted(err.items()))))
    assert e32 <= 1e-4 * scale
    for fam in ("direct", "wino", "split_f32"):  # the other fp32 bodies: the same parity bar
        assert err[fam] <= 1e-4 * scale, (fam, err[fam])
    for fam, e in err.items():
        if fam.startswith(("split_x2", "x3_f16")):
            assert e <= 1.5 * e32 + 1e-7, (fam, e, e32)
    assert err["x3_bf16"] <= 1.0 * e32 + 1e-7, (err["x3_bf16"], e32)


# ------------------------------------------------------------------------------------------------------------------------
# d. GROUPS
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.GROUPS, ids=lambda c: c["name"])
def test_utterance_groups(dev, monkeypatch, c):
    o = R.make_gauss(c, 1, steps=c["steps"], L=c["L"], dcl=c["dcl"], tag="groups")
    d = _operands(dev, o)
    want, philox = R.loop(o)[0], {}
    fusable = R.fusable(c["M"], c["T"])

    def want_philox(seed):  # the model on the noise set_randn draws at the loop's quad offsets
        if seed not in philox:
            philox[seed] = R.loop(o, noise=torch.stack([_philox(dev, o, seed, k) for k in range(o["steps"])]))[0]
        return philox[seed]
    for fam in ("f32_stack", "split_x2", "x3_f16"):  # split_x2: the per-group slices of z_ws and sync_ws
        f = FAMILIES[fam]
        for seed in (None, 79):
            for fused in ((True, False) if fusable else (False,)):
                env = dict(f["env"]) if fused else dict(f["env"], SET_AMD_FUSED_BOUNDARY="0")
                _setenv(monkeypatch, env)
                _check_variant(o, fam)
                base = _run(dev, o, d, seed=seed, persistent=1, n_groups=1)
                assert base["err"] == 0
                _witness(base, o, fused)
                ref = want if seed is None else want_philox(seed)
                e = float((_view(base, "x", o).double() - ref).abs().max())
                assert e <= 1e-4 * max(1.0, float(ref.abs().max())), (fam, seed, fused, e)
                for ng in c["groups"][1:]:
                    _same(_run(dev, o, d, seed=seed, persistent=1, n_groups=ng), base)


def test_philox_seed_delta_reaches_the_fused_boundary(dev, monkeypatch):
    """set_rng_seed_delta: the registered device word is added to the seed by set_randn and set_posterior_step, hence by the unfused
    boundary; the fused boundary kernels must draw the same numbers (csrc/boundary.hip promises bit-identity with the unfused kernels
    on the Philox stream)."""
    c = R.GROUPS[0]
    o = R.make_gauss(c, 1, steps=c["steps"], L=c["L"], dcl=c["dcl"], tag="groups")
    d = _operands(dev, o)
    seed, res = 80, {}
    word = torch.tensor([0x1234567], dtype=torch.int64, device=dev)
    plain = torch.stack([_philox(dev, o, seed, k) for k in range(o["steps"])])
    torch.cuda.synchronize()
    assert _L().set_rng_seed_delta(word.data_ptr()) == 0
    try:
        noise = torch.stack([_philox(dev, o, seed, k) for k in range(o["steps"])])
        for fam in ("f32_stack", "x3_f16"):
            for fused in ("1", "0"):
                _setenv(monkeypatch, dict(FAMILIES[fam]["env"], SET_AMD_FUSED_BOUNDARY=fused))
                res[fam, fused] = _run(dev, o, d, seed=seed, persistent=1, n_groups=2)
                _witness(res[fam, fused], o, fused == "1")
        torch.cuda.synchronize()
    finally:
        assert _L().set_rng_seed_delta(None) == 0
    assert not torch.equal(noise, plain)
    want = R.loop(o, noise=noise)[0]
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    assert float((R.loop(o, noise=plain)[0] - want).abs().max()) > 1e3 * bar  # the delta matters
    for key, out in res.items():
        e = float((_view(out, "x", o).double() - want).abs().max())
        assert e <= bar, ("the %s loop (fused boundary %s) ignores the seed delta" % key, e, bar)
    _same(res["f32_stack", "1"], res["f32_stack", "0"], ("x", "ws_x0", "ws_x1", "ws_skip"))
    # unregistered again: the plain stream
    _setenv(monkeypatch, FAMILIES["f32_stack"]["env"])
    out = _run(dev, o, d, seed=seed, persistent=1)
    assert float((_view(out, "x", o).double() - R.loop(o, noise=plain)[0]).abs().max()) <= bar


# ------------------------------------------------------------------------------------------------------------------------
# e. the range word of the two-piece boundary
# ------------------------------------------------------------------------------------------------------------------------
def _range_case(steps):
    return R.make_gauss(dict(name="range", B=2, M=80, T=68), 1, steps=steps, L=2, tag="range%d" % steps)


def test_x2_boundary_range_word_through_x_prime(dev, monkeypatch):
    """c2 = 2^20 at sid = 1 of a two-step loop with W_in scaled by 2^-30: x' of the first boundary leaves the fp16 split range while
    xin_next = ReLU(W_in x' + b_in) stays ordinary, so the stack of step 2 splits nothing large -> err_flag = 2 comes from the x' -> piece
    conversion alone: the same operands under SET_AMD_BOUNDARY_X2=0 leave the word 0.  The next ordinary call succeeds and matches.
    ops.diffusion_loop turns the word into SplitRangeError.  The same c2 at sid = 0 (the last step: x' is not split) raises nothing and
    x matches the model."""
    from set_amd import ops
    f = FAMILIES["x3_f16"]
    o = _range_case(2)
    o["W_in"] = o["W_in"] * 2.0 ** -30
    o["coef4"][1, 1] = 2.0 ** 20
    assert float((2.0 ** 20 * o["x_T"]).abs().max()) > 32768.0
    xin = R.loop(o)[1][1]["xin"]  # what the second step's stack splits
    assert float(xin.abs().max()) < 8.0
    d = _operands(dev, o)
    ordinary = dict(o, coef4=o["coef4"].clone())
    ordinary["coef4"][1, 1] = -0.4
    do = dict(d, coef4=ordinary["coef4"].to(dev))
    _setenv(monkeypatch, f["env"])
    _check_variant(o, "x3_f16")
    ok = _run(dev, ordinary, do)
    assert ok["err"] == 0
    assert _run(dev, o, d)["err"] == 2
    again = _run(dev, ordinary, do)
    assert again["err"] == 0
    _same(again, ok)
    x = o["x_T"].to(dev).contiguous()
    with pytest.raises(ops.SplitRangeError):
        ops.diffusion_loop(x=x, noise=d["noise"], seed=0, condproj=d["cp"], dstep=d["dstep"], coef4=d["coef4"], w_in=d["cw"]["W_in"],
                           b_in=d["b_in"], packs=d["packs"], w_skip=d["cw"]["W_skip"], b_skip=d["b_skip"], w_outp=d["cw"]["W_out"],
                           b_outp=d["b_out"], L=o["L"], steps=2, dilation_cycle_length=1, n_groups=1, persistent=True)
    _setenv(monkeypatch, dict(f["env"], SET_AMD_BOUNDARY_X2="0"))
    f32 = _run(dev, o, d)
    assert f32["err"] == 0, "the stack, not the boundary, raised the range word"
    want = R.loop(o)[0]
    assert float((_view(f32, "x", o).double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    # the last step does not split x'
    _setenv(monkeypatch, f["env"])
    last = _range_case(2)
    last["coef4"][0, 1] = 2.0 ** 20
    out = _run(dev, last, _operands(dev, last))
    assert out["err"] == 0
    # x_t of the last step: the model's first step (its error against the kernel's x' is amplified by 2^20: compare at the loop bar)
    want = R.loop(last)[0]
    assert float(want.abs().max()) > 32768.0
    assert float((_view(out, "x", last).double() - want).abs().max()) <= 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("through", ["s", "h"])
def test_x2_boundary_range_word_through_s_and_h(dev, monkeypatch, through):
    """One of the two is beyond 32768 and the other ordinary.  s: skip channel 0 carries a large output bias in every layer and column 0
    of W_skip is zero, so s = skip / sqrt(L) is large in that channel alone and h does not see it (phase 1 raises the word).  h: a large
    b_skip under an ordinary s (phase 2 raises it).  Under SET_AMD_BOUNDARY_X2=0 the same case leaves the word 0, so it is the boundary,
    not the stack's own guard, that fires; the fp32 boundary's x is then within its bar."""
    f = FAMILIES["x3_f16"]
    o = _range_case(1)
    if through == "s":
        o["W_skip"][:, 0] = 0.0
        o["bo"][:, DC] += 40000.0
    else:
        o["b_skip"] += 40000.0
    _, trace = R.loop(o)
    s_max = float(trace[0]["skip"].abs().max()) / math.sqrt(o["L"])
    h_max = float(R.head(trace[0]["skip"], o["L"], o["W_skip"], o["b_skip"], o["W_out"], o["b_out"])["h"].max())
    assert (s_max > 32768.0, h_max > 32768.0) == (through == "s", through == "h"), (s_max, h_max)
    d = _operands(dev, o)
    _setenv(monkeypatch, f["env"])
    _check_variant(o, "x3_f16")
    assert _run(dev, o, d)["err"] == 2
    _setenv(monkeypatch, dict(f["env"], SET_AMD_BOUNDARY_X2="0"))
    out = _run(dev, o, d)
    assert out["err"] == 0
    _check_last_step(dev, o, out, o["x_T"], o["noise"][0], False, "bounded", "range_" + through, "fp32 boundary")


def test_worst_ratios(dev):
    """Prints the worst |d| / bar per kernel and output and the e32 of every LOOP case (the numbers of DESIGN.md, "reverse loop sweep")."""
    for k, v in sorted(WORST.items()):
        print("worst |d| / bar  %-12s %-9s %.5f" % (k[0], k[1], v))
    for k, v in sorted(E32.items()):
        print("e32  %-18s %.3e" % (k, v))
    assert all(v <= 1.0 for v in WORST.values())
