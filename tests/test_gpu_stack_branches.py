"""GPU sweep of every form of the DiffNet inference layer stack -- the per-layer kernel (set_diffnet_layer) and the six persistent kernels
behind set_diffnet_stack (csrc/diffnet.hip, csrc/diffnet_x3.hip), each in every form plan_stack (csrc/diffusion_loop.hip) can pick --
against the float64 model of tests/test_stack_reference.py, where the case table lives (each row names the form it must reach and the C
conditions it meets) and where the CPU half of the argument runs (plans pinned, inventory, budgets).  Same shape as the other sweeps:
SetDiffnetStackArgs is filled by hand; xa, xb, skip and the training outputs are views at offset G inside sentinel-filled buffers that are
compared WHOLE; the targets start as NaN (the first layer must not read what skip held); condproj is a view with its own batch stride
(and, for one row, 4 bytes off its alignment) inside a sentinel buffer; every operand -- condproj, the step table, the biases, every
weight image -- is compared with its copy after the launch; sync_ws starts as -1 everywhere.

Which form ran: the words of sync_ws (csrc/stack_queue.h).  A launch clears exactly stack_sync_words() words, the queue kernels leave
tasks + workers in the task counter and the layer count (x3v: 8 waves per layer) in each tile flag -- all functions of the tiling
(tile width, concatenated frame axis, column blocks per tile) that test_stack_reference.tiling mirrors, so a plan that fell back to
another form cannot pass for the one a row names.  sync_ws[1] (a wait gave up) and the error word must be 0.

  exact    condproj +40 on the sigmoid rows, integer operands: GEMM 1 with non-zero dilated weights decides z in {-1, 0, +1}; the skip sum
           is compared bit for bit for every L, x_out bit for bit for L = 1 (one rounding) and within its bar for L > 1 (the model asserts
           the margins that make z independent of the rounding of x_l).  Weight families `sel` and `dense`.
  bounded  Gaussian operands at two scales inside the bars test_stack_reference.bars composes; nothing is fitted to what a kernel returns.
The gate values the exact mode stands on are pinned per form by the first test.  The worst |d| / bar per form and output goes to WORST,
printed by the last test (recorded in profiles/stack_branch_sweep.log).

The images come from set_pack_diffnet_layer / _wino / _x3 per layer and, for L > 1, from set_pack_diffnet_layers on weights stored with
a padded layer stride, which must give the same fp32 and Winograd images; the row-split images from ops.split_images.

Not swept, on purpose: the time-out contract (SET_AMD_FAULT_TILE), SET_AMD_STACK_GRID, the full-chip thresholds of the plan (pinned on the
CPU only), the 2 GiB offset limits, the bf16 layer bodies and the step boundaries (their own sweeps)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_stack_reference as S
from test_gpu_conv_branches import SENTINEL, _ALIVE, _L, _keep_launch_operands, _p, _report, _s, dev  # noqa: F401

pytestmark = pytest.mark.gpu

G = 64
DC = 256
WORST = {}    # (form, output) -> worst observed |d| / bar of bounded mode
PIN = [0.0, 16.0, -16.0, 32.0, -32.0, 64.0, -64.0, 1024.0, -1024.0, 70000.0, -70000.0]  # filter pre-activations of the pin; the gate rows sit at 40


def _setenv(monkeypatch, env):
    for n in S.SWITCHES:
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _images(dev, o, x3_mode):
    """Every weight image of the case's own weights.  L > 1: the fp32 and Winograd images also through the one-launch packer on weights
    stored with a padded layer stride; both ways must agree bit for bit."""
    from set_amd import _lib, ops
    L = o["L"]
    w1, w2 = torch.empty(L, 512 * 768, device=dev), torch.empty(L, 512 * 256, device=dev)
    w1w, w2w = torch.empty(L, 512 * 256 * 4, device=dev), torch.empty(L, 512 * 256, device=dev)
    wx3 = ops.SplitOperandImages(L, x3_mode, dev) if x3_mode else None
    raw = []
    for l in range(L):
        wd, wo = o["Wd"][l].to(dev).contiguous(), o["Wo"][l].to(dev).contiguous()
        raw += [wd, wo]
        ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        ops.pack_diffnet_layer_wino(wd, wo, w1w[l], w2w[l])
        if wx3 is not None:
            wx3.pack(l, wd, wo)
    if L > 1:
        sd, so = 512 * DC * 3 + 5, 512 * DC + 3
        fd, fo = torch.full((L * sd,), SENTINEL, device=dev), torch.full((L * so,), SENTINEL, device=dev)
        for l in range(L):
            fd[l * sd:l * sd + 512 * DC * 3] = raw[2 * l].flatten()
            fo[l * so:l * so + 512 * DC] = raw[2 * l + 1].flatten()
        alt = [torch.empty_like(t) for t in (w1, w2, w1w, w2w)]
        _lib.check(_L().set_pack_diffnet_layers(_p(fd), _p(fo), sd, so, _p(alt[0]), _p(alt[1]), _p(alt[2]), _p(alt[3]), L, _s()), "set_pack_diffnet_layers")
        torch.cuda.synchronize()
        for a, b, n in zip(alt, (w1, w2, w1w, w2w), ("w1p", "w2p", "w1w", "w2w")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "set_pack_diffnet_layers and the per-layer packer disagree on " + n
        w1, w2, w1w, w2w = alt
    w1s, w2s = ops.split_images(w1, w2)
    bd, bo = o["bd"].to(dev).contiguous(), o["bo"].to(dev).contiguous()
    return ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo, w1w=w1w, w2w=w2w, w1s=w1s, w2s=w2s, wx3=wx3)


def _flat(n, fill=SENTINEL):
    t = torch.full((G + n + G,), SENTINEL)
    t[G:G + n] = fill
    return t


def _run(dev, monkeypatch, c, o):
    """One launch (form `layer`: L launches of the per-layer kernel) of the operands `o` in the row's form.  Returns the whole buffers on
    the CPU, sync_ws and the error word."""
    from set_amd import _lib, ops
    f = S.FORMS[c["form"]]
    _setenv(monkeypatch, f["env"])
    B, T, L, dcl = c["B"], c["T"], c["L"], c["dcl"]
    n = B * DC * T
    nan = float("nan")
    cpu = dict(xa=_flat(n), xb=_flat(n, nan), skip=_flat(n, nan))
    cpu["xa"][G:G + n] = o["x0"].flatten()
    if c["train"]:
        cpu.update(x_all=_flat((L + 1) * n, nan), save_y=_flat(2 * L * n, nan), save_z=_flat(L * n, nan))
        cpu["x_all"][G:G + n] = o["x0"].flatten()
        cpu["xa"][G:G + n] = nan  # not an operand of the training forward: must stay as it is
    d = {k: v.to(dev) for k, v in cpu.items()}
    bs = S.cp_bs(c)
    cpf = torch.full((G + c["cp_off"] + B * bs + G,), SENTINEL)
    cpf[G + c["cp_off"]:].as_strided((B, L * 512, T), (bs, T, 1)).copy_(o["cp"])
    cpd, tab = cpf.to(dev), o["tab"].to(dev).contiguous()
    packs = _images(dev, o, f["x3_mode"])
    ro = [cpd, tab] + [v for v in packs[:8] if v is not None] + ([packs.wx3.data] if packs.wx3 is not None else [])
    before = [t.clone() for t in ro]
    ws = torch.full((ops.sync_ws_size(B, T) + 16,), -1, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    cp_ptr, d_ptr, ncol = _p(cpd) + 4 * (G + c["cp_off"]), _p(tab) + 4 * c["col"], c["ncol"]
    view = lambda k: d[k][G:G + n].view(B, DC, T)
    if c["form"] == "layer":
        for l in range(L):
            xi, xo = (view("xb"), view("xa")) if l & 1 else (view("xa"), view("xb"))
            ops.diffnet_layer(xi, cp_ptr + 4 * l * 512 * T, bs, d_ptr + 4 * l * DC * ncol, c["d_bs"], ncol, packs.w1p[l], packs.b_dil[l], packs.w2p[l],
                              packs.b_out[l], xo, view("skip"), o["dils"][l], l == 0)
    else:
        a = _lib.SetDiffnetStackArgs()
        z_ws = ops._set_images(a, packs, B, T, dcl, dev)
        _ALIVE.append(z_ws)
        a.xa, a.xb, a.skip = (_p(d[k]) + 4 * G for k in ("xa", "xb", "skip"))
        if c["train"]:
            a.x_all, a.save_y, a.save_z = (_p(d[k]) + 4 * G for k in ("x_all", "save_y", "save_z"))
        a.condproj, a.dstep = cp_ptr, d_ptr
        a.cp_bs, a.cp_ls = bs, 512 * T
        a.d_bs, a.d_cs, a.d_ls = c["d_bs"], ncol, DC * ncol
        a.B, a.T, a.L, a.dilation_cycle_length = B, T, L, dcl
        a.sync_ws, a.err_flag = _p(ws), _p(err)
        _lib.check(_L().set_diffnet_stack(C.byref(a), _s()), "set_diffnet_stack")
    torch.cuda.synchronize()
    for t, b in zip(ro, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "an operand changed"
    out = {k: v.cpu() for k, v in d.items()}
    out["ws"], out["err"] = ws.cpu(), int(err.item())
    return out


def _tiling_word(c, out):
    """sync_ws against the tiling the row's plan must have used on this device."""
    ws = out["ws"]
    assert out["err"] == 0, "error word %d" % out["err"]
    if c["form"] == "layer":
        assert bool((ws == -1).all())
        return
    n_cu = _n_cu()
    p = S.row_plan(c, n_cu)
    f = S.FORMS[c["form"]]
    assert p["family"] == f["family"] and (p["x3_ncb"] if p["x3_wino"] else 0) == f["x3w"], (c["name"], p, n_cu)
    t = S.tiling(c, p, n_cu)
    nt = t["ntiles"]
    assert int(ws[1]) == 0, "a dependency wait gave up"
    assert bool((ws[t["words"]:] == -1).all()) and bool((ws[:t["words"]] != -1).all()), \
        (c["name"], "the launch did not clear exactly the %d words of its tiling" % t["words"], ws[:t["words"] + 4].tolist())
    assert int(ws[0]) == t["counter"], (c["name"], "task counter %d, the tiling of %s leaves %d" % (int(ws[0]), t["kind"], t["counter"]))
    if t["flag"] is not None:
        assert bool((ws[4:4 + nt] == t["flag"]).all()), (c["name"], ws[4:4 + nt].tolist(), t["flag"])
    if t["kind"] == "wino":
        assert bool((ws[4 + nt:4 + nt + 12] == 0).all())


def _cmp(c, tag, name, got, want, bar, shape=None, record=False):
    """Whole-buffer comparison: `want` / `bar` cover the view (NaN in `want`: the element must still be NaN), the guards must still hold
    the sentinel.  A failure names batch, row, frame (and layer, for the training outputs)."""
    w = torch.full(got.shape, SENTINEL, dtype=torch.float64)
    b = torch.zeros(got.shape, dtype=torch.float64)
    n = want.numel()
    w[G:G + n] = want.double().flatten()
    b[G:G + n] = bar.double().flatten() if torch.is_tensor(bar) else bar
    keep = torch.isnan(w)
    assert bool(torch.isnan(got[keep]).all()), (c["name"], tag, name, "an element that must stay NaN was written")
    g = torch.where(keep, torch.zeros_like(got), got)
    w = torch.where(keep, torch.zeros_like(w), w)
    bad = _report("%s.%s" % (c["name"], name), tag, g, w, b)
    if bad.numel():
        i = int(bad[0]) - G
        where = np.unravel_index(i, tuple(want.shape)) if 0 <= i < n else ("guard", i)
        raise AssertionError((c["name"], tag, name, "%d elements outside; first at (layer,) batch, row, frame = %s: got %r, want %r, bar %.3e" % (
            bad.numel(), tuple(int(v) for v in where), float(g[bad[0]]), float(w[bad[0]]), float(b[bad[0]]))))
    if record and bool((b > 0).any()):
        key = (c["form"] + ("" if c["L"] <= 2 or c["train"] else "(L>2)"), name)
        WORST[key] = max(WORST.get(key, 0.0), float(((g.double() - w).abs() / (b + 1e-300))[b > 0].max()))


def _x_out_exact(t):
    """fl32((x + o) fl32(2^-1/2)) where x + o is an fp32 number: one rounding."""
    s = (t["xin"] + t["o"][:, :DC]).numpy().astype(np.float32)
    assert bool((s.astype(np.float64) == (t["xin"] + t["o"][:, :DC]).numpy()).all())
    return torch.from_numpy(s * np.float32(S.RSQRT2))


def _forced(c, o, out):
    """Bounded mode, teacher-forced wherever the launch leaves a layer's input visible: every layer of the training forward (x_all), the last
    layer of an inference launch (the buffer it read).  The model and its bars then start again from what the kernel itself wrote."""
    B, T, L = c["B"], c["T"], c["L"]
    n = B * DC * T
    if c["train"]:
        forced = {l: out["x_all"][G + l * n:G + (l + 1) * n].view(B, DC, T) for l in range(1, L)}
    elif L > 1:
        forced = {L - 1: out["xa" if L % 2 else "xb"][G:G + n].view(B, DC, T)}
    else:
        return o["tr"], ()
    if not all(bool(torch.isfinite(v).all()) for v in forced.values()):
        return o["tr"], ()  # (the comparison below reports the NaN)
    tr = S.stack(o["x0"], o["cp"], o["d"], o["Wd"], o["bd"], o["Wo"], o["bo"], o["dils"], forced=forced)
    return tr, tuple(forced)


def _check(c, o, out, tag):
    exact = o["mode"] == "exact"
    L, num = c["L"], S.numerics(c)
    tr, forced = (o["tr"], ()) if exact else _forced(c, o, out)
    b = S.bars(tr, o, num, exact0=exact, forced=forced)
    rec = not exact
    last, zero = tr[-1], 0.0
    _cmp(c, tag, "skip", out["skip"], last["skip"], zero if exact else b[-1]["skip"], record=rec)
    x_want, x_bar = (_x_out_exact(last), zero) if exact and L == 1 else (last["x"], b[-1]["x"])
    nanv = torch.full_like(last["x"], float("nan"))
    if c["train"]:
        _cmp(c, tag, "xa", out["xa"], nanv, zero)
        _cmp(c, tag, "xb", out["xb"], nanv, zero)
        xs = [o["x0"].double()] + [_x_out_exact(t).double() if exact and l == 0 else t["x"] for l, t in enumerate(tr)]
        bx = [torch.zeros_like(xs[0])] + [torch.zeros_like(xs[0]) if exact and l == 0 else b[l]["x"] for l in range(L)]
        _cmp(c, tag, "x_all", out["x_all"], torch.stack(xs), torch.stack(bx), record=rec)
        _cmp(c, tag, "save_y", out["save_y"], torch.stack([t["y"] for t in tr]), torch.stack([bb["y"] for bb in b]), record=rec)
        _cmp(c, tag, "save_z", out["save_z"], torch.stack([t["z"] for t in tr]), zero if exact else torch.stack([bb["z"] for bb in b]), record=rec)
    else:
        fin, other = ("xb", "xa") if L % 2 else ("xa", "xb")
        _cmp(c, tag, "x_out", out[fin], x_want, x_bar, record=rec)
        if L == 1:
            _cmp(c, tag, "x_in", out[other], o["x0"], zero)  # still the operand
        else:  # the buffer the last layer read: the output of the layer before it
            prev = (_x_out_exact(tr[0]), zero) if exact and L == 2 else (tr[L - 2]["x"], b[L - 2]["x"])
            _cmp(c, tag, "x_prev", out[other], prev[0], prev[1], record=rec)
    _tiling_word(c, out)


# ------------------------------------------------------------------------------------------------------------------------
# the gate values the exact mode stands on
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [f for f in S.FORMS if f != "x3v_out"])  # (x3v_out names no kernel of its own: the direct two-piece form)
def test_gate_values_of_the_exact_mode(dev, monkeypatch, form):
    """Zero dilated weights, so y is the condproj: 40 on the sigmoid rows, the PIN points on the filter rows; W_out routes z of channel r to
    skip row r.  The form's sigmoid(40) tanh(y_f) must be exactly 0 at 0 and +-1 from 16 on, whatever the magnitude (the exact mode's
    pre-activations reach 4096 x 15), and x_out = fl32(x fl32(2^-1/2))."""
    B, T = 1, 66
    c = S._row(form, B, T, 1, 1, "gate pin")
    g = torch.Generator().manual_seed(7)
    pt = torch.tensor(PIN)[torch.arange(DC) % len(PIN)]
    cp = torch.zeros(B, 512, T)
    cp[:, :DC], cp[:, DC:] = 40.0, pt[None, :, None]
    Wo = torch.zeros(1, 512, DC, 1)
    Wo[0, DC + torch.arange(DC), torch.arange(DC), 0] = 1.0
    o = dict(c, mode="exact", dils=[1], x0=S.ints(g, (B, DC, T), -3, 3), tab=torch.zeros(DC, 1), d=torch.zeros(1, B, DC), Wd=torch.zeros(1, 512, DC, 3),
             bd=torch.zeros(1, 512), Wo=Wo, bo=torch.zeros(1, 512), cp=cp)
    out = _run(dev, monkeypatch, c, o)
    z = out["skip"][G:G + B * DC * T].view(B, DC, T)
    for v in PIN:
        print("GATE %s y_f = %g: z in %s" % (form, v, sorted(set(z[:, pt == v].flatten().tolist()))))
    want = torch.sign(pt)[None, :, None].expand(B, DC, T)
    _cmp(c, "pin", "skip", out["skip"], want, 0.0)
    _cmp(c, "pin", "x_out", out["xb"], torch.from_numpy(o["x0"].numpy() * np.float32(S.RSQRT2)), 0.0)
    _tiling_word(c, out)


# ------------------------------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,fam", S.EXACT_RUNS, ids=["%s-%s" % (c["name"], fam) for c, fam in S.EXACT_RUNS])
def test_stack_form_exact(dev, monkeypatch, c, fam):
    o = S.make_exact(c, fam)
    _check(c, o, _run(dev, monkeypatch, c, o), "exact-" + fam)


BOUNDED_RUNS = [(c, s) for c in S.CASES if c["bounded"] for s in S.SCALES]


@pytest.mark.parametrize("c,scale", BOUNDED_RUNS, ids=["%s-x%g" % (c["name"], s) for c, s in BOUNDED_RUNS])
def test_stack_form_bounded(dev, monkeypatch, c, scale):
    o = S.make_gauss(c, scale)
    _check(c, o, _run(dev, monkeypatch, c, o), "bounded-x%g" % scale)


def test_a_wrong_step_column_is_far_outside_the_bar(dev, monkeypatch):
    """The witness of the step-table rows: the same launch reading the column next to the row's (1000 away) moves the typical element of
    x_1 by more than ten times its bar, and the row's check fails."""
    c = S.BY_NAME["direct32_B2_T31_L2_d2"]
    o = S.make_gauss(c, 1.0)
    out = _run(dev, monkeypatch, dict(c, col=c["col"] + 1), o)
    got = out["xa"][G:-G].view(c["B"], DC, c["T"]).double()  # L = 2: the buffer layer 1 read holds x_1
    b = S.bars(o["tr"], o, "f32")[0]["x"]
    ratio = float(((got - o["tr"][0]["x"]).abs() / b).median())
    print("wrong step column: median |d| / bar of x_1 = %.1f" % ratio)
    assert ratio > 10  # (not one stray element: the typical one, by more than an order of magnitude)
    with pytest.raises(AssertionError):
        _check(c, o, out, "wrong-column")


def test_worst_fractions(dev):
    """Not an assertion of its own: prints the worst observed |d| / bar per form and output of the bounded runs above."""
    for (form, name), v in sorted(WORST.items()):
        print("WORST %-16s %-8s %.3e" % (form, name, v))
    assert all(v <= 1.0 for v in WORST.values())
