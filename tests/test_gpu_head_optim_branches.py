"""GPU branch sweep of the training kernels that had none: the stutter head with its losses (csrc/stutter.hip: set_stutter_head_loss,
set_stutter_head_loss_bwd, set_stutter_head_bwd_reduce, set_stutter_head_scratch_floats), the step projections (csrc/train.hip:
set_step_proj_fwd, set_step_proj_bwd_dh, set_step_proj_bwd_dw, set_step_proj_bwd_scratch_floats), set_adamw, and the small entries set_l1_elem,
set_frame_weight, set_scale_bcast, set_row_sum, set_weight_norm_fold, set_gate and set_res_skip -- every case ONE raw call through the C ABI
against the float64 models of tests/head_optim_models.py (which tests/test_head_optim_reference.py ties to float64 torch), so that a failing
full-size gradient test can be pinned on one kernel.  Each case names the branch it reaches and the C condition it meets.

Every output and scratch buffer is a view 64 floats inside an allocation filled with a sentinel, and the WHOLE allocation is compared: the
view against the model, everything around it against what was there.  Scratch starts as NaN, so what a kernel leaves unwritten shows, and
every operand is read back after the call and must hold the bits it was given.

exact cases must equal the model bit for bit; bounded cases stay within the bars of head_optim_models.py (gamma(k + 2) sum |t| for plain
sums, 4 x the float32 mirror's error with a floor of 2 u |value| where a transcendental or a division enters).  The worst observed
error / bar per output goes to profiles/head_optim_branch_sweep.log when the module finishes; a ratio above 1 is a failure to investigate, not
a bar to widen."""
import itertools
import os

import numpy as np
import pytest
import torch

import head_optim_models as M
from test_gpu_conv_branches import SENTINEL, _ALIVE, _L, _p, _s, _keep_launch_operands, dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
G = M.G
NAN = float("nan")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "head_optim_branch_sweep.log")
WORST = {}   # (family, output) -> [calls, worst ratio, case]
EXACT = {}   # family -> calls that matched bit for bit


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


class Buf:
    """n floats at offset G inside an allocation of n + 2 G floats filled with SENTINEL; the view starts as `init` (an array, or a scalar
    such as NaN).  get() returns the view after checking that nothing around it changed."""

    def __init__(self, dev, n, init=None):
        self.n = int(n)
        self.full = torch.full((self.n + 2 * G,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.full[G:G + self.n]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.broadcast_to(np.asarray(init, dtype=F32).reshape(-1), (self.n,)).copy()).to(dev))
        _ALIVE.append(self.full)

    def ptr(self, off=0):
        assert 0 <= off < self.n
        return self.view.data_ptr() + 4 * off

    def get(self, shape=None):
        a = self.full.cpu().numpy()
        assert (a[:G] == F32(SENTINEL)).all() and (a[G + self.n:] == F32(SENTINEL)).all(), "written outside the buffer"
        v = a[G:G + self.n].copy()
        return v if shape is None else v.reshape(shape)

    def untouched(self, init):
        v = self.get()
        return np.array_equal(_bits(v), _bits(np.broadcast_to(np.asarray(init, dtype=F32).reshape(-1), (self.n,))))


class Operands:
    """device copies of the inputs of a call; check() reads them back: a kernel may not write its operands"""

    def __init__(self, dev, **arrays):
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items() if v is not None}
        self.dev = {k: torch.from_numpy(v).to(dev) for k, v in self.host.items()}

    def __getitem__(self, k):
        return _p(self.dev.get(k))

    def check(self):
        for k, v in self.host.items():
            got = self.dev[k].cpu().numpy()
            assert got.tobytes() == v.tobytes(), "operand %s changed" % k


def _ok(rc, what):
    from set_amd import _lib
    _lib.check(rc, what)


def _exact(family, got, want, what):
    want = np.asarray(want) + 0.0  # a sum that comes to zero is +0.0 in the kernels (they start from +0.0)
    assert np.array_equal(want.astype(F32).astype(F64), want.astype(F64)), (what, "the model is not representable")
    bad = _bits(got) != _bits(want.astype(F32))
    assert not bad.any(), (family, what, int(bad.sum()), np.flatnonzero(bad.reshape(-1))[:8])
    EXACT[family] = EXACT.get(family, 0) + 1


def _bounded(family, output, case, got, want, bar):
    """|got - want| <= bar per element (NaN only where the model has NaN); the worst ratio is printed and recorded before the assertion"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    bar = np.broadcast_to(np.asarray(bar, dtype=F64), want.shape)
    assert got.shape == want.shape, (family, output, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (family, output, case, "NaN where the model has none, or the reverse")
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / bar)
    worst = float(np.nanmax(ratio)) if ratio.size and not np.isnan(ratio).all() else 0.0
    rec = WORST.setdefault((family, output), [0, 0.0, case])
    rec[0] += 1
    if worst >= rec[1]:
        rec[1], rec[2] = worst, case
    print("%s %s %s: worst error / bar %.4f (error %.3e)" % (family, output, case, worst, float(np.max(err[~np.isnan(err)], initial=0.0))))
    assert worst <= 1.0, (family, output, case, worst)


@pytest.fixture(scope="module", autouse=True)
def _sweep_log():
    yield
    if not WORST:
        return
    lines = ["head / optimizer branch sweep (tests/test_gpu_head_optim_branches.py) on one MI355X", "",
             "exact mode: calls bit-identical to the float64 model over the whole guarded buffer, per family"]
    lines += ["  %-28s %4d" % (k, v) for k, v in sorted(EXACT.items())]
    lines += ["", "bounded mode: worst |kernel - model| / bar per output (bars: tests/head_optim_models.py)", "",
              "%-18s %-10s %5s  %-7s  %s" % ("family", "output", "calls", "worst", "case")]
    lines += ["%-18s %-10s %5d  %.4f   %s" % (f, o, n, w, c) for (f, o), (n, w, c) in sorted(WORST.items())]
    text = "\n".join(lines) + "\n"
    print(text)
    try:
        with open(LOG, "w") as f:
            f.write(text)
    except OSError:
        pass  # a read-only checkout: the table is in the output above


# =====================================================================================================================================
# stutter head
# =====================================================================================================================================
STUTTER = {c["name"]: c for c in M.STUTTER_CASES}
_STUTTER_REF = {}


def _stutter_ref(name):
    """operands, float64 model, float32 mirror and bars of a case: computed once, shared, never changed"""
    if name not in _STUTTER_REF:
        c = STUTTER[name]
        ops = M.stutter_operands(c)
        h, w, b, lab, dw0, db0 = ops
        model = M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"], dw0, db0)
        mirror = M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"], dw0, db0, dtype=F32)
        _STUTTER_REF[name] = (ops, model, M.stutter_bars(model, mirror))
    return _STUTTER_REF[name]


def _scalar(dev_ops, v):
    return None if v is None else np.array([v], dtype=F32)


@pytest.mark.parametrize("name", list(STUTTER))
def test_stutter_head_loss_forward(dev, name):
    """set_stutter_head_loss with labels: logits bit for bit (integer operands), stats = {ce, focal, n_valid}, and the scratch: the forward's
    B ceil(T / 64) partial rows of 3 are written, the rest of set_stutter_head_scratch_floats stays NaN."""
    c = STUTTER[name]
    B, C, T = c["B"], c["C"], c["T"]
    (h, w, b, lab, _, _), model, bars = _stutter_ref(name)
    L = _L()
    n_scr = L.set_stutter_head_scratch_floats(B, C, T)
    assert n_scr == M.stutter_scratch_floats(B, C, T)
    o = Operands(dev, h=h, w=w, b=b, lab=lab)
    logits, stats, scratch = Buf(dev, B * T * 3), Buf(dev, 3, NAN), Buf(dev, n_scr, NAN)
    _ok(L.set_stutter_head_loss(o["h"], o["w"], o["b"], o["lab"], logits.ptr(), stats.ptr(), scratch.ptr(), B, C, T, _s()), name)
    _exact("stutter_fwd", logits.get((B, T, 3)), model["logits"], "logits")
    st, sc = stats.get(), scratch.get()
    assert st[2] == model["n_valid"]
    if model["n_valid"] == 0:
        assert np.isnan(st[0]) and np.isfinite(st[1])
    _bounded("stutter_fwd", "ce", name, st[0], model["ce"], bars["ce"])
    _bounded("stutter_fwd", "focal", name, st[1], model["focal"], bars["focal"])
    rows = B * -(-T // 64)
    assert np.isfinite(sc[:rows * 3]).all() and np.isnan(sc[rows * 3:]).all()
    assert sc[1:rows * 3:3].sum() == model["n_valid"]  # the count partials are exact
    o.check()


@pytest.mark.parametrize("name", list(STUTTER))
def test_stutter_head_loss_backward_then_reduce(dev, name):
    """set_stutter_head_loss_bwd with dw = db = NULL (dh and the partial rows; g_ce / g_focal NULL where the case says so), then
    set_stutter_head_bwd_reduce onto NON-ZERO targets: it accumulates, in row order -- bit for bit the fp32 sum of the rows the first call
    left, and within the bar of the model."""
    c = STUTTER[name]
    B, C, T = c["B"], c["C"], c["T"]
    (h, w, b, lab, dw0, db0), model, bars = _stutter_ref(name)
    L = _L()
    n_scr = L.set_stutter_head_scratch_floats(B, C, T)
    stats = np.array([model["ce"], model["focal"], model["n_valid"]], dtype=F32)
    o = Operands(dev, h=h, w=w, lab=lab, logits=model["logits"].astype(F32), stats=stats, g_ce=_scalar(dev, c["g_ce"]),
                 g_fo=_scalar(dev, c["g_fo"]))
    dh, scratch = Buf(dev, B * C * T, NAN), Buf(dev, n_scr, NAN)
    _ok(L.set_stutter_head_loss_bwd(o["h"], o["w"], o["logits"], o["lab"], o["stats"], o["g_ce"], o["g_fo"], dh.ptr(), None, None,
                                    scratch.ptr(), B, C, T, _s()), name)
    rows, n = B * -(-T // 256), 3 * C + 3
    got_dh, sc = dh.get((B, C, T)), scratch.get()
    part = sc[:rows * n].reshape(rows, n)
    assert np.isnan(sc[rows * n:]).all()
    _bounded("stutter_bwd", "dh", name, got_dh, model["dh"], bars["dh"])
    _bounded("stutter_bwd", "part", name, part, model["part"], bars["part"])
    if model["n_valid"] == 0:
        assert not got_dh.any() and not part.any()  # a batch of pad rows: every gradient exactly 0
    dw, db = Buf(dev, 3 * C, dw0), Buf(dev, 3, db0)
    _ok(L.set_stutter_head_bwd_reduce(scratch.ptr(), dw.ptr(), db.ptr(), B, C, T, _s()), name)
    got_dw, got_db = dw.get((3, C)), db.get()
    want_dw, want_db = M.reduce_rows(part, dw0, db0)
    assert np.array_equal(_bits(got_dw), _bits(want_dw)) and np.array_equal(_bits(got_db), _bits(want_db))
    _bounded("stutter_reduce", "dw", name, got_dw, model["dw"], bars["dw"])
    _bounded("stutter_reduce", "db", name, got_db, model["db"], bars["db"])
    assert np.array_equal(_bits(scratch.get()), _bits(sc))  # the reduce reads its rows only
    o.check()


@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (3, 5, 65), (2, 33, 257), (9, 4, 449), (2, 192, 300)])
def test_stutter_head_bwd_reduce_integer_rows(dev, B, C, T):
    """set_stutter_head_bwd_reduce alone on integer-filled partial rows and integer targets: exact.  3 C + 3 = 6 .. 579 columns: one block
    with idle threads up to three blocks, the last one partial."""
    rng = np.random.default_rng(B + C + T)
    rows, n = B * -(-T // 256), 3 * C + 3
    n_scr = _L().set_stutter_head_scratch_floats(B, C, T)
    part = rng.integers(-3, 4, n_scr).astype(F32)
    dw0, db0 = rng.integers(-5, 6, 3 * C).astype(F32), rng.integers(-5, 6, 3).astype(F32)
    o = Operands(dev, part=part)
    dw, db = Buf(dev, 3 * C, dw0), Buf(dev, 3, db0)
    _ok(_L().set_stutter_head_bwd_reduce(o["part"], dw.ptr(), db.ptr(), B, C, T, _s()), "set_stutter_head_bwd_reduce")
    s = part[:rows * n].astype(F64).reshape(rows, n).sum(0)
    _exact("stutter_reduce", dw.get(), dw0 + s[:3 * C], "dw")
    _exact("stutter_reduce", db.get(), db0 + s[3 * C:], "db")
    o.check()


@pytest.mark.parametrize("name", ["b1_c1_t1_three_idle_waves_one_frame", "c5_t65_uneven_share_one_frame_second_tile",
                                  "c192_t300_model_width"])
def test_stutter_head_inference_form_labels_null(dev, name):
    """labels == NULL: the same logits, and neither stats nor scratch is written"""
    c = STUTTER[name]
    B, C, T = c["B"], c["C"], c["T"]
    (h, w, b, _, _, _), model, _ = _stutter_ref(name)
    o = Operands(dev, h=h, w=w, b=b)
    n_scr = _L().set_stutter_head_scratch_floats(B, C, T)
    logits, stats, scratch = Buf(dev, B * T * 3), Buf(dev, 3, NAN), Buf(dev, n_scr, NAN)
    _ok(_L().set_stutter_head_loss(o["h"], o["w"], o["b"], None, logits.ptr(), stats.ptr(), scratch.ptr(), B, C, T, _s()), name)
    _exact("stutter_fwd", logits.get((B, T, 3)), model["logits"], "logits")
    assert np.isnan(stats.get()).all() and np.isnan(scratch.get()).all()
    o.check()


# =====================================================================================================================================
# step projections
# =====================================================================================================================================
def _step_proj_calls(dev, L_, C, N, mode, run=("fwd", "dh", "dw")):
    """-> {entry: (rc, buffer contents)} of one call each, and the model"""
    h, flat, g, pre = M.step_proj_operands(L_, C, N, mode)
    ls = M.step_proj_stride(C)
    o = Operands(dev, h=h, flat=flat, g=g)
    L = _L()
    w_ptr, b_ptr = o["flat"], o["flat"] + 4 * C * C
    res = {}
    if "fwd" in run:
        out = Buf(dev, N * L_ * C, NAN)
        rc = L.set_step_proj_fwd(o["h"], w_ptr, ls, b_ptr, ls, out.ptr(), L_, C, N, _s())
        res["fwd"] = (rc, out)
    if "dh" in run:
        n_scr = L.set_step_proj_bwd_scratch_floats(L_, C, N)
        assert n_scr == L_ * (C // 64) * C * N
        dh, scratch = Buf(dev, C * N, NAN), Buf(dev, max(n_scr, 1), NAN)
        rc = L.set_step_proj_bwd_dh(o["g"], w_ptr, ls, dh.ptr(), scratch.ptr(), L_, C, N, _s())
        res["dh"] = (rc, dh)
        res["scratch"] = (rc, scratch)
    if "dw" in run:
        grad = Buf(dev, L_ * ls, pre)
        rc = L.set_step_proj_bwd_dw(o["h"], o["g"], grad.ptr(), ls, grad.ptr(C * C), ls, L_, C, N, _s())
        res["dw"] = (rc, grad)
    torch.cuda.synchronize()
    o.check()
    return res, M.step_proj(h, flat, g, pre, L_, C, N), pre


def _step_proj_compare(name, mode, res, model, L_, C, N, pre, entries):
    for entry, key, shape in (("fwd", "out", (N, L_ * C)), ("dh", "dh", (C, N)), ("dw", "grad", (-1,))):
        if entry not in entries:
            continue
        rc, buf = res[entry]
        _ok(rc, "set_step_proj_" + entry)
        got = buf.get(shape)
        want, abs_sum, k = model[key]
        if mode == "exact":
            _exact("step_proj_" + entry, got, want, name)
        else:
            _bounded("step_proj", key, name, got, want, M.sum_bar(k, abs_sum))
        if entry == "dw":  # the gaps between one layer's bias and the next layer's weight
            ls = M.step_proj_stride(C)
            gaps = np.concatenate([np.arange(l * ls + C * C + C, (l + 1) * ls) for l in range(L_)])
            assert np.array_equal(_bits(got[gaps]), _bits(pre[gaps]))
        if entry == "dh":  # the partial rows: all of set_step_proj_bwd_scratch_floats is written, nothing beyond
            assert np.isfinite(res["scratch"][1].get()).all()


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("name,L_,C,N", M.STEP_PROJ_CASES)
def test_step_proj_entries(dev, name, L_, C, N, mode):
    """set_step_proj_fwd / _bwd_dh / _bwd_dw, one call each, on parameters at one stride inside a flat buffer with a gap; dw / db accumulate
    into non-zero targets; a second run gives the same bits."""
    res, model, pre = _step_proj_calls(dev, L_, C, N, mode)
    _step_proj_compare(name, mode, res, model, L_, C, N, pre, ("fwd", "dh", "dw"))
    if mode == "bounded":
        again, _, _ = _step_proj_calls(dev, L_, C, N, mode)
        for entry in ("fwd", "dh", "dw"):
            assert np.array_equal(_bits(res[entry][1].get()), _bits(again[entry][1].get())), entry


@pytest.mark.parametrize("name,L_,C,N,refused", M.STEP_PROJ_REFUSED)
def test_step_proj_refusals_leave_the_outputs_alone(dev, name, L_, C, N, refused):
    """C % 64 != 0, N > 64, and (the forward alone) C * NT * 4 > 64 KiB of LDS: SET_E_UNSUPPORTED before any launch.  The two backward
    entries stage nothing of that size and must RUN C = 320."""
    res, model, pre = _step_proj_calls(dev, L_, C, N, "exact")
    for entry in ("fwd", "dh", "dw"):
        rc, buf = res[entry]
        if entry in refused:
            assert rc == M.E_UNSUPPORTED, (entry, rc)
            assert buf.untouched(pre if entry == "dw" else NAN)
            if entry == "dh":
                assert res["scratch"][1].untouched(NAN)
    _step_proj_compare(name, "exact", res, model, L_, C, N, pre, [e for e in ("fwd", "dh", "dw") if e not in refused])


# =====================================================================================================================================
# AdamW
# =====================================================================================================================================
ADAMW = {c["name"]: c for c in M.ADAMW_CASES}


@pytest.mark.parametrize("name", list(ADAMW))
def test_adamw(dev, name):
    """set_adamw in place on p, m, v (one call per step), each compared element by element with the float64 model"""
    c = ADAMW[name]
    n, hy = c["n"], c["hyper"]
    model = M.adamw_run(c)
    bars = [M.mirror_bar(a, b) for a, b in zip(model, M.adamw_run(c, dtype=F32))]
    p0, g, m0, v0, sumsq, max_norm, gs = M.adamw_operands(c)
    p, m, v = Buf(dev, n, p0), Buf(dev, n, m0), Buf(dev, n, v0)
    for k in range(c["steps"]):
        if k:
            _, g, _, _, sumsq, max_norm, gs = M.adamw_operands(c, k)
        o = Operands(dev, g=g, sumsq=None if sumsq is None else np.array([sumsq], dtype=F32))
        _ok(_L().set_adamw(p.ptr(), o["g"], m.ptr(), v.ptr(), n, hy["lr"], hy["beta1"], hy["beta2"], hy["eps"], hy["wd"], c["step"] + k,
                           o["sumsq"], max_norm, gs, _s()), name)
        torch.cuda.synchronize()
        o.check()
    for what, buf, want, bar in zip(("p", "m", "v"), (p, m, v), model, bars):
        _bounded("adamw", what, name, buf.get(), want, bar)


# =====================================================================================================================================
# small entries
# =====================================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("outs", ["absd", "sgn", "both"])
def test_l1_elem(dev, n, outs):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    b[::7] = a[::7]  # d = 0: |d| = +0.0 and sign +0.0
    o = Operands(dev, a=a, b=b)
    absd, sgn = (Buf(dev, n, NAN) if outs != "sgn" else None), (Buf(dev, n, NAN) if outs != "absd" else None)
    _ok(_L().set_l1_elem(o["a"], o["b"], absd.ptr() if absd else None, sgn.ptr() if sgn else None, n, _s()), "set_l1_elem")
    want = M.l1_elem(a, b)
    for buf, w, what in zip((absd, sgn), want, ("absd", "sgn")):
        if buf:
            _exact("l1_elem", buf.get(), w, (what, n, outs))
    assert not _bits(want[1][::7]).any()
    o.check()


@pytest.mark.parametrize("frames,Mm", [(1, 1), (1, 80), (257, 1), (257, 80)])
def test_frame_weight(dev, frames, Mm):
    rng = np.random.default_rng(frames + Mm)
    x = rng.standard_normal((frames, Mm)).astype(F32)
    if frames > 4:
        x[1], x[2] = 0.0, -0.0                    # an all-zero frame, a frame of -0.0
        x[3], x[3, 0], x[3, -1] = 0.0, 2.5, -2.5  # (+a, -a) must give 1 (M = 1: the lone -a)
        x[frames - 1] = 0.0                       # the one frame of the second block
    else:
        x[0, 0] = -0.0 if Mm == 1 else 2.5
    o = Operands(dev, x=x)
    w = Buf(dev, frames, NAN)
    _ok(_L().set_frame_weight(o["x"], w.ptr(), frames, Mm, _s()), "set_frame_weight")
    want = M.frame_weight(x)
    _exact("frame_weight", w.get(), want, (frames, Mm))
    if frames > 4:
        assert want[1:4].tolist() == [0.0, 0.0, 1.0] and want[-1] == 0.0
    o.check()


@pytest.mark.parametrize("inner", [1, 80])
@pytest.mark.parametrize("has_w,has_dev", list(itertools.product([False, True], repeat=2)))
def test_scale_bcast(dev, inner, has_w, has_dev):
    n = 300 * inner if inner == 1 else 3 * inner + 17  # 300 / 257: two blocks, the last partial; the last row of w is partial too
    rng = np.random.default_rng(inner)
    a, w, sd = rng.standard_normal(n).astype(F32), rng.standard_normal(-(-n // inner)).astype(F32), F32(1.7)
    o = Operands(dev, a=a, w=w if has_w else None, sd=np.array([sd]) if has_dev else None)
    out = Buf(dev, n, NAN)
    _ok(_L().set_scale_bcast(o["a"], o["w"], out.ptr(), n, inner, o["sd"], 0.3, _s()), "set_scale_bcast")
    _exact("scale_bcast", out.get(), M.scale_bcast(a, w if has_w else None, inner, sd if has_dev else None, 0.3), (inner, has_w, has_dev))
    o.check()


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("T", [1, 63, 64, 65])
@pytest.mark.parametrize("mode", ["exact", "bounded"])
def test_row_sum(dev, rows, T, mode):
    """one wave per row, four rows per block (rows 1 and 5: the last block is partial), lanes stride 64 over T; scale 0.75"""
    rng = np.random.default_rng(10 * rows + T)
    x = rng.integers(-3, 4, (rows, T)).astype(F32) if mode == "exact" else rng.standard_normal((rows, T)).astype(F32)
    o = Operands(dev, x=x)
    out = Buf(dev, rows, NAN)
    _ok(_L().set_row_sum(o["x"], out.ptr(), rows, T, 0.75, _s()), "set_row_sum")
    want, abs_sum = M.row_sum(x, 0.75)
    if mode == "exact":
        _exact("row_sum", out.get(), want, (rows, T))
    else:
        _bounded("row_sum", "out", "rows%d_T%d" % (rows, T), out.get(), want, M.sum_bar(T, abs_sum))
    o.check()


@pytest.mark.parametrize("n0", [1, 3])
@pytest.mark.parametrize("inner", [1, 255, 256, 3584])
def test_weight_norm_fold(dev, n0, inner):
    """one block per dim-0 slice, 256 threads stride over `inner` (1: 255 idle; 255 / 256: the edge; 3584 = 14 trips: HiFi-GAN's largest)"""
    rng = np.random.default_rng(n0 + inner)
    v, g = rng.standard_normal((n0, inner)).astype(F32), rng.standard_normal(n0).astype(F32)
    o = Operands(dev, g=g, v=v)
    w = Buf(dev, n0 * inner, NAN)
    _ok(_L().set_weight_norm_fold(o["g"], o["v"], w.ptr(), n0, inner, _s()), "set_weight_norm_fold")
    want = M.weight_norm_fold(g, v)
    _bounded("weight_norm_fold", "w", "n0_%d_inner%d" % (n0, inner), w.get((n0, inner)), want, M.mirror_bar(want, M.weight_norm_fold(g, v, F32)))
    o.check()


def test_gate(dev):
    B, C, T = 2, 3, 43  # 258 elements: two blocks, the second with two
    y = np.random.default_rng(5).standard_normal((B, 2 * C, T)).astype(F32) * F32(3.0)
    o = Operands(dev, y=y)
    z = Buf(dev, B * C * T, NAN)
    _ok(_L().set_gate(o["y"], z.ptr(), B, C, T, _s()), "set_gate")
    want = M.gate(y)
    _bounded("gate", "z", "b2_c3_t43", z.get((B, C, T)), want, M.mirror_bar(want, M.gate(y, F32)))
    o.check()


@pytest.mark.parametrize("first", [1, 0])
def test_res_skip(dev, first):
    """first = 1: skip = o[:, C:] and the previous skip (NaN here) is not read; first = 0: skip += o[:, C:], one rounding"""
    B, C, T = 2, 3, 43
    rng = np.random.default_rng(6 + first)
    x, oo, sk = (rng.standard_normal(s).astype(F32) for s in ((B, C, T), (B, 2 * C, T), (B, C, T)))
    o = Operands(dev, x=x, o=oo)
    x_out, skip = Buf(dev, B * C * T, NAN), Buf(dev, B * C * T, NAN if first else sk)
    _ok(_L().set_res_skip(o["x"], o["o"], x_out.ptr(), skip.ptr(), B, C, T, first, _s()), "set_res_skip")
    want_x, want_s = M.res_skip(x, oo, sk, bool(first))
    _exact("res_skip", skip.get((B, C, T)), want_s, ("skip", first))
    _bounded("res_skip", "x_out", "first%d" % first, x_out.get((B, C, T)), want_x, M.mirror_bar(want_x, M.res_skip(x, oo, sk, bool(first), F32)[0]))
    o.check()
