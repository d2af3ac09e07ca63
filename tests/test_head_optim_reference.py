"""CPU checks of tests/head_optim_models.py, on which tests/test_gpu_head_optim_branches.py stands: the float64 models equal float64 torch
(Linear -> CrossEntropyLoss(ignore_index=2) + the focal formula; torch.optim.AdamW after clip_grad_norm_; F.linear), the exact-mode operands
are exact, the float32 mirrors stay near the models, every bounded bar is below 1/8 of the effect of each planted fault on the case meant to
catch it, and every C entry point of csrc/*.hip is named in some GPU test module (or is on the short exemption list below)."""
import fnmatch
import glob
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_optim_models as M

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUTTER = {c["name"]: c for c in M.STUTTER_CASES}
ADAMW = {c["name"]: c for c in M.ADAMW_CASES}


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)  # a copy: the optimizer steps in place


def _close(got, want, rel=1e-11):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape
    scale = max(1e-300, float(np.abs(want).max()))
    assert float(np.abs(got - want).max()) <= rel * scale, (float(np.abs(got - want).max()), scale)


# ---- stutter head ---------------------------------------------------------------------------------------------------------------------------
def _torch_head(h, w, b, lab, g_ce, g_fo):
    """float64 torch: nn.Linear(C, 3) per frame, nn.CrossEntropyLoss(ignore_index=2), MultiFocalLoss (alpha = {5e-3, 1, 0}, gamma 3, smooth
    1e-6, mean over all B T rows) with log p = log_softmax, as test_gpu_stutter.py restates the reference."""
    h, w, b = (_t(a).requires_grad_(True) for a in (h, w, b))
    lab = torch.from_numpy(np.clip(lab, 0, 2))
    with torch.enable_grad():
        z = torch.einsum("bct,jc->btj", h, w) + b
        ce = F.cross_entropy(z.reshape(-1, 3), lab.reshape(-1), ignore_index=2)
        lpy = torch.log_softmax(z, -1).gather(-1, lab[..., None])[..., 0]
        alpha = torch.tensor(M.ALPHA, dtype=torch.float64)[lab]
        focal = (-alpha * (1 - (lpy.exp() + 1e-6)) ** 3 * (lpy + 1e-6)).mean()
        ((g_ce or 0.0) * ce + (g_fo or 0.0) * focal).backward()
    return [t.detach().numpy() for t in (z, ce, focal, h.grad, w.grad, b.grad)]


@pytest.mark.parametrize("name", list(STUTTER))
def test_stutter_model_is_float64_torch(name):
    c = STUTTER[name]
    h, w, b, lab, dw0, db0 = M.stutter_operands(c)
    m = M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"])
    z, ce, focal, dh, dw, db = _torch_head(h, w, b, lab, c["g_ce"], c["g_fo"])
    assert np.array_equal(m["logits"], z)  # exact operands: no rounding in either
    n_valid = int((np.clip(lab, 0, 2) != 2).sum())
    assert m["n_valid"] == n_valid
    if n_valid:
        _close(m["ce"], ce)
    else:  # the whole batch is padding: NaN as torch gives, a finite focal term, and no gradient at all
        assert np.isnan(m["ce"]) and np.isnan(ce) and np.isfinite(m["focal"])
        assert not m["dh"].any() and not m["part"].any() and not dh.any() and not dw.any() and not db.any()
    _close(m["focal"], focal)
    _close(m["dh"], dh)
    _close(M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"], dw0, db0)["dw"] - dw0, dw)
    _close(m["dw"], dw)
    _close(m["db"], db)
    assert np.array_equal(M.stutter_head(h, w, b, None)["logits"], z) and m["part"].shape == (c["B"] * -(-c["T"] // 256), 3 * c["C"] + 3)


@pytest.mark.parametrize("name", list(STUTTER))
def test_stutter_operands_are_exact_and_reach_their_branch(name):
    c = STUTTER[name]
    B, C, T = c["B"], c["C"], c["T"]
    h, w, b, lab, dw0, db0 = M.stutter_operands(c)
    k = M.stutter_w_shift(C)
    for a in (h, w * 2.0 ** k, b, dw0, db0):
        assert np.array_equal(a, np.rint(a))  # integers (w: times 2^-k)
    # every partial sum of the logits is a multiple of 2^-k below 2^24 of them, in any order
    assert (np.einsum("bct,jc->btj", np.abs(h.astype(F64)), np.abs(w.astype(F64))) + np.abs(b)).max() * 2.0 ** k < 2 ** 24
    z = M.stutter_head(h, w, b, None)["logits"]
    assert np.array_equal(z, z.astype(F32).astype(F64))
    if c["logits"] == "plain":
        assert np.abs(z).max() < 16 and z.std() > 0.5  # of order 1: the softmax is not saturated
    y = np.clip(lab, 0, 2)
    if c["labels"] == "all_pad":
        assert (y == 2).all()
    elif c["labels"] == "one_pad":
        assert (y[-1] == 2).all() and (y[0] != 2).any()
    elif c["labels"] == "out_of_range":
        assert lab.min() == -1 and lab.max() == 7
    else:
        assert (y[0, 12:] != 2).all() and (B == 1 or (y[-1, -1] == 2 and y[-1, 0] != 2))  # full length beside ragged pad tails
    zy = np.take_along_axis(z, y[..., None], -1)[..., 0]
    if c["logits"] == "underflow":
        gap = (z.max(-1) - zy)[:, :5]
        assert (gap > 104).all() and (np.exp((zy - z.max(-1))[:, :5].astype(F32)) == 0).all()  # fp32 exp underflows to 0
        m = M.stutter_head(h, w, b, lab, 1.0, 1.0)
        assert np.isfinite(m["ce"]) and np.isfinite(m["focal"]) and np.isfinite(m["dh"]).all()
        assert np.isfinite(M.stutter_head(h, w, b, lab, 1.0, 1.0, dtype=F32)["focal"])
    elif c["logits"] == "equal":
        assert (z[:, :12] == z[:, :12, :1]).all()
    elif c["logits"] == "offset":
        assert z.min() > 9900
    assert M.stutter_scratch_floats(B, C, T) == max(B * -(-T // 64) * 3, B * -(-T // 256) * (3 * C + 3))


def test_stutter_case_table_covers_the_branches():
    shapes = {(c["B"], c["C"], c["T"]) for c in M.STUTTER_CASES}
    assert {(1, 1, 1), (2, 3, 63), (2, 4, 64), (3, 5, 65), (2, 17, 255), (2, 16, 256), (2, 33, 257), (9, 4, 449), (2, 192, 300)} <= shapes
    assert max(c["B"] * -(-c["T"] // 64) for c in M.STUTTER_CASES) > 64  # the final kernel's second trip
    assert {c["labels"] for c in M.STUTTER_CASES} >= {"ragged", "one_pad", "all_pad", "out_of_range"}
    assert {c["logits"] for c in M.STUTTER_CASES} >= {"underflow", "equal", "offset"}
    assert any(c["g_ce"] is None for c in M.STUTTER_CASES) and any(c["g_fo"] is None for c in M.STUTTER_CASES)
    # both sides of max(forward, backward) in the scratch size
    sides = {B * -(-T // 64) * 3 > B * -(-T // 256) * (3 * C + 3) for B, C, T in shapes}
    assert sides == {False, True}


def _stutter_runs(name, fault=None):
    c = STUTTER[name]
    h, w, b, lab, dw0, db0 = M.stutter_operands(c)
    run = lambda **kw: M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"], dw0, db0, **kw)
    return run(), run(dtype=F32), (run(fault=fault) if fault else None)


@pytest.mark.parametrize("name", list(STUTTER))
def test_stutter_mirror_stays_near_the_model(name):
    """The float32 mirror is the kernel's arithmetic: its error is what the bars are made of, so it must be rounding noise, not a second
    opinion -- within 256 u of the largest element per output (sums of up to 600 terms; 1 - p_y cancels where p_y is near 1).  The common
    offset of 1e4 is held to the same figure: log p_y = (z_y - max) - log(sum) does not see it."""
    model, mirror, _ = _stutter_runs(name)
    assert np.array_equal(mirror["logits"].astype(F64), model["logits"])
    assert mirror["n_valid"] == model["n_valid"]
    for k in M.STUTTER_OUTPUTS:
        if np.isnan(model[k]).all():
            assert np.isnan(mirror[k]).all()
            continue
        err = np.abs(mirror[k].astype(F64) - model[k]).max()
        assert err <= 256 * M.U * max(np.abs(model[k]).max(), 1e-30), (k, err)
        assert mirror[k].dtype == F32


STUTTER_FAULT_CASES = [  # (fault, the case meant to catch it)
    ("ce_over_all", "c17_t255_group_guard_below_chunk_edge"), ("focal_valid_only", "c17_t255_group_guard_below_chunk_edge"),
    ("no_smooth", "c17_t255_group_guard_below_chunk_edge"),
    ("alpha_wrong", "c17_t255_group_guard_below_chunk_edge"), ("alpha_wrong", "labels_minus1_and_7_clamped"),
    ("drop_channel", "c17_t255_group_guard_below_chunk_edge"), ("drop_channel", "c5_t65_uneven_share_one_frame_second_tile"),
    ("drop_channel", "c33_t257_three_groups_one_frame_second_chunk"),
    ("drop_frame", "c33_t257_three_groups_one_frame_second_chunk"), ("drop_frame", "c5_t65_uneven_share_one_frame_second_tile"),
    ("drop_frame", "b9_t449_72_partial_rows_final_second_trip"),
]


@pytest.mark.parametrize("fault,name", STUTTER_FAULT_CASES)
def test_stutter_bars_separate_planted_faults(fault, name):
    model, mirror, bad = _stutter_runs(name, fault)
    bars = M.stutter_bars(model, mirror)
    ratio = {k: float((np.abs(np.asarray(bad[k], F64) - model[k]) / bars[k]).max()) for k in M.STUTTER_OUTPUTS}
    print(fault, name, {k: "%.3g" % v for k, v in ratio.items()})
    assert max(ratio.values()) >= 8.0, ratio  # bar < effect / 8 where the fault shows most
    # which outputs must show it
    must = dict(ce_over_all=("ce", "dh"), focal_valid_only=("focal", "dh"), no_smooth=("focal",), alpha_wrong=("focal", "dh", "part"),
                drop_channel=("ce", "focal"), drop_frame=("part", "dw"))[fault]
    for k in must:
        assert ratio[k] >= 8.0, (k, ratio)


def test_common_offset_case_catches_log_p_rounded_at_the_offset():
    """What the sweep found: log p_y = z_y - (max + log(sum)) in fp32 rounds at ulp(1e4) = 2^-10 when the logits share an offset of 1e4.
    The kernel now subtracts the maximum first; its former association misses the bars of the offset case by far, and no other case's."""
    name = "logits_common_offset_1e4"
    c = STUTTER[name]
    h, w, b, lab, dw0, db0 = M.stutter_operands(c)
    model, mirror, _ = _stutter_runs(name)
    bars = M.stutter_bars(model, mirror)
    old = M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"], dw0, db0, dtype=F32, fault="lse_first")
    ratio = {k: float((np.abs(old[k].astype(F64) - model[k]) / bars[k]).max()) for k in M.STUTTER_OUTPUTS}
    print(ratio)
    assert ratio["dh"] >= 8.0 and ratio["part"] >= 8.0 and ratio["ce"] > 1.0, ratio  # (the row errors average out of the mean)
    _close(M.stutter_head(h, w, b, lab, c["g_ce"], c["g_fo"], dw0, db0, fault="lse_first")["dh"], model["dh"], 1e-9)


def test_stutter_fault_list_is_the_issue_list():
    assert {f for f, _ in STUTTER_FAULT_CASES} == set(M.STUTTER_FAULTS)


# ---- step projections -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,C,N", M.STEP_PROJ_CASES + [(n, L, C, N) for n, L, C, N, _ in M.STEP_PROJ_REFUSED])
def test_step_proj_model_is_float64_linear_autograd(name, L, C, N):
    for mode in ("exact", "bounded"):
        h, flat, g, pre = M.step_proj_operands(L, C, N, mode)
        W, b = M.step_proj_params(flat, L, C)
        ht = _t(h).requires_grad_(True)
        Wt, bt = _t(W).requires_grad_(True), _t(b).requires_grad_(True)
        with torch.enable_grad():
            out = torch.cat([F.linear(ht.t(), Wt[l], bt[l]) for l in range(L)], 1)  # [N][L C]
            out.backward(_t(g))
        m = M.step_proj(h, flat, g, pre, L, C, N)
        _close(m["out"][0], out.detach().numpy())
        _close(m["dh"][0], ht.grad.numpy())
        ls = M.step_proj_stride(C)
        grad = m["grad"][0] - pre
        for l in range(L):
            _close(grad[l * ls:l * ls + C * C].reshape(C, C), Wt.grad[l].numpy())
            _close(grad[l * ls + C * C:l * ls + C * C + C], bt.grad[l].numpy())
            assert not grad[l * ls + C * C + C:(l + 1) * ls].any()  # the gaps
        assert ls % 4 == 0
        if mode == "exact":  # |values| <= 2: every sum of |terms| stays below 2^24
            assert max(np.abs(a).max() for a in (h, flat, g)) <= 2 and all(v[1].max() < 2 ** 24 for v in m.values())
            assert all(np.array_equal(v[0], v[0].astype(F32).astype(F64)) for v in m.values())


def test_step_proj_case_table():
    assert {(L, C, N) for _, L, C, N in M.STEP_PROJ_CASES} == {(1, 64, 1), (2, 64, 31), (2, 64, 32), (2, 128, 33), (3, 192, 64), (2, 256, 33),
                                                               (2, 256, 64)}
    lds = lambda C, N: C * (32 if N <= 32 else 64) * 4
    assert [lds(C, N) for _, _, C, N in M.STEP_PROJ_CASES[-2:]] == [65536, 65536]
    for name, L, C, N, refused in M.STEP_PROJ_REFUSED:
        cond = C % 64 != 0 or N > 64
        assert ("dh" in refused) == cond and ("dw" in refused) == cond and "fwd" in refused and (cond or lds(C, N) > 65536), name
    assert {(L, C, N) for _, L, C, N, _ in M.STEP_PROJ_REFUSED} == {(1, 96, 8), (1, 64, 65), (1, 320, 33)}


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------------------
def _torch_adamw(p, g, m, v, hy, step, clip, max_norm, gs):
    P = torch.nn.Parameter(_t(p))
    P.grad = _t(g) * gs
    if clip and max_norm > 0:
        torch.nn.utils.clip_grad_norm_([P], max_norm)
    opt = torch.optim.AdamW([P], lr=hy["lr"], betas=(hy["beta1"], hy["beta2"]), eps=hy["eps"], weight_decay=hy["wd"], amsgrad=False)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=_t(m).clone(), exp_avg_sq=_t(v).clone())
    opt.step()
    st = opt.state[P]
    return P.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("name", list(ADAMW))
def test_adamw_model_is_float64_torch(name):
    """torch.optim.AdamW after clip_grad_norm_ on g * grad_scale, fed the fp32-rounded hyperparameters the C ABI passes.  torch takes the norm
    of the gradient itself, so the model gets the float64 sum of squares here (on the GPU it gets the fp32 operand)."""
    c = ADAMW[name]
    p, g, m, v, sumsq, max_norm, gs = M.adamw_operands(c)
    for k in range(c["steps"]):
        if k:
            _, g, _, _, sumsq, max_norm, gs = M.adamw_operands(c, k)
        ss = None if sumsq is None else float((g.astype(F64) ** 2).sum())
        want = _torch_adamw(p, g, m, v, c["hyper"], c["step"] + k, sumsq is not None, max_norm, gs)
        got = M.adamw(p, g, m, v, step=c["step"] + k, sumsq=ss, max_norm=max_norm, grad_scale=gs, **c["hyper"])
        for a, b in zip(got, want):
            _close(a, b, 1e-10)
        p, m, v = got
    if c["clip"] is not None and c["clip"][0] > 0:  # the clip takes the branch the case's name says
        norm = np.sqrt(F64(sumsq)) * gs
        assert (max_norm / (norm + 1e-6) < 1) == (c["clip"][0] < 1), name
        assert abs(max_norm / (norm + 1e-6) - 1) > 5e-4


def test_adamw_case_table():
    names = set(ADAMW)
    assert {c["n"] for c in M.ADAMW_CASES} >= {1, 255, 256, 257, 1000}
    for fam in ("p0_wd0_step", "wd_unit_p_step"):
        assert {s for s in (2, 1000, 10 ** 6) if fam + str(s) in names} == {2, 1000, 10 ** 6}
    gz, gl, gs = (M.adamw_operands(ADAMW[k])[1] for k in ("g_exact_zeros", "g_1e4", "g_1e-12_squares_stay_normal"))
    assert (gz == 0).sum() >= 100 and np.signbit(gz[gz == 0]).any() and (np.abs(gl) == F32(1e4)).all() and (np.abs(gs) == F32(1e-12)).all()
    assert (gs * gs * F32(1e-3) >= np.finfo(F32).tiny).all()  # (1 - beta2) g^2 stays normal
    one = F32(1.0)
    assert one - np.power(F32(0.999), F32(1e6)) == one and one - np.power(F32(0.9), F32(1000)) == one  # large steps: both corrections reach 1


def _adamw_bars(c):
    model, mirror = M.adamw_run(c), M.adamw_run(c, dtype=F32)
    return model, mirror, [M.mirror_bar(a, b) for a, b in zip(model, mirror)]


@pytest.mark.parametrize("name", list(ADAMW))
def test_adamw_mirror_stays_near_the_model(name):
    model, mirror, bars = _adamw_bars(ADAMW[name])
    for a, b, what in zip(model, mirror, "pmv"):
        assert b.dtype == F32 and np.isfinite(a).all()
        assert np.abs(b.astype(F64) - a).max() <= 128 * ADAMW[name]["steps"] * M.U * np.abs(a).max(), what  # roundings; beta1 m cancels against (1 - beta1) g


ADAMW_FAULT_CASES = [
    ("eps_in_sqrt", "n1000_p0_wd0_step1_off_256", "p"), ("eps_in_sqrt", "p0_wd0_step1000", "p"),
    ("bias_step_minus_1", "p0_wd0_step2", "p"), ("bias_step_minus_1", "p0_wd0_step1000", "p"), ("bias_step_minus_1", "wd_unit_p_step2", "p"),
    ("decay_after", "large_lr_wd_decay_before_update", "p"),
    ("clip_without_scale", "grad_scale_0.25_unscaled_norm_above_scaled_below", "mv"),
    ("clip_without_scale", "grad_scale_4_scaled_norm_above_unscaled_below", "mv"),
]


@pytest.mark.parametrize("fault,name,where", ADAMW_FAULT_CASES)
def test_adamw_bars_separate_planted_faults(fault, name, where):
    c = ADAMW[name]
    model, mirror, bars = _adamw_bars(c)
    bad = M.adamw_run(c, fault=fault)
    ratio = {k: float(np.nanmax(np.abs(b - a) / bar)) for k, a, b, bar in zip("pmv", model, bad, bars)}
    print(fault, name, ratio)
    for k in where:
        assert ratio[k] >= 8.0, (k, ratio)


def test_adamw_fault_list_and_the_old_bar():
    assert {f for f, _, _ in ADAMW_FAULT_CASES} == set(M.ADAMW_FAULTS)
    # what the one earlier test could not see: at |p| ~ 1 a bar of 1e-6 max |p| is 2 % of a step's update; with p0 = 0 the update itself
    # carries the bar, which is below 0.01 % of it
    c = ADAMW["p0_wd0_step2"]
    model, _, bars = _adamw_bars(c)
    assert (bars[0] <= 1e-4 * np.abs(model[0]).max()).all()


def test_near_threshold_clip_shows_in_m_and_v():
    """Adam's update is nearly invariant to the gradient's scale, so a wrong clip shows in m and v, not in p: the 0.1 % cases are compared there."""
    lo, hi = ADAMW["norm_0.999_of_max_norm_no_clip"], ADAMW["norm_1.001_of_max_norm_clips"]
    for c, clipped in ((lo, False), (hi, True)):
        p, g, m, v, sumsq, max_norm, gs = M.adamw_operands(c)
        _, m1, _ = M.adamw(p, g, m, v, step=c["step"], sumsq=sumsq, max_norm=max_norm, grad_scale=gs, **c["hyper"])
        _, m0, _ = M.adamw(p, g, m, v, step=c["step"], **c["hyper"])
        _, _, bars = _adamw_bars(c)
        assert (float((np.abs(m1 - m0) / bars[1]).max()) >= 8.0) == clipped


# ---- small entries --------------------------------------------------------------------------------------------------------------------------
def test_small_models_against_torch():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(300).astype(F32), rng.standard_normal(300).astype(F32)
    b[:5] = a[:5]
    ad, sg = M.l1_elem(a, b)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert np.array_equal(ad, (ta - tb).abs().numpy()) and np.array_equal(sg, torch.sign(ta - tb).numpy()) and not sg[:5].view(np.uint32).any()
    x = rng.standard_normal((7, 5)).astype(F32)
    x[1], x[2], x[3, :2], x[3, 2:] = 0.0, -0.0, (2.5, -2.5), 0.0
    assert M.frame_weight(x).tolist() == [1, 0, 0, 1, 1, 1, 1]
    w = rng.standard_normal(4).astype(F32)
    assert np.array_equal(M.scale_bcast(a, w, 80, F32(1.5), 0.3), ((ta * F32(0.3)) * torch.from_numpy(np.repeat(w, 80)[:300]) * F32(1.5)).numpy())
    v, g = rng.standard_normal((3, 255)).astype(F32), rng.standard_normal(3).astype(F32)
    want = torch._weight_norm(_t(v), _t(g)[:, None], 0).numpy()
    _close(M.weight_norm_fold(g, v), want)
    assert np.abs(M.weight_norm_fold(g, v, F32) - want).max() <= 8 * M.U * np.abs(want).max()
    y = rng.standard_normal((2, 6, 43)).astype(F32)
    _close(M.gate(y), (torch.sigmoid(_t(y[:, :3])) * torch.tanh(_t(y[:, 3:]))).numpy())
    assert np.abs(M.gate(y, F32) - M.gate(y)).max() <= 4 * M.U
    xi, sk = rng.standard_normal((2, 3, 43)).astype(F32), rng.standard_normal((2, 3, 43)).astype(F32)
    xo, so = M.res_skip(xi, y, sk, False)
    _close(xo, (_t(xi) + _t(y[:, :3])).numpy() / float(M.SQRT2_F32))
    assert np.array_equal(so, sk + y[:, 3:]) and np.array_equal(M.res_skip(xi, y, np.full_like(sk, np.nan), True)[1], y[:, 3:])
    s, sa = M.row_sum(x, 0.75)
    _close(s, x.astype(F64).sum(1) * 0.75)
    assert (sa >= np.abs(s)).all()


# ---- every C entry point is named in a GPU test module --------------------------------------------------------------------------------------
# (patterns, a word the GPU tests must contain or None, reason)
EXEMPT = [
    ("set_sizeof_*", None, "struct sizes: the loader compares each with its ctypes mirror when the library is opened"),
    ("set_abi_version", None, "asserted by build() and by the loader"),
    ("set_*_size set_mel_loss_*_floats", None, "size queries: the wrappers size their images and scratch with them, a short buffer faults the guarded tests"),
    ("set_stream_*", "leaf_stream", "stream helpers of leaf_stream.py, no kernel"),
    ("set_selftest_mfma", "selftest_mfma", "is itself a test; run through ops.selftest_mfma"),
    ("set_pack_conv_weight_x2 set_pack_diffnet_layer_wino set_pack_diffnet_layer_x3", "pack_diffnet_layer_wino",
     "pack entries reached through ops: every sweep of the kernels that read the images packs with them"),
    ("set_stoi_*", "stoi_bands", "test_gpu_stoi.py sweeps them through the ops wrappers of the same names"),
    ("set_stft_*", "stft_loss_fwd", "test_gpu_msstft.py, through ops.stft_loss_fwd / _bwd"),
    ("set_dtw_path set_mcd_finish set_zero_fill_dist", "dtw_path", "test_gpu_mcd.py, through ops and metrics"),
    ("set_mel_linear", "mel_linear", "test_gpu_mel_loss.py, through ops.mel_linear"),
    ("set_dur_loss set_pitch_loss set_ssim_map set_ssim_bwd", "ssim_loss",
     "gradient passes swept by test_gpu_kernel_branches.py through autograd_ops.dur_losses / pitch_losses / ssim_loss"),
    ("set_diffnet_stack_variant set_diffnet_stack_x3_winograd set_resblock_pair_x2_supported", "stack_x3_winograd",
     "host-side plan queries, no kernel"),
]


def c_entry_points():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "speech-editing-toolkit_amd", "csrc", "*.hip")):
        with open(path) as f:
            names |= set(re.findall(r'extern\s+"C"\s+[\w\s\*]+?\b(set_\w+)\s*\(', f.read()))
    return names


def test_every_entry_point_is_named_in_a_gpu_test():
    """The next kernel added without a test of its own entry fails here."""
    names = c_entry_points()
    assert len(names) > 150 and {"set_adamw", "set_conv1d", "set_stutter_head_loss"} <= names
    text = ""
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        with open(path) as f:
            text += f.read()
    words = set(re.findall(r"\w+", text))
    unnamed = {n for n in names if n not in words}
    assert len(EXEMPT) <= 12
    for pats, word, reason in EXEMPT:
        hit = {n for n in unnamed if any(fnmatch.fnmatchcase(n, p) for p in pats.split())}
        assert hit, ("a stale exemption", pats)
        assert reason and (word is None or any(word in w for w in words)), (pats, word)
        unnamed -= hit
    assert not unnamed, sorted(unnamed)
    mine = os.path.join(ROOT, "tests", "test_gpu_head_optim_branches.py")
    with open(mine) as f:
        own = set(re.findall(r"\w+", f.read()))
    assert {"set_stutter_head_loss", "set_stutter_head_loss_bwd", "set_stutter_head_bwd_reduce", "set_stutter_head_scratch_floats",
            "set_step_proj_fwd", "set_step_proj_bwd_dh", "set_step_proj_bwd_dw", "set_step_proj_bwd_scratch_floats", "set_adamw", "set_l1_elem",
            "set_frame_weight", "set_scale_bcast", "set_row_sum", "set_weight_norm_fold", "set_gate", "set_res_skip"} <= own
