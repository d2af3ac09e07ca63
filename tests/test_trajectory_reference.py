"""CPU tests of tests/trajectory_models.py, the models behind test_gpu_trajectory.py: the float64 update against torch's clip_grad_norm_ +
AdamW; every planted fault against the table that says which check catches it and at which updates; and the conditions the GPU test
stands on -- the stale-by-one fault is at least 10 bars of check 3 from update 2 on, a float32 run of the oracle stays within half of
every bar at the moved weights of the trajectory, and no batch has an empty loss denominator.  The oracle alone stands in for a run here
(float64, the fixture shapes), so a clean run's ratios are 0 and a fault's are its own size."""
import math
import os

import numpy as np
import pytest
import torch

import trajectory_models as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# =====================================================================================================================================
# the update model against torch
# =====================================================================================================================================
def test_update_model_equals_torch_clip_and_adamw_over_six_updates():
    """six updates on random gradients, large and tiny in turn (norm ~ 95 and ~ 0.03: the clip active and idle), warm-up 2 (the 1e-7 floor,
    the ramp and the plateau): p, m and v to 1e-12 of their largest entry after every update"""
    import head_optim_models as HM
    rng = np.random.default_rng(5)
    n, lr0 = 1000, 1e-3
    p = rng.standard_normal(n)
    m, v = np.zeros(n), np.zeros(n)
    ref_p = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=lr0, betas=(HM.f32f(TM.BETAS[0]), HM.f32f(TM.BETAS[1])), eps=HM.f32f(TM.EPS),
                            weight_decay=HM.f32f(TM.WD))
    lrs, clipped = [], []
    for k in range(6):
        g = rng.standard_normal(n) * (3.0 if k % 2 == 0 else 1e-3)
        lr = TM.lr_at(k, lr0)
        lrs.append(lr)
        opt.param_groups[0]["lr"] = HM.f32f(lr)
        ref_p.grad = torch.from_numpy(g.copy())
        norm = float(torch.nn.utils.clip_grad_norm_([ref_p], TM.CLIP))
        clipped.append(norm > TM.CLIP)
        opt.step()
        p, m, v = TM.update_step(p, g, m, v, k, lr0)
        st = opt.state[ref_p]
        for name, got, want in (("p", p, ref_p.detach().numpy()), ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (k, name)
    assert lrs == [1e-7, 0.5e-3, 1e-3, 1e-3, 1e-3, 1e-3]
    assert clipped == [True, False] * 3


def test_schedule_restatement():
    assert [TM.lr_at(k, 2e-3) for k in range(5)] == [1e-7, 1e-3, 2e-3, 2e-3, 2e-3]
    assert TM.lr_at(1, 1e-8) == 1e-7  # the floor also holds on the ramp
    # the library's own schedule says the same (compared here, not used by the checks)
    import set_amd  # noqa: F401
    from set_amd.training import FlatAdamW
    lib = FlatAdamW.lr_at
    holder = type("H", (), dict(lr0=1e-3, warmup=TM.WARMUP))()
    assert [lib(holder, k) for k in range(6)] == [TM.lr_at(k, 1e-3) for k in range(6)]


# =====================================================================================================================================
# inventory
# =====================================================================================================================================
def test_every_case_names_its_switches_and_route():
    assert [c["name"] for c in TM.CASES] == ["spec_per_op", "spec_fused_stack", "spec_bf16", "spec_accumulate2", "campnet_fp32", "campnet_bf16"]
    src = ""
    pkg = os.path.join(ROOT, "speech-editing-toolkit_amd")
    for d in (pkg, os.path.join(pkg, "csrc")):  # (SET_AMD_WINO is read by the kernel plan in csrc/)
        for fn in sorted(os.listdir(d)):
            if fn.endswith((".py", ".hip", ".h")):
                with open(os.path.join(d, fn)) as f:
                    src += f.read()
    for c in TM.CASES:
        assert set(c) == {"name", "kind", "dtype", "env", "acc", "detour", "lr0", "sinks"}
        assert c["kind"] in ("spec", "campnet") and c["dtype"] in ("f32", "bf16") and c["acc"] in (1, 2)
        for k in c["env"]:
            assert '"%s"' % k in src, k  # a switch the library reads
        assert c["sinks"] == (c["acc"] == 1)
    assert TM.CASE["spec_per_op"]["env"] == {"SET_AMD_TRAIN_STACK": "0"} and TM.CASE["spec_fused_stack"]["env"] == {"SET_AMD_WINO": "2"}
    assert [c["name"] for c in TM.CASES if c["detour"]] == ["spec_fused_stack", "spec_bf16", "campnet_fp32"]
    assert TM.N_UPDATES == 5 and TM.N_BATCHES == 3 and TM.WARMUP == 2 and TM.CLIP == 1.0
    for kind, (B, T, T_txt) in (("spec", (3, 77, 19)), ("campnet", (3, 77, 19))):
        m = TM.fixture_meta(kind)
        assert (m["B"], m["T"], m["T_txt"]) == (B, T, T_txt) and m["pad_tail"]
    for name in TM.FAULT_TENSOR.values():
        assert name.endswith(".weight")


def test_batches_are_distinct_and_no_loss_denominator_is_empty():
    for kind in ("spec", "campnet"):
        bs = [TM.batch(kind, i) for i in range(TM.N_BATCHES)]
        for i in range(TM.N_BATCHES):
            for k, d in TM.loss_denominators(kind, bs[i]).items():
                assert d > 0, (kind, i, k)
            for j in range(i):
                assert not torch.equal(bs[i]["ref_mels"], bs[j]["ref_mels"]) and not torch.equal(bs[i]["txt_tokens"], bs[j]["txt_tokens"])
            assert bool((bs[i]["txt_tokens"] >= 0).all()) and int(bs[i]["txt_tokens"].max()) < 80
        if kind == "campnet":
            pads = [(b["txt_tokens"] == 0) for b in bs]
            assert bool(pads[0].any()) and all(torch.equal(pads[0], q) for q in pads)  # the fixture's padded tails on every batch
    # consecutive updates see different data, also under accumulation
    for c in TM.CASES:
        seen = [TM.batches_of_update(c, k) for k in range(TM.N_UPDATES)]
        assert all(len(set(s)) == c["acc"] for s in seen) and all(seen[k] != seen[k + 1] for k in range(TM.N_UPDATES - 1))


# =====================================================================================================================================
# the oracle's trajectories (one per distinct (kind, acc, lr0) of the case table's f32 cases)
# =====================================================================================================================================
_TRAJ = {}


def _traj(name):
    if name not in _TRAJ:
        _TRAJ[name] = TM.oracle_trajectory(TM.CASE[name])
    return _TRAJ[name]


_PLANTED = {}


def _planted(fault, name, k):
    key = (fault, name, k)
    if key not in _PLANTED:
        layout, W0, recs = _traj(name)
        _PLANTED[key] = TM.plant(fault, TM.CASE[name], layout, W0, recs, k)
    return _PLANTED[key]


def _clean(name, k):
    layout, W0, recs = _traj(name)
    r = recs[k]
    s = slice(0, layout.n, TM.FAULT_STRIDE)
    return dict(losses=r["losses"], g=r["g"], lr=r["lr"], p1=r["p1"][s], m1=r["m1"][s], v1=r["v1"][s])


@pytest.mark.parametrize("name", ["spec_per_op", "spec_accumulate2", "campnet_fp32"])
def test_oracle_trajectory_stays_finite_and_a_clean_run_passes_every_check(name):
    case = TM.CASE[name]
    layout, W0, recs = _traj(name)
    assert len(recs) == TM.N_UPDATES
    for r in recs:
        assert len(r["losses"]) == case["acc"]
        for l in r["losses"]:
            assert all(math.isfinite(x) for x in l.values()), (r["k"], l)
        assert np.isfinite(r["g"]).all() and np.isfinite(r["p1"]).all()
        assert r["lr"] == TM.lr_at(r["k"], case["lr0"])
        assert not r["p1"][layout.n:].any()
    assert [r["lr"] for r in recs] == [1e-7, case["lr0"] / 2] + [case["lr0"]] * 3
    # the weights really move: update 0 by ~1e-7 an element, updates 1.. by ~lr
    step = [float(np.abs(r["p1"] - r["p"]).max()) for r in recs]
    assert step[0] < 2e-7 * 1.1 + TM.WD * 1e-7 * 10 and all(s > 0.1 * case["lr0"] for s in step[1:]), step
    for k in (0, TM.N_UPDATES - 1):
        run = _clean(name, k)
        got = TM.checks_of(case, layout, recs[k], run, run)
        assert max(got[3].values()) == 0.0 and got[5]
        assert max(got[4].values()) <= 1.0, got[4]  # (the strided update sums nothing else: the float64 model itself, ratio 0)


FAULT_RUNS = ([(f, "spec_per_op") for f in TM.FAULTS if f != "accumulate_sum"] + [("accumulate_sum", "spec_accumulate2")]
              + [(f, "campnet_fp32") for f in ("stale_by_one", "grad_dropped", "moments_reset")])


@pytest.mark.parametrize("fault,name", FAULT_RUNS)
def test_each_planted_fault_is_caught_by_the_check_the_table_names(fault, name):
    case = TM.CASE[name]
    layout, W0, recs = _traj(name)
    route, table = TM.FAULTS[fault]
    caught = {3: set(), 4: set(), 5: set()}
    for k in range(TM.N_UPDATES):
        run = _planted(fault, name, k)
        fresh = _clean(name, k) if route else run
        got = TM.checks_of(case, layout, recs[k], run, fresh)
        print(fault, name, k, {c: ("%.3g" % max(got[c].values())) for c in (3, 4)}, got[5])
        for c in (3, 4):
            if max(got[c].values()) > 1.0:
                caught[c].add(k)
        if not got[5]:
            caught[5].add(k)
    want = dict(table)
    if want[4] == "clip_active":
        want[4] = {r["k"] for r in recs if math.sqrt(TM.sumsq64(r["g"])) > TM.CLIP * 1.001}
        assert want[4], "no update of this trajectory clips: the fault has nowhere to show"
    assert caught == want, (fault, name, caught, want)
    assert any(want.values())  # no fault passes all three checks


@pytest.mark.parametrize("name", ["spec_per_op", "campnet_fp32"])
def test_stale_by_one_is_at_least_ten_bars_of_check_3_from_update_2_on(name):
    """lr0 and the shapes make a weight image (or anything else derived from the weights) that is one update old visible to the loss or
    gradient bars of check 3 with a factor 10 to spare at every update k >= 2.  Update 0 has nothing older to show; update 1 shows only the
    1e-7 step of update 0 (the floor of the warm-up), which exceeds the bars but by no margin that is asserted here."""
    case = TM.CASE[name]
    layout, W0, recs = _traj(name)
    ratios = []
    for k in range(1, TM.N_UPDATES):
        run = _planted("stale_by_one", name, k)
        c3, _ = TM.check_forward_backward(case["kind"], "f32", layout, recs[k]["losses"], recs[k]["grads"], run["losses"], run["g"])
        ratios.append(max(c3.values()))
    print(name, "stale-by-one, largest ratio of check 3 at updates 1..:", ["%.3g" % r for r in ratios])
    assert all(r >= 10.0 for r in ratios[1:]), ratios
    assert ratios[0] < min(ratios[1:])  # the floor step is the smallest of them


@pytest.mark.parametrize("name", ["spec_per_op", "campnet_fp32"])
def test_float32_oracle_stays_within_half_of_every_bar_along_the_trajectory(name):
    """the bars of check 3 were set at the seeded weights; they hold with a factor 2 to spare for a float32 evaluation of the oracle at
    every p_k of the trajectory too"""
    case = TM.CASE[name]
    layout, W0, recs = _traj(name)
    for r in recs:
        W = TM.unflatten_state(layout, r["p"], W0, dtype=torch.float32)
        losses, grads = TM.oracle_update_inputs(case, W, r["k"], dtype=torch.float32)
        c3, worst = TM.check_forward_backward(case["kind"], "f32", layout, r["losses"], r["grads"], losses, TM.flatten_grads(layout, grads))
        print(name, r["k"], {k: "%.3g" % v for k, v in c3.items()}, worst)
        assert max(c3.values()) <= 0.5, (r["k"], c3, worst)


# =====================================================================================================================================
# ReLU units float32 cannot decide
# =====================================================================================================================================
def test_one_undecided_relu_unit_moves_a_predictor_gradient_by_more_than_its_bar():
    """Update 1 of spec_accumulate2 reads batch 2 at p_1, where one unit of the pitch predictor's last conv layer has the argument
    +1.5e-6: float32 arithmetic cannot decide its branch (the float32 and float64 oracles differ by 4.6e-6 in that layer), the loss does
    not notice (1e-5 of its bar), and the gradient of that layer's weight moves by 2.4 of the element bar and 2.3 of the norm bar that
    test_gpu_fullsize_training set at B T = 25,600 frames -- here B T = 231.  The MI355X takes the other branch there.  So check 3 may
    take its reference with such a unit on either branch (trajectory_models.references_of_update); the bars stay as they are."""
    import torch.nn.functional as F
    case = TM.CASE["spec_accumulate2"]
    layout, W0, recs = _traj("spec_accumulate2")
    assert TM.batches_of_update(case, 1) == [2, 0]
    W = TM.unflatten_state(layout, recs[1]["p"], W0)
    relu = F.relu
    units = TM.undecided_relu_units("spec", W, TM.batch("spec", 2))
    assert F.relu is relu
    near = [(c, u, x, thr) for c, u, x, thr in units if abs(x) < 2e-6]
    assert [(c, u) for c, u, _, _ in near] == [(7, 36152)], units
    assert all(abs(x) <= thr < 1e-4 for _, _, x, thr in units) and len(units) < 10
    refs = TM.references_of_update(case, W, 1)
    l0, g0, what0 = next(refs)
    l1, g1, what1 = next(refs)
    assert what0 == "" and "relu call 7 unit 36152" in what1 and F.relu is relu
    c3, worst = TM.check_forward_backward("spec", "f32", layout, l0, g0, l1, TM.flatten_grads(layout, g1))
    print({k: "%.4f" % v for k, v in c3.items()}, worst)
    assert worst == "fs.pitch_predictor.conv.4.0.weight"
    assert c3["loss"] < 1e-3 and c3["grad_elem_core"] == 0.0 and c3["unreached"] == 0.0
    assert 2.0 < c3["grad_elem"] < 3.0 and 2.0 < c3["grad_diff_norm"] < 3.0 and c3["grad_norm"] < 1.0
    assert len(list(refs)) == 2 ** TM.MAX_UNDECIDED - 2  # the other subsets of the three units closest to zero
