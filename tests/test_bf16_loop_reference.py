"""CPU checks of tests/bf16_loop_models.py, the models and case table the GPU sweep tests/test_gpu_bf16_loop_branches.py stands on:
the plan of every row pinned (Python mirror of plan_steps, and the library itself where it answers without a GPU), the inventory of
the mirror's branches, the plain model tied to loop() of test_loop_reference.py, the bf16-operand mirror tied to the layer model of
test_diffnet_bf16_reference.py on one layer, the exact budgets, and the fault planters: every wrong value the host code could
compute moves the result by more than 10 of the bars the GPU sweep uses."""
import numpy as np
import pytest
import torch

import bf16_loop_models as Mo
import test_diffnet_bf16_reference as D
import test_loop_reference as R

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Mo.ROWS, ids=lambda c: c["name"])
def test_row_reaches_the_plan_it_names(c):
    p = Mo.plan_mirror(c)
    for g in p["groups"]:
        assert (g["body"], g["fuse"], len(g["launches"]), g["why"]) == (c["body"], c["fuse"], c["n"], c["why"]), (c["name"], g)
        assert sum(nl for _, nl, _ in g["launches"]) == c["L"] and [l0 for l0, _, _ in g["launches"]] == list(range(0, c["L"], c["fuse"]))
    assert p["boundary"] == c["boundary"], c["name"]
    assert c["B"] <= 3 and c["T"] <= 260 and c["L"] <= 7 and c["steps"] <= 3 and c["M"] in (17, 80, 97) and c["reason"]


def test_inventory_is_complete():
    """Every outcome of the mirror of plan_steps has a row: both bodies, every reason for either (WHYS: a new branch in the mirror
    without a row fails here), the three boundary forms, both tile widths with a ragged and a full last tile, the group counts, both
    parities of the ping-pong, the tail groups the issue names."""
    plans = {c["name"]: Mo.plan_mirror(c) for c in Mo.ROWS}
    assert len(plans) == len(Mo.ROWS)
    assert {g["why"] for p in plans.values() for g in p["groups"]} == set(Mo.WHYS)
    assert {p["boundary"] for p in plans.values()} == set(Mo.BOUNDARIES)
    assert {c["body"] for c in Mo.ROWS} == {"GROUPS", "LAYERS"}
    for b in Mo.BOUNDARIES:  # every boundary form under the GROUPS body
        assert any(c["boundary"] == b and c["body"] == "GROUPS" for c in Mo.ROWS), b
    assert {c["env"].get(Mo.FUSE) for c in Mo.ROWS} >= {None, "0", "2", "3", "99"}
    assert {(c["L"], c["n"] % 2) for c in Mo.ROWS if c["env"].get(Mo.FUSE) == "2"} >= {(4, 0), (6, 1)}
    assert any(c["fuse"] == 3 and c["L"] == 4 for c in Mo.ROWS) and any(c["fuse"] == 16 and c["n"] == 1 for c in Mo.ROWS)
    for dcl in (1, 2):  # the default plan: 5 + 2
        assert any(c["L"] == 7 and c["dcl"] == dcl and c["fuse"] == 5 and c["why"] == "plan" for c in Mo.ROWS)
    # dcl 3 and 4 with a workspace: one T below the largest dilation, one above 128
    for dcl in (3, 4):
        ts = [c["T"] for c in Mo.ROWS if c["dcl"] == dcl and c["ws"] is not None]
        assert min(ts) < (1 << (dcl - 1)) and max(ts) > 128 and all(c["L"] >= dcl for c in Mo.ROWS if c["dcl"] == dcl)
    # tiles: what every launch of the GROUPS rows runs on
    tiles = {}
    for c in Mo.ROWS:
        if c["body"] == "GROUPS":
            for g in plans[c["name"]]["groups"]:
                for l0, nl, tile in g["launches"]:
                    r = D.layers_launch(dict(B=g["Bg"], T=c["T"], l0=l0, nl=nl, dcl=c["dcl"], env=c["env"].get(Mo.TILE)))
                    assert r["rc"] == 0, (c["name"], r)
                    tiles.setdefault((tile, c["env"].get(Mo.TILE)), set()).add("full" if c["T"] % r["nv_plain"] == 0 else "ragged")
    assert tiles[64, "64"] == tiles[128, "128"] == {"full", "ragged"} and (64, None) in tiles
    # every GROUPS row has a witness that tells it from one layer per launch: the x_l the ping-pong leaves, or the scratch it writes
    for c in Mo.ROWS:
        if c["body"] == "GROUPS":
            assert Mo.final_x_layers(c["L"], c["fuse"]) != Mo.final_x_layers(c["L"], 1) or Mo.scratch_written(c, plans[c["name"]]).any(), c["name"]
            assert Mo.scratch_written(c, plans[c["name"]]).any() == (c["env"].get(Mo.TILE) == "128"), c["name"]
        else:
            assert not Mo.scratch_written(c, plans[c["name"]]).any()
    # the scratch: exact and one float short at the same shape and plan
    short, exact = Mo.row("scratch_short"), Mo.row("t128_ragged")
    assert all(short[k] == exact[k] for k in ("B", "M", "T", "L", "dcl", "env")) and Mo.ws_floats_of(short) + 1 == Mo.ws_floats_of(exact)
    assert Mo.ws_floats_of(exact) == D.layers_scratch_floats(2, 200, 0, 2, 1) > 0
    # groups at B = 3 on forced 128-frame tiles, and the odd case
    g3 = {c["n_groups"]: plans[c["name"]]["G"] for c in Mo.ROWS if c["B"] == 3 and c["env"].get(Mo.TILE) == "128" and (c["M"] * c["T"]) % 4 == 0}
    assert g3 == {1: 1, 2: 2, 3: 3, 8: 3}
    odd = Mo.row("groups_odd")
    assert (odd["M"] * odd["T"]) % 4 == 2 and plans["groups_odd"]["G"] == 1 and odd["n_groups"] == 3
    assert [(g["b0"], g["Bg"]) for g in plans["groups2"]["groups"]] == [(0, 1), (1, 2)]
    assert {c["M"] for c in Mo.ROWS if c["boundary"] == "unfused"} >= {97} and {c["T"] % 4 for c in Mo.ROWS if c["boundary"] == "unfused"} >= {0, 1, 2, 3}
    assert {c["steps"] for c in Mo.E2E} == {2, 3} and {c["L"] for c in Mo.E2E} >= {3, 7}
    assert {c["body"] for c in Mo.E2E} == {"GROUPS", "LAYERS"} and {c["L"] for c in Mo.EXACT} == {1, 4}
    assert {c["body"] for c in Mo.EXACT} == {"GROUPS", "LAYERS"}


def test_ping_pong_by_hand():
    assert Mo.final_x_layers(3, 1) == {"ws_x0": 2, "ws_x1": 3} and Mo.final_x_layers(4, 1) == {"ws_x0": 4, "ws_x1": 3}
    assert Mo.final_x_layers(7, 5) == {"ws_x0": 7, "ws_x1": 5} and Mo.final_x_layers(6, 2) == {"ws_x0": 4, "ws_x1": 6}
    assert Mo.final_x_layers(4, 3) == {"ws_x0": 4, "ws_x1": 3} and Mo.final_x_layers(4, 16) == {"ws_x0": 0, "ws_x1": 4}
    assert Mo.group_starts(3, 80, 132, 2) == [0, 1, 3] and Mo.group_starts(3, 80, 132, 8) == [0, 1, 2, 3] and Mo.group_starts(3, 17, 66, 3) == [0, 3]


def test_plan_mirror_equals_the_library_without_a_gpu(built_lib, monkeypatch):
    """The two host functions plan_steps asks: the layers-per-launch plan (the library assumes 256 CUs when no device answers; at these
    sizes any chip of more than 12 CUs gives the same answer) and the scratch size of every row."""
    L = built_lib
    for c in Mo.ROWS:
        monkeypatch.delenv(Mo.TILE, raising=False)
        if Mo.TILE in c["env"]:
            monkeypatch.setenv(Mo.TILE, c["env"][Mo.TILE])
        for g in Mo.plan_mirror(c)["groups"]:
            assert L.set_diffnet_layers_bf16_plan(g["Bg"], c["T"], c["L"], c["dcl"]) == D.layers_plan(g["Bg"], c["T"], c["L"], c["dcl"], c["env"].get(Mo.TILE))
            assert D.layers_plan(g["Bg"], c["T"], c["L"], c["dcl"], c["env"].get(Mo.TILE), 13) == D.layers_plan(g["Bg"], c["T"], c["L"], c["dcl"], c["env"].get(Mo.TILE), 1024)
        if c["ws"] is not None and c["dcl"] <= 2:
            fuse = Mo._fuse_before_size(c, c["B"])[0]
            want = L.set_diffnet_layers_bf16_scratch_floats(c["B"], c["T"], 0, max(fuse, 2), c["dcl"])
            assert Mo.ws_floats_of(c) == want - (1 if c["ws"] == "short" else 0)
            # one slice per utterance: the per-group offsets of step_bf16_groups tile the buffer exactly
            assert want == c["B"] * L.set_diffnet_layers_bf16_scratch_floats(1, c["T"], 0, max(fuse, 2), c["dcl"])


# ------------------------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------------------------
def test_plain_model_is_loop_of_the_loop_reference():
    """loop_c on the conditioned operands == loop() of test_loop_reference.py on cp = Wc cond + b_cond, to float64 rounding."""
    for name in ("plan_L3", "dcl3_T3"):
        o = Mo.make_gauss_c(Mo.row(name))
        got, trace = Mo.loop_c(o)
        want, tr = R.loop(o)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        assert float((trace[-1]["skip"] - tr[-1]["skip"]).abs().max()) <= 1e-11 and float((trace[0]["xs"][-1] - tr[0]["xL"]).abs().max()) <= 1e-11


@pytest.mark.parametrize("c", [c for c in D.FWD if c["name"] in ("T129_dil4_B3", "T5_dil8_shorter_than_dil", "T128_dil2")], ids=lambda c: c["name"])
def test_mirror_is_the_layer_model_of_the_kernel_sweep_on_one_layer(c):
    """One layer of the mirror on the exact operands of test_diffnet_bf16_reference.make_forward_exact (rounding probes in x + d and Wo):
    the skip rows bit for bit, x_out to the one fp32 rounding the layer model applies.  The plain model differs: the probes round."""
    e = D.make_forward_exact(c)
    o = dict(L=1, B=c["B"], cond=e["cond"], Wd=e["Wd"][None], Wc=e["Wc"][None], Wo=e["Wo"][None, :, :, None], bd=e["bd"][None], bc=e["bc"][None],
             bo=e["bo"][None], dcl=1, steps=1)
    bk = Mo.book(o)
    bk["dil"] = [c["dil"]]
    outs = {}
    for mirror in (True, False):
        W, r = Mo.weights_of(o, mirror)
        xs, skip = [], []
        for b in range(c["B"]):  # (the layer model's step offset is per utterance)
            ob = dict(o, B=1)
            Wb = dict(W, cond=W["cond"][b:b + 1])
            x_b, s_b = Mo.layers_c(e["x"][b:b + 1], ob, e["d"][b], dict(bk, cond_b=[0]), Wb, r)
            xs.append(x_b[1]), skip.append(s_b)
        outs[mirror] = (torch.cat(xs), torch.cat(skip))
    x16, s16 = outs[True]
    want_skip = e["skip"].double() - (0 if c["first"] else e["skip0"].double())
    assert torch.equal(s16, want_skip)
    assert float((x16 - e["x_out"].double()).abs().max()) <= 2.0 ** -23 * float(e["x_out"].abs().max())
    assert float((outs[False][1] - want_skip).abs().max()) > 2.0 ** -10


def test_mirror_costs_what_bf16_operands_cost():
    """mirror - reference is of the size bf16 rounding predicts (far above fp32 rounding, far below the signal): the first term of the
    end-to-end bar is neither zero nor a licence."""
    o = Mo.make_gauss_c(Mo.row("plan_L3"))
    want, mir = Mo.loop_c(o)[0], Mo.loop_c(o, mirror=True)[0]
    e = float((mir - want).abs().max())
    assert 1e-4 * float(want.abs().max()) < e < 0.05 * float(want.abs().max()), (e, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# exact mode
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Mo.EXACT, ids=lambda c: c["name"])
def test_exact_operands_meet_their_budget(c):
    for steps in (1, 2):
        o = Mo.make_exact_c(c, steps=steps, L=c["L"])
        assert Mo.exact_budget(o)
        # the plain model predicts the same skip sum (sigmoid(40) tanh(+-40) = +-1 in float64 too)
        tr = Mo.loop_c(o)[1]
        assert all(torch.equal(t["skip"], o["skip_want"]) for t in tr)
        assert torch.equal(Mo.loop_c(o, mirror=True)[1][-1]["skip"], o["skip_want"])


# ------------------------------------------------------------------------------------------------------------------------
# the fault planters
# ------------------------------------------------------------------------------------------------------------------------
PLANTED = [  # (fault, row whose plan it lives in)
    ("dstep_reversed", "plan_L7_dcl1"), ("noise_reversed", "plan_L7_dcl1"), ("coef4_reversed", "plan_L7_dcl1"),
    ("dstep_reversed", "no_ws"), ("noise_reversed", "fuse3_L4"), ("coef4_reversed", "boundary_M97"),
    ("cond_of_utterance_0", "groups2"), ("cond_of_utterance_0", "groups3"),
    ("tail_biases_of_l0", "plan_L7_dcl1"), ("tail_image_of_l0", "plan_L7_dcl2"),
    ("dilation_cycle_shifted", "plan_L7_dcl2"), ("dilation_cycle_shifted", "fuse2_L4"),
    ("first_on_a_later_layer", "plan_L7_dcl1"), ("first_on_a_later_layer", "fuse3_L4"), ("first_on_a_later_layer", "fuse2_L4"),
]
_MODELS = {}


def models_of(name):
    """(operands, reference, bars) of a row, computed once: the final x and the skip sum of the last step (ws_skip after the loop), each
    with the bar the GPU sweep holds it to."""
    if name not in _MODELS:
        o = Mo.make_gauss_c(Mo.row(name))
        (x, tr), (xm, trm) = Mo.loop_c(o), Mo.loop_c(o, mirror=True)
        want = dict(x=x, ws_skip=tr[-1]["skip"])
        _MODELS[name] = (o, want, dict(x=Mo.e2e_bar(o, x, xm), ws_skip=Mo.e2e_bar(o, tr[-1]["skip"], trm[-1]["skip"])))
    return _MODELS[name]


# the buffer each fault is held by: the dstep column of the LAST step feeds the last skip sum directly, while the final x sees it through
# c1 = 0.3 of coef4 row 0 only (step_tables); every other fault is held by the final x
HELD_BY = {"dstep_reversed": "ws_skip"}


@pytest.mark.parametrize("fault,name", PLANTED, ids=["%s-%s" % p for p in PLANTED])
def test_planted_fault_moves_the_result_by_more_than_ten_bars(fault, name):
    c = Mo.row(name)
    o, want, bars = models_of(name)
    x, tr = Mo.loop_c(o, bk=Mo.plant(o, fault, c["fuse"], c["n_groups"]))
    got = dict(x=x, ws_skip=tr[-1]["skip"])
    moved = {k: float((got[k] - want[k]).abs().max()) / bars[k] for k in want}
    print("fault %-24s row %-14s moves x by %.1f bars (bar %.3e), ws_skip by %.1f bars (bar %.3e)" % (fault, name, moved["x"], bars["x"], moved["ws_skip"], bars["ws_skip"]))
    k = HELD_BY.get(fault, "x")
    assert moved[k] > 10.0, (fault, name, k, moved, bars)


def test_every_fault_is_planted():
    assert {f for f, _ in PLANTED} == set(Mo.FAULTS)
    assert all(np.isfinite(v) and v > 0 for _, n in PLANTED[:1] for v in models_of(n)[2].values())
