"""CPU checks of tests/tape_models.py, on which tests/test_gpu_tape_branches.py stands: the float64 models equal independent code (a tap-by-tap
conv, torch.nn.functional, the attention model of test_attention_reference.py, the oracle's losses in float64), the float32 mirrors stay near
the models, the integer cases are exact in fp32, every bounded bar is below 1/8 of the effect of each planted fault on the case meant to
catch it, and the inventory: every torch.autograd.Function of autograd_ops.py (parsed, not imported) is in the case table or the "swept
elsewhere" table, every needs_input_grad index a backward reads has a case with that input not requiring grad, every optional operand of a
forward has a case without it."""
import ast
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tape_models as M
from oracle import oracle as O
from test_attention_reference import attn_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "speech-editing-toolkit_amd", "autograd_ops.py")
CASES = M.BY_NAME
F64 = torch.float64


def _close(got, want, rel=1e-11):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    scale = max(1e-300, float(want.abs().max())) if want.numel() else 1.0
    if want.numel():
        assert float((got - want).abs().max()) <= rel * scale + 1e-13, (float((got - want).abs().max()), scale)


def _t64(cs):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in M.operands(cs).items()}


def _of(node):
    return [c["name"] for c in M.CASES if c["node"] == node]


# ---- the models against independent code ------------------------------------------------------------------------------------------------
def _conv_by_taps(t, c):
    """set_amd.h, SetConv1dArgs: out[b][co][s] = act((sum_ci sum_k W[co][ci][k] P(x[b][ci][s + k dil - pad] + add[b][ci]) + bias) alpha),
    + res, * mask; the input is zero outside [0, T_in)"""
    x, w = t["x"], t["w"]
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    dil, pad = c.get("dil", 1), c["pad"]
    T_out = c.get("T_out", T + 2 * pad - dil * (K - 1))
    if "add" in t:
        x = x + t["add"][:, :, None]
    if c.get("pro") == "div":
        x = x / c["pro_param"]
    y = torch.zeros(B, Cout, T_out, dtype=F64)
    for k in range(K):
        for s in range(T_out):
            i = s + k * dil - pad
            if 0 <= i < T:
                y[:, :, s] += x[:, :, i] @ w[:, :, k].t()
    if "b" in t:
        y = y + t["b"][None, :, None]
    y = y * c.get("alpha", 1.0)
    y = {"none": lambda v: v, "relu": lambda v: v.clamp(min=0), "gelu": lambda v: 0.5 * v * (1 + torch.erf(v / 2 ** 0.5)), "mish": F.mish,
         "softplus": lambda v: torch.log1p(torch.exp(v)), "tanh": lambda v: torch.tanh(v)}[c.get("act", "none")](y)
    if "res" in t:
        y = y + t["res"]
    if "mask" in t:
        y = y * t["mask"][:, None]
    return y


@pytest.mark.parametrize("name", _of("_Conv1dFn"))
def test_conv_model_is_the_tap_sum_of_the_header(name):
    cs = CASES[name]
    _close(M.reference(cs)["outs"][0], _conv_by_taps(_t64(cs), cs["c"]))


def test_small_models_against_torch_functional_and_the_oracle():
    for name in _of("_LayerNormChFn"):
        cs, t = CASES[name], _t64(CASES[name])
        want = F.layer_norm(t["x"].transpose(1, 2), (t["x"].shape[1],), t["gamma"], t["beta"], cs["c"]["eps"]).transpose(1, 2)
        _close(M.reference(cs)["outs"][0], want * t["mask"][:, None] if "mask" in t else want)
        _close(M.layernorm_ch(t["x"], t["gamma"], t["beta"], 1e-5), O.layer_norm_ch(t["x"], t["gamma"], t["beta"]))
    z = torch.linspace(-6, 6, 241, dtype=F64)
    _close(M.ACTS["mish"](z), F.mish(z))
    _close(M.ACTS["mish"](z), O.mish(z))
    _close(M.ACTS["gelu"](z), 0.5 * z * (1 + torch.erf(z / 2 ** 0.5)))
    _close(M.ACTS["softplus"](z), torch.log1p(torch.exp(z)))
    for name in _of("_GateFn"):
        y = _t64(CASES[name])["y"]
        C = y.shape[1] // 2
        _close(M.reference(CASES[name])["outs"][0], F.glu(torch.cat([torch.tanh(y[:, C:]), y[:, :C]], 1), 1))
    for name in _of("_EmbeddingFn"):
        cs, t = CASES[name], _t64(CASES[name])
        tab = t["table"].clone().requires_grad_(True)
        with torch.enable_grad():
            out = cs["c"]["scale"] * F.embedding(t["idx"], tab, padding_idx=cs["c"].get("padding_idx")).transpose(1, 2)
            out = out + t["base"] if "base" in t else out
            (out * M.reference(cs)["ups"][0].double()).sum().backward()
        _close(M.reference(cs)["outs"][0], out.detach())
        _close(M.reference(cs)["grads"]["table"], tab.grad)
        if cs["c"].get("padding_idx") is not None:
            assert (t["idx"] == cs["c"]["padding_idx"]).any() and not tab.grad[cs["c"]["padding_idx"]].any()
    for name in _of("_ExpandStatesFn"):
        t = _t64(CASES[name])
        _close(M.reference(CASES[name])["outs"][0], O.expand_states(t["enc"].transpose(1, 2), t["mel2ph"]).transpose(1, 2))
        if t["enc"].shape[0] > 1:
            assert not t["mel2ph"][-1].any()  # an utterance whose mel2ph is all 0
    for name in _of("_DropoutFn") + [n for n in _of("_PreLnFfnFn") if CASES[n]["c"].get("drop")]:
        c = CASES[name]["c"]
        p, seed, off = (c["p"], c["seed"], c["offset"]) if "p" in c else c["drop"]
        assert off > 2 ** 32
        s = M.dropout_scale((3, 32, 33), p, seed, off, F64)
        assert set(s.unique().tolist()) == {0.0, 2.0} and 0.4 < float((s > 0).double().mean()) < 0.6


@pytest.mark.parametrize("name", _of("_AttnFn"))
def test_attention_model_is_the_attention_reference_model(name):
    cs, t = CASES[name], _t64(CASES[name])
    c = cs["c"]
    if "qkv" in t:
        H = t["qkv"].shape[1] // 3
        q, k, v = t["qkv"][:, :H], t["qkv"][:, H:2 * H], t["qkv"][:, 2 * H:]
    else:
        H = t["q"].shape[1]
        q, k, v = t["q"], t["kv"][:, :H], t["kv"][:, H:]
    ref = M.reference(cs)
    want = attn_model(q.float(), k.float(), v.float(), t.get("kpm"), c["fill"], c["alpha"], c["heads"], do=ref["ups"][0])
    _close(ref["outs"][0], want["o"], 1e-10)
    if c.get("want_p"):
        _close(ref["outs"][1], want["p"], 1e-10)
    dq, dk, dv = want["dq"], want["dk"], want["dv"]
    if "qkv" in t:
        _close(ref["grads"]["qkv"], torch.cat([dq, dk, dv], 1), 1e-10)
    else:
        _close(ref["grads"]["q"], dq, 1e-10)
        _close(ref["grads"]["kv"], torch.cat([dk, dv], 1), 1e-10)


def test_loss_models_are_the_oracles_losses_in_float64():
    for name in _of("_MaskedL1Fn"):
        t = _t64(CASES[name])
        _close(M.reference(CASES[name])["outs"][0], O.l1_loss(t["pred"], t["target"]))
        assert torch.equal(t["w"], O.weights_nonzero_speech(t["target"])[..., 0].reshape(-1).double())
    for name in _of("_SSIMLossFn"):
        t = _t64(CASES[name])
        _close(M.reference(CASES[name])["outs"][0], O.ssim_loss(t["pred"], t["target"], CASES[name]["c"]["bias"]))
    for name in _of("_DurLossFn"):
        t, c = _t64(CASES[name]), CASES[name]["c"]
        pd, wd = O.dur_losses(t["dur_pred"], t["mel2ph"], t["txt"], (1, 2, 3), c["lam_p"], c["lam_w"])
        got = M.reference(CASES[name])["outs"]
        _close(got[0], pd)
        _close(got[1], wd)
        assert float(pd) > 0 and float(wd) > 0 and (t["txt"] == 0).any()
    for name in _of("_PitchLossFn"):
        t, c = _t64(CASES[name]), CASES[name]["c"]
        uvl, f0l = O.pitch_losses(t["pp"].transpose(1, 2), t["f0"], t["uv"], t["mel2ph"], c["lam_uv"], c["lam_f0"])
        got = M.reference(CASES[name])["outs"]
        _close(got[0], uvl)
        _close(got[1], f0l)


def test_composed_models_are_their_parts():
    """the fused nodes' models are compositions of the pinned pieces: spot-check one of each against a restatement with torch modules"""
    cs, t = CASES["ffn_same_k3_mask"], _t64(CASES["ffn_same_k3_mask"])
    c = cs["c"]
    h = F.layer_norm(t["x"].transpose(1, 2), (32,), t["gamma"], t["beta"], c["eps"]).transpose(1, 2)
    f = F.conv1d(F.gelu(F.conv1d(h, t["w1"], t["b1"], padding=1) * c["alpha"]), t["w2"], t["b2"])
    _close(M.reference(cs)["outs"][0], (t["x"] + f) * t["mask"][:, None])
    cs, t = CASES["preln_cross_attn_kpm_want_p"], _t64(CASES["preln_cross_attn_kpm_want_p"])
    H = 64
    mha = torch.nn.MultiheadAttention(H, 2, bias=False, batch_first=True, dtype=F64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(t["w_in"][:, :, 0])
        mha.out_proj.weight.copy_(t["w_out"][:, :, 0])
        h = F.layer_norm(t["x"].transpose(1, 2), (H,), t["gamma"], t["beta"], 1e-5)
        o, p = mha(h, t["enc"].transpose(1, 2), t["enc"].transpose(1, 2), key_padding_mask=t["kpm"] != 0, average_attn_weights=False)
    _close(M.reference(cs)["outs"][0], t["x"] + o.transpose(1, 2), 1e-7)  # (-1e8 against torch's -inf on padded keys: the same to 1e-7)
    _close(M.reference(cs)["outs"][1], p, 1e-7)


# ---- mirrors, budgets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in M.CASES if c["mode"] == "bounded"])
def test_mirror_stays_near_the_model(name):
    ref = M.reference(CASES[name])
    pairs = list(zip(ref["outs"], ref["m_outs"])) + [(ref["grads"][k], ref["m_grads"][k]) for k in CASES[name]["diff"]]
    whole = max(float(m.abs().max()) for m, _ in pairs if m.numel())
    for model, mirror in pairs:
        scale = float(model.abs().max()) if model.numel() else 0.0
        # 2e-4 of the tensor (ssim: differences of near-equal moments), or 64 u of the case where the tensor itself cancels to nothing
        # (attention over ONE key: dq = 0 in the model, the documented form of the kernels leaves the rounding of two equal sums)
        assert float((mirror.double() - model).abs().max()) <= 2e-4 * scale + 64 * M.U * whole, name
        assert bool(torch.isfinite(mirror).all())


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES if c["mode"] == "exact"])
def test_exact_cases_are_exact_in_fp32(name):
    """every operand, output and gradient is an integer multiple of 2^-4 whose absolute-value model -- the same expression on |operands|,
    without the activation: an upper bound of every partial sum in any order -- stays below 2^24 / 16"""
    cs = CASES[name]
    ref = M.reference(cs)
    values = list(ref["outs"]) + [ref["grads"][k] for k in cs["diff"]] + [v for v in M.operands(cs).values() if v.is_floating_point()]
    for v in values:
        assert torch.equal(v.double() * 16, (v.double() * 16).round()), name
    for a, b in zip(ref["outs"] + [ref["grads"][k] for k in cs["diff"]], ref["m_outs"] + [ref["m_grads"][k] for k in cs["diff"]]):
        assert torch.equal(a, b.double()), name
    absolute = dict(cs, name=name + "_abs", c=dict(cs["c"], act="none") if "act" in cs["c"] else cs["c"])
    M._OPS[absolute["name"]] = {k: (v.abs() if v.is_floating_point() else v) for k, v in M.operands(cs).items()}
    outs, grads = M.evaluate(absolute, F64, ups=[u.abs() for u in ref["ups"]])
    budget = max([float(o.abs().max()) for o in outs] + [float(g.abs().max()) for g in grads.values()])
    assert budget * 16 < 2 ** 24, (name, budget)


def test_relu_residual_case_flips_the_sign_of_a_quarter_of_the_outputs():
    cs = CASES[M.RELU_RES_CASE]
    t = _t64(cs)
    z = M.conv_z({k: v for k, v in t.items() if k != "res"}, cs["c"])
    flipped = ((F.relu(z) + t["res"]) > 0) != (z > 0)
    assert float(flipped.double().mean()) >= 0.25, float(flipped.double().mean())
    assert cs["mode"] == "exact" and "res" in cs["diff"]


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
def _separation(cs, faulty, keys):
    """the largest |fault - model| / bar over the gradients `keys`: the bar of the GPU comparison (0 on an exact case: any effect counts)"""
    ref = M.reference(cs)
    best = 0.0
    for k in keys:
        eff = (faulty[k].double() - ref["grads"][k]).abs()
        if cs["mode"] == "exact":
            best = max(best, float("inf") if bool(eff.any()) else 0.0)
        else:
            bar = torch.from_numpy(np.broadcast_to(np.asarray(M.bar(ref["grads"][k], ref["m_grads"][k])), tuple(eff.shape)).copy())
            best = max(best, float((eff / bar).max()))
    return best


def _swapped(cs):
    ups = M.reference(cs)["ups"]
    if cs["node"] == "_ResSkipFn":  # the two scales of the upstream pair exchanged
        s = cs["c"]["up_scale"]
        ups = [ups[0] / s[0] * s[1], ups[1] / s[1] * s[0]]
    else:
        ups = [ups[1], ups[0]]
    return M.evaluate(cs, F64, ups=ups)[1]


def _kv_rows_off_by_h(cs):
    g = M.reference(cs)["grads"]["w_in"].clone()
    H = g.shape[1]
    g[H:] = torch.roll(g[H:], H, 0)
    return dict(w_in=g)


def _dalpha_without_the_incoming_gradient(cs):
    t = _t64(cs)
    return dict(alpha=t["table"][t["pos"]].sum().reshape(1))


FAULTS = [
    ("relu gated on y + res", M.RELU_RES_CASE, lambda cs: M.evaluate(cs, F64, fault="relu_gate_on_y_res")[1], ("x", "w", "b")),
    ("swapped upstream scalars, duration", M.SWAP_CASES[0], _swapped, ("dur_pred",)),
    ("swapped upstream scalars, pitch", M.SWAP_CASES[1], _swapped, ("pp",)),
    ("swapped upstream scalars, res_skip", M.SWAP_CASES[2], _swapped, ("x", "o", "skip")),
    ("missing 1 / pro_param in dx", M.PRO_CASE, lambda cs: M.evaluate(cs, F64, fault="no_inv_pro")[1], ("x", "add")),
    ("alpha applied twice in _PreLnFfnFn", M.FFN_ALPHA_CASE, lambda cs: M.evaluate(cs, F64, fault="alpha_twice")[1], ("x", "w1", "b1")),
    ("residual gradient taken before the mask", M.PRO_CASE, lambda cs: M.evaluate(cs, F64, fault="res_before_mask")[1], ("res",)),
    ("k / v row offset of the packed weight off by H", M.KV_CASE, _kv_rows_off_by_h, ("w_in",)),
    ("dalpha of _PosAddFn without the incoming gradient", M.POS_CASE, _dalpha_without_the_incoming_gradient, ("alpha",)),
]


@pytest.mark.parametrize("what,name,fault,keys", FAULTS, ids=[f[0] for f in FAULTS])
def test_bars_separate_planted_faults(what, name, fault, keys):
    cs = CASES[name]
    for k in keys:
        assert _separation(cs, fault(cs), (k,)) >= 8.0, (what, k)


def test_equal_upstream_scalars_would_hide_a_swap():
    """why the (1, 1) pair alone was not enough: under it the swapped node gives the same gradient"""
    for name in ("dur_loss_ups_1_1", "pitch_loss_ups_1_1"):
        assert _separation(CASES[name], _swapped(CASES[name]), CASES[name]["diff"]) == 0.0
    assert M.TWO_OUTPUT_UPS == ((1.0, 1.0), (3.0, 0.25), (0.0, 1.0))
    for node in ("_DurLossFn", "_PitchLossFn", "_ResSkipFn"):
        pairs = {CASES[n].get("ups") or CASES[n]["c"].get("up_scale") for n in _of(node)}
        assert set(M.TWO_OUTPUT_UPS) <= pairs, node


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_shapes_and_branches():
    convs = [CASES[n]["c"] for n in _of("_Conv1dFn")]
    assert {c["B"] for c in convs} >= {1, 3} and {c["T"] for c in convs} >= {1, 15, 16, 33, 70}
    assert {c["Cin"] for c in convs} | {c["Cout"] for c in convs} >= {7, 32, 96}
    for form in ("identity", "alpha", "mask", "relu", "relu_mask", "relu_alpha", "pro_div"):
        for r in ("", "_res"):
            assert "conv_epilogue_" + form + r in CASES
    first = CASES["conv_all_operands_b3_c7_t33_k3_dil2"]
    assert ("x", "w", "b", "res") in first["nograd"] and ("x", "w", "b", "add") in first["nograd"]  # dadd without dx; nothing but res
    assert {CASES[n]["c"]["act"] for n in _of("_Conv1dFn") if n.startswith("conv_split")} == {"gelu", "mish", "softplus", "tanh"}
    ffn = [CASES[n]["c"] for n in _of("_PreLnFfnFn")]
    assert {(c["C"], c["Cmid"], c["K"], c["pad"], bool(c.get("mask"))) for c in ffn} >= {(32, 64, 3, 1, True), (32, 64, 9, 8, False)}
    assert any(c.get("drop") and c["drop"][0] == 0.5 and c["drop"][2] > 2 ** 32 for c in ffn)
    assert {CASES[n]["c"]["T_txt"] for n in _of("_ExpandStatesFn")} >= {1, 14}
    assert {CASES[n]["c"]["T"] for n in _of("_SSIMLossFn")} == {7, 33} and all(CASES[n]["c"]["M"] == 80 for n in _of("_SSIMLossFn") + _of("_MaskedL1Fn"))
    attn = [CASES[n]["c"] for n in _of("_AttnFn")]
    assert {(c["form"], c["H"] // c["heads"]) for c in attn} >= {("self", 32), ("cross", 32), ("self", 7)}
    assert {bool(c.get("want_p")) for c in attn} == {True, False} and {bool(c.get("kpm")) for c in attn} == {True, False}
    assert M.BF16_WGRAD == {"conv_wgrad_dtype_cin31_cout32": False, "conv_wgrad_dtype_cin32_cout31": False, "conv_wgrad_dtype_cin32_cout32": True}
    assert all(CASES[n]["c"]["T"] == 16 for n in M.BF16_WGRAD)


# ---- the inventory ----------------------------------------------------------------------------------------------------------------------
def _nodes(src):
    """{class name: (forward FunctionDef, backward FunctionDef)} of every torch.autograd.Function subclass in the source"""
    out = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and any(ast.unparse(b) == "torch.autograd.Function" for b in node.bases):
            fns = {f.name: f for f in node.body if isinstance(f, ast.FunctionDef)}
            out[node.name] = (fns["forward"], fns["backward"])
    return out


def _needs_input_grad_reads(backward):
    return sorted({n.slice.value for n in ast.walk(backward) if isinstance(n, ast.Subscript) and ast.unparse(n.value) == "ctx.needs_input_grad"
                   and isinstance(n.slice, ast.Constant)})


def _optional_operands(forward):
    """forward arguments that may be None: compared with None in the body, or given a default of None"""
    args = [a.arg for a in forward.args.args]
    found = {n.left.id for n in ast.walk(forward) if isinstance(n, ast.Compare) and isinstance(n.left, ast.Name) and n.left.id in args
             and any(isinstance(o, (ast.Is, ast.IsNot)) for o in n.ops)}
    defaults = forward.args.defaults
    found |= {a for a, d in zip(args[len(args) - len(defaults):], defaults) if isinstance(d, ast.Constant) and d.value is None}
    return sorted(found)


def _inventory(src, table, elsewhere):
    """-> list of what is missing"""
    missing = []
    for name, (fwd, bwd) in _nodes(src).items():
        if name in elsewhere:
            continue
        cases = [c for c in M.CASES if c["node"] == name]
        if name not in table or not cases:
            missing.append("%s: no case" % name)
            continue
        args = [a.arg for a in fwd.args.args][1:]  # (without ctx)
        for i in _needs_input_grad_reads(bwd):
            operand = M.NEEDS_INPUT_GRAD.get(name, {}).get(i)
            if operand is None or not any(operand in off for c in cases for off in c["nograd"]):
                missing.append("%s: needs_input_grad[%d] (%s) has no case with that input not requiring grad" % (name, i, args[i]))
        for arg in _optional_operands(fwd):
            if not any(M.ARG_NAMES.get(arg, arg) in c["absent"] for c in cases):
                missing.append("%s: no case without %s" % (name, arg))
    return missing


def test_every_tape_node_has_its_cases():
    src = open(SRC).read()
    nodes = _nodes(src)
    assert len(nodes) >= 29 and set(M.MODELS) <= set(nodes) and set(M.SWEPT_ELSEWHERE) <= set(nodes)
    assert not set(M.MODELS) & set(M.SWEPT_ELSEWHERE)
    assert _inventory(src, M.MODELS, M.SWEPT_ELSEWHERE) == []
    # the reads the table is held to are the reads of the source
    assert _needs_input_grad_reads(nodes["_Conv1dFn"][1]) == [0, 1, 2, 3, 4]
    assert set(_optional_operands(nodes["_Conv1dFn"][0])) >= {"bias", "chan_add", "res", "t_out"}
    assert _optional_operands(nodes["_ResSkipFn"][0]) == ["skip_in"] and "drop" in _optional_operands(nodes["_PreLnFfnFn"][0])


def test_inventory_fails_for_a_node_without_cases():
    """a node added later without a case, a new needs_input_grad read and a new optional operand each fail the inventory"""
    src = open(SRC).read()
    table = {k: v for k, v in M.MODELS.items() if k != "_GateFn"}
    assert _inventory(src, table, M.SWEPT_ELSEWHERE) == ["_GateFn: no case"]
    new = src + "\n\nclass _NewFn(torch.autograd.Function):\n    @staticmethod\n    def forward(ctx, x):\n        return x\n\n" \
                "    @staticmethod\n    def backward(ctx, d):\n        return d\n"
    assert _inventory(new, M.MODELS, M.SWEPT_ELSEWHERE) == ["_NewFn: no case"]
    more = src.replace("        return d, d\n", "        return (d if ctx.needs_input_grad[0] else None), d\n", 1)
    assert more != src and _inventory(more, M.MODELS, M.SWEPT_ELSEWHERE) == \
        ["_AddFn: needs_input_grad[0] (a) has no case with that input not requiring grad"]
    opt = src.replace("    def forward(ctx, y):\n        y = y.contiguous()", "    def forward(ctx, y, extra=None):\n        y = y.contiguous()", 1)
    assert opt != src and _inventory(opt, M.MODELS, M.SWEPT_ELSEWHERE) == ["_GateFn: no case without extra"]


def test_nodes_swept_elsewhere_name_a_test_that_mentions_them():
    for node, (module, test, mention) in M.SWEPT_ELSEWHERE.items():
        text = open(os.path.join(ROOT, "tests", module)).read()
        m = re.search(r"^def %s\(.*?(?=^def |^@pytest|\Z)" % re.escape(test), text, re.S | re.M)
        assert m, (node, module, test)
        assert mention in m.group(0), (node, test, mention)
        assert "pytest.mark.gpu" in text
    mine = open(os.path.join(ROOT, "tests", "test_gpu_tape_branches.py")).read()
    m = re.search(r"^def test_diffnet_stack_node_with_cond_detached\(.*?(?=^def |\Z)", mine, re.S | re.M)
    assert m and "_DiffNetStackFn" in m.group(0) and "diffnet_stack_train" in m.group(0)
