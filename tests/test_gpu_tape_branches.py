"""GPU branch sweep of the autograd tape (set_amd/autograd_ops.py): every hand-written torch.autograd.Function node, ONE forward and ONE
backward per case, against the float64 torch models of tests/tape_models.py (torch autograd in float64 supplies every gradient; the models
are tied to torch.nn.functional, the attention model and the oracle's losses by tests/test_tape_reference.py).

What a `backward` decides on the host is what is swept: which inputs get a gradient (`needs_input_grad`: an input that does not require grad
comes back None and the others keep their bits), absent optional operands, the epilogue forms of _Conv1dFn, upstream gradients that are not
contiguous (same bits as with the contiguous copy, the incoming buffer unchanged), distinct upstream scalars for the nodes with two outputs,
the weight-gradient selection of conv_wgrad, and where a parameter gradient is written: through autograd, through autograd with the zero
arena open, in place into the flat optimizer's .grad view on the leaf stream, a parameter used twice, a row slice of a packed parameter,
two backwards before one step.

exact cases (integer operands) must equal the float64 model bit for bit; bounded cases stay within mirror_bar(model, float32 mirror)
elementwise, per output and per gradient.  Floating operands and upstream gradients live 64 floats inside NaN-filled allocations that are
compared afterwards: a node may not write its operands or around them.  The largest |gpu - model| / bar per node goes to
profiles/tape_branch_sweep.log when the module finishes; a ratio above 1 is a finding about the node, not a bar to widen."""
import os
import types

import numpy as np
import pytest
import torch

import tape_models as M
from test_gpu_conv_branches import _keep_launch_operands, dev  # noqa: F401

pytestmark = pytest.mark.gpu

G = M.G
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tape_branch_sweep.log")
WORST = {}  # node -> [comparisons, worst ratio, case, tensor]
EXACT = {}  # node -> tensors that matched bit for bit
CASES = M.BY_NAME


def _lib():
    from set_amd import autograd_ops as A, ops
    return A, ops


# =====================================================================================================================================
# guarded operands, comparisons, the log
# =====================================================================================================================================
class Guarded:
    """a float tensor G floats inside a NaN-filled allocation (the view is 256-byte aligned and contiguous); check(): nothing around it was
    written and it still holds the bits it was given"""

    def __init__(self, dev, t):
        self.host = t.detach().float().contiguous().cpu()
        n = self.host.numel()
        self.full = torch.full((n + 2 * G,), float("nan"), dtype=torch.float32, device=dev)
        self.view = self.full[G:G + n].view(self.host.shape)
        self.view.copy_(self.host)
        self.n = n

    def check(self, what):
        a = self.full.cpu()
        assert bool(torch.isnan(a[:G]).all()) and bool(torch.isnan(a[G + self.n:]).all()), "%s: written outside the buffer" % what
        got = a[G:G + self.n].numpy().view(np.uint32)
        assert np.array_equal(got, self.host.reshape(-1).numpy().view(np.uint32)), "%s: the node wrote into its operand" % what


def _exact(node, case, what, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (case, what, tuple(got.shape), tuple(want.shape))
    assert torch.equal(want.float().double(), want.double()), (case, what, "the model is not representable")
    bad = got.double() != want.double()
    assert not bool(bad.any()), (node, case, what, int(bad.sum()), got[bad][:4], want[bad][:4])
    EXACT[node] = EXACT.get(node, 0) + 1


def _bounded(node, case, what, got, want, mirror):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (case, what, tuple(got.shape), tuple(want.shape))
    bar = torch.from_numpy(np.broadcast_to(np.asarray(M.bar(want, mirror.detach().cpu()), dtype=np.float64), tuple(want.shape)).copy())
    assert bool(torch.isfinite(got).all()), (node, case, what, "not finite")
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    rec = WORST.setdefault(node, [0, 0.0, case, what])
    rec[0] += 1
    if worst >= rec[1]:
        rec[1], rec[2], rec[3] = worst, case, what
    print("%s %s %s: worst error / bar %.4f (error %.3e)" % (node, case, what, worst, float(err.max()) if err.numel() else 0.0))
    assert worst <= 1.0, (node, case, what, worst)


def _compare(cs, what, got, want, mirror):
    if cs["mode"] == "exact":
        _exact(cs["node"], cs["name"], what, got, want)
    else:
        _bounded(cs["node"], cs["name"], what, got, want, mirror)


@pytest.fixture(scope="module", autouse=True)
def _sweep_log():
    yield
    if not WORST and not EXACT:
        return
    lines = ["autograd tape branch sweep (tests/test_gpu_tape_branches.py) on one MI355X", "",
             "exact mode: outputs and gradients bit-identical to the float64 model, tensors per node"]
    lines += ["  %-22s %4d" % (k, v) for k, v in sorted(EXACT.items())]
    lines += ["", "bounded mode: largest |node - model| / bar per node over its outputs and gradients (bars: tests/tape_models.py)", "",
              "%-22s %7s  %-7s  %s" % ("node", "tensors", "worst", "case, tensor")]
    lines += ["%-22s %7d  %.4f   %s, %s" % (k, n, w, c, t) for k, (n, w, c, t) in sorted(WORST.items())]
    text = "\n".join(lines) + "\n"
    print(text)
    try:
        with open(LOG, "w") as f:
            f.write(text)
    except OSError:
        pass  # a read-only checkout: the table is in the output above


# =====================================================================================================================================
# the nodes: d = operands by name on the device, c = the case's settings -> tuple of outputs
# =====================================================================================================================================
def _cw(d, name, base=0, rows=None):
    _, ops = _lib()
    w = d[name]
    return ops.ConvWeight(lambda: d[name], w.shape[0] if rows is None else rows, w.shape[1], w.shape[2], base=base)


def r_conv(A, d, c):
    return (A.conv1d(d["x"], _cw(d, "w"), d.get("b"), dil=c.get("dil", 1), pad=c["pad"], pro=c.get("pro", "none"),
                     pro_param=c.get("pro_param", 0.0), act=c.get("act", "none"), alpha=c.get("alpha", 1.0), res=d.get("res"),
                     mask=d.get("mask"), in_chan_add=d.get("add"), T_out=c.get("T_out")),)


def r_ffn(A, d, c):
    return (A.preln_ffn(d["x"], (d["gamma"], d["beta"]), _cw(d, "w1"), d["b1"], _cw(d, "w2"), d["b2"], pad=c["pad"], alpha=c["alpha"],
                        act=c["act"], mask=d.get("mask"), eps=c["eps"], T_out=d["x"].shape[2], drop=c.get("drop")),)


def _attn_module(d, c):
    H = d["x"].shape[1]
    return types.SimpleNamespace(embed_dim=H, num_heads=c["heads"], scaling=c["alpha"], _w_qkv=_cw(d, "w_in"), _w_q=_cw(d, "w_in", rows=H),
                                 _w_kv=_cw(d, "w_in", base=H * H, rows=2 * H), _w_out=_cw(d, "w_out"))


def _with_p(c, o, p):
    if c.get("want_p"):
        return (o, p)
    if _lib()[1].attention_fused_on(o.shape[1] // c["heads"]):
        assert p.numel() == 0  # not asked for: the fused kernels do not materialise it, the node returns the empty tensor
    return (o,)


def r_attn(A, d, c):
    if c["form"] == "self":
        o, p = A.self_attention(d["qkv"], c["heads"], d.get("kpm"), c["fill"], c["alpha"], want_p=bool(c.get("want_p")))
    else:
        o, p = A.cross_attention(d["q"], d["kv"], c["heads"], d.get("kpm"), c["fill"], c["alpha"], want_p=bool(c.get("want_p")))
    return _with_p(c, o, p)


def r_cross(A, d, c):
    y, p = A.preln_cross_attn(d["x"], (d["gamma"], d["beta"]), _attn_module(d, c), d["enc"], d.get("kpm"), want_p=bool(c.get("want_p")),
                              eps=c["eps"])
    return _with_p(c, y, p)


RUN = {
    "_Conv1dFn": r_conv,
    "_ActFn": lambda A, d, c: (A.activation(d["z"], c["act"]),),
    "_LayerNormChFn": lambda A, d, c: (A.layernorm_ch(d["x"], d["gamma"], d["beta"], d.get("mask"), c["eps"]),),
    "_PreLnFfnFn": r_ffn,
    "_AddFn": lambda A, d, c: (A.add(d["a"], d["b"]),),
    "_EmbeddingFn": lambda A, d, c: (A.embedding_bct(d["idx"], d["table"], scale=c["scale"], out=d.get("base"), accumulate="base" in d,
                                                      padding_idx=c.get("padding_idx")),),
    "_ExpandStatesFn": lambda A, d, c: (A.expand_states(d["enc"], d["mel2ph"]),),
    "_AddChanMaskFn": lambda A, d, c: (A.add_chan_mask(d["x"], d.get("add"), d.get("mask")),),
    "_TransposeFn": lambda A, d, c: ((A.btc_to_bct if c["to_bct"] else A.bct_to_btc)(d["x"]),),
    "_GateFn": lambda A, d, c: (A.gate(d["y"]),),
    "_ResSkipFn": lambda A, d, c: tuple(A.res_skip_fn(d["x"], d["o"], d.get("skip"))),
    "_DropoutFn": lambda A, d, c: (A.dropout(d["x"], c["p"], c["seed"], c["offset"]),),
    "_FanoutFn": lambda A, d, c: tuple(A.fanout(d["x"], c["n"])),
    "_GradScaleFn": lambda A, d, c: (A.grad_scale(d["x"], c["s"]),),
    "_SumLossesFn": lambda A, d, c: (A.sum_losses([d["v%d" % i] for i in range(c["n"])]),),
    "_AttnFn": r_attn,
    "_PreLnSelfAttnFn": lambda A, d, c: (A.preln_self_attn(d["x"], (d["gamma"], d["beta"]), _attn_module(d, c), d.get("kpm"), d.get("mask"),
                                                           c["eps"]),),
    "_PreLnCrossAttnFn": r_cross,
    "_PosAddFn": lambda A, d, c: (A.pos_add(d["x"], d["alpha"], d["pos"], d["table"]),),
    "_MaskFillChanFn": lambda A, d, c: (A.mask_fill_chan(d["x"], d["e"], d["m"]),),
    "_AddMaskedFn": lambda A, d, c: (A.add_masked(d["a"], d["b"], d["m"]),),
    "_MaskedL1Fn": lambda A, d, c: (A.masked_l1(d["pred"], d["target"], d["w"]),),
    "_SSIMLossFn": lambda A, d, c: (A.ssim_loss(d["pred"], d["target"], d["w"], c["bias"]),),
    "_DurLossFn": lambda A, d, c: tuple(A.dur_losses(d["dur_pred"], d["mel2ph"], d["txt"], d["word_id"], int(d["word_id"].max()), c["lam_p"],
                                                     c["lam_w"])),
    "_PitchLossFn": lambda A, d, c: tuple(A.pitch_losses(d["pp"], d["f0"], d["uv"], d["mel2ph"], c["lam_uv"], c["lam_f0"])),
}
assert set(RUN) == set(M.MODELS)


def _n_diff(cs, outs):
    return M.n_diff_outputs(cs) or len(outs)


def _layout(dev, u, layout):
    """the upstream gradient u (CPU) on the device as (guard, tensor handed to backward): contiguous, a transposed view of a buffer that holds
    its transpose, or a stride-0 expansion of one element"""
    if layout == "transposed":
        g = Guarded(dev, u.transpose(-1, -2).contiguous())
        return g, g.view.transpose(-1, -2)
    if layout == "expand":
        g = Guarded(dev, u.reshape(-1)[:1])
        return g, g.view.reshape(()).expand(u.shape)
    g = Guarded(dev, u)
    return g, g.view


def run_case(dev, cs, nograd=(), layout="contig", ups=None, params=None):
    """one forward and one backward of the case -> (outputs, {operand: .grad or None}).  nograd: operands that do not require grad in this
    run; layout: of every upstream gradient; params: {name: nn.Parameter} used in place of the operands of those names."""
    A, _ = _lib()
    host = M.operands(cs)
    guards, d = {}, {}
    for k, v in host.items():
        if params is not None and k in params:
            d[k] = params[k]
        elif v.is_floating_point():
            guards[k] = Guarded(dev, v)
            d[k] = guards[k].view.detach().requires_grad_(k in cs["diff"] and k not in nograd)
        else:
            d[k] = v.to(dev)
    with torch.enable_grad():
        outs = RUN[cs["node"]](A, d, cs["c"])
    nd = _n_diff(cs, outs)
    ups = M.reference(cs)["ups"] if ups is None else ups
    placed = [_layout(dev, u, layout if u.dim() >= 2 or layout == "expand" else "contig") for u in ups]
    wanted = [o for o in outs[:nd] if o.requires_grad]
    if wanted:
        torch.autograd.backward(list(outs[:nd]), [t for _, t in placed])
    torch.cuda.synchronize()
    for k, g in guards.items():
        g.check("%s operand %s" % (cs["name"], k))
    for i, (g, _) in enumerate(placed):
        g.check("%s upstream gradient %d" % (cs["name"], i))
    return [o.detach() for o in outs], {k: d[k].grad for k in cs["diff"]}


def _check_against_model(cs, outs, grads):
    ref = M.reference(cs)
    assert len(outs) == len(ref["outs"])
    for i, (o, want, mirror) in enumerate(zip(outs, ref["outs"], ref["m_outs"])):
        _compare(cs, "out%d" % i, o, want, mirror)
    for k in cs["diff"]:
        assert grads[k] is not None, (cs["name"], k)
        _compare(cs, "d" + k, grads[k], ref["grads"][k], ref["m_grads"][k])


# =====================================================================================================================================
# the sweep
# =====================================================================================================================================
@pytest.mark.parametrize("name", list(CASES))
def test_node_matches_the_float64_model(dev, name):
    """every output and every gradient of the all-wanted run: bit for bit (exact) or within the mirror bar (bounded); then every
    `needs_input_grad` combination of the case: an input that does not require grad comes back None, the others keep their bits"""
    cs = CASES[name]
    outs, grads = run_case(dev, cs)
    _check_against_model(cs, outs, grads)
    for off in cs["nograd"]:
        outs2, grads2 = run_case(dev, cs, nograd=off)
        for a, b in zip(outs, outs2):
            assert torch.equal(a, b), (name, off)
        for k in cs["diff"]:
            if k in off:
                assert grads2[k] is None, (name, off, k)
            else:
                assert grads2[k] is not None and torch.equal(grads2[k], grads[k]), (name, off, k)


def test_conv_relu_with_a_residual_gates_on_the_pre_residual_sign(dev):
    """The defect this sweep was written around: _Conv1dFn gates ReLU on its saved output, which is relu(z) + res when a residual is fused.
    conv1d() now runs the residual (and the mask) as nodes of their own; the exact case has relu(z) + res and z of opposite sign wherever
    z != 0, so a gate on the sum fails on most of dx, dW and db.  The fused form is refused by the node itself."""
    A, ops = _lib()
    cs = CASES[M.RELU_RES_CASE]
    outs, grads = run_case(dev, cs)
    _check_against_model(cs, outs, grads)
    x, w, res = (torch.zeros(s, device=dev) for s in ((1, 7, 16), (7, 7, 1), (1, 7, 16)))
    with pytest.raises(AssertionError):
        A._Conv1dFn.apply(x, w, None, None, res, ops.ConvWeight(lambda: w, 7, 7, 1), 1, 0, "none", 0.0, "relu", 1.0, None, None)


def test_conv_identity_epilogue_hands_the_incoming_gradient_on(dev):
    """act none, alpha 1, no mask: no epilogue launch -- the residual's gradient IS the incoming tensor"""
    A, ops = _lib()
    cs = CASES["conv_epilogue_identity_res"]
    host = M.operands(cs)
    d = {k: v.to(dev).requires_grad_(True) for k, v in host.items()}
    with torch.enable_grad():
        (y,) = r_conv(A, d, cs["c"])
    dy = M.reference(cs)["ups"][0].to(dev)
    back = A._Conv1dFn.backward(y.grad_fn, dy)  # (the node object is the ctx of its backward)
    torch.cuda.synchronize()
    assert back[4] is dy
    _exact("_Conv1dFn", cs["name"], "dx by hand", back[0], M.reference(cs)["grads"]["x"])


_FIRST = {}
for _cs in M.CASES:
    _FIRST.setdefault(_cs["node"], _cs["name"])
LAYOUT_CASES = sorted(set(_FIRST.values()) | {"conv_epilogue_relu_mask", "conv_split_gelu_mask_alpha", "ffn_drop_offset_above_2_32_mask",
                                              "preln_cross_attn_kpm_want_p", "attn_cross_d32_kpm_want_p"})


LAYOUT_RUNS = [(n, "expand") for n in LAYOUT_CASES] + \
    [(n, "transposed") for n in LAYOUT_CASES if any(u.dim() >= 2 for u in M.reference(CASES[n])["ups"])]  # (a loss has no transposed view)


@pytest.mark.parametrize("name,layout", LAYOUT_RUNS)
def test_upstream_gradient_that_is_not_contiguous(dev, name, layout):
    """a transposed view, and a stride-0 expansion as y.sum().backward() produces: the bits of the run on the contiguous copy, and the
    incoming buffer unchanged (run_case compares it)"""
    cs = CASES[name]
    ups = M.reference(cs)["ups"]
    if layout == "expand":
        ups = [u if u.dim() == 0 else torch.ones(()).expand(u.shape) for u in ups]
    _, want = run_case(dev, cs, ups=[u.contiguous() for u in ups])
    _, got = run_case(dev, cs, ups=ups, layout=layout)
    for k in cs["diff"]:
        assert got[k] is not None and torch.equal(got[k], want[k]), (name, layout, k)


@pytest.mark.parametrize("name", ["attn_self_d32_kpm_want_p", "attn_self_d32_no_kpm_no_p", "attn_cross_d32_kpm_want_p",
                                  "attn_cross_d32_no_kpm_no_p"])
def test_attention_node_three_launch_form(dev, name, monkeypatch):
    """SET_AMD_ATTN_FUSED=0: bmm -> softmax -> bmm with the probabilities saved, at the head size the fused kernels take by default"""
    monkeypatch.setenv("SET_AMD_ATTN_FUSED", "0")
    cs = CASES[name]
    outs, grads = run_case(dev, cs)
    _check_against_model(cs, outs, grads)


@pytest.mark.parametrize("name", list(M.BF16_WGRAD))
def test_conv_wgrad_operand_type_under_bf16(dev, name):
    """set_compute_dtype("bf16") at T = 16 (the convs stay on the fp32 kernels): Cin or Cout of 31 keeps fp32 weight-gradient operands -- the
    f32 run's bits; 32 x 32 takes bf16 operands -- dW differs, and only dW"""
    _, ops = _lib()
    cs = CASES[name]
    _, f32 = run_case(dev, cs)
    ops.set_compute_dtype("bf16")
    try:
        _, b16 = run_case(dev, cs)
    finally:
        ops.set_compute_dtype("f32")
    assert torch.equal(b16["x"], f32["x"]) and torch.equal(b16["b"], f32["b"])
    assert torch.equal(b16["w"], f32["w"]) != M.BF16_WGRAD[name], name


# =====================================================================================================================================
# gradient routes
# =====================================================================================================================================
ROUTES = {  # case -> (its parameters, does the node launch their gradient kernels on the leaf stream when every target is a .grad view)
    "conv_all_operands_b3_c7_t33_k3_dil2": (("w", "b"), True),
    "conv_t15_naive_wgrad": (("w", "b"), True),
    "conv_epilogue_relu_mask": (("w", "b"), True),
    "conv_bounded_pro_div_alpha_res_mask": (("w", "b"), True),
    "layernorm_mask_b3_c7_t33": (("gamma", "beta"), False),
    "ffn_same_k3_mask": (("gamma", "beta", "w1", "b1", "w2", "b2"), True),
    "ffn_drop_offset_above_2_32_mask": (("gamma", "beta", "w1", "b1", "w2", "b2"), True),
    "embedding_base_scale2": (("table",), True),
    "preln_self_attn_kpm_mask": (("gamma", "beta", "w_in", "w_out"), True),
    "preln_cross_attn_kpm_want_p": (("gamma", "beta", "w_in", "w_out"), True),
}


class Holder(torch.nn.Module):
    """a minimal module that holds just a node's parameters"""

    def __init__(self, dev, tensors):
        super().__init__()
        for k, v in tensors.items():
            setattr(self, k, torch.nn.Parameter(v.clone().to(dev)))

    def params(self):
        return dict(self.named_parameters())


def _optimizer(holder):
    from set_amd.training import FlatAdamW
    return FlatAdamW(holder, lr=1e-3, warmup_updates=0, clip_grad_norm=1.0)


def _restore(opt, p0):
    """put the parameters back after a step() (and every weight image with them): the next step sees the operands of the case again"""
    opt.flat_p.copy_(p0)
    _lib()[1].bump_weights_epoch()


def _grads(holder):
    return {k: p.grad.clone() for k, p in holder.params().items()}


def run_routes(dev, cs, pnames, monkeypatch):
    """(a) no optimizer; (b) the learning step of a FlatAdamW: through autograd, temporaries from the zero arena; (c) the next step: in place
    into the .grad views.  -> {route: (outputs, input gradients, parameter gradients)}, and whether (c) launched on the leaf stream"""
    A, _ = _lib()
    from set_amd import leaf_stream
    host = M.operands(cs)
    holder = Holder(dev, {k: host[k] for k in pnames})
    res = {}
    outs, ins = run_case(dev, cs, params=holder.params())
    res["a"] = (outs, ins, _grads(holder))
    for p in holder.parameters():
        p.grad = None
    opt = _optimizer(holder)
    p0 = opt.flat_p.clone()
    arena = []
    real = A._gzeros
    monkeypatch.setattr(A, "_gzeros", lambda shape, device: (arena.append(A._ACTIVE[0] is not None), real(shape, device))[1])
    opt.zero_grad()
    outs, ins = run_case(dev, cs, params=holder.params())
    res["b"] = (outs, ins, _grads(holder))
    opt.step()
    _restore(opt, p0)
    assert arena and all(arena)  # every zeroed temporary of the learning step was asked for with the arena open
    used = []

    class Rec(leaf_stream.leaf_work):
        def __enter__(self):
            on = super().__enter__()
            used.append(on)
            return on
    monkeypatch.setattr(leaf_stream, "leaf_work", Rec)
    opt.zero_grad()
    assert all(opt.sink(p) is p.grad for p in holder.parameters())
    outs, ins = run_case(dev, cs, params=holder.params())
    res["c"] = (outs, ins, _grads(holder))  # views of opt.flat_g: backward()'s callback has joined the leaf stream
    n = sum(p.numel() for p in holder.parameters())
    if opt.flat_g.numel() > n:
        assert float(opt.flat_g[n:].abs().max()) == 0.0  # the pad of the flat buffer stays 0
    opt.step()
    return res, any(used)


@pytest.mark.parametrize("name", list(ROUTES))
def test_parameter_gradient_routes_agree(dev, name, monkeypatch):
    """Routes (a), (b) and (c) of run_routes: outputs, input gradients and parameter gradients bit-identical across the three, (a) the
    model's; (c) on the leaf stream where the node has leaf kernels."""
    cs = CASES[name]
    pnames, leaf = ROUTES[name]
    res, on_leaf = run_routes(dev, cs, pnames, monkeypatch)
    outs_a, in_a, ga = res["a"]
    _check_against_model(cs, outs_a, dict(in_a, **ga))
    assert on_leaf == leaf, name
    for r in ("b", "c"):
        outs, ins, gp = res[r]
        for a, b in zip(outs_a, outs):
            assert torch.equal(a, b), (name, r)
        for k in pnames:
            assert torch.equal(ga[k], gp[k]), (name, r, k)
        for k in cs["diff"]:
            if k not in pnames:
                assert torch.equal(in_a[k], ins[k]), (name, r, k)


def test_bf16_weight_gradient_routes_agree(dev, monkeypatch):
    """set_compute_dtype("bf16") with bf16 weight-gradient operands (32 x 32 channels): route (a) against route (c) only -- the numerics of
    the bf16 kernels belong to test_gpu_bf16_branches.py"""
    _, ops = _lib()
    ops.set_compute_dtype("bf16")
    try:
        res, on_leaf = run_routes(dev, CASES["conv_wgrad_dtype_cin32_cout32"], ("w", "b"), monkeypatch)
    finally:
        ops.set_compute_dtype("f32")
    assert on_leaf
    for k in ("w", "b"):
        assert torch.equal(res["a"][2][k], res["c"][2][k]), k


_SHARED = {}


def _with_weights_of(cs2, host):
    """the case cs2 with the weight and bias of `host`: a case of its own, made once"""
    name = cs2["name"] + "_shared_weights"
    if name not in _SHARED:
        M._OPS[name] = dict(M.operands(cs2), w=host["w"], b=host["b"])
        _SHARED[name] = dict(cs2, name=name)
    return _SHARED[name]


def _pair():
    """two convs of the same shapes, the second with the weight and bias of the first, and the float64 sum of their weight / bias gradients"""
    cs = CASES["conv_epilogue_mask"]
    cs2 = _with_weights_of(CASES["conv_epilogue_relu_mask"], M.operands(cs))
    want = {k: M.reference(cs)["grads"][k] + M.reference(cs2)["grads"][k] for k in ("w", "b")}
    return cs, cs2, want


def test_parameter_fed_to_two_nodes_keeps_the_autograd_route(dev):
    """(d) one weight and one bias read by two convs of ONE backward: the learning step counts two uses, the sink refuses them from then on,
    and .grad holds the sum -- bit for bit the float64 sum on integer operands"""
    A, _ = _lib()
    cs, cs2, want = _pair()
    holder = Holder(dev, {k: M.operands(cs)[k] for k in ("w", "b")})
    opt = _optimizer(holder)
    p0 = opt.flat_p.clone()
    for step in range(2):
        opt.zero_grad()
        if step:
            assert all(opt.sink(p) is None for p in holder.parameters())
        ys, us = [], []
        with torch.enable_grad():
            for c_ in (cs, cs2):
                d = {k: v.to(dev) for k, v in M.operands(c_).items() if k not in ("w", "b")}
                d.update(holder.params())
                ys.append(r_conv(A, d, c_["c"])[0])
                us.append(M.reference(c_)["ups"][0].to(dev))
        torch.autograd.backward(ys, us)
        torch.cuda.synchronize()
        for k, p in holder.params().items():
            _exact("_Conv1dFn", "two_uses_step%d" % step, "d" + k, p.grad, want[k])
        opt.step()
        _restore(opt, p0)


@pytest.mark.parametrize("learned", [False, True])
def test_two_backwards_before_one_step_accumulate(dev, learned):
    """(f) zero_grad(accumulate=True), two backwards, one step(): the float64 sum of both gradients, bit for bit on integer operands --
    through autograd in the learning step, and in place (the kernels add into the .grad views twice) after a learning step of one backward"""
    cs, cs2, want = _pair()
    holder = Holder(dev, {k: M.operands(cs)[k] for k in ("w", "b")})
    opt = _optimizer(holder)
    p0 = opt.flat_p.clone()
    if learned:
        opt.zero_grad()
        run_case(dev, cs, params=holder.params())
        opt.step()
        _restore(opt, p0)
    opt.zero_grad(accumulate=True)
    if learned:
        assert all(opt.sink(p) is p.grad for p in holder.parameters())
    run_case(dev, cs, params=holder.params())
    run_case(dev, cs2, params=holder.params())
    for k, p in holder.params().items():
        _exact("_Conv1dFn", "accumulate_learned%d" % learned, "d" + k, p.grad, want[k])
    opt.step()


def test_row_slice_of_a_packed_parameter_never_goes_in_place(dev):
    """(e) a ConvWeight that is rows [7, 39) of a [46, 7, 3] parameter: the gradient travels through autograd on every step (the sink is not
    even asked), and only the owned rows of .grad change -- the others keep a sentinel pattern bit for bit"""
    A, ops = _lib()
    cs = CASES["conv_epilogue_mask"]  # Cout 32, Cin 7, K 3
    host, want = M.operands(cs), M.reference(cs)["grads"]
    lo, rows, Cin, K = 7, 32, 7, 3
    big = torch.arange(46 * Cin * K, dtype=torch.float32).reshape(46, Cin, K) % 5 - 2
    big[lo:lo + rows] = host["w"]
    holder = Holder(dev, dict(wbig=big, b=host["b"]))
    sentinel = (torch.arange(big.numel(), dtype=torch.float32).reshape(big.shape) % 7 - 3).to(dev)

    def once():
        x = host["x"].to(dev).requires_grad_(True)
        cw = ops.ConvWeight((holder, "wbig"), rows, Cin, K, base=lo * Cin * K)
        with torch.enable_grad():
            y = A.conv1d(x, cw, holder.b, pad=cs["c"]["pad"], mask=host["mask"].to(dev))
            y.backward(M.reference(cs)["ups"][0].to(dev))
        torch.cuda.synchronize()
        return y.detach(), x.grad

    holder.wbig.grad = sentinel.clone()
    y, dx = once()
    g = holder.wbig.grad
    _exact("_Conv1dFn", "row_slice", "y", y, M.reference(cs)["outs"][0])
    _exact("_Conv1dFn", "row_slice", "dx", dx, want["x"])
    _exact("_Conv1dFn", "row_slice", "dw owned rows", g[lo:lo + rows] - sentinel[lo:lo + rows], want["w"])
    assert torch.equal(g[:lo], sentinel[:lo]) and torch.equal(g[lo + rows:], sentinel[lo + rows:])
    holder.wbig.grad, holder.b.grad = None, None
    opt = _optimizer(holder)
    p0 = opt.flat_p.clone()
    for step in range(2):
        opt.zero_grad()
        once()
        assert id(holder.wbig) not in opt._uses  # a row slice does not ask for the sink
        if step:
            assert opt.sink(holder.b) is holder.b.grad
        _exact("_Conv1dFn", "row_slice_step%d" % step, "dw", holder.wbig.grad[lo:lo + rows], want["w"])
        assert float(holder.wbig.grad[:lo].abs().max()) == 0.0 and float(holder.wbig.grad[lo + rows:].abs().max()) == 0.0
        _exact("_Conv1dFn", "row_slice_step%d" % step, "db", holder.b.grad, want["b"])
        opt.step()
        _restore(opt, p0)


def test_cross_attention_writes_both_row_ranges_of_the_packed_weight_once(dev):
    """(e) _PreLnCrossAttnFn: rows [0, H) of w_in from the queries, rows [H, 3H) from the keys and values, through autograd onto a sentinel
    pattern: .grad - sentinel is the model's gradient within the bar plus the rounding of the one addition -- a range written twice, or
    H rows off, is many bars away"""
    cs = CASES[M.KV_CASE]
    host = M.operands(cs)
    holder = Holder(dev, {k: host[k] for k in ("gamma", "beta", "w_in", "w_out")})
    sentinel = ((torch.arange(host["w_in"].numel(), dtype=torch.float32).reshape(host["w_in"].shape) % 7) - 3.0).to(dev)
    holder.w_in.grad = sentinel.clone()
    run_case(dev, cs, params=holder.params())
    ref = M.reference(cs)
    want, mirror = ref["grads"]["w_in"], ref["m_grads"]["w_in"]
    got = (holder.w_in.grad.double() - sentinel.double()).cpu()
    bar = torch.from_numpy(np.broadcast_to(np.asarray(M.bar(want, mirror)), tuple(want.shape)).copy()) + 2.0 * M.U * (want.abs() + 3.0)
    assert bool(((got - want).abs() <= bar).all())


# =====================================================================================================================================
# _DiffNetStackFn: the one case of the "swept elsewhere" table that lives here
# =====================================================================================================================================
def test_diffnet_stack_node_with_cond_detached(dev, monkeypatch):
    """_DiffNetStackFn (diffnet_stack_train) with cond detached, so needs_input_grad[2] is false: dcond comes back None, and dx, dd and every
    parameter gradient are bit for bit those of the run with cond attached.  L = 2 layers, B = 1, T = 32."""
    A, _ = _lib()
    from conftest import base_hparams
    from set_amd.diffnet import DiffNet
    monkeypatch.setenv("SET_AMD_WINO", "2")  # the kernel choice the training forward makes at its own sizes
    L_, B, T = 2, 1, 32
    torch.manual_seed(5)
    dn = DiffNet(80, base_hparams(residual_layers=L_)).to(dev)
    C, H = dn.C, dn.encoder_hidden
    g = torch.Generator().manual_seed(6)
    hx, cond, dmat, gsk = (torch.randn(*s, generator=g) for s in ((B, C, T), (B, H, T), (B, L_ * C), (B, C, T)))
    runs = []
    for attached in (True, False):
        for p in dn.parameters():
            p.grad = None
        x, c, dm = (t.clone().to(dev).requires_grad_(True) for t in (hx, cond, dmat))
        if not attached:
            c = c.detach()
        with torch.enable_grad():
            skip = A.diffnet_stack_train(dn, x, c, dm)
            skip.backward(gsk.to(dev))
        torch.cuda.synchronize()
        assert (c.grad is not None) == attached
        runs.append([skip.detach(), x.grad, dm.grad] + [p.grad.clone() for p in dn.stack_params()])
    assert float(runs[0][1].abs().max()) > 0 and float(runs[0][2].abs().max()) > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b)
