"""The leaf stream's operand, writer and join rules, audited call by call on the real training tape (tests/stream_audit.py), at the
tiny shapes of the training tests.  Every case is three updates: the learning step that goes through autograd, then two with direct
gradient sinks -- the ones that use the leaf stream.  The audit is deterministic: it reads the order of the library calls and their
pointer arguments, no race has to happen for a broken rule to show.  What the proxy cannot see (ATen kernels) is covered by the starved
runs at the end: the leaf stream is held back until the compute stream has finished the whole backward pass, and the result must still
be bit-identical to the single-stream run.  Figures: profiles/stream_audit.log."""
import json

import pytest
import torch

import stream_audit as S
from conftest import base_hparams, load_golden
from oracle import weights as Wt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _report(case, **figures):
    print("STREAM_AUDIT %s %s" % (case, json.dumps(figures, sort_keys=True)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases: (task, optimizer, step(it) -> (sample, kwargs))
# ---------------------------------------------------------------------------------------------------------------------------------
def _spec(dev):
    from test_gpu_training import _train_setup
    from set_amd.training import FlatAdamW
    task, _ = _train_setup(dev, 8, 31)
    task.model.train()
    opt = FlatAdamW(task.model, lr=1e-3, warmup_updates=4, clip_grad_norm=1.0)

    def batch(it):
        inp = Wt.synthetic_inputs(4, 96, 24, seed=77 + it, pad_tail=True)
        sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                      time_mel_masks=inp["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=inp["spk_embed"])
        t = torch.tensor([(1 + it) % 9, 3, (5 + 2 * it) % 9, 7], device=dev)
        return {k: v.to(dev) for k, v in sample.items()}, dict(t=t, seed=500 + 13 * it)

    return task, opt, batch


def _stutter(dev):
    from set_amd import hparams as H
    from set_amd import tasks
    from set_amd.training import FlatAdamW
    g = load_golden("train_losses_stutter")
    m = g["meta"]
    H.hparams.clear()  # test_gpu_stutter._stutter_task cut to 3 layers, as in its _task_hparams
    H.hparams.update(base_hparams(timesteps=m["steps"], residual_layers=3, residual_channels=256, dilation_cycle_length=1, sil_token_ids=[1, 2, 3]))
    task = tasks.StutterSpeechTask(build_vocoder=False)
    task.build_model()
    task.model.load_state_dict(Wt.seeded_weights(Wt.load_manifest("stutter_speech"), m["wseed"]), strict=False)
    task.model.to(dev).train()
    opt = FlatAdamW(task.model, lr=1e-3, warmup_updates=4, clip_grad_norm=1.0)
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=inp["spk_embed"],
                  stutter_mel_masks=torch.from_numpy(g["raw_masks"]))
    sample = {k: v.to(dev) for k, v in sample.items()}
    t = torch.from_numpy(g["t"]).to(dev)
    return task, opt, lambda it: (sample, dict(t=t, seed=40 + it))


def _camp(dev):
    from test_gpu_campnet import _campnet
    from set_amd.training import FlatAdamW
    task, model, sample = _campnet(dev, load_golden("campnet_tiny"))  # B = 2, T = 48: the smallest of its fixtures
    opt = FlatAdamW(model, lr=2e-3, warmup_updates=1)
    return task, opt, lambda it: (sample, {})


CASES = {  # name -> (builder, environment, compute dtype)
    "spec_f32_stack": (_spec, {"SET_AMD_WINO": "2"}, "f32"),          # (tiny batch: the kernel choice the big batches get)
    "spec_f32_per_op": (_spec, {"SET_AMD_TRAIN_STACK": "0"}, "f32"),
    "spec_bf16_grouped": (_spec, {}, "bf16"),
    "stutter": (_stutter, {}, "f32"),
    "campnet_fused": (_camp, {}, "f32"),
    "campnet_per_op": (_camp, {"SET_AMD_FUSED_NODES": "0"}, "f32"),
}
assert tuple(CASES) == S.CASE_NAMES

# what runs on the leaf stream in each case: coverage cannot shrink (or grow) silently
WGRAD, WGRAD_DET, WGRAD_GROUPED = "set_conv1d_wgrad", "set_conv1d_wgrad_det", "set_conv1d_wgrad_det_grouped"
CSUM, SCATTER, STEP_DW, STUTTER = "set_channel_sum_det", "set_scatter_rows_det", "set_step_proj_bwd_dw", "set_stutter_head_bwd_reduce"
LEAF_ENTRY_POINTS = {
    "spec_f32_stack": {WGRAD, WGRAD_DET, CSUM, SCATTER, STEP_DW},
    "spec_f32_per_op": {WGRAD, WGRAD_DET, CSUM, SCATTER},
    "spec_bf16_grouped": {WGRAD, WGRAD_DET, WGRAD_GROUPED, CSUM, SCATTER, STEP_DW},
    "stutter": {WGRAD, WGRAD_DET, CSUM, SCATTER, STUTTER},            # (three layers at T = 64: the layers run op by op)
    "campnet_fused": {WGRAD, WGRAD_DET, CSUM, SCATTER},
    "campnet_per_op": {WGRAD, WGRAD_DET, CSUM, SCATTER},
}


def _long_lived(opt):
    """The buffers a leaf kernel may read without holding them, one by one: the flat optimizer's, which live as long as the optimizer.
    (The leaf stream's own scratch-pool buffers are the other members; the checker takes them from the pool snapshots of each block.)"""
    return [(t.data_ptr(), t.numel() * t.element_size(), why) for t, why in (
        (opt.flat_p, "flat parameters: owned by the optimizer"), (opt.flat_g, "flat gradients: owned by the optimizer"),
        (opt.m, "first Adam moment"), (opt.v, "second Adam moment"))]


def _audit(rec, opt):
    return S.check(rec.events, _long_lived(opt), (opt.flat_g.data_ptr(), opt.flat_g.numel() * 4))


def _setup(name, dev, monkeypatch):
    from set_amd import ops
    builder, env, dtype = CASES[name]
    monkeypatch.setenv("SET_AMD_LEAF_STREAM", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops.set_compute_dtype(dtype)
    return builder(dev)


@pytest.fixture
def f32_after():
    from set_amd import leaf_stream, ops
    yield
    ops.set_compute_dtype("f32")
    for st in leaf_stream._STREAMS.values():
        st.ledger.mark_bytes, st.ledger.cap_bytes = 128 << 20, 8192 << 20


def _manual_step(task, opt, sample, kw, backwards=1):
    """zero_grad -> forward -> backward (x backwards) with the optimizer step left to the caller."""
    from set_amd import autograd_ops as A
    opt.zero_grad(accumulate=backwards > 1)
    for _ in range(backwards):
        losses, _out = task.run_model(sample, infer=False, **kw)
        with torch.enable_grad():
            total = A.sum_losses(task.loss_terms(losses))
        total.backward()
    return total.detach()


# ---------------------------------------------------------------------------------------------------------------------------------
# audited steps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_three_updates_obey_every_rule(dev, name, monkeypatch, f32_after):
    task, opt, batch = _setup(name, dev, monkeypatch)
    rec = S.Recorder().install(monkeypatch)
    for it in range(3):
        sample, kw = batch(it)
        task.training_step(sample, opt, **kw)
    torch.cuda.synchronize()
    bad = _audit(rec, opt)
    st = S.stats(rec.events)
    _report(name, **st, sites=sorted(rec.sites_reached), violations=[tuple(v) for v in bad[:10]])
    assert bad == [], bad[:10]
    assert st["blocks"] > 0 and set(st["leaf_entry_points"]) == LEAF_ENTRY_POINTS[name], st["leaf_entry_points"]
    mine = {s for s, case in S.SITE_CASES.items() if case == name}
    assert mine <= set(rec.sites_reached), sorted(mine - set(rec.sites_reached))
    # the first update teaches the optimizer which parameters take one gradient: no block before the second
    first_block = next(i for i, e in enumerate(rec.events) if e["k"] == "enter" and e.get("on"))
    assert sum(1 for e in rec.events[:first_block] if e["k"] == "call" and e["name"] == "set_adamw") == 1


def test_bf16_per_layer_form_keeps_its_weight_gradients_on_the_compute_stream(dev, monkeypatch, f32_after):
    """autograd_ops._bf16_wgrad: the next layer's launch overwrites dy16 / do16, so the per-layer form (mixed dilations, or dy / d_o of
    all layers over SET_AMD_GROUPED_WGRAD_MB) must NOT move its GEMMs to the leaf stream; the audit (R4) would flag it if it did."""
    monkeypatch.setenv("SET_AMD_GROUPED_WGRAD_MB", "0")
    task, opt, batch = _setup("spec_bf16_grouped", dev, monkeypatch)
    rec = S.Recorder().install(monkeypatch)
    for it in range(2):
        sample, kw = batch(it)
        task.training_step(sample, opt, **kw)
    torch.cuda.synchronize()
    assert _audit(rec, opt) == []
    leaf = S.stats(rec.events)
    assert leaf["blocks"] > 0 and WGRAD_GROUPED not in leaf["leaf_entry_points"]
    assert "_bf16_stack_bwd_grouped#0:_leaves" not in rec.sites_reached
    leaf_raw = next(e["leaf_stream"] for e in rec.events if e["k"] == "enter" and e.get("on"))
    bwd = [i for i, e in enumerate(rec.events) if e["k"] == "call" and e["name"] == "set_diffnet_layer_bwd_bf16"]
    assert bwd
    # between two layer launches of one sweep lie that layer's reduce and its three weight-gradient GEMMs: on the compute stream
    n_gemm = 0
    for a, b in zip(bwd, bwd[1:]):
        part = rec.events[a:b]
        if any(e["k"] == "backward_begin" for e in part):
            continue  # (the last launch of one pass and the first of the next)
        gemms = [e for e in part if e["k"] == "call" and e["name"] == WGRAD_DET]
        assert len(gemms) == 3 and all(e["stream"] != leaf_raw and not e["leaf"] for e in gemms)
        assert not any(e["k"] == "enter" and e.get("on") for e in part)
        n_gemm += len(gemms)
    assert n_gemm > 0


def test_budget_paths_release_by_marker_and_join_early_under_audit(dev, monkeypatch, f32_after):
    """mark_bytes = 1: a marker after every block.  Update 2 runs with the leaf stream held back by a short sleep and a cap of one byte:
    no marker can complete, every later block finds the ledger over its cap and joins early.  Update 3 runs with the default cap: the
    markers of the first blocks have completed by the time later blocks poll them.  Both paths obey R5 (and every other rule)."""
    from set_amd import leaf_stream
    task, opt, batch = _setup("spec_f32_stack", dev, monkeypatch)
    idx = torch.cuda.current_device()
    st = leaf_stream._STREAMS.get(idx)
    if st is None:
        st = leaf_stream._STREAMS[idx] = leaf_stream.LeafStream(idx)
    rec = S.Recorder().install(monkeypatch)
    cyc = _cycles_per_ms()
    sample, kw = batch(0)
    task.training_step(sample, opt, **kw)
    st.ledger.mark_bytes, st.ledger.cap_bytes = 1, 1
    starver = _Starver(monkeypatch, lambda: int(20 * cyc))
    lo = len(rec.events)
    sample, kw = batch(1)
    task.training_step(sample, opt, **kw)
    early = S.stats(rec.events[lo:])
    st.ledger.cap_bytes = 8192 << 20
    starver.delay = None
    lo = len(rec.events)
    sample, kw = batch(2)
    task.training_step(sample, opt, **kw)
    torch.cuda.synchronize()
    late = S.stats(rec.events[lo:])
    bad = _audit(rec, opt)
    _report("budget_paths", early_joins=early["early_joins"], marker_releases=late["marker_releases"], blocks=late["blocks"],
            peak_held_bytes=max(early["peak_held_bytes"], late["peak_held_bytes"]), violations=[tuple(v) for v in bad[:10]])
    assert bad == [], bad[:10]
    assert early["early_joins"] > 0 and late["marker_releases"] > 0
    assert any(e["k"] == "call" and e["name"] == "set_stream_mark_done" and e["ret"] == 1 for e in rec.events)


def test_second_backward_of_a_step_is_joined_like_the_first(dev, monkeypatch, f32_after):
    task, opt, batch = _setup("spec_f32_per_op", dev, monkeypatch)
    rec = S.Recorder().install(monkeypatch)
    sample, kw = batch(0)
    task.training_step(sample, opt, **kw)
    lo = len(rec.events)
    _manual_step(task, opt, sample, kw, backwards=2)
    opt.step()
    torch.cuda.synchronize()
    assert _audit(rec, opt) == []
    ev = rec.events[lo:]
    ends = [i for i, e in enumerate(ev) if e["k"] == "backward_end"]
    assert len(ends) == 2 and all(ev[i]["ok"] for i in ends)
    lo_i = 0
    for i in ends:  # each pass launched leaf work and ended with its own join + release
        part = ev[lo_i:i]
        assert any(e["k"] == "enter" and e.get("on") for e in part)
        assert [e["k"] for e in part if e["k"] in ("ls_join", "release_all")][-2:] == ["ls_join", "release_all"]
        lo_i = i


class _Boom(RuntimeError):
    pass


def _arm_raise_after_first_block(monkeypatch, rec):
    """autograd_ops._tape_tgt raises once, in the first backward node that asks for a gradient target after a leaf block has run."""
    from set_amd import autograd_ops as A
    orig, state = A._tape_tgt, {"armed": True, "from": len(rec.events)}

    def tape_tgt(*a, **kw):
        if state["armed"] and any(e["k"] == "exit" and not e.get("off") for e in rec.events[state["from"]:]):
            state["armed"] = False
            raise _Boom("planted")
        return orig(*a, **kw)

    monkeypatch.setattr(A, "_tape_tgt", tape_tgt)
    return state


@pytest.mark.parametrize("recovery", ["abort_step", "zero_grad", "next_backward"])
def test_backward_that_raises_is_followed_by_a_joined_backward(dev, recovery, monkeypatch, f32_after):
    """A node after the first leaf block throws: the engine drops the pass's callbacks, so the pass ends without its join and the leaf
    stream stays marked dirty.  What the caller does next:
      abort_step     abort_step() joins (tasks._optimisation_step, trainer.py), then a normal step;
      zero_grad      straight to the next zero_grad(): it joins before it clears the flat gradient buffer -- it used not to, and the
                     failed pass's gradient kernels could still add into the buffer after the fill;
      next_backward  the failed micro-batch is skipped and the next backward() runs in the same step: leaf_work used to queue the
                     end-of-pass join only when the stream was clean, so the stale flag skipped the join of THIS pass and backward()
                     returned with gradient kernels still queued; the join is now queued once per graph task.
    In all three the next pass ends with a join; in the first two it leaves the single-stream replica's gradients, bit for bit."""
    from set_amd import leaf_stream
    task, opt, batch = _setup("spec_f32_per_op", dev, monkeypatch)
    task_b, opt_b, _ = _setup("spec_f32_per_op", dev, monkeypatch)
    rec = S.Recorder().install(monkeypatch)
    sample, kw = batch(0)
    task.training_step(sample, opt, **kw)
    monkeypatch.setenv("SET_AMD_LEAF_STREAM", "0")
    task_b.training_step(sample, opt_b, **kw)
    monkeypatch.setenv("SET_AMD_LEAF_STREAM", "1")
    assert torch.equal(opt.flat_p, opt_b.flat_p)
    sample, kw = batch(1)
    state = _arm_raise_after_first_block(monkeypatch, rec)
    with pytest.raises(_Boom):
        _manual_step(task, opt, sample, kw)
    assert not state["armed"]
    assert any(st.dirty for st in leaf_stream._STREAMS.values())  # the pass never reached its join
    lo = len(rec.events)
    if recovery == "next_backward":
        from set_amd import autograd_ops as A
        losses, _out = task.run_model(sample, infer=False, **kw)
        with torch.enable_grad():
            total = A.sum_losses(task.loss_terms(losses))
        total.backward()
    else:
        if recovery == "abort_step":
            opt.abort_step()
            assert not any(st.dirty for st in leaf_stream._STREAMS.values())
        total = _manual_step(task, opt, sample, kw)
    ev = rec.events[lo:]
    end = next(i for i, e in enumerate(ev) if e["k"] == "backward_end")
    assert ev[end]["ok"] and any(e["k"] == "enter" and e.get("on") for e in ev[:end])
    assert [e["k"] for e in ev[:end] if e["k"] in ("ls_join", "release_all")][-2:] == ["ls_join", "release_all"]
    assert not any(st.dirty for st in leaf_stream._STREAMS.values())
    if recovery == "next_backward":
        opt.abort_step()  # (the failed pass left half a gradient behind: nothing to compare)
    else:
        monkeypatch.setenv("SET_AMD_LEAF_STREAM", "0")
        total_b = _manual_step(task_b, opt_b, sample, kw)
        torch.cuda.synchronize()
        assert torch.equal(total, total_b) and torch.equal(opt.flat_g, opt_b.flat_g)
        opt.step(), opt_b.step()
        torch.cuda.synchronize()
        assert torch.equal(opt.flat_p, opt_b.flat_p) and torch.equal(opt.m, opt_b.m) and torch.equal(opt.v, opt_b.v)
    torch.cuda.synchronize()
    assert _audit(rec, opt) == []


# ---------------------------------------------------------------------------------------------------------------------------------
# plants: the audit flags each of them on the real tape, deterministically (no kernel reads freed memory: the test keeps the tensors)
# ---------------------------------------------------------------------------------------------------------------------------------
def _plant_drop_operand(monkeypatch, kept):
    from set_amd import autograd_ops as A
    orig = A._leaves

    def leaves(dev, rets, *operands):
        kept.append(operands[0])
        return orig(dev, rets, *operands[1:])

    monkeypatch.setattr(A, "_leaves", leaves)


def _plant_allocation(monkeypatch, kept):
    from set_amd import autograd_ops as A
    orig = A._leaves

    class Allocating:
        def __init__(self, inner, dev):
            self.inner, self.dev = inner, dev

        def __enter__(self):
            on = self.inner.__enter__()
            kept.append(torch.empty(4096, dtype=torch.float32, device=self.dev))
            return on

        def __exit__(self, *exc):
            return self.inner.__exit__(*exc)

    monkeypatch.setattr(A, "_leaves", lambda dev, rets, *operands: Allocating(orig(dev, rets, *operands), dev))


def _plant_temporary_target(monkeypatch, kept):
    from set_amd import autograd_ops as A
    orig = A._tape_tgt

    def tape_tgt(param, dev, cw=None):
        tgt, ret = orig(param, dev, cw)
        if ret is None:  # the optimizer's .grad view: hand the kernel a zeroed temporary instead, and still claim "written in place"
            tgt = torch.zeros_like(tgt)
            kept.append(tgt)
        return tgt, ret

    monkeypatch.setattr(A, "_tape_tgt", tape_tgt)


@pytest.mark.parametrize("plant,rule", [(_plant_drop_operand, "R1"), (_plant_allocation, "R2"), (_plant_temporary_target, "R3")])
def test_planted_faults_are_flagged_on_the_real_tape(dev, plant, rule, monkeypatch, f32_after):
    task, opt, batch = _setup("spec_f32_per_op", dev, monkeypatch)
    rec = S.Recorder().install(monkeypatch)
    sample, kw = batch(0)
    task.training_step(sample, opt, **kw)
    assert _audit(rec, opt) == []
    kept = []
    plant(monkeypatch, kept)
    sample, kw = batch(1)
    task.training_step(sample, opt, **kw)
    torch.cuda.synchronize()
    bad = _audit(rec, opt)
    blocks = S.stats(rec.events)["blocks"]
    _report("plant_" + rule, blocks=blocks, flagged=len(bad), rules=sorted({v.rule for v in bad}))
    assert kept and bad and {v.rule for v in bad} == {rule}, bad[:10]
    flagged = {v.index for v in bad}
    if rule == "R2":    # every block allocated
        assert len(flagged) == blocks
    elif rule == "R3":  # every block has at least one call with a planted target
        assert len(flagged) >= blocks
    assert all(rec.events[i]["k"] == ("exit" if rule == "R2" else "call") for i in flagged)


# ---------------------------------------------------------------------------------------------------------------------------------
# starved leaf stream
# ---------------------------------------------------------------------------------------------------------------------------------
_CYCLES = []


def _cycles_per_ms():
    """Device cycles torch.cuda._sleep spins per millisecond, measured once."""
    if not _CYCLES:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)  # (first call: module load)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(2_000_000)
        b.record()
        b.synchronize()
        _CYCLES.append(2_000_000 / a.elapsed_time(b))
    return _CYCLES[0]


class _Starver:
    """Before the first fork of each backward pass: a bounded spin on the leaf stream (torch.cuda._sleep), an event behind it, and at each
    join an event on the compute stream just before it and one on the leaf stream behind the last leaf kernel."""

    def __init__(self, monkeypatch, delay_cycles):
        from set_amd import leaf_stream
        self.delay = delay_cycles  # () -> cycles; None: off
        self.passes = []  # per backward pass: [after the sleep (leaf), before the join (compute), after the last leaf kernel (leaf)]
        fork0, join0, me = leaf_stream.LeafStream.fork, leaf_stream.LeafStream.join, self
        self.task = -1

        def fork(st):
            task = torch._C._current_graph_task_id()
            if me.delay is not None and task != -1 and task != me.task:
                me.task = task
                with torch.cuda.stream(st.stream):
                    torch.cuda._sleep(me.delay())
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record()
                me.passes.append([ev, None, None])
            return fork0(st)

        def join(st):
            if me.delay is not None and me.passes and me.passes[-1][1] is None:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()  # (the current stream: everything the compute stream did in this pass lies before it)
                with torch.cuda.stream(st.stream):
                    b.record()
                me.passes[-1][1:] = [a, b]
            return join0(st)

        monkeypatch.setattr(leaf_stream.LeafStream, "fork", fork)
        monkeypatch.setattr(leaf_stream.LeafStream, "join", join)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_starved_leaf_stream_still_equals_the_single_stream_run(dev, dtype, monkeypatch, f32_after):
    """What the proxy cannot see: ATen kernels (and the autograd engine's own accumulations) that might reuse or overwrite what a leaf
    kernel still reads.  Here EVERY leaf kernel of a pass runs after the compute stream has finished the whole pass: a spin of three times
    the measured backward time (the single-stream replica's, same step and shape; the factor covers the clock spread of a shared
    machine) is enqueued on the leaf stream before its first fork.  The schedule is proven in every step, not assumed: the event behind
    the spin completes later than the event recorded on the compute stream just before the join, and so does the event behind the last
    leaf kernel.  No use-after-free is staged; the power of the test is that ordering: whatever the compute stream could do to a leaf
    operand during the pass, it has done before the first leaf kernel reads it -- and losses, parameters and both Adam moments are still
    bit-identical to the single-stream replica's after each of three updates."""
    from set_amd import leaf_stream, ops
    ops.set_compute_dtype(dtype)
    leaf_stream.leaf_stats(reset=True)
    env = {"SET_AMD_WINO": "2"} if dtype == "f32" else {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (ta, oa, batch), (tb, ob, _) = _spec(dev), _spec(dev)
    assert torch.equal(oa.flat_p, ob.flat_p)
    cyc = _cycles_per_ms()
    measured = [0.0]
    starver = _Starver(monkeypatch, lambda: int(3.0 * measured[0] * cyc))
    rows = []
    for it in range(3):
        sample, kw = batch(it)
        # the single-stream replica first: its backward pass, timed with events
        monkeypatch.setenv("SET_AMD_LEAF_STREAM", "0")
        from set_amd import autograd_ops as A
        ob.zero_grad()
        losses_b, _ = tb.run_model(sample, infer=False, **kw)
        with torch.enable_grad():
            tot_b = A.sum_losses(tb.loss_terms(losses_b))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tot_b.backward()
        e1.record()
        ob.step()
        e1.synchronize()
        measured[0] = e0.elapsed_time(e1)
        delay_ms = 3.0 * measured[0]
        assert 0.0 < delay_ms < 400.0, delay_ms  # a bounded wait of tens of milliseconds
        # the starved replica
        monkeypatch.setenv("SET_AMD_LEAF_STREAM", "1")
        n_pass = len(starver.passes)
        tot_a, parts_a, _ = ta.training_step(sample, oa, **kw)
        torch.cuda.synchronize()
        assert torch.equal(tot_a, tot_b.detach()), it
        assert all(torch.equal(parts_a[k], losses_b[k].detach()) for k in parts_a), it
        assert torch.equal(oa.flat_p, ob.flat_p) and torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), it
        if it == 0:
            assert len(starver.passes) == n_pass  # the learning step goes through autograd: no leaf work to starve
            rows.append(dict(step=it, backward_ms=round(measured[0], 3)))
            continue
        assert len(starver.passes) == n_pass + 1, "one starved pass per update"
        slept, before_join, last_leaf = starver.passes[-1]
        assert before_join is not None, "the pass ended without a join"
        margin_first, margin_last = before_join.elapsed_time(slept), before_join.elapsed_time(last_leaf)
        rows.append(dict(step=it, backward_ms=round(measured[0], 3), delay_ms=round(delay_ms, 3),
                         first_leaf_after_compute_ms=round(margin_first, 3), last_leaf_after_compute_ms=round(margin_last, 3)))
        # every leaf kernel of the pass started after the compute stream had finished the pass
        assert margin_first > 0.0 and margin_last >= margin_first, rows[-1]
    st = leaf_stream.leaf_stats()
    _report("starved_" + dtype, steps=rows, early_joins=st["early_joins"])
    assert st["early_joins"] == 0  # (an early join would make the compute stream wait for the spin in mid-pass)
    assert sum(1 for r in rows if "delay_ms" in r) == 2
