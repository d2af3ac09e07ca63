"""GPU test of multi-step training against the float64 oracle, update by update (models, bars and the case table: trajectory_models.py;
what each check catches: test_trajectory_reference.py).

Every other whole-model test of the training route either runs ONE backward on a freshly loaded model with `.grad = None` (the plain
autograd route: no FlatAdamW, no direct gradient sinks, no zero arena, no re-packed weight images) or compares two runs of the same code
bit for bit.  Here N = 5 real optimizer updates run per case on three distinct batches, and every update k is checked in isolation
against references that are fed the run's own state (teacher-forced: comparing parameters after N updates with a float64 trainer cannot
work, the first Adam updates being lr * sign(g)):

  3  losses and every parameter's gradient of update k against the oracle under float64 autograd at the run's own p_k (where a gradient
     bar is missed, once more with the ReLU units float32 cannot decide on the other branch: trajectory_models.references_of_update);
  4  p_{k+1}, m_{k+1}, v_{k+1} against the float64 clip + AdamW model fed p_k, the run's g_k, m_k, v_k; zero pad tails; the returned lr;
     the sum of squares the clip was taken on;
  5  a fresh task and optimizer loaded with p_k, m_k, v_k and the update count repeat update k bit for bit (run after the continuing
     trajectory has finished, so that nothing bumps the weights epoch or re-packs an image between its updates).

Between updates 2 and 3 three cases take a detour -- a validation pass (tape=False) and an inference -- compared with the oracle at p_3:
the only place where inference images, step tables and conditioner caches are checked after an optimizer update rather than a load.

The model is in .eval() as in the oracle gradient tests (the oracle has no dropout stream; test_gpu_philox.py and the stutter tests cover
dropout).  Out of scope: StutterSpeech (the oracle has no live restatement of its head and losses, only goldens at the seeded weights),
dropout-on trajectories, more than one rank.  The largest error / bar per case, update and check goes to
profiles/trajectory_gpu_accuracy.log when the module finishes; a ratio above 1 is a finding about the code, not a bar to widen."""
import os
import time

import pytest
import torch

import trajectory_models as TM
from conftest import base_hparams
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "trajectory_gpu_accuracy.log")
RESULTS = {}   # case -> list of lines
T0 = [None]


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _trajectory_log():
    T0[0] = time.time()
    yield
    if not RESULTS:
        return
    lines = ["teacher-forced training trajectory (tests/test_gpu_trajectory.py) on one MI355X",
             "N = %d updates per case, %d batches cycling, warm-up %d, clip %.1f; largest error / bar per update and check" %
             (TM.N_UPDATES, TM.N_BATCHES, TM.WARMUP, TM.CLIP),
             "check 3: losses and gradients vs the float64 oracle at the run's p_k; check 4: p, m, v vs the float64 update model fed the run's",
             "own g_k (bar: its float32 mirror); check 5: a fresh restart from p_k, m_k, v_k repeats the update bit for bit", ""]
    for c in TM.CASES:
        lines += RESULTS.get(c["name"], [])
    lines += ["", "module wall time %.1f s (N = %d kept: the budget is about two minutes)" % (time.time() - T0[0], TM.N_UPDATES)]
    text = "\n".join(lines) + "\n"
    print(text)
    try:
        with open(LOG, "w") as f:
            f.write(text)
    except OSError:
        pass  # a read-only checkout: the table is in the output above


def _hparams(kind):
    import yaml
    if kind == "spec":
        return base_hparams(timesteps=TM.fixture_meta("spec")["steps"])
    with open(os.path.join(ROOT, "speech-editing-toolkit_amd", "egs", "campnet.yaml")) as f:
        return yaml.safe_load(f)


def _new_task(kind, dev, seed):
    """a task with a random init of its own (the state is loaded by the caller), model on the device in eval mode"""
    from set_amd import tasks
    torch.manual_seed(seed)
    if kind == "spec":
        task = tasks.SpeechDenoiserTask(build_vocoder=False)
        task.build_model()
    else:
        task = tasks.CampNetTask(80, 100)
        task.build_tts_model()
    task.model.to(dev).eval()
    return task


def _new_optimizer(case, model):
    from set_amd.training import FlatAdamW
    return FlatAdamW(model, lr=case["lr0"], betas=TM.BETAS, eps=TM.EPS, weight_decay=TM.WD, clip_grad_norm=TM.CLIP, warmup_updates=TM.WARMUP)


def _count_sink_views(opt, counter):
    real = opt.sink

    def sink(param):
        view = real(param)
        counter[0] += view is not None
        return view
    opt.sink = sink  # (an instance attribute: the library is unchanged)


def _record_sumsq(opt, box):
    real = opt.step

    def step():
        lr, sumsq = real()
        box.append(None if sumsq is None else float(sumsq))
        return lr, sumsq
    opt.step = step


def _to(dev, d):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _run_update(case, task, opt, k, dev):
    """update k the way a trainer drives it -> (per-micro-batch losses as floats, lr)"""
    kind = case["kind"]
    bs = [TM.batch(kind, i) for i in TM.batches_of_update(case, k)]

    def kwargs(b):
        return dict(t=b["t"].to(dev), noises=b["eps"].to(dev)) if kind == "spec" else {}
    if case["acc"] == 1:
        _, parts, lr = task.training_step(_to(dev, TM.sample_of(kind, bs[0])), opt, **kwargs(bs[0]))
        losses = [{n: float(v) for n, v in parts.items()}]
    else:  # as test_gradient_accumulation_matches_one_big_step drives it: loss / acc per micro-batch into one step()
        opt.zero_grad(accumulate=True)
        losses = []
        try:
            for j, b in enumerate(bs):
                loss, log = task._training_step(_to(dev, TM.sample_of(kind, b)), case["acc"] * k + j, **kwargs(b))
                with torch.enable_grad():
                    (loss / case["acc"]).backward()
                losses.append({n: float(v) for n, v in log.items() if n != "batch_size"})
        except BaseException:
            opt.abort_step()
            raise
        lr, _ = opt.step()
    torch.cuda.synchronize()
    return losses, lr


def _cpu_state(model):
    return {n: v.detach().cpu().clone() for n, v in model.state_dict().items()}


def _cpu_opt_state(opt):
    sd = opt.state_dict()
    return {"state": {i: {n: v.detach().cpu().clone() for n, v in st.items()} for i, st in sd["state"].items()}, "param_groups": sd["param_groups"]}


def _np(t):
    return t.detach().cpu().numpy()


def _detour(case, task, W3, dev, notes, bad):
    """a validation pass and an inference at p_3, both against the oracle at p_3 (the fixture tests' bars)"""
    kind, dtype = case["kind"], case["dtype"]
    b = TM.batch(kind, 1)
    sample = _to(dev, TM.sample_of(kind, b))
    ref_l, _ = TM.oracle_step(kind, W3, b)
    kw = dict(t=b["t"].to(dev), noises=b["eps"].to(dev)) if kind == "spec" else {}
    losses, _ = task.run_model(sample, infer=False, tape=False, **kw)
    r = {"validation_loss": TM.check_losses(kind, dtype, ref_l, {n: float(v) for n, v in losses.items()})}
    kw = dict(noises=b["infer_noises"].to(dev)) if kind == "spec" else {}
    out = task.run_model(sample, infer=True, **kw)
    torch.cuda.synchronize()
    ref = TM.oracle_infer(kind, W3, b)
    if kind == "spec":
        got, want = out["mel_out"].cpu().double(), ref["mel_out"]
        assert bool(torch.isfinite(got).all())
        if dtype == "bf16":  # the bar of test_bf16_inference_loop_tolerance: mel-level MCD per utterance
            mcd = max(O.mel_mcd(got[i].float().numpy(), want[i].float().numpy()) for i in range(got.shape[0]))
            r["inference_mcd"] = mcd / TM.bf16_bars()["mcd"]
        else:
            r["inference_mel"] = float((got - want).abs().max()) / TM.INFER_MEL
    else:
        assert dtype == "f32"
        for n, bar in (("mel_out_coarse", TM.INFER_MEL), ("mel_out_fine", TM.INFER_MEL), ("attn", TM.INFER_ATTN)):
            r["inference_" + n] = float((out[n].cpu().double() - ref[n]).abs().max()) / bar
    notes.append("  detour at p_3   " + "  ".join("%s %.4f" % kv for kv in r.items()))
    bad += [("detour", n, v) for n, v in r.items() if not v <= 1.0]


@pytest.mark.parametrize("name", [c["name"] for c in TM.CASES])
def test_every_update_matches_the_oracle_the_update_model_and_a_fresh_restart(dev, monkeypatch, name):
    from set_amd import autograd_ops as A, hparams as H, ops
    case = TM.CASE[name]
    kind = case["kind"]
    for k_, v_ in case["env"].items():
        monkeypatch.setenv(k_, v_)
    saved = dict(H.hparams)
    notes, bad = ["%s  (%s, %s, env %s, %d micro-batch%s per update, lr0 %g)"
                  % (name, kind, case["dtype"], case["env"] or "{}", case["acc"], "" if case["acc"] == 1 else "es", case["lr0"])], []
    ops.set_compute_dtype(case["dtype"])
    try:
        H.hparams.clear()
        H.hparams.update(_hparams(kind))
        # ---- the route the case names --------------------------------------------------------------------------------------------------
        m = TM.fixture_meta(kind)
        grouped = [0]
        if name == "spec_fused_stack":
            assert ops.stack_variant(m["B"], m["T"], H.hparams["dilation_cycle_length"], have_split=False, x3_mode=0) == 2
            real_sp = A.step_projections

            def counted(dn, h):  # the grouped step projections (one launch for all layers: the flat optimizer lays them at one stride)
                out = real_sp(dn, h)
                grouped[0] += out is not None
                return out
            monkeypatch.setattr(A, "step_projections", counted)
        assert ops.compute_dtype() == case["dtype"]
        # ---- the continuing run ---------------------------------------------------------------------------------------------------------
        W0, names = TM.seeded_state(kind)
        task = _new_task(kind, dev, seed=1)
        missing, unexpected = task.model.load_state_dict(W0, strict=False)
        assert not unexpected
        opt = _new_optimizer(case, task.model)
        assert opt.param_names == names
        layout = TM.Layout.of_optimizer(opt)
        views = [0]
        _count_sink_views(opt, views)
        sumsqs = []
        _record_sumsq(opt, sumsqs)
        before, after, refs = [], [], []
        for k in range(TM.N_UPDATES):
            assert opt.num_updates == k
            snap = dict(W=_cpu_state(task.model), opt=_cpu_opt_state(opt), p=_np(opt.flat_p), m=_np(opt.m), v=_np(opt.v),
                        step=getattr(task, "global_step", 0))
            if case["detour"] and k == TM.DETOUR_AFTER + 1:
                _detour(case, task, snap["W"], dev, notes, bad)
            views[0] = 0
            losses, lr = _run_update(case, task, opt, k, dev)
            before.append(snap)
            after.append(dict(losses=losses, lr=lr, views=views[0], sumsq=sumsqs[k], g=opt.flat_g.clone(), p=opt.flat_p.clone(), m=opt.m.clone(), v=opt.v.clone()))
        if name == "spec_fused_stack":
            assert grouped[0] >= TM.N_UPDATES, "the grouped step projections were not taken"
        # ---- checks 3 and 4 on every update ------------------------------------------------------------------------------------------
        for k in range(TM.N_UPDATES):
            s, a = before[k], after[k]
            g = _np(a["g"])
            first = None
            for ref_l, ref_g, branch in TM.references_of_update(case, s["W"], k):  # (one reference unless a gradient bar is missed)
                c3, worst = TM.check_forward_backward(kind, case["dtype"], layout, ref_l, ref_g, a["losses"], g)
                first = first or (c3, worst)
                if all(v <= 1.0 for v in c3.values()):
                    if branch:
                        notes.append("  update %d  check 3 holds with the undecided ReLU unit(s) on the branch the GPU took: %s; the float64 "
                                     "branch gives %s" % (k, branch, "  ".join("%s %.4f" % kv for kv in first[0].items())))
                    break
            else:
                c3, worst = first
            c4 = TM.check_update(s["p"], g, s["m"], s["v"], k, case["lr0"], _np(a["p"]), _np(a["m"]), _np(a["v"]), layout.n, got_lr=a["lr"],
                                 got_sumsq=a["sumsq"])
            notes.append("  update %d  lr %-8g sink views %3d  check 3: %s (worst %s)  check 4: %s"
                         % (k, a["lr"], a["views"], "  ".join("%s %.4f" % kv for kv in c3.items()), worst, "  ".join("%s %.4f" % kv for kv in c4.items())))
            print(notes[-1])
            bad += [(k, 3, n, v) for n, v in c3.items() if not v <= 1.0] + [(k, 4, n, v) for n, v in c4.items() if not v <= 1.0]
            # the route: from the second update on the gradients take the direct sinks (never under accumulation, see the case table)
            if (a["views"] > 0) != (case["sinks"] and k >= 1):
                bad.append((k, "route", "sink views", a["views"]))
        # ---- check 5: a fresh restart of every update --------------------------------------------------------------------------------
        same = []
        for k in range(TM.N_UPDATES):
            s, a = before[k], after[k]
            task2 = _new_task(kind, dev, seed=100 + k)  # another random init
            task2.model.load_state_dict(s["W"])
            task2.global_step = s["step"]
            opt2 = _new_optimizer(case, task2.model)
            opt2.load_state_dict(s["opt"])
            assert opt2.num_updates == k
            losses, lr = _run_update(case, task2, opt2, k, dev)
            eq = dict(losses=losses == a["losses"], lr=lr == a["lr"], g=torch.equal(opt2.flat_g, a["g"]), p=torch.equal(opt2.flat_p, a["p"]),
                      m=torch.equal(opt2.m, a["m"]), v=torch.equal(opt2.v, a["v"]))
            same.append(all(eq.values()))
            if not same[-1]:
                bad.append((k, 5, {n: v for n, v in eq.items() if not v},
                            float((opt2.flat_g - a["g"]).abs().max()), float((opt2.flat_p - a["p"]).abs().max())))
            del task2, opt2
        notes.append("  check 5: fresh restart bit-identical at updates %s" % [k for k in range(TM.N_UPDATES) if same[k]])
        print(notes[-1])
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):  # a faulted device: run nothing more on it in this session
            pytest.exit("GPU error in %s: %s" % (name, str(e)[:300]), returncode=3)
        raise
    finally:
        ops.set_compute_dtype("f32")
        H.hparams.clear()
        H.hparams.update(saved)
        RESULTS[name] = notes
    assert not bad, bad
