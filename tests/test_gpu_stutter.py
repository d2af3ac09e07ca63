"""StutterSpeech on the MI355X: the fused head + loss kernel against a float64 torch composition, dropout inside the fused pre-LN FFN node
against the per-op tape, training / inference parity with the reference's own model and losses (tools/make_stutter_golden.py), and
the task end to end on a binarised set with stutter masks."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, base_hparams, load_golden
from oracle import weights as Wt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_globals():
    """The tests below set the global hparams and may switch the compute dtype: leave both as they were found."""
    from set_amd import hparams as H, ops
    saved, dtype = dict(H.hparams), ops.compute_dtype()
    yield
    H.hparams.clear()
    H.hparams.update(saved)
    ops.set_compute_dtype(dtype)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
# head + loss kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_head(h, w, b, lab, g_ce, g_fo):
    """float64: logits = Linear(C, 3) per frame; CrossEntropyLoss(ignore_index=2); MultiFocalLoss with log p = z - logsumexp(z).
    Gradients are enabled here: other test modules switch autograd off globally when they are imported."""
    h, w, b = (t.double().cpu().requires_grad_(True) for t in (h, w, b))
    lab = lab.cpu()
    with torch.enable_grad():
        z = torch.einsum("bct,jc->btj", h, w) + b
        lp = z - torch.logsumexp(z, -1, keepdim=True)
        lpy = lp.gather(-1, lab[..., None])[..., 0]
        valid = lab != 2
        ce = -(lpy * valid).sum() / valid.sum()
        alpha = torch.tensor([5e-3, 1.0, 0.0], dtype=torch.float64)[lab]
        focal = (-alpha * (1 - (lpy.exp() + 1e-6)) ** 3 * (lpy + 1e-6)).mean()
        (g_ce * ce + g_fo * focal).backward()
    return z.detach(), ce.detach(), focal.detach(), h.grad, w.grad, b.grad


@pytest.mark.parametrize("C", [192, 80])
@pytest.mark.parametrize("T", [64, 77, 800])
def test_head_loss_kernel_matches_torch(dev, C, T):
    from set_amd import autograd_ops as A, ops
    g = torch.Generator().manual_seed(C * 1000 + T)
    B = 3
    h = torch.randn(B, C, T, generator=g)
    lengths = [T, T - T // 5, T // 2]
    lab = (torch.rand(B, T, generator=g) < 0.3).long()
    for i, n in enumerate(lengths):
        h[i, :, n:] = 0
        lab[i, n:] = 2
    w = torch.randn(3, C, generator=g) / C ** 0.5
    b = 0.1 * torch.randn(3, generator=g)
    g_ce, g_fo = 0.37, 1.9
    z_r, ce_r, fo_r, dh_r, dw_r, db_r = _torch_head(h, w, b, lab, g_ce, g_fo)

    def run():
        hd = h.to(dev).requires_grad_(True)
        wd = w.to(dev).requires_grad_(True)
        bd = b.to(dev).requires_grad_(True)
        with torch.enable_grad():
            logits, ce, fo = A.stutter_losses(hd, wd, bd, lab.to(dev))
            (g_ce * ce + g_fo * fo).backward()
        torch.cuda.synchronize()
        return logits, ce, fo, hd.grad, wd.grad, bd.grad

    r1, r2 = run(), run()
    for a, c in zip(r1, r2):  # deterministic: no atomics anywhere
        assert torch.equal(a, c)
    logits, ce, fo, dh, dw, db = r1
    assert logits.shape == (B, T, 3)
    assert _rel(logits, z_r) < 1e-6
    assert abs(float(ce.detach()) - float(ce_r)) <= 1e-6 * abs(float(ce_r))
    assert abs(float(fo.detach()) - float(fo_r)) <= 1e-6 * abs(float(fo_r))
    assert _rel(dh, dh_r) < 1e-5 and _rel(dw, dw_r) < 1e-5 and _rel(db, db_r) < 1e-5
    assert torch.equal(ops.stutter_head(h.to(dev), w.to(dev), b.to(dev)), logits)  # the inference form: same logits


# ---------------------------------------------------------------------------------------------------------------------------------
# dropout inside the fused pre-LN FFN node
# ---------------------------------------------------------------------------------------------------------------------------------
def _ffn_case(dev, C=192, B=2, T=77, k=5):
    from set_amd.fs import ResidualBlock
    torch.manual_seed(3)
    rb = ResidualBlock(C, k, 1, n=1, dropout=0.3).to(dev)
    for p in rb.parameters():
        p.data.normal_(0, 0.1)
    x = torch.randn(B, C, T, device=dev)
    x[1, :, 60:] = 0
    mask = (x.abs().sum(1) > 0).float()
    return rb, x, mask


def _ffn_run(rb, x, mask, drop, fused, monkeypatch):
    from set_amd import autograd_ops as A
    monkeypatch.setenv("SET_AMD_FUSED_NODES", "1" if fused else "0")
    b = rb.blocks[0]
    w1, w2 = rb._cw[0]
    for p in rb.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(True)
    with torch.enable_grad():
        y = A.preln_ffn(xi, (b[0].weight, b[0].bias), w1, b[1].bias, w2, b[4].bias, dil=1, pad=2, alpha=5 ** -0.5, act="gelu",
                        mask=mask, eps=1e-5, drop=drop)
        dy = torch.randn(y.shape, generator=torch.Generator(device=y.device).manual_seed(9), device=y.device)
        y.backward(dy)
    torch.cuda.synchronize()
    return [y.detach(), xi.grad] + [p.grad.clone() for p in rb.parameters()]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ffn_dropout_fused_equals_per_op_tape(dev, monkeypatch, dtype):
    from set_amd import ops
    rb, x, mask = _ffn_case(dev)
    prev = ops.compute_dtype()
    ops.set_compute_dtype(dtype)
    try:
        drop = (0.3, 1234, 49 << 28)
        fused = _ffn_run(rb, x, mask, drop, True, monkeypatch)
        per_op = _ffn_run(rb, x, mask, drop, False, monkeypatch)
        for a, c in zip(fused, per_op):
            assert torch.equal(a, c)
        # the keep-mask is set_dropout's: about p of the branch is dropped, and a different seed draws another mask
        plain = _ffn_run(rb, x, mask, None, True, monkeypatch)
        other = _ffn_run(rb, x, mask, (0.3, 1235, 49 << 28), True, monkeypatch)
        assert not torch.equal(fused[0], plain[0]) and not torch.equal(fused[0], other[0])
        # p = 0 keeps every element: the unfused epilogue gives the conv epilogue's bits
        zero = _ffn_run(rb, x, mask, (0.0, 1234, 0), True, monkeypatch)
        for a, c in zip(zero, plain):
            assert torch.equal(a, c)
        plain_op = _ffn_run(rb, x, mask, None, False, monkeypatch)
        for a, c in zip(plain, plain_op):
            assert torch.equal(a, c)
    finally:
        ops.set_compute_dtype(prev)


def test_ffn_dropout_keep_mask_is_set_dropouts(dev):
    from set_amd import ops
    x = torch.randn(2, 16, 37, device=dev)
    z = torch.randn_like(x)
    y = ops.residual_dropout(x, z, None, 0.3, 77, 5 << 28)
    d = torch.empty_like(z)
    ops._lib.lib().set_dropout(ops._p(z), ops._p(d), z.numel(), 0.3, 77, 5 << 28, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(y, x + d)
    frac = float((d == 0).float().mean())
    assert 0.2 < frac < 0.4


# ---------------------------------------------------------------------------------------------------------------------------------
# training / inference parity with the reference model
# ---------------------------------------------------------------------------------------------------------------------------------
def _stutter_task(dev, steps, wseed):
    from set_amd import hparams as H
    from set_amd import tasks
    H.hparams.clear()
    H.hparams.update(base_hparams(timesteps=steps, residual_layers=20, residual_channels=256, dilation_cycle_length=1,
                                  sil_token_ids=[1, 2, 3]))
    task = tasks.StutterSpeechTask(build_vocoder=False)
    task.build_model()
    W = Wt.seeded_weights(Wt.load_manifest("stutter_speech"), wseed)
    task.model.load_state_dict(W, strict=False)
    task.model.to(dev).eval()  # eval: no dropout, as in the fixtures
    return task


@pytest.mark.parametrize("fixture", ["train_losses_stutter", "train_losses_stutter_ragged"])
@pytest.mark.parametrize("stack", ["per_op", "default"])
def test_training_losses_and_gradients_match_reference(dev, monkeypatch, stack, fixture):
    if stack == "per_op":
        monkeypatch.setenv("SET_AMD_TRAIN_STACK", "0")
    g = load_golden(fixture)
    m = g["meta"]
    task = _stutter_task(dev, m["steps"], m["wseed"])
    task.global_step = m["global_step"]
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1), spk_embed=inp["spk_embed"],
                  stutter_mel_masks=torch.from_numpy(g["raw_masks"]))
    sample = {k: v.to(dev) for k, v in sample.items()}
    raw = sample["stutter_mel_masks"].clone()
    total, log = task._training_step(sample, 0, t=torch.from_numpy(g["t"]).to(dev), noises=torch.from_numpy(g["eps"]).to(dev))
    assert torch.equal(sample["stutter_mel_masks"], raw)  # the caller's batch is not remapped in place
    assert list(log)[:8] == ["l1_coarse", "ssim_coarse", "pdur", "wdur", "ce", "focal", "uv", "f0"]
    for k in ("l1_coarse", "ssim_coarse", "pdur", "wdur", "ce", "focal", "uv", "f0"):
        ref = float(g["loss_" + k])
        assert abs(float(log[k]) - ref) < 2e-5 * max(1.0, abs(ref)), (k, float(log[k]), ref)
    assert abs(float(total.detach()) - float(g["total"])) < 1e-4 * max(1.0, abs(float(g["total"])))
    total.backward()
    torch.cuda.synchronize()
    params = dict(task.model.named_parameters())
    norms = dict(zip(m["param_names"], g["grad_norms"]))
    assert list(params) == m["param_names"]
    worst = 0.0
    for k, p in params.items():
        worst = max(worst, abs(float(p.grad.norm()) - norms[k]) / (norms[k] + 1e-12))
    assert worst < 1e-3, worst
    for key in [k for k in g if k.startswith("grad::")]:
        name = key[len("grad::"):]
        # sums of the decoder-input gradient over frames (a stutter-embedding row: every frame of its class; the mel encoder's output
        # bias: every frame, from both of its uses): the terms cancel, and both fp32 sums carry an error of ~1e-6 absolute -- up to
        # ~2e-3 of the largest entry at the ragged sizes.  Their norms are within the 1e-3 above.
        bar = {"stutter_embed.weight": 5e-3, "mel_encoder.fc_out.bias": 1e-3}.get(name, 2e-4)
        assert _rel(params[name].grad, torch.from_numpy(g[key])) < bar, name


def test_inference_and_detection_match_reference(dev):
    g = load_golden("infer_stutter")
    m = g["meta"]
    task = _stutter_task(dev, m["steps"], m["wseed"])
    model = task.model
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    d = {k: v.to(dev) for k, v in inp.items()}
    with torch.no_grad():
        ret = model(d["txt_tokens"], d["time_mel_masks"], None, d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"], infer=True,
                    noises=torch.from_numpy(g["noises"]).to(dev))
    assert float((ret["mel_out"].cpu() - torch.from_numpy(g["mel_out"])).abs().max()) < 1e-4
    assert float((ret["stutter_predictor_out"].cpu() - torch.from_numpy(g["stutter_predictor_out"])).abs().max()) < 2e-5
    det = model.forward_stutter_predictor(d["txt_tokens"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"])
    assert float((det.cpu() - torch.from_numpy(g["detect_logits"])).abs().max()) < 2e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# the task end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _task_hparams(tmp_path, work):
    return base_hparams(timesteps=4, residual_layers=3, binary_data_dir=os.path.join(GOLDEN, "binary_stutter_tiny"), train_set_name="train",
                        valid_set_name="valid", infer=False, test_ids=[], max_sentences=2, max_tokens=1000, val_check_interval=3,
                        max_updates=3, num_sanity_val_steps=1, work_dir=str(tmp_path / work), num_ckpt_keep=2, warmup_updates=2,
                        tb_log_interval=2, eval_max_batches=2, lr=1e-3)


def test_task_trains_validates_and_resumes(dev, tmp_path):
    from set_amd import hparams as H, tasks
    from set_amd.trainer import move_to_device
    saved = dict(H.hparams)
    try:
        H.hparams.clear()
        H.hparams.update(_task_hparams(tmp_path, "run"))
        torch.manual_seed(77)
        tr = tasks.StutterSpeechTask.start()  # updates 0..3 with validation + checkpoint before update 3
        assert tr.global_step == 4 and len(tr.history) == 4
        assert all(np.isfinite(float(h[1])) for h in tr.history)
        assert {"ce", "focal"} <= set(tr.history[0][2])
        loss_a = float(tr.history[3][1])
        p_a = tr.optimizer.flat_p.clone()
        torch.manual_seed(78)
        tr2 = tasks.StutterSpeechTask.start()  # resume from model_ckpt_steps_3: update 3 again, bit for bit
        assert tr2.global_step == 4 and tr2.history[0][0] == 3
        assert float(tr2.history[0][1]) == loss_a and torch.equal(tr2.optimizer.flat_p, p_a)
        # a few updates on one fixed batch lower the optimised total; the weights follow global_step
        task, opt = tr2.task, tr2.optimizer
        batch = move_to_device(task.train_dataloader().fetch(0), dev)
        task.model.train()
        totals = []
        for step in range(6):
            task.global_step = 1000 * step
            w = task.loss_weights()
            opt.zero_grad()
            total, log = task._training_step(batch, 0, seed=5, t=torch.zeros(batch["txt_tokens"].shape[0], dtype=torch.long, device=dev))
            with torch.no_grad():
                want = sum(w.get(k, 1) * v for k, v in log.items() if k != "batch_size")
            assert abs(float(total) - float(want)) <= 1e-6 * abs(float(want))
            total.backward()
            opt.step()
            totals.append(float(total))
        assert totals[-1] < totals[0], totals
        # validation: the reference's acc / acc_1 formula on the same outputs
        task.model.eval()
        vb = move_to_device(task.val_dataloader().fetch(0), dev)
        with torch.no_grad():
            out = task.validation_step(vb, 0)
            _, o = task.run_model(vb, infer=False, tape=False, seed=0)
        lab = o["stutter_mel_masks"]
        pred = o["stutter_predictor_out"].argmax(-1)
        acc = (((pred == lab) & (pred == 0)).float().sum() + ((pred == lab) & (pred == 1)).float().sum()) / lab.numel()
        assert out["losses"]["acc"] == float(acc)
        if bool((lab == 1).any()):
            acc_1 = (pred[lab == 1] == 1).float().sum() / (lab == 1).sum()
            assert out["losses"]["acc_1"] == float(acc_1)
        assert abs(out["total_loss"] - sum(out["losses"].values())) < 1e-9
        ids = task.predict_stutter(vb)
        assert ids.shape == lab.shape and ids.dtype == torch.int64
    finally:
        H.hparams.clear()
        H.hparams.update(saved)


def test_infer_writes_wavs(dev, tmp_path, monkeypatch):
    """`--infer` of the stutter task: binarised test set -> edit the masked span -> HiFi-GAN -> wavs + meta.csv."""
    import yaml
    from scipy.io import wavfile
    from set_amd import hparams as H
    from set_amd import tasks
    monkeypatch.chdir(tmp_path)
    voc = tmp_path / "voc"
    voc.mkdir()
    yaml.safe_dump(Wt.HIFIGAN_TINY_RB2, open(voc / "config.yaml", "w"))
    torch.save({"state_dict": {"model_gen": Wt.seeded_weights(Wt.load_manifest("hifigan_tiny_rb2"), 22)}}, voc / "model_ckpt_steps_0.ckpt")
    cfg = os.path.join(ROOT, "speech-editing-toolkit_amd", "egs", "stutter_speech.yaml")
    H.set_hparams(config=cfg, exp_name="e2e", print_hparams=False,
                  hparams_str="timesteps=4,binary_data_dir=%s,vocoder_ckpt=%s" % (os.path.join(GOLDEN, "binary_stutter_tiny"), voc))
    H.hparams["infer"] = True
    H.hparams["test_ids"] = []
    torch.manual_seed(0)
    task0 = tasks.StutterSpeechTask(build_vocoder=False)
    sd = task0.build_model().state_dict()
    sd.update({k: v for k, v in Wt.seeded_weights(Wt.load_manifest("stutter_speech"), 5).items() if v.shape == sd[k].shape})
    os.makedirs("checkpoints/e2e", exist_ok=True)
    torch.save({"state_dict": {"model": sd}, "global_step": 7}, "checkpoints/e2e/model_ckpt_steps_7.ckpt")
    task = tasks.StutterSpeechTask()
    res = task.test()
    assert len(res) == 2
    for r in res:
        sr, wav = wavfile.read(r["files"]["P"])
        assert sr == 22050 and wav.dtype == np.int16 and wav.shape == (r["mel_pred"].shape[0] * 16,)
        assert np.isfinite(r["mel_pred"]).all()
