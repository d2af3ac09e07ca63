"""GPU tests of the training rows: every differentiable op against torch CPU autograd of the
same op, the whole loss + gradient computation against the oracle / the reference-generated golden, the fused
clip+AdamW step against torch.optim.AdamW.  fp32 tolerances are written at each check."""
import math

import numpy as np
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import base_hparams, load_golden
from oracle import oracle as O
from oracle import weights as Wt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


CONV_BWD = [
    # B, Cin, Cout, K, dil, T, extras
    (2, 48, 96, 3, 2, 70, dict(chan_add=True, res=True)),
    (2, 256, 512, 3, 1, 64, dict(chan_add=True, res=True)),
    (2, 512, 256, 1, 1, 33, dict()),
    (1, 256, 256, 1, 1, 40, dict(pro="div", pro_param=math.sqrt(20.0), act="relu")),
    (2, 192, 384, 5, 1, 50, dict(alpha=5 ** -0.5, act="gelu")),
    (2, 384, 192, 1, 1, 50, dict(res=True, mask=True)),
    (3, 192, 2, 1, 1, 90, dict()),
    (2, 192, 1, 1, 1, 20, dict(act="softplus", mask=True)),
    (2, 256, 192, 1, 1, 1, dict()),
    (1, 256, 1024, 1, 1, 5, dict(act="mish")),
    (2, 80, 256, 1, 1, 100, dict(act="relu")),
]


@pytest.mark.parametrize("case", CONV_BWD)
def test_conv1d_backward(dev, case):
    from set_amd import autograd_ops as A, ops
    B, Cin, Cout, K, dil, T, ex = case
    g = torch.Generator().manual_seed(Cin + Cout + K + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, K, generator=g) / math.sqrt(Cin * K)
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, Cout, T, generator=g) if ex.get("res") else None
    mask = (torch.rand(B, T, generator=g) > 0.3).float() if ex.get("mask") else None
    add = torch.randn(B, Cin, generator=g) if ex.get("chan_add") else None
    gy = torch.randn(B, Cout, T, generator=g)
    pad = dil * (K - 1) // 2

    def ref(xr, wr, br, addr, resr):
        xin = xr if addr is None else xr + addr[:, :, None]
        if ex.get("pro") == "div":
            xin = xin / ex["pro_param"]
        y = F.conv1d(F.pad(xin, (pad, pad)), wr, br, dilation=dil) * ex.get("alpha", 1.0)
        y = {"none": lambda v: v, "relu": F.relu, "gelu": F.gelu, "softplus": F.softplus, "mish": O.mish}[ex.get("act", "none")](y)
        if resr is not None:
            y = y + resr
        if mask is not None:
            y = y * mask[:, None, :]
        return y

    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, b, add, res)]
    with torch.enable_grad():
        ref(*leaves).backward(gy)
    d = [t.clone().to(dev).requires_grad_(True) if t is not None else None for t in (x, w, b, add, res)]
    cw = ops.ConvWeight(lambda: d[1], Cout, Cin, K)
    kw = {k: ex[k] for k in ("pro", "pro_param", "act", "alpha") if k in ex}
    with torch.enable_grad():
        y = A.conv1d(d[0], cw, d[2], dil=dil, pad=pad, in_chan_add=d[3], res=d[4],
                     mask=None if mask is None else mask.to(dev), **kw)
        y.backward(gy.to(dev))
    torch.cuda.synchronize()
    for name, a, r in zip(("dx", "dw", "db", "dadd", "dres"), d, leaves):
        if r is not None:
            assert _rel(a.grad, r.grad) < 2e-5, name


def test_small_op_backwards(dev):
    from set_amd import autograd_ops as A
    g = torch.Generator().manual_seed(9)
    B, C, T, Tt = 3, 192, 70, 21
    # LayerNorm over channels (+ mask)
    x = torch.randn(B, C, T, generator=g)
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    mask = (torch.rand(B, T, generator=g) > 0.2).float()
    gy = torch.randn(B, C, T, generator=g)
    lv = [t.clone().requires_grad_(True) for t in (x, gam, bet)]
    with torch.enable_grad():
        (O.layer_norm_ch(lv[0], lv[1], lv[2]) * mask[:, None]).backward(gy)
    dv = [t.clone().to(dev).requires_grad_(True) for t in (x, gam, bet)]
    with torch.enable_grad():
        A.layernorm_ch(dv[0], dv[1], dv[2], mask.to(dev)).backward(gy.to(dev))
    for a, r in zip(dv, lv):
        assert _rel(a.grad, r.grad) < 2e-5
    # the entry point itself on a NaN-poisoned scratch (its contents are irrelevant): dgamma/dbeta are accumulated (+=)
    from set_amd import _lib
    from set_amd.ops import _p, _stream
    xd, gd, md, gyd = x.to(dev), gam.to(dev), mask.to(dev), gy.to(dev)
    dx2, dg2, db2 = torch.empty_like(xd), torch.ones(C, device=dev), torch.full((C,), 2.0, device=dev)
    part = torch.full((_lib.lib().set_layernorm_ch_bwd_scratch(B, C, T),), float("nan"), device=dev)
    _lib.check(_lib.lib().set_layernorm_ch_bwd(_p(xd), _p(gd), _p(md), _p(gyd), _p(dx2), _p(dg2), _p(db2), _p(part), B, C, T,
                                               1e-5, _stream()), "set_layernorm_ch_bwd")
    assert _rel(dx2, lv[0].grad) < 2e-5 and _rel(dg2 - 1.0, lv[1].grad) < 2e-5 and _rel(db2 - 2.0, lv[2].grad) < 2e-5
    # embedding (+ base), expand_states, add_chan_mask, transposes
    idx = torch.randint(0, 50, (B, T), generator=g)
    tab = torch.randn(50, C, generator=g)
    lt, lb = tab.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with torch.enable_grad():
        (lb + 2.0 * F.embedding(idx, lt).transpose(1, 2)).backward(gy)
    dt, db_ = tab.clone().to(dev).requires_grad_(True), x.clone().to(dev).requires_grad_(True)
    with torch.enable_grad():
        A.embedding_bct(idx.to(dev), dt, scale=2.0, out=db_, accumulate=True).backward(gy.to(dev))
    assert _rel(dt.grad, lt.grad) < 1e-5 and _rel(db_.grad, lb.grad) == 0.0
    lt2, dt2 = tab.clone().requires_grad_(True), tab.clone().to(dev).requires_grad_(True)
    with torch.enable_grad():
        F.embedding(idx, lt2, padding_idx=0).transpose(1, 2).backward(gy)
        A.embedding_bct(idx.to(dev), dt2, padding_idx=0).backward(gy.to(dev))
    assert float(dt2.grad[0].abs().max()) == 0.0 and _rel(dt2.grad, lt2.grad) < 1e-5
    enc = torch.randn(B, C, Tt, generator=g)
    m2p = torch.sort(torch.randint(0, Tt + 1, (B, T), generator=g), dim=1).values
    le = enc.clone().requires_grad_(True)
    with torch.enable_grad():
        O.expand_states(le.transpose(1, 2), m2p).transpose(1, 2).backward(gy)
    de = enc.clone().to(dev).requires_grad_(True)
    with torch.enable_grad():
        A.expand_states(de, m2p.to(dev)).backward(gy.to(dev))
    assert _rel(de.grad, le.grad) < 1e-5
    add = torch.randn(B, C, generator=g)
    lx, la = x.clone().requires_grad_(True), add.clone().requires_grad_(True)
    with torch.enable_grad():
        ((lx + la[:, :, None]) * mask[:, None]).backward(gy)
    dx, da = x.clone().to(dev).requires_grad_(True), add.clone().to(dev).requires_grad_(True)
    with torch.enable_grad():
        A.add_chan_mask(dx, da, mask.to(dev)).backward(gy.to(dev))
    assert _rel(dx.grad, lx.grad) == 0.0 and _rel(da.grad, la.grad) < 1e-5
    # activations
    z = torch.randn(4000, generator=g) * 3
    for act, fn in (("gelu", F.gelu), ("mish", O.mish), ("softplus", F.softplus), ("tanh", torch.tanh)):
        lz = z.clone().requires_grad_(True)
        with torch.enable_grad():
            fn(lz).backward(torch.ones_like(z))
        dz = z.clone().to(dev).requires_grad_(True)
        with torch.enable_grad():
            yy = A.activation(dz, act)
            yy.backward(torch.ones_like(dz))
        assert _rel(yy, fn(z)) < 1e-5 and _rel(dz.grad, lz.grad) < 1e-5, act
    # gate + res_skip (functional)
    y2 = torch.randn(B, 2 * C, T, generator=g)
    ly = y2.clone().requires_grad_(True)
    with torch.enable_grad():
        a_, b_ = torch.chunk(ly, 2, dim=1)
        (torch.sigmoid(a_) * torch.tanh(b_)).backward(gy)
    dy = y2.clone().to(dev).requires_grad_(True)
    with torch.enable_grad():
        A.gate(dy).backward(gy.to(dev))
    assert _rel(dy.grad, ly.grad) < 1e-5
    o = torch.randn(B, 2 * C, T, generator=g)
    sk = torch.randn(B, C, T, generator=g)
    g2 = torch.randn(B, C, T, generator=g)
    ls = [t.clone().requires_grad_(True) for t in (x, o, sk)]
    with torch.enable_grad():
        r_, s_ = torch.chunk(ls[1], 2, dim=1)
        (((ls[0] + r_) / math.sqrt(2.0)) * gy + (ls[2] + s_) * g2).sum().backward()
    ds = [t.clone().to(dev).requires_grad_(True) for t in (x, o, sk)]
    with torch.enable_grad():
        xo, so = A.res_skip_fn(ds[0], ds[1], ds[2])
        (xo * gy.to(dev) + so * g2.to(dev)).sum().backward()
    for a, r in zip(ds, ls):
        assert _rel(a.grad, r.grad) < 1e-6
    # dropout: same mask forward/backward, keep-rate, scaling
    xd = torch.ones(1 << 18, device=dev, requires_grad=True)
    with torch.enable_grad():
        yd = A.dropout(xd, 0.2, seed=3, offset=7)
        yd.sum().backward()
    assert torch.equal(yd.detach(), xd.grad) and abs(float((yd > 0).float().mean()) - 0.8) < 5e-3
    assert abs(float(yd.max()) - 1.25) < 1e-6
    # grad_scale
    xs = torch.randn(100, device=dev, requires_grad=True)
    with torch.enable_grad():
        A.grad_scale(xs, 0.1).sum().backward()
    assert _rel(xs.grad, torch.full((100,), 0.1)) < 1e-7


def test_losses_forward_backward(dev):
    from set_amd import autograd_ops as A, ops
    g = torch.Generator().manual_seed(21)
    B, T, M, Tt = 3, 60, 80, 14
    pred = torch.randn(B, T, M, generator=g) * 0.5 - 3.0
    target = torch.clamp(torch.randn(B, T, M, generator=g) * 1.5 - 3.0, -6, 1.5)
    target[1, 50:] = 0
    target[2, 30:] = 0
    lp = pred.clone().requires_grad_(True)
    with torch.enable_grad():
        l1, ss = O.l1_loss(lp, target), O.ssim_loss(lp, target)
        (l1 * 0.5 + ss * 0.5).backward()
    dp = pred.clone().to(dev).requires_grad_(True)
    w = A.frame_weights(target.to(dev))
    with torch.enable_grad():
        l1d, ssd = A.masked_l1(dp, target.to(dev), w), A.ssim_loss(dp, target.to(dev), w)
        (l1d * 0.5 + ssd * 0.5).backward()
    assert abs(float(l1d) - float(l1)) < 1e-5 and abs(float(ssd) - float(ss)) < 2e-5
    assert _rel(dp.grad, lp.grad) < 5e-4  # ssim: differences of nearly equal second moments
    # duration + pitch losses
    inp = Wt.synthetic_inputs(B, T, Tt, seed=5, pad_tail=True)
    dur = torch.rand(B, Tt, generator=g) * 5
    dur[:, -2:] = 0
    pp = torch.randn(B, T, 2, generator=g)
    ld, lpp = dur.clone().requires_grad_(True), pp.clone().requires_grad_(True)
    with torch.enable_grad():
        pd, wd = O.dur_losses(ld, inp["mel2ph"], inp["txt_tokens"], (1, 2, 3), 0.1, 1.0)
        uvl, f0l = O.pitch_losses(lpp, inp["f0"], inp["uv"], inp["mel2ph"], 1.0, 1.0)
        (pd + wd + uvl + f0l).backward()
    sil = torch.zeros_like(inp["txt_tokens"], dtype=torch.bool)
    for i in (1, 2, 3):
        sil |= inp["txt_tokens"] == i
    sil = sil.long()
    word_id = (sil.cumsum(-1) * (1 - sil)).contiguous()
    dd = dur.clone().to(dev).requires_grad_(True)
    dpp = pp.transpose(1, 2).contiguous().to(dev).requires_grad_(True)
    with torch.enable_grad():
        pd2, wd2 = A.dur_losses(dd, inp["mel2ph"].to(dev), inp["txt_tokens"].to(dev), word_id.to(dev),
                                int(word_id.max()), 0.1, 1.0)
        uv2, f02 = A.pitch_losses(dpp, inp["f0"].to(dev), inp["uv"].to(dev), inp["mel2ph"].to(dev), 1.0, 1.0)
        (pd2 + wd2 + uv2 + f02).backward()
    for a, r in ((pd2, pd), (wd2, wd), (uv2, uvl), (f02, f0l)):
        assert abs(float(a) - float(r)) < 1e-5 * max(1.0, abs(float(r)))
    assert _rel(dd.grad, ld.grad) < 1e-5
    assert _rel(dpp.grad.transpose(1, 2), lpp.grad) < 1e-5


def _train_setup(dev, steps, wseed, over=None, manifest="spec_denoiser", task_cls="SpeechDenoiserTask"):
    from set_amd import hparams as H
    from set_amd import tasks
    H.hparams.clear()
    H.hparams.update(base_hparams(timesteps=steps, **(over or {})))
    task = getattr(tasks, task_cls)(build_vocoder=False)
    task.build_model()
    W = Wt.seeded_weights(Wt.load_manifest(manifest), wseed)
    task.model.load_state_dict(W, strict=False)
    task.model.to(dev).eval()  # eval: predictor dropout off, as in the fixtures
    return task, W


@pytest.mark.parametrize("fixture", ["train_losses", "train_losses_ragged"])
@pytest.mark.parametrize("stack", ["per_op", "fused_stack"])
def test_training_losses_and_all_gradients_match_reference(dev, monkeypatch, stack, fixture):
    """tests/golden/train_losses.npz: the reference's own model + loss functions + autograd (oracle/make_golden.py).
    `fused_stack`: the DiffNet layers run as one persistent Winograd launch with saved activations and the
    hand-ordered backward (what large batches use); `per_op`: one differentiable kernel per op.
    `train_losses_ragged` (round 5): B = 3, T = 77, T_txt = 19 with padded tails -- sizes that are multiples of nothing."""
    if stack == "fused_stack":
        monkeypatch.setenv("SET_AMD_WINO", "2")       # tiny batch: force the kernel choice the big batches get
    else:
        monkeypatch.setenv("SET_AMD_TRAIN_STACK", "0")
    g = load_golden(fixture)
    m = g["meta"]
    task, W = _train_setup(dev, m["steps"], m["wseed"])
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1), spk_embed=inp["spk_embed"])
    sample = {k: v.to(dev) for k, v in sample.items()}
    losses, out = task.run_model(sample, infer=False, t=torch.from_numpy(g["t"]).to(dev),
                                 noises=torch.from_numpy(g["eps"]).to(dev))
    for k in ("l1_coarse", "ssim_coarse", "pdur", "wdur", "uv", "f0"):
        ref = float(g["loss_" + k])
        assert abs(float(losses[k]) - ref) < 2e-5 * max(1.0, abs(ref)), (k, float(losses[k]), ref)
    with torch.enable_grad():
        total = sum(losses.values())
    assert abs(float(total) - float(g["total"])) < 1e-4
    total.backward()
    torch.cuda.synchronize()
    params = dict(task.model.named_parameters())
    norms = dict(zip(m["param_names"], g["grad_norms"]))
    worst = 0.0
    for k, p in params.items():
        ref = norms[k]
        if ref < 0:  # the reference leaves .grad None (fs.decoder, fs.mel_out never run)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        got = float(p.grad.norm())
        worst = max(worst, abs(got - ref) / (ref + 1e-12))
    assert worst < 1e-3, worst
    for key in [k for k in g if k.startswith("grad::")]:
        name = key[len("grad::"):]
        gr = params[name].grad.cpu()
        ref = torch.from_numpy(g[key])
        gr = gr[:ref.shape[0]] if gr.shape != ref.shape else gr
        assert _rel(gr, ref) < 2e-4, name


def test_training_without_pitch_embed_matches_reference(dev):
    """egs/spec_denoiser_libritts.yaml (use_pitch_embed false): losses l1_coarse / ssim_coarse / pdur / wdur only
    (tasks/speech_editing/spec_denoiser.py:55), no pitch parameters, f0 / uv are None in the batch
    (tasks/speech_editing/dataset_utils.py:125-127).  Fixture: tests/golden/train_losses_nopitch.npz."""
    g = load_golden("train_losses_nopitch")
    m = g["meta"]
    task, W = _train_setup(dev, m["steps"], m["wseed"], over=dict(use_pitch_embed=False),
                           manifest="spec_denoiser_nopitch")
    assert not any(k.startswith("fs.pitch_") for k in task.model.state_dict())
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1), spk_embed=inp["spk_embed"])
    sample = {k: v.to(dev) for k, v in sample.items()}
    sample.update(f0=None, uv=None, pitch=None)
    losses, out = task.run_model(sample, infer=False, t=torch.from_numpy(g["t"]).to(dev),
                                 noises=torch.from_numpy(g["eps"]).to(dev))
    assert sorted(losses) == ["l1_coarse", "pdur", "ssim_coarse", "wdur"]
    for k in losses:
        ref = float(g["loss_" + k])
        assert abs(float(losses[k]) - ref) < 2e-5 * max(1.0, abs(ref)), (k, float(losses[k]), ref)
    with torch.enable_grad():
        total = sum(losses.values())
    total.backward()
    torch.cuda.synchronize()
    params = dict(task.model.named_parameters())
    assert list(params) == m["param_names"]
    worst = 0.0
    for k, ref in zip(m["param_names"], g["grad_norms"]):
        p = params[k]
        if ref < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        worst = max(worst, abs(float(p.grad.norm()) - ref) / (ref + 1e-12))
    assert worst < 1e-3, worst
    for key in [k for k in g if k.startswith("grad::")]:
        gr = params[key[len("grad::"):]].grad.cpu()
        ref = torch.from_numpy(g[key])
        gr = gr[:ref.shape[0]] if gr.shape != ref.shape else gr
        assert _rel(gr, ref) < 2e-4, key


def test_training_normal_variant_matches_reference(dev):
    """egs/spec_denoiser_wo_masked_predictor.yaml: SpeechDenoiserNormalTask (tasks/speech_editing/spec_denoiser_normal.py)
    over the plain-FastSpeech conditioner, incl. the reference's positional binding uv -> f0 (spec_denoiser_normal.py:158).
    Fixture: tests/golden/train_losses_normal.npz (reference model + its own loss functions + autograd)."""
    g = load_golden("train_losses_normal")
    m = g["meta"]
    task, W = _train_setup(dev, m["steps"], m["wseed"], manifest="spec_denoiser_normal",
                           task_cls="SpeechDenoiserNormalTask")
    assert "fs.dur_embed.weight" not in task.model.state_dict()
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1), spk_embed=inp["spk_embed"])
    sample = {k: v.to(dev) for k, v in sample.items()}
    losses, out = task.run_model(sample, infer=False, t=torch.from_numpy(g["t"]).to(dev),
                                 noises=torch.from_numpy(g["eps"]).to(dev))
    assert int(out["pitch"].max()) == 1 and int(out["pitch"].min()) == 1
    for k in ("l1_coarse", "ssim_coarse", "pdur", "wdur", "uv", "f0"):
        ref = float(g["loss_" + k])
        assert abs(float(losses[k]) - ref) < 2e-5 * max(1.0, abs(ref)), (k, float(losses[k]), ref)
    with torch.enable_grad():
        total = sum(losses.values())
    total.backward()
    torch.cuda.synchronize()
    params = dict(task.model.named_parameters())
    assert list(params) == m["param_names"]
    worst = 0.0
    for k, ref in zip(m["param_names"], g["grad_norms"]):
        p = params[k]
        if ref < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        worst = max(worst, abs(float(p.grad.norm()) - ref) / (ref + 1e-12))
    assert worst < 1e-3, worst
    for key in [k for k in g if k.startswith("grad::")]:
        gr = params[key[len("grad::"):]].grad.cpu()
        ref = torch.from_numpy(g[key])
        gr = gr[:ref.shape[0]] if gr.shape != ref.shape else gr
        assert _rel(gr, ref) < 2e-4, key


def test_adamw_step_matches_torch(dev):
    from set_amd import autograd_ops as A
    g = torch.Generator().manual_seed(4)
    n = 10000
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=2e-4, betas=(0.9, 0.98), weight_decay=0.01)
    dp = p0.clone().to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(1, 6):
        gr = torch.randn(n, generator=g) * (3.0 if step % 2 else 0.001)
        ref_p.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        dg = gr.to(dev)
        A.adamw_step(dp, dg, m, v, 2e-4, 0.9, 0.98, 1e-8, 0.01, step, A.grad_sumsq(dg), 1.0)
        assert _rel(dp, ref_p) < 1e-6, step
    # grad_scale = 1/world reproduces the step on the mean gradient
    dp2, m2, v2 = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    dp3, m3, v3 = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    gs = (torch.randn(n, generator=g) * 4).to(dev)
    A.adamw_step(dp2, gs, m2, v2, 2e-4, 0.9, 0.98, 1e-8, 0.0, 1, A.grad_sumsq(gs), 1.0, 0.25)
    gm = (gs * 0.25).contiguous()
    A.adamw_step(dp3, gm, m3, v3, 2e-4, 0.9, 0.98, 1e-8, 0.0, 1, A.grad_sumsq(gm), 1.0, 1.0)
    assert _rel(dp2, dp3) < 1e-6


def test_training_step_decreases_loss_and_repacks_weights(dev):
    from set_amd.training import FlatAdamW
    task, W = _train_setup(dev, 8, 31)
    task.model.train()  # dropout on (Philox), as in real training
    opt = FlatAdamW(task.model, lr=1e-3, warmup_updates=1, clip_grad_norm=1.0)
    inp = Wt.synthetic_inputs(4, 96, 24, seed=77, pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1), spk_embed=inp["spk_embed"])
    sample = {k: v.to(dev) for k, v in sample.items()}
    t = torch.tensor([1, 3, 5, 7], device=dev)
    eps = torch.randn(4, 80, 96, generator=torch.Generator().manual_seed(1)).to(dev)
    hist = []
    for it in range(6):
        total, parts, lr = task.training_step(sample, opt, t=t, noises=eps, seed=123)
        hist.append(float(total))
    assert all(np.isfinite(hist)) and hist[-1] < hist[0], hist
    # parameters are views of the flat buffer and inference after the update sees the new weights (re-packed)
    p = next(task.model.parameters())
    assert p.data_ptr() >= opt.flat_p.data_ptr()
    with torch.no_grad():
        task.model.eval()
        out = task.model(sample["txt_tokens"], sample["time_mel_masks"][:, :, None], sample["mel2ph"], sample["spk_embed"],
                         sample["mels"], sample["f0"], sample["uv"], infer=True, seed=1)
    assert torch.isfinite(out["mel_out"]).all()


# ----------------------------------------------------------------------------------------------------
# Trainer counterpart: train from an IndexedDataset with token-budget batches, save, resume
# ----------------------------------------------------------------------------------------------------
def _trainer_hparams(tmp_path, work):
    import os
    from conftest import GOLDEN
    return base_hparams(timesteps=4, residual_layers=3, binary_data_dir=os.path.join(GOLDEN, "binary_tiny"),
                        train_set_name="test", valid_set_name="test", infer=False, test_ids=[], max_sentences=2,
                        max_tokens=1000, val_check_interval=3, max_updates=3, num_sanity_val_steps=1,
                        work_dir=str(tmp_path / work), num_ckpt_keep=2, warmup_updates=2, tb_log_interval=2,
                        eval_max_batches=2, sil_token_ids=[1, 21, 22],  # every fixture item has a silence + a word
                        ds_workers=1)  # batch k + 1 is assembled on a background thread while update k runs


def test_trainer_trains_saves_and_resumes_bit_identically(dev, tmp_path):
    """`start()` without --infer trains from the binarised set (written by the reference's builder) with
    batch_by_size batches, validates + saves every val_check_interval updates, and a restart from
    model_ckpt_steps_3.ckpt repeats update 3 of the uninterrupted run bit for bit (batches, t, noise and dropout are
    functions of (seed, update); every reduction on the path is order-deterministic)."""
    import os
    from set_amd import hparams as H, tasks
    saved = dict(H.hparams)
    try:
        H.hparams.clear()
        H.hparams.update(_trainer_hparams(tmp_path, "run"))
        torch.manual_seed(77)
        tr = tasks.SpeechDenoiserTask.start()          # updates 0..3; validation + checkpoint before update 3
        assert tr.global_step == 4 and len(tr.history) == 4
        assert sorted(os.listdir(tmp_path / "run")) == ["model_ckpt_steps_3.ckpt"]
        ck = torch.load(tmp_path / "run" / "model_ckpt_steps_3.ckpt", map_location="cpu", weights_only=False)
        assert ck["global_step"] == 3 and list(ck["state_dict"]) == ["model"] and len(ck["optimizer_states"]) == 1
        assert ck["checkpoint_callback_best"] is not None
        loss_a = float(tr.history[3][1])
        parts_a = {k: float(v) for k, v in tr.history[3][2].items()}
        p_a = tr.optimizer.flat_p.clone()
        assert all(np.isfinite(float(h[1])) for h in tr.history)
        # restart: a fresh process would do exactly this (new task, new model with a DIFFERENT random init, restore)
        torch.manual_seed(78)
        tr2 = tasks.SpeechDenoiserTask.start()
        assert tr2.global_step == 4 and len(tr2.history) == 1 and tr2.history[0][0] == 3
        assert tr2.optimizer.num_updates == 4
        loss_b = float(tr2.history[0][1])
        parts_b = {k: float(v) for k, v in tr2.history[0][2].items()}
        assert loss_b == loss_a and parts_b == parts_a
        assert torch.equal(tr2.optimizer.flat_p, p_a)
    finally:
        H.hparams.clear()
        H.hparams.update(saved)


def test_gradient_accumulation_matches_one_big_step(dev, tmp_path):
    """accumulate_grad_batches=2 (utils/commons/trainer.py:331-340,365-372): two backwards into one optimizer step,
    loss / 2 each -- the parameters after it equal those after one step on the two micro-batches' mean gradient."""
    from set_amd import hparams as H, tasks
    from set_amd.trainer import Trainer
    saved = dict(H.hparams)
    try:
        H.hparams.clear()
        H.hparams.update(_trainer_hparams(tmp_path, "acc"))
        H.hparams.update(accumulate_grad_batches=2, max_updates=0, num_sanity_val_steps=0, max_sentences=1)
        torch.manual_seed(5)
        tr = tasks.SpeechDenoiserTask.start()
        assert tr.global_step == 1 and tr.optimizer.num_updates == 1
        g_acc = tr.optimizer.flat_g.clone()
        # the same two micro-batches by hand
        task, opt = tr.task, tr.optimizer
        loader = task.train_dataloader()  # (built from hparams['seed']: the same batch list the trainer used)
        from set_amd.trainer import move_to_device, step_seed
        want = torch.zeros_like(g_acc)
        for k in range(2):
            opt.zero_grad()
            batch = move_to_device(loader.fetch(k), dev)
            t = torch.from_numpy(np.random.default_rng([tr.seed, k]).integers(0, 5, size=(1,), dtype=np.int64)).to(dev)
            # NB parameters moved by the accumulated step above: gradients are compared on the UPDATED weights for
            # both, so re-run the accumulated pass too
            loss, _ = task._training_step(batch, k, seed=step_seed(tr.seed, k), t=t)
            loss.backward()
            from set_amd import autograd_ops as A
            A.zero_arena_end()
            want += opt.flat_g / 2
        opt.zero_grad(accumulate=True)
        for k in range(2):
            batch = move_to_device(loader.fetch(k), dev)
            t = torch.from_numpy(np.random.default_rng([tr.seed, k]).integers(0, 5, size=(1,), dtype=np.int64)).to(dev)
            loss, _ = task._training_step(batch, k, seed=step_seed(tr.seed, k), t=t)
            with torch.enable_grad():  # other test modules switch autograd off globally at import
                (loss / 2).backward()
        from set_amd import autograd_ops as A
        A.zero_arena_end()
        got = opt.flat_g.clone()
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
        assert float(g_acc.abs().max()) > 0
    finally:
        H.hparams.clear()
        H.hparams.update(saved)


# ----------------------------------------------------------------------------------------------------
# BASELINE size (B=32, T=800): run-to-run determinism of a whole step, oracle gradients at full length
# ----------------------------------------------------------------------------------------------------
def _full_size_step(dev, task, B, dtype, seed=3):
    from set_amd import ops
    from set_amd.synthetic import synthetic_inputs
    inp = synthetic_inputs(B, 800, 100, seed=1234, pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=inp["spk_embed"])
    sample = {k: v.to(dev) for k, v in sample.items()}
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 9, (B,), generator=g)
    eps = torch.randn(B, 80, 800, generator=g)
    for p in task.model.parameters():
        p.grad = None
    ops.set_compute_dtype(dtype)
    try:
        losses, _ = task.run_model(sample, infer=False, t=t.to(dev), noises=eps.to(dev))
        with torch.enable_grad():
            total = sum(losses.values())
        total.backward()
    finally:
        ops.set_compute_dtype("f32")
    torch.cuda.synchronize()
    flat = torch.cat([p.grad.reshape(-1) for p in task.model.parameters() if p.grad is not None])
    return {k: float(v) for k, v in losses.items()}, flat, inp, t, eps


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_full_size_training_step_is_bit_stable(dev, dtype):
    """B=32, T=800 (BASELINE configs[1] shape), the whole forward + losses + backward twice from the
    same state: every loss and every gradient element bit-identical (no order-dependent reduction left on the path)."""
    task, _ = _train_setup(dev, 8, 18)
    l1, g1, *_ = _full_size_step(dev, task, 32, dtype)
    l2, g2, *_ = _full_size_step(dev, task, 32, dtype)
    assert l1 == l2
    assert torch.equal(g1, g2)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0


def test_full_length_training_matches_oracle_on_two_utterances(dev):
    """T=800 (13 tiles per utterance, every halo / tail path of the fused kernels) against the oracle's autograd on CPU
    (fp32 path): losses to 2e-5; DiffNet / mel-encoder gradients to 2e-4 of their largest entry; the conditioner's
    predictors sit behind sign(pred - f0) and ReLU masks that flip on 1e-7 forward differences, so there the bar is on
    the whole tensor (norm-wise 2e-3) -- measured 7.7e-4 worst."""
    task, W = _train_setup(dev, 8, 18)
    losses, flat, inp, t, eps = _full_size_step(dev, task, 2, "f32")
    Wg = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in W.items()}
    with torch.enable_grad():
        olosses, _ = O.training_losses(Wg, 8, inp, t, eps[:, None])
        sum(olosses.values()).backward()
    for k in olosses:
        assert abs(losses[k] - float(olosses[k])) < 2e-5 * max(1.0, abs(float(olosses[k]))), k
    rows = []
    for k, p in task.model.named_parameters():
        og = Wg[k].grad
        if og is None or p.grad is None:
            assert og is None and (p.grad is None or float(p.grad.abs().max()) == 0.0), k
            continue
        a, b = p.grad.detach().cpu().double(), og.double()
        rows.append((_rel(p.grad, og), float((a - b).norm() / (b.norm() + 1e-30)), float(b.abs().max()), k))
    rows.sort(reverse=True)
    for r in rows[:6]:
        print("max-rel %.3e  norm-rel %.3e  |g|max %.3e  %s" % r)
    for mx, nr, _, k in rows:
        if k.startswith("denoise_fn.") or k.startswith("mel_encoder."):
            assert mx < 2e-4, (k, mx)
        assert nr < 2e-3 and mx < 5e-3, (k, mx, nr)


def test_training_forward_uses_the_fused_stack_at_the_benchmark_size(dev):
    """Regression guard: the fp32 training forward decides for the persistent Winograd stack kernel by asking the library
    which fp32-pipe kernel it would pick; the inference-only kernels (row-split, split-operand) must not enter that answer."""
    from set_amd import ops
    assert ops.stack_variant(32, 800, 1, have_split=False, x3_mode=0) == 2
    assert ops.stack_variant(32, 800, 1) in (4, 5)      # inference: the split-operand kernel
    assert ops.stack_variant(1, 800, 1) == 3            # one utterance: the row-split kernel


@pytest.mark.parametrize("L_,Cc,N,gap", [(20, 256, 32, 0), (3, 128, 5, 7), (2, 64, 64, 1), (4, 192, 33, 0)])
def test_step_projections_of_all_layers_equal_the_per_layer_linears(dev, L_, Cc, N, gap):
    """diffusion_projection of every residual layer in one launch (reference diffnet.py:66,72; csrc/train.hip step_proj_*): forward
    and every gradient against fp64 torch Linear layers; parameters at one stride inside a flat buffer (what the flat optimizer
    builds), gradients handed back through autograd (no sinks here).  fp32 FMA chains: 1e-5 relative."""
    from set_amd import autograd_ops as A, ops
    g = torch.Generator().manual_seed(L_ * 1000 + Cc + N)
    per = Cc * Cc + Cc + gap
    flat = (torch.randn(L_ * per, generator=g) / math.sqrt(Cc)).to(dev)
    ws = [flat[l * per:l * per + Cc * Cc].view(Cc, Cc).requires_grad_(True) for l in range(L_)]
    bs = [flat[l * per + Cc * Cc:l * per + Cc * Cc + Cc].requires_grad_(True) for l in range(L_)]
    h = torch.randn(1, Cc, N, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(N, L_ * Cc, generator=g).to(dev)
    assert ops._uniform_stride(ws) == per and ops._uniform_stride(bs) == per
    with torch.enable_grad():
        out = A._StepProjFn.apply(h, per, per, *ws, *bs)
        out.backward(gy)
    torch.cuda.synchronize()
    hd = h.detach().cpu().double().requires_grad_(True)
    wd = [w.detach().cpu().double().requires_grad_(True) for w in ws]
    bd = [b.detach().cpu().double().requires_grad_(True) for b in bs]
    with torch.enable_grad():  # (other test modules switch the global grad mode off)
        want = torch.cat([F.linear(hd[0].t(), wd[l], bd[l]) for l in range(L_)], dim=1)
        want.backward(gy.cpu().double())
    assert _rel(out, want.float()) < 1e-5
    assert _rel(h.grad, hd.grad.float()) < 1e-5
    for l in range(L_):
        assert _rel(ws[l].grad, wd[l].grad.float()) < 1e-5
        assert _rel(bs[l].grad, bd[l].grad.float()) < 1e-5
    # a second backward gives the same bits (ordered sums, no atomics)
    h2 = h.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        A._StepProjFn.apply(h2, per, per, *[w.detach().requires_grad_(True) for w in ws], *[b.detach().requires_grad_(True) for b in bs]).backward(gy)
    assert torch.equal(h2.grad, h.grad)


def test_step_projections_fall_back_when_the_layers_are_not_at_one_stride(dev):
    from set_amd import autograd_ops as A, ops
    ws = [torch.randn(64, 64, device=dev), torch.randn(64, 64, device=dev), torch.randn(70, 64, device=dev)[:64]]
    ws2 = [torch.randn(64, 64, device=dev) for _ in range(2)] + [torch.randn(64, 64, device=dev).t()]
    assert ops._uniform_stride(ws2) is None
    flat = torch.randn(3 * 64 * 64 + 5, device=dev)
    assert ops._uniform_stride([flat[0:4096].view(64, 64), flat[4096:8192].view(64, 64), flat[8197:].view(64, 64)]) is None


def test_training_step_with_grouped_step_projections_equals_the_per_layer_path(dev, monkeypatch):
    """The whole loss + gradient computation (fp32, fused layer stack) with the 20 diffusion_projection layers laid out at one stride
    (as the flat optimizer lays them out) -> `set_step_proj_*` -- against the same step with SET_AMD_STEP_PROJ=0 (one 1x1 conv per
    layer): losses to 1e-6, every gradient to 2e-5 of its largest entry."""
    from set_amd import autograd_ops as A, ops
    monkeypatch.setenv("SET_AMD_WINO", "2")  # two utterances: force the kernel choice (and with it the fused path) of the big batches
    task, _ = _train_setup(dev, 8, 18)
    layers = list(task.model.denoise_fn.residual_layers)
    Cc = layers[0].diffusion_projection.weight.shape[0]
    per = Cc * Cc + Cc
    flat = torch.empty(len(layers) * per, device=dev)
    for l, layer in enumerate(layers):
        w, b = layer.diffusion_projection.weight, layer.diffusion_projection.bias
        flat[l * per:l * per + Cc * Cc].copy_(w.data.reshape(-1))
        flat[l * per + Cc * Cc:(l + 1) * per].copy_(b.data)
        w.data = flat[l * per:l * per + Cc * Cc].view(Cc, Cc)
        b.data = flat[l * per + Cc * Cc:(l + 1) * per]
    assert ops._uniform_stride([ly.diffusion_projection.weight for ly in layers]) == per
    calls = []
    real = A._StepProjFn.apply
    monkeypatch.setattr(A, "step_projections", (lambda f: (lambda dn, h: (calls.append(1), f(dn, h))[1]))(A.step_projections))
    l1, g1, *_ = _full_size_step(dev, task, 2, "f32")
    assert calls, "the grouped step projections were not taken"
    monkeypatch.setenv("SET_AMD_STEP_PROJ", "0")
    l0, g0, *_ = _full_size_step(dev, task, 2, "f32")
    for k in l0:
        assert abs(l1[k] - l0[k]) < 1e-6 * max(1.0, abs(l0[k])), k
    off = 0
    for name, p in task.model.named_parameters():
        if p.grad is None:
            continue
        n = p.numel()
        a, b = g1[off:off + n], g0[off:off + n]
        off += n
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-12, name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 192, 384, 5, 2, 70, True), (3, 192, 768, 9, 8, 100, False), (2, 64, 128, 3, 1, 33, True)])
def test_preln_ffn_node_equals_the_per_op_tape(dev, dtype, shape, monkeypatch):
    """autograd_ops._PreLnFfnFn (round 5): LayerNorm -> conv k (* alpha) -> GELU -> conv 1x1 (+ x, * mask) as ONE tape node against the five
    nodes of the per-op tape on the same kernels: output and every gradient (x, LayerNorm affine, both convs) bit-identical -- 'SAME' padding
    with a mask (ResidualBlock of the conv encoder, modules/commons/conv.py:24-65) and causal 'LEFT' padding k - 1 without one
    (TransformerFFNLayer, modules/speech_editing/commons/transformer.py:76-113)."""
    from set_amd import autograd_ops as A, ops
    B, Cc, Cmid, K, pad, T, with_mask = shape
    g = torch.Generator().manual_seed(Cc + K + T)
    x0 = torch.randn(B, Cc, T, generator=g)
    gy = torch.randn(B, Cc, T, generator=g)
    mask = (torch.rand(B, T, generator=g) > 0.2).float().to(dev) if with_mask else None
    ref = [torch.randn(Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cmid, Cc, K, generator=g) * 0.1, torch.randn(Cmid, generator=g) * 0.1,
           torch.randn(Cc, Cmid, 1, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1]
    ops.set_compute_dtype(dtype)
    try:
        results = []
        for fused in ("1", "0"):
            monkeypatch.setenv("SET_AMD_FUSED_NODES", fused)
            x = x0.clone().to(dev).requires_grad_(True)
            ps = [t.clone().to(dev).requires_grad_(True) for t in ref]

            class Holder:
                pass
            hold = Holder()
            hold.w1, hold.w2 = ps[2], ps[4]
            cw1 = ops.ConvWeight((hold, "w1"), Cmid, Cc, K)
            cw2 = ops.ConvWeight((hold, "w2"), Cc, Cmid, 1)
            with torch.enable_grad():
                y = A.preln_ffn(x, (ps[0], ps[1]), cw1, ps[3], cw2, ps[5], pad=pad, alpha=K ** -0.5, act="gelu", mask=mask, T_out=T)
                y.backward(gy.to(dev))
            torch.cuda.synchronize()
            results.append([y.detach(), x.grad] + [p_.grad for p_ in ps])
        for a, b in zip(*results):
            assert a is not None and b is not None and torch.equal(a, b)
    finally:
        ops.set_compute_dtype("f32")


@pytest.mark.parametrize("dtype,size", [("f32", "tiny"), ("bf16", "tiny"), ("bf16", "full")])
def test_leaf_stream_updates_equal_the_single_stream_updates_bit_for_bit(dev, dtype, size, monkeypatch):
    """Round 5: weight / bias gradients that go straight into the flat optimizer's .grad run on a second HIP stream beside the
    chain of input-gradient kernels (leaf_stream.leaf_work), joined at the end of backward().  Same kernels, same operands, every target
    written by one stream: two identical replicas -- one with the leaf stream, one with SET_AMD_LEAF_STREAM=0 -- must hold bit-identical
    losses, parameters and Adam moments after every one of six updates (dropout on, different batches and seeds, warm-up moving the lr).
    `full` is the benchmark shape (B = 32, T = 800, 20 layers: the grouped layer weight gradients really do overlap the conditioner's
    backward there); a race between the streams, or an operand freed under a leaf kernel, would show up as a difference."""
    from set_amd import leaf_stream, ops
    from set_amd.synthetic import synthetic_inputs
    from set_amd.training import FlatAdamW
    ops.set_compute_dtype(dtype)
    try:
        reps = []
        for _ in range(2):
            task, W = _train_setup(dev, 8, 31) if size == "tiny" else _train_setup(dev, 8, 18)
            task.model.train()
            reps.append((task, FlatAdamW(task.model, lr=1e-3, warmup_updates=4, clip_grad_norm=1.0)))
        (ta, oa), (tb, ob) = reps
        assert torch.equal(oa.flat_p, ob.flat_p)
        for it in range(6):
            if size == "tiny":
                inp = Wt.synthetic_inputs(4, 96, 24, seed=77 + it, pad_tail=True)
                t = torch.tensor([(1 + it) % 9, 3, (5 + 2 * it) % 9, 7], device=dev)
            else:
                inp = synthetic_inputs(32, 800, 100, seed=1234 + it, pad_tail=True)
                t = torch.randint(0, 9, (32,), generator=torch.Generator().manual_seed(it)).to(dev)
            sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                          time_mel_masks=inp["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=inp["spk_embed"])
            sample = {k: v.to(dev) for k, v in sample.items()}
            monkeypatch.setenv("SET_AMD_LEAF_STREAM", "1")
            tot_a, parts_a, _ = ta.training_step(sample, oa, t=t, seed=500 + 13 * it)
            used_leaf = any(st.stream is not None for st in leaf_stream._STREAMS.values())
            monkeypatch.setenv("SET_AMD_LEAF_STREAM", "0")
            tot_b, parts_b, _ = tb.training_step(sample, ob, t=t, seed=500 + 13 * it)
            torch.cuda.synchronize()
            assert torch.equal(tot_a, tot_b), it
            assert all(torch.equal(parts_a[k], parts_b[k]) for k in parts_a), it
            assert torch.equal(oa.flat_p, ob.flat_p) and torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), it
        assert used_leaf  # (from the second update on the gradients take the direct sinks, i.e. the leaf stream)
    finally:
        ops.set_compute_dtype("f32")


def test_leaf_stream_operands_are_released_as_their_kernels_finish(dev):
    """Round 6 (advisor): the operands of leaf kernels used to be held until the end of backward() -- the fp32 DiffNet stack kept d_o and dy of all
    20 layers alive (2.1 GB at B = 32, T = 800), without a bound.  Now a marker event every ~128 MB of held operands releases what has already
    run, and a byte cap (8 GB of operand storage by default) makes the compute stream wait for the leaf stream.  Full-size fp32 step: (a) default budgets -- the peak of
    held bytes stays under the cap without an early join; (b) budgets of 1 MB / 64 MB -- early joins happen and the peak drops to the cap plus
    the largest single set of operands (the fused stack's, ~1.1 GB); (c) a replica without the leaf stream: losses, parameters and Adam
    moments bit-identical after each of three updates in all three."""
    from set_amd import leaf_stream
    from set_amd.synthetic import synthetic_inputs
    from set_amd.training import FlatAdamW
    reps = []
    for _ in range(3):
        task, W = _train_setup(dev, 8, 18)
        task.model.train()
        reps.append((task, FlatAdamW(task.model, lr=1e-3, warmup_updates=4, clip_grad_norm=1.0)))
    stats = {}
    old_env = os.environ.get("SET_AMD_LEAF_STREAM")
    try:
        for it in range(3):
            inp = synthetic_inputs(32, 800, 100, seed=4321 + it, pad_tail=True)
            t = torch.randint(0, 9, (32,), generator=torch.Generator().manual_seed(it)).to(dev)
            sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                          time_mel_masks=inp["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=inp["spk_embed"])
            sample = {k: v.to(dev) for k, v in sample.items()}
            outs = []
            for name, (task, opt) in zip(("default", "tight", "single"), reps):
                os.environ["SET_AMD_LEAF_STREAM"] = "0" if name == "single" else "1"
                for st in leaf_stream._STREAMS.values():
                    st.ledger.mark_bytes, st.ledger.cap_bytes = ((1 << 20, 64 << 20) if name == "tight" else (128 << 20, 8192 << 20))
                leaf_stream.leaf_stats(reset=True)
                tot, parts, _ = task.training_step(sample, opt, t=t, seed=900 + it)
                torch.cuda.synchronize()
                stats[name] = leaf_stream.leaf_stats()
                outs.append((tot, opt))
            for tot, opt in outs[1:]:
                assert torch.equal(tot, outs[0][0]), it
                assert torch.equal(opt.flat_p, outs[0][1].flat_p) and torch.equal(opt.m, outs[0][1].m) and torch.equal(opt.v, outs[0][1].v), it
        print("leaf operand bookkeeping (fp32, B=32, T=800), last step:", stats)
        assert stats["single"]["max_keep_bytes"] == 0
        assert 0 < stats["default"]["max_keep_bytes"] <= (8192 << 20) and stats["default"]["early_joins"] == 0
        assert stats["tight"]["early_joins"] > 0 and stats["tight"]["max_keep_bytes"] < stats["default"]["max_keep_bytes"]
        assert stats["tight"]["max_keep_bytes"] <= (64 << 20) + (1280 << 20)
    finally:
        for st in leaf_stream._STREAMS.values():
            st.ledger.mark_bytes, st.ledger.cap_bytes = 128 << 20, 8192 << 20
        if old_env is None:
            os.environ.pop("SET_AMD_LEAF_STREAM", None)
        else:
            os.environ["SET_AMD_LEAF_STREAM"] = old_env


def test_gate_and_res_skip_backward_vector_and_scalar_forms(dev):
    """set_gate_bwd / set_res_skip_bwd (diffnet.py:74-81 backward, fp32 per-op tape): the 16-byte form (C * T a multiple of 4, aligned operands)
    and the one-element form (odd sizes, or an operand that starts 4 bytes off) against the closed-form gradients -- and against each other bit
    for bit on the same data."""
    from set_amd import _lib
    from set_amd.ops import _p, _stream
    L = _lib.lib()
    g = torch.Generator().manual_seed(31)
    for B, C, T in ((2, 4, 8), (2, 5, 7), (3, 256, 100)):
        y = torch.randn(B, 2 * C, T, generator=g).to(dev)
        dz = torch.randn(B, C, T, generator=g).to(dev)
        dxo, dsk = torch.randn(B, C, T, generator=g).to(dev), torch.randn(B, C, T, generator=g).to(dev)
        outs = []
        for off in (0, 1):  # off = 1: every operand starts one float into its allocation -> the one-element form
            def shifted(t):
                buf = torch.empty(t.numel() + 4, device=dev)
                v = buf[off:off + t.numel()].view(t.shape)
                v.copy_(t)
                return v
            yy, dd, a, b = shifted(y), shifted(dz), shifted(dxo), shifted(dsk)
            dy, dx, do = shifted(torch.zeros_like(y)), shifted(torch.zeros_like(dz)), shifted(torch.zeros_like(y))
            _lib.check(L.set_gate_bwd(_p(yy), _p(dd), _p(dy), B, C, T, _stream()), "set_gate_bwd")
            _lib.check(L.set_res_skip_bwd(_p(a), _p(b), _p(dx), _p(do), B, C, T, _stream()), "set_res_skip_bwd")
            torch.cuda.synchronize()
            outs.append((dy.clone(), dx.clone(), do.clone()))
        for u, v in zip(*outs):
            assert torch.equal(u, v), (B, C, T)
        s_, th = torch.sigmoid(y[:, :C].double()), torch.tanh(y[:, C:].double())
        want = torch.cat([dz.double() * th * s_ * (1 - s_), dz.double() * s_ * (1 - th * th)], 1)
        assert _rel(outs[0][0], want) < 2e-6
        assert _rel(outs[0][1], dxo.double() / math.sqrt(2.0)) < 1e-7
        assert _rel(outs[0][2], torch.cat([dxo.double() / math.sqrt(2.0), dsk.double()], 1)) < 1e-7


@pytest.mark.parametrize("stack", ["per_op", "fused_stack"])
def test_batched_fp32_image_repack_equals_the_per_image_packs_and_marks_them_current(dev, monkeypatch, stack):
    """ops.repack_f32_images / set_pack_conv_weights_batch and set_pack_diffnet_layers (round 5): after an fp32 optimizer step every weight
    image the step used has been re-packed by ONE launch (two for the DiffNet stack).  Each must equal, bit for bit, the image the
    one-launch-per-weight entry points (set_pack_conv_weight, set_pack_conv_weight_v2, set_pack_diffnet_layer(_wino)) make of the
    updated weight, and the next step must not pack anything again lazily."""
    from set_amd import _lib, ops
    from set_amd.ops import _p, _stream
    from set_amd.training import FlatAdamW
    if stack == "fused_stack":
        monkeypatch.setenv("SET_AMD_WINO", "2")
    else:
        monkeypatch.setenv("SET_AMD_TRAIN_STACK", "0")
    task, W = _train_setup(dev, 8, 31)
    task.model.train()
    opt = FlatAdamW(task.model, lr=1e-3, warmup_updates=2)
    inp = Wt.synthetic_inputs(4, 96, 24, seed=5, pad_tail=True)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=inp["spk_embed"])
    sample = {k: v.to(dev) for k, v in sample.items()}
    for it in range(2):
        task.training_step(sample, opt, seed=it)
    L = _lib.lib()
    n0 = n2 = 0
    for cw in list(ops._F32_IMAGES):
        w = cw.raw()
        if w.device != dev:
            continue
        key = ops.weights_key((w,))
        if cw._img32.value is not None and cw._img32.key == key:  # current for this epoch without having been asked for: the batch launch did it
            ref = torch.empty_like(cw._img32.value)
            _lib.check(L.set_pack_conv_weight(_p(w), _p(ref), cw.Cout, cw.Cin, cw.K, cw.base, cw.sco, cw.sci, cw.stap, _stream()), "pack")
            assert torch.equal(ref, cw._img32.value), (cw.Cout, cw.Cin, cw.K)
            n0 += 1
        for slot, ent in cw._img2.items():
            if ent.key == key:
                wp, dil = ent.value
                ref = torch.empty_like(wp)
                _lib.check(L.set_pack_conv_weight_v2(_p(w), _p(ref), cw.Cout, cw.Cin, cw.K, dil, cw.base, cw.sco, cw.sci, cw.stap,
                                                     _stream()), "pack v2")
                assert torch.equal(ref, wp), (cw.Cout, cw.Cin, cw.K, slot)
                n2 += 1
    print("images current after the step: %d plain, %d big-tile" % (n0, n2))
    assert n0 >= 20
    # the DiffNet stack images: one launch per family against the per-layer entry points
    net = task.model.denoise_fn if hasattr(task.model, "denoise_fn") else task.model.decoder.denoise_fn
    packs = net.fused_packs(inference=False)
    for i, l in enumerate(net.residual_layers):
        w1, w2 = ops.pack_diffnet_layer(l.dilated_conv.weight.detach(), l.output_projection.weight.detach())
        assert torch.equal(packs.w1p[i], w1) and torch.equal(packs.w2p[i], w2), i
        if packs.w1w is not None:
            a, b = torch.empty_like(packs.w1w[i]), torch.empty_like(packs.w2w[i])
            ops.pack_diffnet_layer_wino(l.dilated_conv.weight.detach(), l.output_projection.weight.detach(), a, b)
            assert torch.equal(packs.w1w[i], a) and torch.equal(packs.w2w[i], b), i
    # nothing left for the lazy path: a third step asks for the same images and finds them current
    calls = []
    real = L.set_pack_conv_weight

    class Spy:
        def __getattr__(self, name):
            if name in ("set_pack_conv_weight", "set_pack_conv_weight_v2"):
                calls.append(name)
            return getattr(L, name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    task.training_step(sample, opt, seed=9)
    monkeypatch.undo()
    assert not calls, calls[:5]
    assert real is L.set_pack_conv_weight
