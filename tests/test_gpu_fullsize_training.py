"""GPU tests of whole training steps at the benchmark batch sizes against the oracle's CPU autograd: spec_denoiser at
B=32, T=800 in fp32 (the persistent Winograd training stack and the 512-thread LayerNorm backward) and in bf16 (the fused
per-layer bf16 kernels), one clip + AdamW update on the real flat parameter buffer, and CampNet at B=16, T=800 in fp32 and
bf16.  The oracle runs once per module, in float64: an fp32 oracle at these sizes carries rounding error of the same order
as the kernels' (its weight gradients are sums over B * T = 25,600 frames, in an order set by the host's CPU convolution
code), so it could not tell a kernel error from its own.  Every utterance of a batch is distinct (synthetic_inputs draws
each row), so a kernel that mixes utterances up cannot hide behind copies.  fp32 tolerances are written at each check."""
import math

import pytest
import torch

from oracle import oracle as O
from test_gpu_bf16 import BF16_GRAD_COS, BF16_GRAD_REL, BF16_GRAD_REL_ALL, BF16_LOSS_REL
from test_gpu_campnet import _full_size_campnet
from test_gpu_kernel_branches import N_FLAT
from test_gpu_training import _full_size_step, _train_setup

pytestmark = pytest.mark.gpu

B_TRAIN, B_CAMPNET, T_FULL = 32, 16, 800


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _grads(model):
    return {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}


def _leaves64(W):
    """float64 leaf copies of the floating-point weights (the others as they are)."""
    return {k: (v.detach().clone().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in W.items()}


def _f64(d):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}


def _bf16_rows(names, ref_g, got_g):
    """(rel, cos, |g|, name) per tensor against the oracle, and the all-gradient relative error (test_gpu_bf16's measures)."""
    rows, num, den = [], 0.0, 0.0
    for k in names:
        og, got = ref_g[k], got_g[k]
        if og is None or float(og.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        a, b = og.double().reshape(-1), got.cpu().double().reshape(-1)
        rows.append((float((a - b).norm() / a.norm()), float((a @ b) / (a.norm() * b.norm())), float(a.norm()), k))
        num += float((a - b).norm() ** 2)
        den += float(a.norm() ** 2)
    rows.sort(reverse=True)
    return rows, math.sqrt(num / den)


@pytest.fixture(scope="module")
def spec_denoiser_step(dev):
    """One fp32 and one bf16 training step at the bench size from the same seeded state, and the oracle's step in float64."""
    task, W = _train_setup(dev, 8, 18)
    l32, _, inp, t, eps = _full_size_step(dev, task, B_TRAIN, "f32")
    g32 = _grads(task.model)
    l16, *_ = _full_size_step(dev, task, B_TRAIN, "bf16")
    g16 = _grads(task.model)
    Wg = _leaves64(W)
    with torch.enable_grad():
        olosses, _ = O.training_losses(Wg, 8, _f64(inp), t, eps.double()[:, None])
        sum(olosses.values()).backward()
    ref_l = {k: float(v) for k, v in olosses.items()}
    ref_g = {k: (Wg[k].grad if k in Wg else None) for k in g32}
    names = [k for k, _ in task.model.named_parameters()]
    return dict(task=task, l32=l32, g32=g32, l16=l16, g16=g16, ref_l=ref_l, ref_g=ref_g, names=names, W=W)


def test_fp32_step_at_the_bench_size_takes_the_fused_stack_and_the_wide_layernorm_backward(dev, spec_denoiser_step):
    """If a later change moves the benchmark off these kernels, the gradient checks below would quietly test something
    else: fail here instead."""
    from set_amd import hparams as H, ops
    assert ops.stack_variant(B_TRAIN, T_FULL, 1, have_split=False, x3_mode=0) == 2  # persistent Winograd training stack
    # train.hip layernorm_ch_bwd_launch: big = C <= 256 && B * ceil(T / 32) >= n_cu (256) -> layernorm_ch_bwd_kernel<32, 16, 16>, 512 threads
    C = H.hparams["hidden_size"]
    assert C <= 256 and B_TRAIN * ((T_FULL + 31) // 32) >= 256, C


def test_fp32_losses_and_gradients_match_the_oracle_at_the_bench_size(dev, spec_denoiser_step):
    """Bars of test_full_length_training_matches_oracle_on_two_utterances: losses to 2e-5; DiffNet / mel-encoder gradients
    to 2e-4 of their largest entry; every tensor norm-wise 2e-3 and element-wise 5e-3 (the conditioner's predictors sit
    behind sign(pred - f0) and ReLU masks that flip on 1e-7 forward differences)."""
    s = spec_denoiser_step
    for k, ref in s["ref_l"].items():
        assert abs(s["l32"][k] - ref) < 2e-5 * max(1.0, abs(ref)), (k, s["l32"][k], ref)
    rows = []
    for k in s["names"]:
        og, got = s["ref_g"][k], s["g32"][k]
        if og is None or got is None:
            assert og is None and (got is None or float(got.abs().max()) == 0.0), k
            continue
        a, b = got.cpu().double(), og.double()
        rows.append((_rel(got, og), float((a - b).norm() / (b.norm() + 1e-30)), float(b.abs().max()), k))
    assert len(rows) > 100
    rows.sort(reverse=True)
    for r in rows[:6]:
        print("max-rel %.3e  norm-rel %.3e  |g|max %.3e  %s" % r)
    for mx, nr, _, k in rows:
        if k.startswith("denoise_fn.") or k.startswith("mel_encoder."):
            assert mx < 2e-4, (k, mx)
        assert nr < 2e-3 and mx < 5e-3, (k, mx, nr)


def test_bf16_losses_and_gradients_are_within_the_bf16_bars_of_the_oracle(dev, spec_denoiser_step):
    """The `--dtype bf16` bench step (fused per-layer bf16 kernels) against the same fp32 oracle, with the bars of
    test_gpu_bf16."""
    s = spec_denoiser_step
    for k, ref in s["ref_l"].items():
        assert abs(s["l16"][k] - ref) < BF16_LOSS_REL * max(1.0, abs(ref)), (k, s["l16"][k], ref)
    assert any(s["l16"][k] != s["l32"][k] for k in s["l16"])  # bf16 really ran
    rows, rel_all = _bf16_rows(s["names"], s["ref_g"], s["g16"])
    worst_rel, worst_cos = rows[0][0], min(r[1] for r in rows)
    print("bf16 vs oracle at B=%d: all-gradient rel %.3e, worst tensor rel %.3e, worst cos %.6f" % (B_TRAIN, rel_all, worst_rel, worst_cos))
    for r in rows[:6]:
        print("   rel %.3e cos %.6f |g| %.3e  %s" % r)
    assert rel_all < BF16_GRAD_REL_ALL and worst_rel < BF16_GRAD_REL and worst_cos > BF16_GRAD_COS, (rel_all, worst_rel, worst_cos)


def test_clipped_adamw_update_on_the_full_flat_buffer_matches_torch(dev, spec_denoiser_step):
    """The oracle's gradients as fp32, flattened in model order (n = N_FLAT: set_sumsq_det at its 2048-block cap, set_adamw
    over the real buffer), through three clip(1.0) + AdamW steps against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in fp64.
    The steps are scaled so that clipping fires on steps 1 and 3 (norm 5, 20) and not on step 2 (norm 0.5, a rotated
    vector): Adam's m / sqrt(v) is scale-free within one step, but not across steps with different clip factors."""
    from set_amd import autograd_ops as A
    s = spec_denoiser_step
    W = s["W"]
    p0 = torch.cat([W[k].reshape(-1).float() for k in s["names"]])
    g0 = torch.cat([(s["ref_g"][k] if s["ref_g"][k] is not None else torch.zeros_like(W[k])).reshape(-1).float()
                    for k in s["names"]])
    n = p0.numel()
    assert n == sum(p.numel() for p in s["task"].model.parameters()) == N_FLAT  # the size test_gpu_kernel_branches sweeps
    assert n > 2048 * 256  # above the block cap of set_sumsq_det
    g0n = float(g0.double().norm())
    steps = [g0 * (5.0 / g0n), torch.roll(g0, 12345) * (0.5 / g0n), g0.flip(0) * (20.0 / g0n)]
    lr, b1, b2, eps, wd = 2e-4, 0.9, 0.98, 1e-8, 0.01
    ref_p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    dp, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    # sumsq: per-thread fma chain of ceil(n / (2048 * 256)) terms, a 256-wide tree (8), the partial-row sum (rows / 64 + 2 chain
    # adds + 16 group adds): every term is >= 0, so the error is <= depth * u * the sum
    depth = -(-n // (2048 * 256)) + 8 + 2048 // 64 + 18
    u = 2.0 ** -24
    for step, gs in enumerate(steps, 1):
        ref_p.grad = gs.double().clone()
        want_sq = float((gs.double() ** 2).sum())
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        dg = gs.to(dev)
        sq = A.grad_sumsq(dg)
        assert abs(float(sq) - want_sq) <= depth * u * want_sq, (step, float(sq), want_sq)
        A.adamw_step(dp, dg, m, v, lr, b1, b2, eps, wd, step, sq, 1.0)
        torch.cuda.synchronize()
        # each step rounds p three times (the fp32 factor 1 - lr wd, p times it, minus the update: 3 u |p|) and computes its update
        # lr * m_hat / (sqrt(v_hat) + eps) (|.| <= lr) from a handful of fp32 operations plus the clip factor (relative error
        # <= depth * u): <= (depth + 16) * u * lr per element and step.  A clip factor left out would move elements by ~ lr.
        got, want = dp.cpu().double(), ref_p.detach()
        bound = step * u * (3 * want.abs() + (depth + 16) * lr) + 1e-30
        err = (got - want).abs()
        assert bool((err <= bound).all()), (step, float((err / bound).max()))


@pytest.fixture(scope="module")
def campnet_step(dev):
    """One fp32 and one bf16 CampNet training step (bench.py's campnet train lines) and the oracle's step in float64."""
    from set_amd import ops
    task, model, sample, inp, W = _full_size_campnet(dev, B=B_CAMPNET, T=T_FULL)
    got = {}
    for dtype in ("f32", "bf16"):
        for p in model.parameters():
            p.grad = None
        ops.set_compute_dtype(dtype)
        try:
            losses, _ = task.run_model(sample, infer=False)
            with torch.enable_grad():
                total = sum(losses.values())
            total.backward()
        finally:
            ops.set_compute_dtype("f32")
        torch.cuda.synchronize()
        got[dtype] = ({k: float(v) for k, v in losses.items()}, _grads(model))
    Wg = _leaves64(W)
    with torch.enable_grad():
        ol, _ = O.campnet_losses(Wg, inp["txt_tokens"], inp["ref_mels"].double(), inp["time_mel_masks"].double())
        sum(ol.values()).backward()
    names = [k for k, _ in model.named_parameters()]
    return got, {k: float(v) for k, v in ol.items()}, {k: Wg[k].grad for k in names}, names


def test_campnet_losses_and_gradients_match_the_oracle_at_the_bench_size(dev, campnet_step):
    """CampNet at B=16, T=800 (the bench shape): losses to 2e-5; every gradient element to 2e-3 of the tensor's largest
    entry (the bar of the tiny CampNet gradient test) and every tensor norm-wise to 2e-3."""
    got, ref_l, ref_g, _ = campnet_step
    got_l, got_g = got["f32"]
    assert set(got_l) == set(ref_l)
    for k, ref in ref_l.items():
        assert abs(got_l[k] - ref) < 2e-5 * max(1.0, abs(ref)), (k, got_l[k], ref)
    rows = []
    for k, got in got_g.items():
        want = ref_g[k]
        if want is None or got is None:
            assert want is None and (got is None or float(got.abs().max()) == 0.0), k
            continue
        a, b = got.cpu().double(), want.double()
        rows.append((_rel(got, want), float((a - b).norm() / (b.norm() + 1e-30)), float(b.abs().max()), k))
    assert len(rows) > 50
    rows.sort(reverse=True)
    for r in rows[:6]:
        print("max-rel %.3e  norm-rel %.3e  |g|max %.3e  %s" % r)
    for mx, nr, _, k in rows:
        assert mx < 2e-3 and nr < 2e-3, (k, mx, nr)


def test_campnet_bf16_losses_and_gradients_are_within_the_bf16_bars_of_the_oracle(dev, campnet_step):
    """The bf16 CampNet step at B=16, T=800 against the same float64 oracle, with the bars of test_gpu_bf16."""
    got, ref_l, ref_g, names = campnet_step
    l16, g16 = got["bf16"]
    for k, ref in ref_l.items():
        assert abs(l16[k] - ref) < BF16_LOSS_REL * max(1.0, abs(ref)), (k, l16[k], ref)
    assert any(l16[k] != got["f32"][0][k] for k in l16)  # bf16 really ran
    rows, rel_all = _bf16_rows(names, ref_g, g16)
    worst_rel, worst_cos = rows[0][0], min(r[1] for r in rows)
    print("CampNet bf16 vs oracle at B=%d: all-gradient rel %.3e, worst tensor rel %.3e, worst cos %.6f" % (B_CAMPNET, rel_all, worst_rel, worst_cos))
    for r in rows[:6]:
        print("   rel %.3e cos %.6f |g| %.3e  %s" % r)
    assert rel_all < BF16_GRAD_REL_ALL and worst_rel < BF16_GRAD_REL and worst_cos > BF16_GRAD_COS, (rel_all, worst_rel, worst_cos)
