"""Multi-resolution STFT loss cost: hipEvent time of vocoder_losses.MultiResolutionSTFTLoss forward + backward (gradient in the second
argument, the task's case, upstream pair (1, 1)) at B=64, N=800*256 (the shape the other tools use, with the HiFi-GAN V1 generator
forward beside it for scale) and at B=64, N=8192 (a vocoder training segment), against the same loss as torch.stft + elementwise ops
under autograd on the same GPU in the same process, written here from the formula (centred reflect-padded Hann STFT at the three
resolutions, sqrt(clamp(re^2 + im^2, 1e-7)), Frobenius-norm ratio and mean |log difference|, means over the resolutions).  The baseline
runs three times; the spread of those is the margin a comparison has to clear.  Both backward variants are timed: the other signal's
magnitudes kept by the forward (the default) and its spectrum computed again (recompute=True); and per resolution the launches on their
own.  One JSON line, also written to profiles/ms_stft_bench_b64.json.
  python tools/ms_stft_bench.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd import ops  # noqa: E402
from set_amd.hifigan import HifiGanGenerator  # noqa: E402
from set_amd.vocoder_losses import MultiResolutionSTFTLoss  # noqa: E402

V1 = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
B, REPS = int(os.environ.get("MB_B", 64)), int(os.environ.get("MB_REPS", 5))
dev = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


kept_fn, again_fn = MultiResolutionSTFTLoss(), MultiResolutionSTFTLoss(recompute=True)
GEOS = kept_fn.geometries
windows = [torch.hann_window(g[2], device=dev) for g in GEOS]


def torch_loss(x, y):
    sc = mg = 0.0
    for g, w in zip(GEOS, windows):
        def mag(s):
            z = torch.stft(s, g[0], g[1], g[2], w, return_complex=True)
            return torch.sqrt(torch.clamp(z.real ** 2 + z.imag ** 2, min=1e-7)).transpose(2, 1)
        xm, ym = mag(x), mag(y)
        sc = sc + torch.norm(ym - xm, p="fro") / torch.norm(ym, p="fro")
        mg = mg + torch.nn.functional.l1_loss(torch.log(ym), torch.log(xm))
    return sc / len(GEOS), mg / len(GEOS)


def one_shape(n):
    torch.manual_seed(0)
    y = 0.3 * torch.randn(B, n, device=dev)
    y_hat = (y + 0.02 * torch.randn(B, n, device=dev)).requires_grad_(True)

    def run(fn):
        def step():
            y_hat.grad = None
            sc, mg = fn(y, y_hat)
            (sc + mg).backward()
            return y_hat.grad
        return step

    ours, again, baseline = run(kept_fn), run(again_fn), run(torch_loss)
    g_ours, g_base = ours().clone(), baseline().clone()
    rel = float((g_ours - g_base).abs().max() / g_base.abs().max())
    losses = [float(v) for v in kept_fn(y, y_hat.detach())] + [float(v) for v in torch_loss(y, y_hat.detach())]
    base = [timed(baseline, REPS) for _ in range(3)]
    ms, ms_again = timed(ours, REPS), timed(again, REPS)
    # the launches on their own (no autograd around them), per resolution
    w = y_hat.detach()
    one = torch.ones(1, device=dev)
    tables = kept_fn._tables(dev)
    parts = {}
    for g, (table, itable) in zip(GEOS, tables):
        kw = dict(n_fft=g[0], hop=g[1], win=g[2])
        _, stats, kept = ops.stft_loss_fwd(y, w, table, which=1, keep=True, **kw)
        parts["%d_%d_%d" % g] = {
            "forward_ms": round(timed(lambda: ops.stft_loss_fwd(y, w, table, which=1, keep=False, **kw), REPS), 4),
            "forward_keeping_magnitudes_ms": round(timed(lambda: ops.stft_loss_fwd(y, w, table, which=1, keep=True, **kw), REPS), 4),
            "backward_kept_ms": round(timed(lambda: ops.stft_loss_bwd(y, w, table, itable, which=1, stats=stats, u_sc=one, u_mag=one, mag=kept,
                                                                     **kw), REPS), 4),
            "backward_recompute_ms": round(timed(lambda: ops.stft_loss_bwd(y, w, table, itable, which=1, stats=stats, u_sc=one, u_mag=one,
                                                                          **kw), REPS), 4),
            "frames": int(ops.stft_sizes(g[0], g[1], g[2], B, n)["T"]),
        }
    return {"N": n, "ms": round(ms, 4), "ms_recompute": round(ms_again, 4), "torch_autograd_ms": [round(b, 4) for b in base],
            "torch_autograd_spread_ms": round(max(base) - min(base), 4), "ratio_to_torch": round(ms / min(base), 4),
            "not_slower": bool(ms <= min(base) + (max(base) - min(base))), "per_resolution": parts,
            "losses_ours_sc_mag_torch_sc_mag": [float("%.6e" % v) for v in losses],
            "max_rel_gradient_difference_to_torch": float("%.3e" % rel)}


out = {"metric": "multi-resolution STFT loss forward + backward vs torch.stft autograd", "B": B, "reps": REPS,
       "resolutions": [list(g) for g in GEOS], "b64_n204800": one_shape(800 * 256), "b64_n8192": one_shape(8192)}
with torch.no_grad():
    g = HifiGanGenerator(V1).to(dev).eval()
    mel_in = torch.randn(B, 80, 800, device=dev)
    out["hifigan_v1_forward_ms"] = round(timed(lambda: g(mel_in), 3), 3)
out["ratio_to_hifigan_forward"] = round(out["b64_n204800"]["ms"] / out["hifigan_v1_forward_ms"], 5)
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ms_stft_bench_b64.json"), "w") as f:
    f.write(line + "\n")
