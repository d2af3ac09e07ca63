"""Mel loss cost: hipEvent time of vocoder_losses.MelSpectrogramLoss forward + backward at B=64, N=800*256 (the shape the other tools
use, with the HiFi-GAN V1 generator forward beside it for scale) and at B=64, N=8192 (a vocoder training segment: 32 frames, half a
tile per row), against torch.stft + matmul + l1_loss under autograd on the same GPU, written here from the formula (clamp, reflect pad of
384, Hann STFT, sqrt(re^2 + im^2 + 1e-9), filterbank, ln(max(., 1e-5)), mean |difference|).  The baseline runs three times; the spread of
those is the margin a comparison has to clear.  Also the shares of the entry points (the copy of both waveforms into one buffer, the
linear mel of its 2 B rows, the loss launch, the three backward launches), each timed on its own.  The largest difference between the
two gradients is reported as seen: both sides are fp32, and wherever |L_hat - L_y| is within rounding of 0 they may pick opposite signs,
which moves a sample by a whole entry's share (the GPU tests compare against a float64 model with those entries named).  One JSON
line, also written to profiles/mel_loss_bench_b64.json.
  python tools/mel_loss_bench.py"""
import json
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd import ops  # noqa: E402
from set_amd.hifigan import HifiGanGenerator  # noqa: E402
from set_amd.melspec import FLAVOURS  # noqa: E402
from set_amd.vocoder_losses import MelSpectrogramLoss  # noqa: E402

V1 = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
B, REPS = int(os.environ.get("MB_B", 64)), int(os.environ.get("MB_REPS", 10))
dev = torch.device("cuda:0")
with open(os.path.join(ROOT, "speech-editing-toolkit_amd", "egs", "spec_denoiser.yaml")) as f:
    HP = yaml.safe_load(f)


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


loss_fn = MelSpectrogramLoss(HP)
fe = loss_fn.fe
basis = torch.from_numpy(fe._basis).to(dev)
window = torch.hann_window(fe.win_length, device=dev)


def torch_mel(w):
    w = torch.nn.functional.pad(torch.clamp(w, -1.0, 1.0).unsqueeze(1), (fe.pad, fe.pad), mode="reflect").squeeze(1)
    spec = torch.stft(w, fe.n_fft, hop_length=fe.hop, win_length=fe.win_length, window=window, center=False, normalized=False,
                      onesided=True, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5))


def one_shape(n):
    torch.manual_seed(0)
    y = (0.3 * torch.randn(B, n, device=dev)).clamp(-1.0, 1.0)
    y_hat = (y + 0.02 * torch.randn(B, n, device=dev)).requires_grad_(True)

    def ours():
        y_hat.grad = None
        loss_fn(y_hat, y).backward()
        return y_hat.grad

    def baseline():
        y_hat.grad = None
        torch.nn.functional.l1_loss(torch_mel(y_hat), torch_mel(y)).backward()
        return y_hat.grad

    g_ours, g_base = ours().clone(), baseline().clone()
    rel = float((g_ours - g_base).abs().max() / g_base.abs().max())
    base = [timed(baseline, REPS) for _ in range(3)]
    ms = timed(ours, REPS)
    # the entry points on their own (no autograd around them)
    table, fb, fb_t, itable = loss_fn._images.get((dev,), lambda old: loss_fn._build_images(dev))
    geo = loss_fn._geometry()
    hg = FLAVOURS["hifigan"]
    front = dict(geo, reflect=1, clamp_input=1, mag_eps=hg["mag_eps"])
    w = y_hat.detach()
    both = torch.cat([w, y])
    mel = ops.mel_linear(both, table, fb, **front)
    mel_hat, mel_y = mel[:B], mel[B:]
    g_mel = ops.mel_loss_fwd(mel_hat, mel_y, floor=hg["floor"], log_scale=1.0)[1]
    parts = {
        "concat_ms": timed(lambda: torch.cat([w, y]), REPS),
        "linear_mel_2b_rows_ms": timed(lambda: ops.mel_linear(both, table, fb, **front), REPS),
        "loss_and_g_mel_ms": timed(lambda: ops.mel_loss_fwd(mel_hat, mel_y, floor=hg["floor"], log_scale=1.0), REPS),
        "backward_3_launches_ms": timed(lambda: ops.mel_loss_bwd(w, g_mel, table, fb_t, itable, mag_eps=hg["mag_eps"], count=g_mel.numel(),
                                                                 **geo), REPS),
    }
    tot = sum(parts.values())
    T = fe.frames(n)
    tiles = B * ((T + 63) // 64)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return {"N": n, "frames": T, "ms": round(ms, 4), "torch_autograd_ms": [round(b, 4) for b in base],
            "torch_autograd_spread_ms": round(max(base) - min(base), 4), "ratio_to_torch": round(ms / min(base), 4),
            "not_slower": bool(ms <= min(base) + (max(base) - min(base))),
            "entry_points_ms": {k: round(v, 4) for k, v in parts.items()}, "entry_point_shares": {k: round(v / tot, 3) for k, v in parts.items()},
            "tiles_of_64_frames_per_signal": tiles, "compute_units": n_cu, "tiles_per_cu": round(tiles / n_cu, 2),
            "frames_per_tile_used": round(T / (64.0 * ((T + 63) // 64)), 3),
            "max_rel_gradient_difference_to_torch": float("%.3e" % rel)}


out = {"metric": "HiFi-GAN mel loss forward + backward vs torch.stft autograd", "B": B, "reps": REPS, "bins": [fe.bin_lo, fe.bin_hi],
       "b64_n204800": one_shape(800 * 256), "b64_n8192": one_shape(8192)}
with torch.no_grad():
    g = HifiGanGenerator(V1).to(dev).eval()
    mel_in = torch.randn(B, 80, 800, device=dev)
    out["hifigan_v1_forward_ms"] = round(timed(lambda: g(mel_in), 3), 3)
out["ratio_to_hifigan_forward"] = round(out["b64_n204800"]["ms"] / out["hifigan_v1_forward_ms"], 5)
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "mel_loss_bench_b64.json"), "w") as f:
    f.write(line + "\n")
