"""Mel-cepstral distortion cost: hipEvent times of metrics.mel_mcd(use_dtw=True), metrics.mel_mcd(use_dtw=False) and set_dtw alone at
B=64, T=800 against 760, K=39 and, for scale, the HiFi-GAN V1 generator forward at B=64, T=800 in the same process.  One JSON line, also
written to profiles/mcd_bench_b64_t800.json; `ratio_dtw` is mel_mcd(use_dtw=True) over the forward and must stay below 1.
  python tools/mcd_bench.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd import metrics, ops  # noqa: E402
from set_amd.hifigan import HifiGanGenerator  # noqa: E402

V1 = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
B, T1, T2 = int(os.environ.get("MB_B", 64)), int(os.environ.get("MB_T", 800)), int(os.environ.get("MB_T2", 760))
K, M, REPS = 39, 80, int(os.environ.get("MB_REPS", 20))
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


torch.manual_seed(0)
mel_1 = torch.randn(B, T1, M, device=dev) - 3.0
mel_2 = torch.randn(B, T2, M, device=dev) - 3.0
c1, c2 = metrics.mfcc(mel_1, n_mfcc=K), metrics.mfcc(mel_2, n_mfcc=K)
out = {"metric": "mel-cepstral distortion vs HiFi-GAN V1 forward", "B": B, "T": [T1, T2], "K": K, "n_mels": M, "reps": REPS,
       "strip_rows": 256, "ring_columns": 320, "lds_bytes_per_block": (320 * 41 + 2 * T2 + 16) * 4}
ms, r = timed(lambda: metrics.mel_mcd(mel_1, mel_2, use_dtw=True), REPS)
out["mel_mcd_dtw_ms"] = round(ms, 4)
out["finite"] = bool(torch.isfinite(r[0]).all())
out["frames_mean"] = round(float(r[2].float().mean()), 1)
ms, r = timed(lambda: metrics.mel_mcd(mel_1, mel_2, use_dtw=False), REPS)
out["mel_mcd_zero_fill_ms"] = round(ms, 4)
ms, _ = timed(lambda: ops.dtw(c1, c2), REPS)
out["set_dtw_ms"] = round(ms, 4)
dir_ = torch.empty(B, T1, T2, dtype=torch.uint8, device=dev)
ms, _ = timed(lambda: ops.dtw(c1, c2, dir=dir_), REPS)
out["set_dtw_with_dir_ms"] = round(ms, 4)
ms, _ = timed(lambda: metrics.mfcc(mel_1, n_mfcc=K), REPS)
out["set_mfcc_ms"] = round(ms, 4)
ms, _ = timed(lambda: ops.dtw(c1[:1], c2[:1]), REPS)
out["set_dtw_one_pair_ms"] = round(ms, 4)
out["cell_updates_per_s"] = round(B * T1 * T2 / (out["set_dtw_ms"] * 1e-3), 0)
g = HifiGanGenerator(V1).to(dev).eval()
mel_in = torch.randn(B, 80, T1, device=dev)
ms, _ = timed(lambda: g(mel_in), 3)
out["hifigan_v1_forward_ms"] = round(ms, 3)
out["ratio_dtw"] = round(out["mel_mcd_dtw_ms"] / ms, 5)
out["below_the_forward"] = out["ratio_dtw"] < 1.0
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "mcd_bench_b64_t800.json"), "w") as f:
    f.write(line + "\n")
