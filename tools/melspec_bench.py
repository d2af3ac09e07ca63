"""Log-mel front end cost: hipEvent time of melspec.LogMel at B=64, N=800*256 samples (both flavours, shipped hparams) and, for scale, the
HiFi-GAN V1 generator forward at B=64, T=800 in the same process.  One JSON line; `ratio_librosa` must stay at or below 0.05.
  python tools/melspec_bench.py"""
import json
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd.hifigan import HifiGanGenerator  # noqa: E402
from set_amd.melspec import LogMel  # noqa: E402

V1 = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
B, T, REPS = int(os.environ.get("MB_B", 64)), int(os.environ.get("MB_T", 800)), int(os.environ.get("MB_REPS", 20))
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
with open(os.path.join(ROOT, "speech-editing-toolkit_amd", "egs", "spec_denoiser.yaml")) as f:
    HP = yaml.safe_load(f)


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
wav = (0.3 * torch.randn(B, T * 256, device=dev)).clamp(-1.0, 1.0)
out = {"metric": "log-mel front end vs HiFi-GAN V1 forward", "B": B, "N": T * 256, "reps": REPS, "tile_frames": 64,
       "lds_bytes_per_block": 256 * 67 * 4}
for flavour in ("librosa", "hifigan"):
    fe = LogMel(HP, flavour)
    ms, mel = timed(lambda: fe(wav), REPS)
    gemm1 = 2.0 * 2 * ((fe.nbins + 31) // 32 * 32) * 1024 * B * mel.shape[1]
    out[flavour] = {"ms": round(ms, 4), "frames": int(mel.shape[1]), "bins": [fe.bin_lo, fe.bin_hi], "gemm1_tflops": round(gemm1 / ms / 1e9, 1),
                    "finite": bool(torch.isfinite(mel).all())}
g = HifiGanGenerator(V1).to(dev).eval()
mel_in = torch.randn(B, 80, T, device=dev)
ms, wav_out = timed(lambda: g(mel_in), 3)
out["hifigan_v1_forward_ms"] = round(ms, 3)
out["ratio_librosa"] = round(out["librosa"]["ms"] / ms, 5)
out["ratio_hifigan"] = round(out["hifigan"]["ms"] / ms, 5)
out["within_5_percent"] = out["ratio_librosa"] <= 0.05
print(json.dumps(out))
