"""STOI cost: hipEvent times of metrics.stoi and of each of its four launches at B=64, N=800*256 samples, of one metrics.stoi call cut into
contiguous event segments between its launches, and, in the same process, of the log-mel launch at the same B, N and of the HiFi-GAN V1
generator forward at B=64, T=800.  One JSON line, also written to profiles/stoi_bench_b64_t800.json.  `bands_over_log_mel` is the band
launch over the log-mel launch of the same run: the band launch issues 14/17 of its GEMM-1 instructions (2 signals x 7 chunks against
17) and a third of its GEMM 2 per chunk.
  python tools/stoi_bench.py"""
import json
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd import metrics, ops  # noqa: E402
from set_amd.hifigan import HifiGanGenerator  # noqa: E402
from set_amd.melspec import LogMel  # noqa: E402

V1 = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
B, T, REPS = int(os.environ.get("MB_B", 64)), int(os.environ.get("MB_T", 800)), int(os.environ.get("MB_REPS", 20))
N = T * 256
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
ref = (0.3 * torch.randn(B, N, device=dev)).clamp(-1.0, 1.0)
ref[:, N // 3: N // 3 + N // 8] *= 1e-4  # a silent stretch: an eighth of the frames is removed
deg = ref + 0.1 * torch.randn(B, N, device=dev)
win, table, basis, nbins = metrics._stoi_images(metrics.STOI_SR, dev)
f_max, S, T_env = ops.stoi_sizes(N)
out = {"metric": "STOI vs the log-mel launch and the HiFi-GAN V1 forward", "B": B, "N": N, "reps": REPS, "energy_frames": f_max,
       "compacted_samples": S, "envelope_frames": T_env, "bins": nbins, "chunks": (nbins + 31) // 32}

ms, (d, valid) = timed(lambda: metrics.stoi(ref, deg), REPS)
out["stoi_ms"] = round(ms, 4)
out["valid"] = int(valid.sum())
out["d_mean"] = round(float(metrics.stoi_mean(d, valid)), 6)

# the four launches, each alone on the outputs of the one before
kept, K, nrm = ops.stoi_select(ref, win)
sil, sil_len = ops.stoi_compact(ref, deg, win, kept, K)
tob = ops.stoi_bands(sil, table, basis, sil_len, n_bands=metrics.STOI_BANDS, bin_lo=0, nbins=nbins)
out["kept_frames_mean"] = round(float(K.float().mean()), 1)
ms, _ = timed(lambda: ops.stoi_select(ref, win, nrm=nrm, kept=kept, K=K), REPS)
out["select_ms"] = round(ms, 4)
ms, _ = timed(lambda: ops.stoi_compact(ref, deg, win, kept, K, sil=sil, sil_len=sil_len), REPS)
out["compact_ms"] = round(ms, 4)
ms, _ = timed(lambda: ops.stoi_bands(sil, table, basis, sil_len, n_bands=metrics.STOI_BANDS, bin_lo=0, nbins=nbins, tob=tob), REPS)
out["bands_ms"] = round(ms, 4)
out["bands_gemm1_tflops"] = round(2.0 * 2 * ((nbins + 31) // 32 * 32) * 1024 * float((2 * (K - 1)).clamp(min=0).sum()) * 2 / ms / 1e9, 1)
ms, _ = timed(lambda: ops.stoi_score(tob, sil_len[:B]), REPS)
out["score_ms"] = round(ms, 4)

# one metrics.stoi call cut into contiguous segments: events between its launches (allocations included), averaged over REPS calls
seg = [0.0] * 4
for _ in range(REPS):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    kept_, K_, _ = ops.stoi_select(ref, win)
    ev[1].record()
    sil_, len_ = ops.stoi_compact(ref, deg, win, kept_, K_)
    ev[2].record()
    tob_ = ops.stoi_bands(sil_, table, basis, len_, n_bands=metrics.STOI_BANDS, bin_lo=0, nbins=nbins)
    ev[3].record()
    ops.stoi_score(tob_, len_[:B])
    ev[4].record()
    torch.cuda.synchronize()
    for i in range(4):
        seg[i] += ev[i].elapsed_time(ev[i + 1]) / REPS
out["segments_ms"] = dict(zip(("select", "compact", "bands", "score"), (round(s, 4) for s in seg)))
out["segments_sum_ms"] = round(sum(seg), 4)

fe = LogMel(HP, "librosa")
ms, mel = timed(lambda: fe(ref), REPS)
out["log_mel_ms"] = round(ms, 4)
out["log_mel_chunks"] = (fe.nbins + 31) // 32
out["bands_over_log_mel"] = round(out["bands_ms"] / ms, 4)
g = HifiGanGenerator(V1).to(dev).eval()
mel_in = torch.randn(B, 80, T, device=dev)
ms, _ = timed(lambda: g(mel_in), 3)
out["hifigan_v1_forward_ms"] = round(ms, 3)
out["stoi_over_forward"] = round(out["stoi_ms"] / ms, 5)
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "stoi_bench_b64_t800.json"), "w") as f:
    f.write(line + "\n")
