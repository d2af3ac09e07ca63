"""Wav-level MCD cost: hipEvent times at B=64, N=800*256 samples of metrics.htk_mfcc, both modes of metrics.wav_mcd_htk and
metrics.eval_wav_pairs, of each launch of htk_mfcc alone, and, in the same process, of the log-mel launch at the same B, N and of the
HiFi-GAN V1 generator forward at B=64, T=800.  One JSON line, also written to profiles/wav_mcd_bench_b64_t800.json.
`db_mel_over_log_mel` is set_db_mel over the log-mel launch of the same run: the same kernel body over the same 12 bin chunks (the shipped
hparams end the filterbank at 7.6 kHz too), one frame more per row, a power where the log-mel takes a square root.
  python tools/wav_mcd_bench.py"""
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
ref[:, N // 3: N // 3 + N // 8] *= 1e-4  # a silent stretch, as in tools/stoi_bench.py
est = ref + 0.1 * torch.randn(B, N, device=dev)
est_short = est[:, :N - 9 * 256].contiguous()  # the DTW mode's partner: nine frames fewer
table, basis, lo, nbins, n_mels = metrics._htk_images(dev)
out = {"metric": "wav-level MCD vs the log-mel launch and the HiFi-GAN V1 forward", "B": B, "N": N, "reps": REPS, "frames": 1 + N // 256,
       "bins": nbins, "chunks": (nbins + 31) // 32}

ms, c = timed(lambda: metrics.htk_mfcc(ref), REPS)
out["htk_mfcc_ms"] = round(ms, 4)
ms, (mcd, valid) = timed(lambda: metrics.wav_mcd_htk(ref, est), REPS)
out["wav_mcd_htk_ms"] = round(ms, 4)
out["valid"] = int(valid.sum())
out["mcd_mean"] = round(float(metrics.mcd_mean(mcd, valid)), 6)
ms, (mcd_d, valid_d) = timed(lambda: metrics.wav_mcd_htk(ref, est_short, use_dtw=True), 3)
out["wav_mcd_htk_dtw_ms"] = round(ms, 3)
out["mcd_dtw_mean"] = round(float(metrics.mcd_mean(mcd_d, valid_d)), 6)
ms, both = timed(lambda: metrics.eval_wav_pairs(ref, est), REPS)
out["eval_wav_pairs_ms"] = round(ms, 4)
out["stoi_mean"] = round(float(both["stoi"]), 6)

# the launches of htk_mfcc and the distance, each alone on the outputs of the one before
tab = torch.from_numpy(metrics.dct_ortho_table(metrics.HTK_MFCC, n_mels)).to(dev)
db = ops.db_mel(ref, table, basis, n_mels=n_mels, bin_lo=lo, nbins=nbins)
peak = ops.db_peak(db)
c2 = metrics.htk_mfcc(est)
ms, _ = timed(lambda: ops.db_mel(ref, table, basis, n_mels=n_mels, bin_lo=lo, nbins=nbins, out=db), REPS)
out["db_mel_ms"] = round(ms, 4)
out["db_mel_gemm1_tflops"] = round(2.0 * 2 * ((nbins + 31) // 32 * 32) * 1024 * B * (1 + N // 256) / ms / 1e9, 1)
ms, _ = timed(lambda: ops.db_peak(db, peak=peak), REPS)
out["db_peak_ms"] = round(ms, 4)
ms, _ = timed(lambda: ops.db_mfcc(db, tab, peak, out=c), REPS)
out["db_mfcc_ms"] = round(ms, 4)
ms, _ = timed(lambda: ops.coef_rms_dist(c, c2, mcd=mcd, valid=valid), REPS)
out["coef_rms_dist_ms"] = round(ms, 4)

fe = LogMel(HP, "librosa")
ms, mel = timed(lambda: fe(ref), REPS)
out["log_mel_ms"] = round(ms, 4)
out["log_mel_chunks"] = (fe.nbins + 31) // 32
out["db_mel_over_log_mel"] = round(out["db_mel_ms"] / ms, 4)
g = HifiGanGenerator(V1).to(dev).eval()
mel_in = torch.randn(B, 80, T, device=dev)
ms, _ = timed(lambda: g(mel_in), 3)
out["hifigan_v1_forward_ms"] = round(ms, 3)
out["wav_mcd_htk_over_forward"] = round(out["wav_mcd_htk_ms"] / ms, 5)
out["eval_wav_pairs_over_forward"] = round(out["eval_wav_pairs_ms"] / ms, 5)
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "wav_mcd_bench_b64_t800.json"), "w") as f:
    f.write(line + "\n")
