"""The discriminator step's cost: hipEvent time of both discriminators on (y, y_hat.detach()), two discriminator_loss calls and a
backward to every parameter -- MultiPeriodDiscriminator and MultiScaleDiscriminator (train mode, as the task runs them) with
trainable_(), full-size weights -- at B=64, N=8192 (and B=8, N=800*256 with DS_SHAPES=64:8192,8:204800 where it fits), the MPD and the
MSD alone and together, against the same step in torch on the same GPU in the same process: trainable weight_norm / spectral_norm
Conv2d / Conv1d(groups) modules under autograd.  The baseline runs three times; their spread is the margin a comparison has to clear.
Per layer the weight gradient is timed alone and reported as TFLOP/s beside the layer's forward rate from profiles/msd_bench_b64.json
(the MPD's bench keeps no layer table), which does the same FLOPs.  One JSON line, also written to profiles/disc_step_bench_b64.json.
  python tools/disc_step_bench.py
DS_MODE=profile runs only this project's step (for `rocprofv3 --kernel-trace --stats`, a run of its own); DS_STATS_CSV=<that run's
kernel stats csv> adds the per-kernel split.  DS_SHAPES (B:N pairs), DS_REPS change the shapes."""
import csv
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm, weight_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd import ops  # noqa: E402
from set_amd.discriminators import (LRELU_SLOPE, MSD_CHANNELS, MSD_GROUPS, PERIODS, MultiPeriodDiscriminator,  # noqa: E402
                                    MultiScaleDiscriminator, discriminator_loss)

REPS = int(os.environ.get("DS_REPS", 5))
SHAPES = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("DS_SHAPES", "64:8192").split(",")]
MODE = os.environ.get("DS_MODE", "bench")
dev = torch.device("cuda:0")
_K, _S = (15, 41, 41, 41, 41, 41, 5), (1, 2, 2, 4, 4, 1, 1)


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


class TorchP(nn.Module):
    def __init__(self, period):
        super().__init__()
        self.period = period
        ch = [1, 32, 128, 512, 1024, 1024]
        self.convs = nn.ModuleList([weight_norm(nn.Conv2d(ch[i], ch[i + 1], (5, 1), (3 if i < 4 else 1, 1), padding=(2, 0))) for i in range(5)])
        self.conv_post = weight_norm(nn.Conv2d(1024, 1, (3, 1), 1, padding=(1, 0)))

    def forward(self, x):
        b, c, t = x.shape
        if t % self.period:
            x = F.pad(x, (0, self.period - t % self.period), "reflect")
        x = x.view(b, c, -1, self.period)
        for layer in self.convs:
            x = F.leaky_relu(layer(x), LRELU_SLOPE)
        return torch.flatten(self.conv_post(x), 1, -1)


class TorchS(nn.Module):
    def __init__(self, spectral):
        super().__init__()
        norm = spectral_norm if spectral else weight_norm
        ch = [1] + list(MSD_CHANNELS)
        self.convs = nn.ModuleList([norm(nn.Conv1d(ch[j], ch[j + 1], _K[j], _S[j], groups=MSD_GROUPS[j], padding=(_K[j] - 1) // 2)) for j in range(7)])
        self.conv_post = norm(nn.Conv1d(ch[7], 1, 3, 1, padding=1))

    def forward(self, x):
        for layer in self.convs:
            x = F.leaky_relu(layer(x), LRELU_SLOPE)
        return torch.flatten(self.conv_post(x), 1, -1)


class TorchDisc(nn.Module):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.discriminators = nn.ModuleList([TorchP(p) for p in PERIODS] if kind == "mpd" else [TorchS(i == 0) for i in range(3)])

    def forward(self, y, y_hat):
        rs, gs = [], []
        for i, d in enumerate(self.discriminators):
            if self.kind == "msd" and i:
                y, y_hat = F.avg_pool1d(y, 4, 2, 1), F.avg_pool1d(y_hat, 4, 2, 1)
            rs.append(d(y))
            gs.append(d(y_hat))
        return rs, gs


def torch_loss(rs, gs):
    return sum((1 - a).square().mean() for a in rs) / len(rs) + sum(a.square().mean() for a in gs) / len(gs)


def step_of(nets, ours):
    params = [q for n in nets for q in n.parameters()]

    def step(y, y_hat):
        for q in params:
            q.grad = None
        total = 0.0
        for n in nets:
            if ours:
                rs, gs, _fr, _fg = n(y, y_hat)
                r, f = discriminator_loss(rs, gs)
                total = total + r + f
            else:
                total = total + torch_loss(*n(y, y_hat))
        total.backward()
    return step, params


def wgrad_table(B, n, reps, fwd_rates):
    """Per discriminator and layer 2..: rows, frames, weight-gradient ms over all rows and its TFLOP/s (multiply-adds x 2)."""
    rows = []
    for p in PERIODS:
        H, ch = -(-n // p), [1, 32, 128, 512, 1024, 1024, 1]
        H = ops.sconv_out_len(H, 5, 3, 2)
        for li in range(1, 6):
            K, s, pad = (5, 3 if li < 4 else 1, 2) if li < 5 else (3, 1, 1)
            Ho, R = ops.sconv_out_len(H, K, s, pad), 2 * B * p
            x, dz = torch.randn(R, ch[li], H, device=dev), torch.randn(R, ch[li + 1], Ho, device=dev)
            t = timed(lambda: ops.gconv1d_wgrad(dz, x, K, stride=s, pad=pad, want_db=True), reps)
            fl = 2.0 * ch[li] * ch[li + 1] * K * Ho * R
            rows.append({"net": "mpd", "period": p, "layer": li + 1, "rows": R, "frames_out": Ho, "slices": ops.gconv_wgrad_plan(R, ch[li], ch[li + 1], 1, H, K, s, pad),
                         "wgrad_ms": round(t, 4), "wgrad_tflops": round(fl / t / 1e9, 2)})
            H = Ho
            del x, dz
    T, ch = n, [1] + list(MSD_CHANNELS) + [1]
    ks, ss, gs = _K + (3,), _S + (1,), tuple(MSD_GROUPS) + (1,)
    for si in range(3):
        if si:
            T = ops.avgpool4s2_out_len(T)
        H = T
        for li in range(1, 8):
            K, s, G = ks[li], ss[li], gs[li]
            pad = (K - 1) // 2
            Ho, R = ops.gconv_out_len(H, K, s, pad), 2 * B
            x, dz = torch.randn(R, ch[li], H, device=dev), torch.randn(R, ch[li + 1], Ho, device=dev)
            t = timed(lambda: ops.gconv1d_wgrad(dz, x, K, stride=s, pad=pad, groups=G, want_db=True), reps)
            fl = 2.0 * (ch[li] // G) * ch[li + 1] * K * Ho * R
            row = {"net": "msd", "scale": si, "layer": li + 1, "rows": R, "frames_out": Ho, "slices": ops.gconv_wgrad_plan(R, ch[li], ch[li + 1], G, H, K, s, pad),
                   "wgrad_ms": round(t, 4), "wgrad_tflops": round(fl / t / 1e9, 2)}
            if (si, li + 1) in fwd_rates:
                row["fwd_tflops_msd_bench"] = fwd_rates[(si, li + 1)]
            rows.append(row)
            H = Ho
            del x, dz
    return rows


def kernel_split(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append([r["Name"][:96], int(r["Calls"]), round(float(r["TotalDurationNs"]) / 1e6, 3), round(float(r["Percentage"]), 2)])
    rows.sort(key=lambda r: -r[2])
    return rows[:12]


torch.manual_seed(1)
mpd, msd = MultiPeriodDiscriminator().to(dev), MultiScaleDiscriminator().to(dev).train()
with torch.no_grad():  # freshly drawn u, v are far from the leading singular pair: forty power iterations first
    warm = 0.3 * torch.randn(2, 1, 1024, device=dev)
    for _ in range(20):
        msd(warm, warm)
mpd.trainable_(), msd.trainable_()
base = {}
if MODE != "profile":
    for kind, net in (("mpd", mpd), ("msd", msd)):
        base[kind] = TorchDisc(kind).to(dev).train()
        base[kind].load_state_dict(net.state_dict(), strict=True)
fwd_rates = {}
try:
    with open(os.path.join(ROOT, "profiles", "msd_bench_b64.json")) as f:
        for r in json.load(f)["b64_n8192"]["layers"]:
            fwd_rates[(r["scale"], r["layer"])] = r["fwd_tflops"]
except (OSError, KeyError, ValueError):
    pass
out = {"metric": "discriminator step (MPD + MSD on (y, y_hat.detach()), discriminator_loss, backward to every parameter) vs torch autograd on "
                 "trainable weight_norm / spectral_norm modules", "reps": REPS}
for B, n in SHAPES:
    torch.manual_seed(0)
    y = 0.3 * torch.randn(B, 1, n, device=dev)
    y_hat = y + 0.02 * torch.randn(B, 1, n, device=dev)
    res = {"B": B, "N": n}
    for name, kinds in (("mpd", ("mpd",)), ("msd", ("msd",)), ("both", ("mpd", "msd"))):
        ours, p_ours = step_of([dict(mpd=mpd, msd=msd)[k] for k in kinds], True)
        entry = {}
        if MODE != "profile":
            keep = {k: v.clone() for k, v in msd.state_dict().items()}
            theirs, p_base = step_of([base[k] for k in kinds], False)
            for k in kinds:
                base[k].load_state_dict(dict(mpd=mpd, msd=msd)[k].state_dict(), strict=True)
            ours(y, y_hat), theirs(y, y_hat)       # one step each from the same weights and buffers: the gradients side by side
            rel = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp_min(1e-30)) for a, b in zip(p_ours, p_base))
            msd.load_state_dict(keep, strict=True)
            tb = [timed(lambda: theirs(y, y_hat), REPS) for _ in range(3)]
            entry.update(torch_autograd_ms=[round(b, 4) for b in tb], torch_autograd_spread_ms=round(max(tb) - min(tb), 4),
                         max_rel_parameter_gradient_difference_to_torch=float("%.3e" % rel))
        ms = [timed(lambda: ours(y, y_hat), REPS) for _ in range(3)]
        entry.update(ms=[round(m, 4) for m in ms])
        if MODE != "profile":
            entry.update(ratio_to_torch=round(min(ms) / min(entry["torch_autograd_ms"]), 4))
        res[name] = entry
        torch.cuda.empty_cache()
    if MODE != "profile" and n <= 16384:
        res["wgrad_layers"] = wgrad_table(B, n, REPS, fwd_rates)
    out["b%d_n%d" % (B, n)] = res
stats = os.environ.get("DS_STATS_CSV")
if stats and os.path.exists(stats):
    out["kernel_split_b%d_n%d_profiled_run" % SHAPES[0]] = kernel_split(stats)
line = json.dumps(out)
print(line)
if MODE != "profile":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "disc_step_bench_b64.json"), "w") as f:
        f.write(line + "\n")
