"""Multi-period discriminator cost on the generator side: hipEvent time of one forward + backward -- MultiPeriodDiscriminator on the
real and the generated waveform, a_p + fm_f = generator_loss * lambda_adv + feature_loss, backward to the generated waveform -- at B=64,
N=8192 (a vocoder training segment) and B=64, N=800*256, against the same computation in torch on the same GPU in the same process:
F.pad(reflect) to a multiple of the period, a reshape to [B, 1, H, p], float32 F.conv2d with (K, 1) kernels on the weights torch folds from
the module's own parameters (frozen), leaky ReLU and the two losses under autograd.  The baseline runs three times; the spread of those is
the margin a comparison has to clear.  At the small shape the same step also runs in float64 (torch): each fp32 gradient against it, and
the count of gate and sign decisions that fall differently between the evaluations.  One JSON line, also written to profiles/mpd_bench_b64.json.
  python tools/mpd_bench.py
MB_MODE=profile runs only this project's step (the command for `rocprofv3 --kernel-trace --stats --output-format csv`, a run of its
own); MB_STATS_CSV=<that run's kernel stats csv> adds the per-kernel split to the JSON.  MB_B, MB_SHAPES, MB_REPS change the shapes."""
import csv
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd.discriminators import LRELU_SLOPE, PERIODS, MultiPeriodDiscriminator, feature_loss, generator_loss  # noqa: E402

B, REPS = int(os.environ.get("MB_B", 64)), int(os.environ.get("MB_REPS", 5))
SHAPES = [int(v) for v in os.environ.get("MB_SHAPES", "8192,204800").split(",")]
MODE = os.environ.get("MB_MODE", "bench")
LAMBDA_ADV = 4.0
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


def torch_nets(mpd, dtype=torch.float32):
    """Per period (period, [(weight, bias, stride, padding)]) of the baseline: the module's weight-normed parameters folded by torch, frozen."""
    nets = []
    for d in mpd.discriminators:
        layers = [(torch._weight_norm(m.weight_v.detach().to(dtype), m.weight_g.detach().to(dtype), 0), m.bias.detach().to(dtype), m.stride, m.padding)
                  for m in list(d.convs) + [d.conv_post]]
        nets.append((d.period, layers))
    return nets


def torch_maps(wave, period, layers):
    """The six maps [B, C, H, period] of one signal: F.pad to a multiple of the period, reshape, conv2d chain; the last has no activation."""
    x = F.pad(wave, (0, -wave.shape[-1] % period), mode="reflect").unflatten(-1, (-1, period))
    maps = []
    for i, (w, b, stride, padding) in enumerate(layers):
        x = F.conv2d(x, w, b, stride=stride, padding=padding)
        maps.append(x if i == len(layers) - 1 else F.leaky_relu_(x, LRELU_SLOPE))
        x = maps[-1]
    return maps


def torch_step_fn(nets, keep=None):
    """a_p * lambda_adv + fm_f from torch's own ops; `keep` (a list) receives every (real, generated) map pair."""
    def step(y, y_hat):
        adv, fm = 0.0, 0.0
        for period, layers in nets:
            real, gen = torch_maps(y, period, layers), torch_maps(y_hat, period, layers)
            adv = adv + (1 - gen[-1]).square().mean()
            fm = fm + sum((r - g).abs().mean() for r, g in zip(real, gen))
            if keep is not None:
                keep.extend((r.detach(), g.detach()) for r, g in zip(real, gen))
        return adv * (LAMBDA_ADV / len(nets)) + fm * 2
    return step


def decision_flips(pairs_a, pairs_b):
    """How many gate (generated map > 0; the sixth map has none) and sign (generated - real) decisions differ between two evaluations."""
    gate = sign = entries = 0
    for k, ((ra, ga), (rb, gb)) in enumerate(zip(pairs_a, pairs_b)):
        sign += int((torch.sign(ga - ra) != torch.sign(gb - rb)).sum())
        if k % 6 != 5:
            gate += int(((ga > 0) != (gb > 0)).sum())
        entries += ga.numel()
    return {"gate_flips": gate, "sign_flips": sign, "map_entries": entries}


def ours_step_fn(mpd):
    def step(y, y_hat):
        _rs, gs, fr, fg = mpd(y, y_hat)
        return generator_loss(gs) * LAMBDA_ADV + feature_loss(fr, fg)
    return step


def flops(n):
    """Multiply-adds x 2 of the convolutions: forward on both signals, input gradient on the generated one."""
    total = 0
    for p in PERIODS:
        H = -(-n // p)
        chans = [1, 32, 128, 512, 1024, 1024]
        for j in range(6):
            cin, cout, K, s, pad = (chans[j], chans[j + 1], 5, 3 if j < 4 else 1, 2) if j < 5 else (1024, 1, 3, 1, 1)
            Ho = (H + 2 * pad - K) // s + 1
            total += 2 * cin * cout * K * Ho * B * p * 3
            H = Ho
    return total


def one_shape(mpd, base, n):
    torch.manual_seed(0)
    y = 0.3 * torch.randn(B, 1, n, device=dev)
    y_hat = (y + 0.02 * torch.randn(B, 1, n, device=dev)).requires_grad_(True)

    def run(fn):
        def step():
            y_hat.grad = None
            fn(y, y_hat).backward()
            return y_hat.grad
        return step

    ours = run(ours_step_fn(mpd))
    if MODE == "profile":
        return {"N": n, "ms": round(timed(ours, REPS), 4)}
    baseline = run(torch_step_fn(base))
    g_ours, g_base = ours().clone(), baseline().clone()
    rel = float((g_ours - g_base).abs().max() / g_base.abs().max())
    with torch.no_grad():
        l_ours, l_base = float(ours_step_fn(mpd)(y, y_hat)), float(torch_step_fn(base)(y, y_hat))
    extra = {}
    if n <= 16384:
        # where the two fp32 gradients part: the same step in float64 (torch), each fp32 path against it, and the decisions -- gates and
        # signs -- that fall differently between the two fp32 paths and between each of them and float64
        y64, yh64 = y.double(), y_hat.detach().double().requires_grad_(True)
        maps64, maps32 = [], []
        torch_step_fn(torch_nets(mpd, torch.float64), maps64)(y64, yh64).backward()
        g64 = yh64.grad
        with torch.no_grad():
            torch_step_fn(base, maps32)(y, y_hat)
            rs, gs, fr, fg = mpd(y, y_hat)
        ours32 = [(r, g) for dr, dg in zip(fr, fg) for r, g in zip(dr, dg)]
        top = float(g64.abs().max())
        extra = {"max_gradient_difference_to_float64_over_largest_entry": {"ours": float("%.3e" % (float((g_ours.double() - g64).abs().max()) / top)),
                                                                            "torch_fp32": float("%.3e" % (float((g_base.double() - g64).abs().max()) / top))},
                 "median_gradient_difference_to_float64_over_largest_entry": {
                     "ours": float("%.3e" % (float((g_ours.double() - g64).abs().median()) / top)),
                     "torch_fp32": float("%.3e" % (float((g_base.double() - g64).abs().median()) / top))},
                 "decisions_ours_vs_torch_fp32": decision_flips(ours32, maps32),
                 "decisions_ours_vs_float64": decision_flips(ours32, maps64),
                 "decisions_torch_fp32_vs_float64": decision_flips(maps32, maps64)}
        del maps64, maps32, ours32, rs, gs, fr, fg, g64, y64, yh64
        torch.cuda.empty_cache()
    reps = REPS if n <= 16384 else max(2, REPS // 2)
    tb = [timed(baseline, reps) for _ in range(3)]
    ms = timed(ours, reps)
    with torch.no_grad():
        fwd_ms = timed(lambda: mpd(y, y_hat), reps)
    return {"N": n, "ms": round(ms, 4), "forward_only_ms": round(fwd_ms, 4), "torch_autograd_ms": [round(b, 4) for b in tb],
            "torch_autograd_spread_ms": round(max(tb) - min(tb), 4), "ratio_to_torch": round(ms / min(tb), 4),
            "not_slower": bool(ms <= min(tb) + (max(tb) - min(tb))), "conv_tflop_per_step": round(flops(n) / 1e12, 4),
            "conv_tflops_achieved": round(flops(n) / 1e9 / ms, 2), "loss_ours_torch": [float("%.6e" % l_ours), float("%.6e" % l_base)],
            "max_rel_gradient_difference_to_torch": float("%.3e" % rel), **extra}


def kernel_split(path):
    """[name, calls, total ms, percent] of the ten longest kernels of a rocprofv3 kernel stats csv."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append([r["Name"][:96], int(r["Calls"]), round(float(r["TotalDurationNs"]) / 1e6, 3), round(float(r["Percentage"]), 2)])
    rows.sort(key=lambda r: -r[2])
    return rows[:10]


torch.manual_seed(1)
mpd = MultiPeriodDiscriminator().to(dev)
base = None if MODE == "profile" else torch_nets(mpd)
out = {"metric": "MPD generator-side forward + backward (a_p + fm_f -> d/d y_hat) vs torch Conv2d autograd", "B": B, "reps": REPS,
       "lambda_adv": LAMBDA_ADV}
for n in SHAPES:
    out["b%d_n%d" % (B, n)] = one_shape(mpd, base, n)
    torch.cuda.empty_cache()
stats = os.environ.get("MB_STATS_CSV")
if stats and os.path.exists(stats):
    out["kernel_split_n%d_profiled_run" % SHAPES[0]] = kernel_split(stats)
line = json.dumps(out)
print(line)
if MODE != "profile":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mpd_bench_b64.json"), "w") as f:
        f.write(line + "\n")
