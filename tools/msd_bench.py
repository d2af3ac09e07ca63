"""Multi-scale discriminator cost on the generator side: hipEvent time of one forward + backward -- MultiScaleDiscriminator (eval mode) on
the real and the generated waveform, a_s + fm_s = generator_loss * lambda_adv + feature_loss, backward to the generated waveform -- at
B=64, N=8192 (a vocoder training segment) and B=8, N=800*256 (the maps of the three scales are about 7.6 GB there), against the same
computation in torch on the same GPU in the same process: float32 F.avg_pool1d + F.conv1d(groups=...) on the weights torch folds from
the module's own parameters (frozen), leaky ReLU and the two losses under autograd.  The baseline runs three times; the spread of those
is the margin a comparison has to clear.  The same step in train() mode (the first scale's power iterations, folds and packs in every forward)
is timed beside it.  Per layer and scale the forward and the input gradient are timed alone and reported as
TFLOP/s.  One JSON line, also written to profiles/msd_bench_b64.json.
  python tools/msd_bench.py
MB_MODE=profile runs only this project's step (the command for `rocprofv3 --kernel-trace --stats --output-format csv`, a run of its
own); MB_STATS_CSV=<that run's kernel stats csv> adds the per-kernel split to the JSON.  MB_SHAPES (B:N pairs), MB_REPS change the shapes."""
import csv
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import set_amd  # noqa: E402,F401
from set_amd import ops  # noqa: E402
from set_amd.discriminators import LRELU_SLOPE, MultiScaleDiscriminator, feature_loss, generator_loss  # noqa: E402

REPS = int(os.environ.get("MB_REPS", 5))
SHAPES = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("MB_SHAPES", "64:8192,8:204800").split(",")]
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


def torch_nets(msd):
    """Per scale [(weight, bias, stride, padding, groups)] of the baseline: the weights torch folds from the module's parameters
    (spectral norm with the stored u, v as in eval(); weight norm), frozen."""
    nets = []
    for d in msd.discriminators:
        layers = []
        for m in list(d.convs) + [d.conv_post]:
            if d.use_spectral_norm:
                w = m.weight_orig.detach()
                w = w / torch.dot(m.weight_u, w.reshape(w.shape[0], -1).mv(m.weight_v))
            else:
                w = torch._weight_norm(m.weight_v.detach(), m.weight_g.detach(), 0)
            layers.append((w, m.bias.detach(), m.stride[0], m.padding[0], m.groups))
        nets.append(layers)
    return nets


def torch_maps(x, layers):
    maps = []
    for i, (w, b, stride, padding, groups) in enumerate(layers):
        x = F.conv1d(x, w, b, stride=stride, padding=padding, groups=groups)
        maps.append(x if i == len(layers) - 1 else F.leaky_relu_(x, LRELU_SLOPE))
        x = maps[-1]
    return maps


def torch_step_fn(nets):
    def step(y, y_hat):
        adv, fm = 0.0, 0.0
        for i, layers in enumerate(nets):
            if i:
                y, y_hat = F.avg_pool1d(y, 4, 2, 1), F.avg_pool1d(y_hat, 4, 2, 1)
            real, gen = torch_maps(y, layers), torch_maps(y_hat, layers)
            adv = adv + (1 - gen[-1]).square().mean()
            fm = fm + sum((r - g).abs().mean() for r, g in zip(real, gen))
        return adv * (LAMBDA_ADV / len(nets)) + fm * 2
    return step


def ours_step_fn(msd):
    def step(y, y_hat):
        _rs, gs, fr, fg = msd(y, y_hat)
        return generator_loss(gs) * LAMBDA_ADV + feature_loss(fr, fg)
    return step


def layer_table(msd, B, n, reps):
    """Per scale and layer 2..8: frames, forward ms on 2 B rows, dgrad ms on B rows, and their TFLOP/s (multiply-adds x 2)."""
    rows = []
    T = n
    for si, d in enumerate(msd.discriminators):
        if si:
            T = ops.avgpool4s2_out_len(T)
        H = T
        for li, c in enumerate(d._convs):
            Ho = c.out_len(H)
            if li:
                _w, op = c.fixed()
                x = torch.randn(2 * B, c.cin, H, device=dev)
                dz = torch.randn(B, c.cout, Ho, device=dev)
                f_in = x[:B].contiguous()
                fwd = ops.sconv1d_fwd if c.kind == "dense" else ops.gconv1d_fwd
                bwd = ops.sconv1d_dgrad if c.kind == "dense" else ops.gconv1d_dgrad
                t_f = timed(lambda: fwd(x, op, c.mod.bias.data, stride=c.stride, pad=c.pad, slope=LRELU_SLOPE), reps)
                t_b = timed(lambda: bwd(dz, op, H, stride=c.stride, pad=c.pad, f_in=f_in, add=f_in, slope=LRELU_SLOPE), reps)
                fl = 2.0 * c.cout * (c.cin // c.groups) * c.K * Ho
                rows.append({"scale": si, "layer": li + 1, "kind": c.kind, "frames_out": Ho, "fwd_ms": round(t_f, 4), "dgrad_ms": round(t_b, 4),
                             "fwd_tflops": round(fl * 2 * B / t_f / 1e9, 2), "dgrad_tflops": round(fl * B / t_b / 1e9, 2)})
                del x, dz, f_in
            H = Ho
    return rows


def flops(msd, B, n):
    total, T = 0, n
    for si, d in enumerate(msd.discriminators):
        if si:
            T = ops.avgpool4s2_out_len(T)
        H = T
        for c in d._convs:
            H = c.out_len(H)
            total += 2 * c.cout * (c.cin // c.groups) * c.K * H * B * 3
    return total


def one_shape(msd, base, B, n):
    torch.manual_seed(0)
    y = 0.3 * torch.randn(B, 1, n, device=dev)
    y_hat = (y + 0.02 * torch.randn(B, 1, n, device=dev)).requires_grad_(True)

    def run(fn):
        def step():
            y_hat.grad = None
            fn(y, y_hat).backward()
            return y_hat.grad
        return step

    ours = run(ours_step_fn(msd))
    reps = REPS if n <= 16384 else max(2, REPS // 2)
    if MODE == "profile":
        return {"B": B, "N": n, "ms": round(timed(ours, reps), 4)}
    baseline = run(torch_step_fn(base))
    g_ours, g_base = ours().clone(), baseline().clone()
    rel = float((g_ours - g_base).abs().max() / g_base.abs().max())
    med = float((g_ours - g_base).abs().median() / g_base.abs().max())
    with torch.no_grad():
        l_ours, l_base = float(ours_step_fn(msd)(y, y_hat)), float(torch_step_fn(base)(y, y_hat))
    tb = [timed(baseline, reps) for _ in range(3)]
    ms = timed(ours, reps)
    with torch.no_grad():
        fwd_ms = timed(lambda: msd(y, y_hat), reps)
    keep = {k: v.clone() for k, v in msd.state_dict().items()}
    msd.train()   # as the task runs it: two power iterations, two folds and two sets of images for the first scale in every forward
    train_ms = timed(ours, reps)
    msd.eval()
    msd.load_state_dict(keep, strict=True)   # u, v as the baseline's weights were folded with
    fl = flops(msd, B, n)
    out = {"B": B, "N": n, "ms": round(ms, 4), "forward_only_ms": round(fwd_ms, 4), "train_mode_ms": round(train_ms, 4), "torch_autograd_ms": [round(b, 4) for b in tb],
           "torch_autograd_spread_ms": round(max(tb) - min(tb), 4), "ratio_to_torch": round(ms / min(tb), 4),
           "not_slower": bool(ms <= min(tb) + (max(tb) - min(tb))), "conv_tflop_per_step": round(fl / 1e12, 4),
           "conv_tflops_achieved": round(fl / 1e9 / ms, 2), "loss_ours_torch": [float("%.6e" % l_ours), float("%.6e" % l_base)],
           "max_rel_gradient_difference_to_torch": float("%.3e" % rel), "median_rel_gradient_difference_to_torch": float("%.3e" % med)}
    del g_ours, g_base
    torch.cuda.empty_cache()
    if n <= 16384:
        out["layers"] = layer_table(msd, B, n, reps)
    return out


def kernel_split(path):
    """[name, calls, total ms, percent] of the ten longest kernels of a rocprofv3 kernel stats csv."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append([r["Name"][:96], int(r["Calls"]), round(float(r["TotalDurationNs"]) / 1e6, 3), round(float(r["Percentage"]), 2)])
    rows.sort(key=lambda r: -r[2])
    return rows[:10]


torch.manual_seed(1)
msd = MultiScaleDiscriminator().to(dev).train()
with torch.no_grad():  # freshly drawn u, v are far from the leading singular pair (sigma near 0, maps near 1e25): forty power iterations first
    warm = 0.3 * torch.randn(2, 1, 1024, device=dev)
    for _ in range(20):
        msd(warm, warm)
msd.eval()
base = None if MODE == "profile" else torch_nets(msd)
out = {"metric": "MSD generator-side forward + backward (a_s + fm_s -> d/d y_hat) vs torch conv1d(groups) autograd", "reps": REPS,
       "lambda_adv": LAMBDA_ADV}
for B, n in SHAPES:
    out["b%d_n%d" % (B, n)] = one_shape(msd, base, B, n)
    torch.cuda.empty_cache()
stats = os.environ.get("MB_STATS_CSV")
if stats and os.path.exists(stats):
    out["kernel_split_b%d_n%d_profiled_run" % SHAPES[0]] = kernel_split(stats)
line = json.dumps(out)
print(line)
if MODE != "profile":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "msd_bench_b64.json"), "w") as f:
        f.write(line + "\n")
