"""Models, case table, checks and fault planters of the teacher-forced training trajectory (test_trajectory_reference.py ties them to
torch and shows which check catches which planted fault; test_gpu_trajectory.py applies them to real optimizer updates on the GPU).
Nothing here touches the GPU and nothing here is a test.

Why teacher-forced.  Comparing the parameters after N updates with a float64 trainer does not work: the first Adam updates are
lr * sign(g), so a rounding-level difference where g ~ 0 moves a parameter by 2 lr.  Instead every update k of a run is checked in isolation
against references that are FED THE RUN'S OWN STATE:

  check 3  forward and gradient at the same weights: the oracle in float64 on leaf copies of the run's p_k, same batch, t and noise; every
           loss and every parameter's gradient (addressed through the optimizer's offsets, in model order); parameters the oracle never
           reaches must hold all-zero gradients.  Bars: the ones the fixture tests already assert (restated below with their source).
           Where a gradient bar is missed the reference is taken again with ReLU units whose branch float32 cannot decide on the other
           branch (undecided_relu_units, references_of_update): at B T = 231 frames one such unit is worth 2.4 bars.  Same bars.
  check 4  the update given the run's own gradient: head_optim_models.adamw in float64 on p_k, g_k, m_k, v_k, Adam step k + 1, the clip
           factor from the float64 sum of squares of g_k; p_{k+1}, m_{k+1}, v_{k+1} over the whole flat buffer within the bar of that
           module's float32 mirror; the pad tail of every buffer stays zero; the returned lr equals lr_at(k) as a Python float.
  check 5  fresh-restart equality, bit for bit: a second task (another random init) loaded with p_k, a new optimizer loaded with m_k, v_k
           and the update count, the same step -- its losses, gradient buffer, p_{k+1}, m_{k+1} and v_{k+1} must equal the continuing
           run's bits.  The fresh run packs every weight image from scratch and goes through the autograd route; the continuing one uses
           re-packed images and the direct gradient sinks.

Update k (0-based) is the (k + 1)-th call of step(): it runs at lr_at(k) and Adam bias-correction step k + 1."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

import head_optim_models as HM
from conftest import load_golden
from oracle import oracle as O
from oracle import weights as Wt

F32, F64 = np.float32, np.float64

N_UPDATES = 5        # updates per case
N_BATCHES = 3        # distinct synthetic batches, cycling: consecutive updates see different data
WARMUP = 2           # update 0 runs at the 1e-7 floor, update 1 on the ramp (lr0 / 2), updates 2.. on the plateau
CLIP = 1.0
BETAS = (0.9, 0.98)  # egs/*.yaml: optimizer_adam_beta1 / beta2
EPS = 1e-8
WD = 0.01            # (the yamls train with 0; a decay that is on also checks its place in the update)


# =====================================================================================================================================
# the schedule, restated (utils/nn/schedulers.py WarmupSchedule in the reference; NOT imported from set_amd.training)
# =====================================================================================================================================
def lr_at(k, lr0, warmup=WARMUP):
    """learning rate of update k (0-based: the number of updates already made)"""
    return max(lr0 * min(k / warmup, 1.0), 1e-7)


# =====================================================================================================================================
# the float64 update (and its float32 mirror): clip_grad_norm_ + AdamW on the flat buffers
# =====================================================================================================================================
UPDATE_FAULTS = ("lr_next", "bias_step_k", "clip_skipped", "moments_reset")


def sumsq64(g):
    return float((np.asarray(g, dtype=F64) ** 2).sum())


def _chunks(n, size=1 << 20):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)] or [slice(0, 0)]


def _threaded(fn, items):
    """fn over items on a few threads (numpy releases the interpreter lock inside its loops); results in order"""
    if len(items) == 1:
        return [fn(items[0])]
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(fn, items))


def update_step(p, g, m, v, k, lr0, grad_scale=1.0, dtype=F64, fault=None, warmup=WARMUP, sumsq=None):
    """update k on numpy vectors -> (p, m, v).  The hyper-parameters are the fp32 values the C ABI passes; the sum of squares is taken in
    float64 whatever `dtype` is (the float32 mirror rounds it once, as the best fp32 reduction would).  The update is elementwise but for
    that sum: handed `sumsq` (of the whole gradient), the vectors may be any subset of the elements (long vectors are updated in chunks)."""
    lr = lr_at(k + 1 if fault == "lr_next" else k, lr0, warmup)
    step = k if fault == "bias_step_k" else k + 1
    sumsq = None if fault == "clip_skipped" else (sumsq64(g) if sumsq is None else sumsq)
    if fault == "moments_reset":
        m, v = np.zeros_like(m), np.zeros_like(v)

    def one(s):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return HM.adamw(p[s], g[s], m[s], v[s], lr=HM.f32f(lr), beta1=HM.f32f(BETAS[0]), beta2=HM.f32f(BETAS[1]), eps=HM.f32f(EPS),
                            wd=HM.f32f(WD), step=step, sumsq=sumsq, max_norm=CLIP, grad_scale=grad_scale, dtype=dtype)
    parts = _threaded(one, _chunks(len(p)))
    return tuple(np.concatenate([q[i] for q in parts]) for i in range(3)) if len(parts) > 1 else parts[0]


def sumsq_bar(n):
    """relative error bound of the optimizer's fp32 sum of squares over n floats, as test_gpu_fullsize_training derives it: a per-thread fma
    chain of ceil(n / (2048 * 256)) terms, a 256-wide tree (8), the partial-row sum (rows / 64 + 2 chain adds + 16 group adds); every term
    is >= 0, so the error is <= depth * u * the sum"""
    return (-(-n // (2048 * 256)) + 8 + 2048 // 64 + 18) * HM.U


def check_update(p, g, m, v, k, lr0, got_p, got_m, got_v, n, got_lr=None, grad_scale=1.0, sumsq=None, got_sumsq=None):
    """check 4 -> {what: largest error / bar}.  All vectors are the whole flat buffers (n parameters + pad), or with `sumsq` the same
    subset of each; `pad` is 0 when the tail of every buffer handed in is zero, else inf; `lr` is 0 when got_lr == lr_at(k, lr0) exactly.
    The bar is head_optim_models.mirror_bar: max(4 x the float32 mirror's largest error on that output, 2 u |value|) per element."""
    sumsq = sumsq64(g[:n]) if sumsq is None else sumsq
    want = update_step(p[:n], g[:n], m[:n], v[:n], k, lr0, grad_scale, sumsq=sumsq)
    mirror = update_step(p[:n], g[:n], m[:n], v[:n], k, lr0, grad_scale, dtype=F32, sumsq=sumsq)
    out = {}
    for name, got, w, mi in zip(("p", "m", "v"), (got_p, got_m, got_v), want, mirror):
        def mirror_err(s):
            d = np.abs(mi[s].astype(F64) - w[s])
            d = d[np.isfinite(d)]
            return float(d.max()) if d.size else 0.0
        err = max(_threaded(mirror_err, _chunks(n)))  # mirror_bar's first term, over the whole output

        def ratio(s):
            bar = np.maximum(HM.BAR_FACTOR * err, 2.0 * HM.U * np.abs(w[s]))
            e = np.abs(np.asarray(got[:n][s], dtype=F64) - w[s])
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(e == 0.0, 0.0, e / bar)
            r = np.where(np.isfinite(r), r, np.inf)
            return float(r.max()) if r.size else 0.0
        out[name] = max(_threaded(ratio, _chunks(n)))
    tails = [a[n:] for a in (p, g, m, v, got_p, got_m, got_v)]
    out["pad"] = 0.0 if all(not np.any(t) for t in tails) else float("inf")
    if got_lr is not None:
        out["lr"] = 0.0 if got_lr == lr_at(k, lr0) else float("inf")
    if got_sumsq is not None:  # the norm the clip was taken on: the run's own reduction of the same buffer
        out["sumsq"] = abs(got_sumsq - sumsq) / (sumsq_bar(len(g)) * sumsq) if sumsq > 0 else (0.0 if got_sumsq == 0 else float("inf"))
    return out


# =====================================================================================================================================
# state dicts <-> oracle leaves <-> flat vectors
# =====================================================================================================================================
class Layout:
    """where each parameter (model order) lives in the flat buffers: names, shapes, offsets, n parameters, n_pad floats"""

    def __init__(self, names, shapes, offs, n_pad=None):
        self.names, self.shapes, self.offs = list(names), [tuple(s) for s in shapes], list(offs)
        self.numels = [int(np.prod(s, dtype=np.int64)) for s in self.shapes]
        self.n = sum(self.numels)
        self.n_pad = (self.n + 255) // 256 * 256 if n_pad is None else int(n_pad)

    @classmethod
    def contiguous(cls, names, shapes):
        offs, off = [], 0
        for s in shapes:
            offs.append(off)
            off += int(np.prod(tuple(s), dtype=np.int64))
        return cls(names, shapes, offs)

    @classmethod
    def of_optimizer(cls, opt):
        return cls(opt.param_names, [p.shape for p in opt.params], opt.offs, opt.flat_p.numel())

    def segments(self):
        return zip(self.names, self.shapes, self.offs, self.numels)


def leaves64(W, dtype=torch.float64):
    """leaf copies of the floating-point entries of a CPU state dict (the others as they are)"""
    return {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in W.items()}


def flatten_grads(layout, grads):
    """{name: tensor or None} -> float64 vector of n_pad in the layout's order (None and the pad: zeros)"""
    flat = np.zeros(layout.n_pad, dtype=F64)
    for name, _, off, n in layout.segments():
        g = grads.get(name)
        if g is not None:
            flat[off:off + n] = g.detach().reshape(-1).double().numpy()
    return flat


def flatten_state(layout, W):
    return flatten_grads(layout, {k: W[k] for k in layout.names})


def unflatten_state(layout, flat, template, dtype=torch.float64):
    """the template state dict with its parameters replaced by the flat vector's segments"""
    W = dict(template)
    for name, shape, off, n in layout.segments():
        W[name] = torch.from_numpy(np.array(flat[off:off + n], dtype=F64)).reshape(shape).to(dtype)
    return W


# =====================================================================================================================================
# cases, batches and the oracle's step
# =====================================================================================================================================
SPEC_FIXTURE, CAMPNET_FIXTURE = "train_losses_ragged", "campnet_ragged"  # B = 3, T = 77, T_txt = 19, padded tails


def _case(name, kind, dtype="f32", env=None, acc=1, detour=False, lr0=1e-3, sinks=True):
    return dict(name=name, kind=kind, dtype=dtype, env=dict(env or {}), acc=acc, detour=detour, lr0=lr0, sinks=sinks)


# env: the environment switches the case sets (monkeypatch.setenv); dtype: ops.set_compute_dtype; acc: micro-batches per update;
# detour: a validation pass and an inference between updates 2 and 3; sinks: whether updates k >= 1 take the direct gradient sinks.
# spec_accumulate2 does not: the optimizer learns on its first update which parameters receive exactly one gradient per update, and with
# two backward passes per update every parameter receives two -- the whole run stays on the autograd route, which the test pins (0 views).
# The stale-by-one fault (forward at p_{k-1}) is at least 10 bars of check 3 from update 2 on in the f32 cases.  The first update (0) has
# no earlier weights and cannot show it; it runs at the 1e-7 floor, so at update 1 the fault is only p_1 - p_0 ~ 1e-7 an element -- the
# oracle still sees that (measured 71 bars for spec_denoiser, 29 for CampNet: 2e7 parameters move the f0 loss by ~1e-7 |g|_1), but with
# less than the factor the GPU test is entitled to rely on.  In the bf16 cases the bars are too loose at any update: check 5 has it.
CASES = [
    _case("spec_per_op", "spec", env={"SET_AMD_TRAIN_STACK": "0"}),
    _case("spec_fused_stack", "spec", env={"SET_AMD_WINO": "2"}, detour=True),  # grouped step projections on (flat optimizer layout)
    _case("spec_bf16", "spec", dtype="bf16", detour=True),
    _case("spec_accumulate2", "spec", acc=2, sinks=False),
    _case("campnet_fp32", "campnet", lr0=2e-3, detour=True),
    _case("campnet_bf16", "campnet", dtype="bf16", lr0=2e-3),
]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)
DETOUR_AFTER = 2  # the detour runs at p_3: after update 2, before update 3


def fixture_meta(kind):
    return load_golden(SPEC_FIXTURE if kind == "spec" else CAMPNET_FIXTURE)["meta"]


def seeded_state(kind):
    """the fixture's seeded weights (float32, CPU) and the parameter names in model order"""
    g = load_golden(SPEC_FIXTURE if kind == "spec" else CAMPNET_FIXTURE)
    m = g["meta"]
    if kind == "spec":
        W = Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), m["wseed"])
    else:
        W = Wt.seeded_weights(Wt.load_manifest("campnet"), m["wseed"])
        W["mask_emb"] = torch.from_numpy(g["mask_emb"])
        W["decoder_coarse.pos_embed_alpha"] = torch.from_numpy(g["pos_embed_alpha"])
    return W, list(m["param_names"])


def batch(kind, i):
    """synthetic batch i (0 .. N_BATCHES - 1) at the fixture's shapes; batch 0 is the fixture's own.  CPU tensors:
    spec: txt_tokens, mel2ph, ref_mels, time_mel_masks [B,T,1], f0, uv, spk_embed, t [B], eps [B,1,80,T], infer_noises [steps+1,B,1,80,T]
    campnet: txt_tokens (the fixture's padded tails on every batch), ref_mels, time_mel_masks [B,T,1]"""
    g = load_golden(SPEC_FIXTURE if kind == "spec" else CAMPNET_FIXTURE)
    m = g["meta"]
    b = dict(Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"] + 17 * i, pad_tail=True))
    if kind == "spec":
        if i == 0:
            b["t"], b["eps"] = torch.from_numpy(g["t"]), torch.from_numpy(g["eps"])
        else:
            gen = torch.Generator().manual_seed(900 + i)
            b["t"] = torch.randint(0, m["steps"], (m["B"],), generator=gen)
            b["eps"] = torch.randn(m["B"], 1, 80, m["T"], generator=gen)
        b["infer_noises"] = torch.stack(Wt.synthetic_noises(m["B"], m["T"], m["steps"], seed=m["iseed"] + 17 * i + 1))
        b["steps"] = m["steps"]
    else:
        gt = torch.from_numpy(g["txt_tokens"])
        b["txt_tokens"] = gt.clone() if i == 0 else b["txt_tokens"] * (gt != 0).long()
    return b


def batches_of_update(case, k):
    """indices of the micro-batches update k consumes"""
    a = case["acc"]
    return [(a * k + j) % N_BATCHES for j in range(a)]


def sample_of(kind, b):
    """the task's `sample` dict (CPU tensors) of a batch"""
    if kind == "spec":
        return dict(txt_tokens=b["txt_tokens"], mels=b["ref_mels"], mel2ph=b["mel2ph"], f0=b["f0"], uv=b["uv"],
                    time_mel_masks=b["time_mel_masks"].squeeze(-1).contiguous(), spk_embed=b["spk_embed"])
    return dict(txt_tokens=b["txt_tokens"], mels=b["ref_mels"], time_mel_masks=b["time_mel_masks"][:, :, 0].contiguous())


def loss_denominators(kind, b):
    """every denominator of a loss of this batch (none may be zero)"""
    tm = b["time_mel_masks"]
    d = {"masked_nonzero_frames": float(((b["ref_mels"] * tm).abs().sum(-1) != 0).sum())}
    if kind == "spec":
        nonpad = (b["mel2ph"] != 0).float()
        d["nonpad_frames"] = float(nonpad.sum())
        d["voiced_frames"] = float((nonpad * (b["uv"] == 0).float()).sum())
        d["nonpad_tokens"] = float((b["txt_tokens"] != 0).sum())
    return d


def _cast(b, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}


class _ReluTap:
    """torch.nn.functional.relu while the oracle runs: records every call's argument, and evaluates the units named in `flips`
    -- (call index, flat index) -- on the other branch (value x or 0 and slope 1 or 0 swapped)"""

    def __init__(self, flips=()):
        self.flips, self.pre, self.real = set(flips), [], None

    def __enter__(self):
        self.real = F.relu
        F.relu = self
        return self

    def __exit__(self, *exc):
        F.relu = self.real

    def __call__(self, x, *a, **k):
        i = len(self.pre)
        self.pre.append(x.detach())
        ids = [u for c, u in self.flips if c == i]
        if not ids:
            return self.real(x, *a, **k)
        mask = (x.detach() > 0).reshape(-1).clone()
        mask[ids] = ~mask[ids]
        return x * mask.reshape(x.shape).to(x.dtype)


def _oracle_losses(kind, Wx, b, bb):
    if kind == "spec":
        return O.training_losses(Wx, b["steps"], bb, b["t"], bb["eps"])[0]
    return O.campnet_losses(Wx, b["txt_tokens"], bb["ref_mels"], bb["time_mel_masks"])[0]


def oracle_step(kind, W, b, dtype=torch.float64, flips=()):
    """losses and gradients of the oracle under torch autograd at the weights W (a CPU state dict) on batch b
    -> ({loss: float}, {parameter name: gradient or None}); flips: see undecided_relu_units"""
    Wg, bb = leaves64(W, dtype), _cast(b, dtype)
    with torch.enable_grad(), _ReluTap(flips):
        losses = _oracle_losses(kind, Wg, b, bb)
        sum(losses.values()).backward()
    return {k: float(v.detach()) for k, v in losses.items()}, {k: v.grad for k, v in Wg.items() if torch.is_tensor(v) and v.is_floating_point()}


def undecided_relu_units(kind, W, b):
    """The ReLU units of the oracle's forward whose branch float32 arithmetic cannot decide at the weights W on batch b: |x| <= 4 x the
    largest difference between a float32 and the float64 evaluation of that ReLU's argument (the rule of every bar here: BAR_FACTOR x the
    float32 mirror's largest error).  -> [(call index, flat index, float64 argument, threshold)].  At such a unit the loss is not
    differentiable to float32 precision and either slope is a correct gradient; at B T = 231 frames ONE unit on the other branch moves a
    predictor weight's gradient by 2.4 of the bars that were set at B T = 25,600 (test_trajectory_reference.py shows it)."""
    taps = []
    for dtype in (torch.float64, torch.float32):
        Wd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in W.items()}
        with torch.no_grad(), _ReluTap() as tap:
            _oracle_losses(kind, Wd, b, _cast(b, dtype))
        taps.append(tap.pre)
    out = []
    for i, (x64, x32) in enumerate(zip(*taps)):
        thr = HM.BAR_FACTOR * float((x32.double() - x64).abs().max())
        for u in torch.nonzero(x64.reshape(-1).abs() <= thr).reshape(-1).tolist():
            out.append((i, u, float(x64.reshape(-1)[u]), thr))
    return out


def oracle_update_inputs(case, W, k, dtype=torch.float64, flips=None):
    """what the oracle makes of update k at weights W: per micro-batch losses and the gradient of the mean over the micro-batches;
    flips: {micro-batch position: units of undecided_relu_units to evaluate on the other branch}"""
    kind, acc = case["kind"], case["acc"]
    losses, grads = [], None
    for j, i in enumerate(batches_of_update(case, k)):
        l, g = oracle_step(kind, W, batch(kind, i), dtype, flips=(flips or {}).get(j, ()))
        losses.append(l)
        if grads is None:
            grads = {n: (None if x is None else x / acc) for n, x in g.items()}
        else:
            for n, x in g.items():
                if x is not None:
                    grads[n] = x / acc if grads[n] is None else grads[n] + x / acc
    return losses, grads


MAX_UNDECIDED = 3  # only the three undecided units closest to zero are tried on the other branch (2^3 - 1 alternative references at most)


def references_of_update(case, W, k):
    """the oracle's reference of update k, then -- lazily, only asked for when the first misses a bar -- the references with undecided ReLU
    units on the other branch: every non-empty subset of the MAX_UNDECIDED closest to zero -> yields (losses, grads, description)"""
    yield oracle_update_inputs(case, W, k) + ("",)
    units = []
    for j, i in enumerate(batches_of_update(case, k)):
        units += [(j, c, u, x, thr) for c, u, x, thr in undecided_relu_units(case["kind"], W, batch(case["kind"], i))]
    units = sorted(units, key=lambda q: abs(q[3]))[:MAX_UNDECIDED]  # the closest to zero: the likeliest to have gone the other way
    subsets = sorted(range(1, 1 << len(units)), key=lambda bits: (bin(bits).count("1"), bits))  # single units first, closest first
    for bits in subsets:
        pick = [units[n] for n in range(len(units)) if bits >> n & 1]
        flips = {}
        for j, c, u, x, thr in pick:
            flips.setdefault(j, []).append((c, u))
        what = ", ".join("micro-batch %d relu call %d unit %d (argument %.2e, float32 decides to +-%.1e)" % q for q in pick)
        yield oracle_update_inputs(case, W, k, flips=flips) + (what,)


def oracle_infer(kind, W, b, dtype=torch.float64):
    """the detour's inference at weights W -> {name: tensor} (spec: mel_out pasted into the original; campnet: coarse, fine, attn)"""
    Wd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in W.items()}
    bb = _cast(b, dtype)
    with torch.no_grad():
        if kind == "spec":
            ret = O.gaussian_diffusion_infer(Wd, b["steps"], bb, list(bb["infer_noises"]))
            tm = bb["time_mel_masks"]
            return {"mel_out": ret["mel_out"] * tm + bb["ref_mels"] * (1 - tm)}
        out = O.campnet_forward(Wd, b["txt_tokens"], bb["ref_mels"], bb["time_mel_masks"])
        return {k: out[k] for k in ("mel_out_coarse", "mel_out_fine", "attn")}


# =====================================================================================================================================
# check 3: the bars the fixture tests assert, restated
# =====================================================================================================================================
# spec_denoiser fp32 (test_gpu_training.test_training_losses_and_all_gradients_match_reference and
# test_gpu_fullsize_training.test_fp32_losses_and_gradients_match_the_oracle_at_the_bench_size)
SPEC_LOSS, SPEC_NORM, SPEC_ELEM_CORE = 2e-5, 1e-3, 2e-4   # losses: * max(1, |ref|); | |g| - |ref| | / |ref|; max|d| / max|ref| (denoise_fn.*, mel_encoder.*)
SPEC_ELEM_ANY, SPEC_DIFF_NORM = 5e-3, 2e-3                # the predictor bars: max|d| / max|ref| and |d| / |ref| of every tensor
# CampNet fp32 (test_gpu_campnet.test_campnet_forward_losses_and_gradients_match_reference)
CAMP_LOSS, CAMP_NORM, CAMP_ELEM = 1e-5, 2e-3, 2e-3
# inference after a load (the fixture tests' bars; the detour holds them after an update): |dmel| fp32, attention rows fp32
INFER_MEL, INFER_ATTN = 1e-4, 1e-5


def bf16_bars():
    from test_gpu_bf16 import BF16_GRAD_COS, BF16_GRAD_REL, BF16_GRAD_REL_ALL, BF16_LOSS_REL, BF16_MEL_MCD
    return dict(loss=BF16_LOSS_REL, rel_all=BF16_GRAD_REL_ALL, rel=BF16_GRAD_REL, cos=BF16_GRAD_COS, mcd=BF16_MEL_MCD)


def check_losses(kind, dtype, ref, got):
    """-> largest |got - ref| / bar over the losses (both dicts must name the same losses)"""
    assert set(ref) == set(got), (sorted(ref), sorted(got))
    bar = bf16_bars()["loss"] if dtype == "bf16" else (SPEC_LOSS if kind == "spec" else CAMP_LOSS)
    worst = 0.0
    for k, r in ref.items():
        d = abs(float(got[k]) - r)
        worst = max(worst, (d / (bar * max(1.0, abs(r)))) if math.isfinite(d) else float("inf"))
    return worst


def check_forward_backward(kind, dtype, layout, ref_losses, ref_grads, got_losses, got_flat):
    """check 3 -> ({what: largest error / bar}, worst tensor name).  ref_losses / got_losses: one dict per micro-batch; ref_grads: the
    oracle's {name: gradient or None}; got_flat: the run's flat gradient buffer (numpy)."""
    assert len(ref_losses) == len(got_losses)
    out = {"loss": max(check_losses(kind, dtype, r, g) for r, g in zip(ref_losses, got_losses))}
    got_flat = torch.as_tensor(np.asarray(got_flat)).double()
    unreached, rows = 0.0, []
    num = den = 0.0
    for name, _, off, n in layout.segments():
        got = got_flat[off:off + n]
        ref = ref_grads.get(name)
        if ref is None or not bool(ref.any()):
            if bool(got.any()):
                unreached = float("inf")
            continue
        ref = ref.detach().reshape(-1).double()
        d = got - ref
        nr, ng, nd, mx, dm = float(ref.norm()), float(got.norm()), float(d.norm()), float(ref.abs().max()), float(d.abs().max())
        if not (math.isfinite(ng) and math.isfinite(nd)):
            rows.append((name, float("inf"), float("inf"), float("inf"), -1.0))
            num = float("inf")
            continue
        cos = float(got @ ref) / (nr * ng) if ng > 0 else -1.0
        rows.append((name, abs(ng - nr) / nr, nd / nr, dm / mx, cos))
        num += nd * nd
        den += nr * nr
    out["unreached"] = unreached
    assert rows
    if dtype == "bf16":
        bars = bf16_bars()
        out["grad_rel_all"] = math.sqrt(num / den) / bars["rel_all"] if math.isfinite(num) else float("inf")
        out["grad_rel"] = max(r[2] for r in rows) / bars["rel"]
        out["grad_cos"] = max(1.0 - r[4] for r in rows) / (1.0 - bars["cos"])
        worst = max(rows, key=lambda r: r[2])[0]
    elif kind == "spec":
        core = [r for r in rows if r[0].startswith(("denoise_fn.", "mel_encoder."))]
        out["grad_norm"] = max(r[1] for r in rows) / SPEC_NORM
        out["grad_elem_core"] = max(r[3] for r in core) / SPEC_ELEM_CORE
        out["grad_elem"] = max(r[3] for r in rows) / SPEC_ELEM_ANY
        out["grad_diff_norm"] = max(r[2] for r in rows) / SPEC_DIFF_NORM
        worst = max(rows, key=lambda r: max(r[1] / SPEC_NORM, r[2] / SPEC_DIFF_NORM, r[3] / SPEC_ELEM_ANY))[0]
    else:
        out["grad_norm"] = max(r[1] for r in rows) / CAMP_NORM
        out["grad_elem"] = max(r[3] for r in rows) / CAMP_ELEM
        worst = max(rows, key=lambda r: max(r[1] / CAMP_NORM, r[3] / CAMP_ELEM))[0]
    return out, worst


# =====================================================================================================================================
# the float64 trajectory of the oracle alone (the stand-in for a run in test_trajectory_reference.py) and the fault planters
# =====================================================================================================================================
def oracle_trajectory(case, n_updates=N_UPDATES):
    """N updates of the oracle + update_step in float64 from the seeded weights -> (layout, template state dict, records); record k holds
    what a run exposes around update k: p, m, v (before), losses (per micro-batch), g, lr, p1, m1, v1 (after)."""
    W0, names = seeded_state(case["kind"])
    layout = Layout.contiguous(names, [W0[n].shape for n in names])
    p = flatten_state(layout, W0)
    m, v = np.zeros_like(p), np.zeros_like(p)
    recs = []
    for k in range(n_updates):
        losses, grads = oracle_update_inputs(case, unflatten_state(layout, p, W0), k)
        g = flatten_grads(layout, grads)
        n = layout.n
        p1, m1, v1 = (np.concatenate([a, np.zeros(layout.n_pad - n)]) for a in update_step(p[:n], g[:n], m[:n], v[:n], k, case["lr0"]))
        recs.append(dict(k=k, p=p, m=m, v=v, losses=losses, grads=grads, g=g, lr=lr_at(k, case["lr0"]), p1=p1, m1=m1, v1=v1))
        p, m, v = p1, m1, v1
    return layout, W0, recs


# which check catches which planted fault, and at which updates (N_UPDATES = 5).  "route": the fault lives on the continuing route only (a
# re-packed image, a direct sink), so the fresh restart of check 5 does not share it; the others are in code both runs execute, and check
# 5 is blind to them by construction.  clip_skipped shows wherever the clip is active (the test derives those updates from the gradient
# norms of the trajectory; with these batches: all).
ALL, FROM1, FROM2 = {0, 1, 2, 3, 4}, {1, 2, 3, 4}, {2, 3, 4}
FAULTS = {
    # name:               route, {check: updates}
    "stale_by_one":       (True, {3: FROM1, 4: set(), 5: FROM1}),   # forward and gradient at p_{k-1} (update 1: the 1e-7 step of update 0 only)
    "grad_dropped":       (True, {3: FROM1, 4: set(), 5: FROM1}),   # one conv weight's sink never written (sinks open at update 1)
    "grad_doubled":       (True, {3: FROM1, 4: set(), 5: FROM1}),   # written to the sink AND added by autograd
    "lr_next":            (False, {3: set(), 4: {0, 1}, 5: set()}),  # lr_at(k + 1): the plateau hides it from update 2 on
    "bias_step_k":        (False, {3: set(), 4: ALL, 5: set()}),    # bias correction with k instead of k + 1
    "clip_skipped":       (False, {3: set(), 4: "clip_active", 5: set()}),
    "moments_reset":      (False, {3: set(), 4: FROM1, 5: set()}),  # m, v not carried (update 0 starts from zeros either way)
    "accumulate_sum":     (False, {3: ALL, 4: set(), 5: set()}),    # micro-batch gradients averaged with 1 instead of 1 / acc
}
FAULT_TENSOR = {"spec": "denoise_fn.residual_layers.7.dilated_conv.weight", "campnet": "decoder_fine.res_blocks.2.blocks.0.1.weight"}


FAULT_STRIDE = 61  # the planted runs update every 61st element (the update is elementwise given the whole gradient's sum of squares)


def plant(fault, case, layout, W0, recs, k, stride=FAULT_STRIDE):
    """what a run with `fault` exposes at update k, started from the clean state of record k -> dict(losses, g, lr, p1, m1, v1); p1, m1
    and v1 hold every stride-th element"""
    r = recs[k]
    n, lr0 = layout.n, case["lr0"]
    losses, g, ufault, lr = r["losses"], r["g"], None, r["lr"]
    if fault == "stale_by_one":
        if k >= 1:
            losses, grads = oracle_update_inputs(case, unflatten_state(layout, recs[k - 1]["p"], W0), k)
            g = flatten_grads(layout, grads)
    elif fault in ("grad_dropped", "grad_doubled"):
        if k >= 1:
            i = layout.names.index(FAULT_TENSOR[case["kind"]])
            g = g.copy()
            g[layout.offs[i]:layout.offs[i] + layout.numels[i]] *= 0.0 if fault == "grad_dropped" else 2.0
    elif fault == "accumulate_sum":
        g = g * case["acc"]
    elif fault in UPDATE_FAULTS:
        ufault = fault
        if fault == "lr_next":
            lr = lr_at(k + 1, lr0)
    else:
        raise KeyError(fault)
    s = slice(0, n, stride)
    p1, m1, v1 = update_step(r["p"][s], g[s], r["m"][s], r["v"][s], k, lr0, fault=ufault, sumsq=sumsq64(g))
    return dict(losses=losses, g=g, lr=lr, p1=p1, m1=m1, v1=v1)


def checks_of(case, layout, rec, run, fresh, stride=FAULT_STRIDE):
    """the three checks on what a planted run exposes at one update given the clean state of record `rec` and what a fresh restart
    exposes -> {3: ratios, 4: ratios, 5: bool (bit-identical)}"""
    c3, _ = check_forward_backward(case["kind"], case["dtype"], layout, rec["losses"], rec["grads"], run["losses"], run["g"])
    s = slice(0, layout.n, stride)
    c4 = check_update(rec["p"][s], run["g"][s], rec["m"][s], rec["v"][s], rec["k"], case["lr0"], run["p1"], run["m1"], run["v1"],
                      len(run["p1"]), got_lr=run["lr"], sumsq=sumsq64(run["g"]))
    same = (run["losses"] == fresh["losses"] and run["lr"] == fresh["lr"]
            and all(np.array_equal(run[x], fresh[x], equal_nan=True) for x in ("g", "p1", "m1", "v1")))
    return {3: c3, 4: c4, 5: same}
