"""Float64 torch models, case tables and float32 mirrors for the branch sweep of the autograd tape (set_amd/autograd_ops.py: the
hand-written torch.autograd.Function nodes that drive the kernels in training).  Nothing here touches the GPU or imports the library:
test_tape_reference.py ties the models to independent code (torch.nn.functional, the attention model, the oracle's losses), checks the
exactness budgets, shows that the bars separate planted faults and holds the inventory; test_gpu_tape_branches.py runs the nodes.

Every model is a plain differentiable torch expression of the node's FORWARD in the reference's form, so torch autograd in float64 supplies
every gradient: nothing of a node's hand-written backward is restated here.  `evaluate(case, dtype)` runs it: float64 is the model,
float32 (the same expression on the CPU) the mirror; `reference(case)` holds both.  Two mirrors follow the kernels' documented order
instead, because the plain float32 expression is no mirror of them (measured: error / bar 3.3 and infinite): `ssim_mirror` (the fmaf chains
of csrc/train.hip) and `_FlashCore` (the attention backward as dS = P (dP - sum_d dO O)).

Two modes, as in the other sweeps.
  exact    operands are small integers (times a power of two): every product and partial sum is exact in fp32 in any order, the node must
           equal the float64 model bit for bit, outputs and gradients.
  bounded  Gaussian-magnitude operands: |gpu - model| <= mirror_bar(model, mirror) elementwise, per output and per gradient
           (head_optim_models.mirror_bar: 4 x the mirror's largest error for that tensor, floor 2 u |value|)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import philox_models as PH
from head_optim_models import BAR_FACTOR, SQRT2_F32, U, mirror_bar  # noqa: F401  (the bar of every bounded comparison)

G = 64  # floats around every guarded operand
F64 = torch.float64


def f32f(v):
    """a Python float that is exactly the fp32 the C ABI passes"""
    return float(np.float32(v))


def mish(x):
    return x * torch.tanh(F.softplus(x))


ACTS = {"none": lambda v: v, "relu": F.relu, "gelu": F.gelu, "mish": mish, "softplus": F.softplus, "tanh": torch.tanh}


def _grad_only(v, factor):
    """v in the forward, `factor` times its gradient in the backward (how the planted faults are written)"""
    return v.detach() + factor * (v - v.detach())


# =====================================================================================================================================
# models: t = operands by name (floating ones already in the evaluation dtype), c = the case's settings -> tuple of outputs
# =====================================================================================================================================
def conv_z(t, c):
    """(acc + b) alpha of set_conv1d: taps at t + tap dil - pad, zero outside the input, T_out frames"""
    x = t["x"]
    if "add" in t:
        x = x + t["add"][:, :, None]
    if c.get("pro", "none") == "div":
        x = _grad_only(x / c["pro_param"], c["pro_param"]) if c.get("fault") == "no_inv_pro" else x / c["pro_param"]
    K, dil, pad = t["w"].shape[2], c.get("dil", 1), c["pad"]
    T_out = c.get("T_out", x.shape[2] + 2 * pad - dil * (K - 1))
    right = T_out - x.shape[2] + (K - 1) * dil - pad
    return F.conv1d(F.pad(x, (pad, right)), t["w"], t.get("b"), dilation=dil) * c.get("alpha", 1.0)


def m_conv(t, c):
    z = conv_z(t, c)
    y = ACTS[c.get("act", "none")](z)
    if "res" in t:
        res = t["res"]
        if c.get("fault") == "relu_gate_on_y_res":  # the defect: the gate of the backward is y > 0 with y = relu(z) + res
            gate = ((y + res) > 0).to(z.dtype).detach()
            y = y.detach() + gate * (z - z.detach())
        if c.get("fault") == "res_before_mask" and "mask" in t:
            res = (res * t["mask"][:, None]).detach() + (res - res.detach())  # the residual's gradient taken before the mask
            return (y * t["mask"][:, None] + res,)
        y = y + res
    if "mask" in t:
        y = y * t["mask"][:, None]
    return (y,)


def m_act(t, c):
    return (ACTS[c["act"]](t["z"]),)


def layernorm_ch(x, gamma, beta, eps):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma[None, :, None] + beta[None, :, None]


def m_layernorm(t, c):
    y = layernorm_ch(t["x"], t["gamma"], t["beta"], c["eps"])
    return (y * t["mask"][:, None] if "mask" in t else y,)


def dropout_scale(shape, p, seed, offset, dtype):
    """keep / (1 - p) per element of a contiguous tensor (set_dropout: the decision is keyed by the element index)"""
    n = int(np.prod(shape))
    keep = PH.dropout_keep(int(seed), int(offset), n, p)
    return torch.from_numpy(keep.astype(np.float64)).reshape(shape).to(dtype) / (1.0 - f32f(p))


def m_preln_ffn(t, c):
    x = t["x"]
    h = layernorm_ch(x, t["gamma"], t["beta"], c["eps"])
    z = conv_z(dict(x=h, w=t["w1"], b=t["b1"]), dict(pad=c["pad"], T_out=x.shape[2], alpha=c["alpha"]))
    if c.get("fault") == "alpha_twice":
        z = _grad_only(z, c["alpha"])
    f = F.conv1d(ACTS[c["act"]](z), t["w2"], t["b2"])
    if c.get("drop") is not None:
        f = f * dropout_scale(f.shape, *c["drop"], f.dtype)
    y = x + f
    return (y * t["mask"][:, None] if "mask" in t else y,)


def m_add(t, c):
    return (t["a"] + t["b"],)


def m_embedding(t, c):
    e = t["table"][t["idx"]]  # [B, T, C]
    if c.get("padding_idx") is not None:  # nn.Embedding: the row is read, its gradient is not written
        e = torch.where((t["idx"] == c["padding_idx"])[..., None], e.detach(), e)
    out = c["scale"] * e.transpose(1, 2)
    return (t["base"] + out if "base" in t else out,)


def m_expand_states(t, c):
    enc, m2p = t["enc"], t["mel2ph"]
    B, C, _ = enc.shape
    return (torch.gather(F.pad(enc, (1, 0)), 2, m2p[:, None, :].expand(B, C, m2p.shape[1])),)


def m_add_chan_mask(t, c):
    y = t["x"] + t["add"][:, :, None] if "add" in t else t["x"] * 1.0
    return (y * t["mask"][:, None] if "mask" in t else y,)


def m_transpose(t, c):
    return (t["x"].transpose(1, 2),)


def m_gate(t, c):
    C = t["y"].shape[1] // 2
    return (torch.sigmoid(t["y"][:, :C]) * torch.tanh(t["y"][:, C:]),)


def m_res_skip(t, c):
    C = t["x"].shape[1]
    x_out = (t["x"] + t["o"][:, :C]) / float(SQRT2_F32)
    return (x_out, t["skip"] + t["o"][:, C:] if "skip" in t else t["o"][:, C:] * 1.0)


def m_dropout(t, c):
    return (t["x"] * dropout_scale(t["x"].shape, c["p"], c["seed"], c["offset"], t["x"].dtype),)


def m_fanout(t, c):
    return tuple(t["x"] * 1.0 for _ in range(c["n"]))


def m_grad_scale(t, c):
    return (_grad_only(t["x"], c["s"]),)


def m_sum_losses(t, c):
    return (torch.stack([t["v%d" % i] for i in range(c["n"])]).sum(),)


def _heads(x, heads):
    B, H, T = x.shape
    return x.reshape(B, heads, H // heads, T).transpose(2, 3)  # [B, heads, T, d]


class _FlashCore(torch.autograd.Function):
    """The attention core with the backward in the form the fused kernels document (csrc/attention_fused.hip, attn_model of
    test_attention_reference.py): delta = sum_d dO O, dS = P (dP - delta).  The same function as the plain softmax backward, dS = P (dP -
    sum_k P dP), but not the same roundings: where the two sums cancel (one key: dS = 0 exactly in the plain form) the plain float32 mirror
    has no error at all and its bar would be 0.  Used by the float32 MIRROR only; the float64 model is the plain expression."""

    @staticmethod
    def forward(ctx, qh, kh, vh, alpha, pad, fill):
        s = alpha * (qh @ kh.transpose(2, 3))
        if pad is not None:
            s = s.masked_fill(pad, fill)
        p = torch.softmax(s, -1)
        o = p @ vh
        ctx.save_for_backward(qh, kh, vh, p, o)
        ctx.alpha, ctx.pad = alpha, pad
        ctx.mark_non_differentiable(p)
        return o, p

    @staticmethod
    def backward(ctx, do, _dp):
        qh, kh, vh, p, o = ctx.saved_tensors
        dS = p * (do @ vh.transpose(2, 3) - (do * o).sum(-1, keepdim=True))
        if ctx.pad is not None:
            dS = dS.masked_fill(ctx.pad, 0.0)
        return ctx.alpha * (dS @ kh), ctx.alpha * (dS.transpose(2, 3) @ qh), p.transpose(2, 3) @ do, None, None, None


def attention(q, k, v, kpm, fill, alpha, heads):
    """softmax(alpha q k^T, padded keys filled) v per head, channel-major in and out; -> (o [B, H, Tq], p [B, heads, Tq, Tk])"""
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    pad = None if kpm is None else (kpm != 0)[:, None, None, :]
    if q.dtype == torch.float32:  # the mirror
        o, p = _FlashCore.apply(qh, kh, vh, alpha, pad, fill)
    else:
        s = alpha * (qh @ kh.transpose(2, 3))
        if pad is not None:
            s = s.masked_fill(pad, fill)
        p = torch.softmax(s, -1)
        o = p @ vh
    B, h, T, d = o.shape
    return o.transpose(2, 3).reshape(B, h * d, T), p


def m_attn(t, c):
    if "qkv" in t:
        H = t["qkv"].shape[1] // 3
        q, k, v = t["qkv"][:, :H], t["qkv"][:, H:2 * H], t["qkv"][:, 2 * H:]
    else:
        H = t["q"].shape[1]
        q, k, v = t["q"], t["kv"][:, :H], t["kv"][:, H:]
    o, p = attention(q, k, v, t.get("kpm"), c["fill"], c["alpha"], c["heads"])
    return (o, p.detach()) if c.get("want_p") else (o,)


def m_preln_self_attn(t, c):
    x = t["x"]
    H = x.shape[1]
    qkv = F.conv1d(layernorm_ch(x, t["gamma"], t["beta"], c["eps"]), t["w_in"])
    o, _ = attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], t.get("kpm"), float("-inf"), c["alpha"], c["heads"])
    y = x + F.conv1d(o, t["w_out"])
    return (y * t["mask"][:, None] if "mask" in t else y,)


def m_preln_cross_attn(t, c):
    x = t["x"]
    H = x.shape[1]
    q = F.conv1d(layernorm_ch(x, t["gamma"], t["beta"], c["eps"]), t["w_in"][:H])
    kv = F.conv1d(t["enc"], t["w_in"][H:])
    o, p = attention(q, kv[:, :H], kv[:, H:], t.get("kpm"), -1e8, c["alpha"], c["heads"])
    y = x + F.conv1d(o, t["w_out"])
    return (y, p.detach()) if c.get("want_p") else (y,)


def m_pos_add(t, c):
    return (t["x"] + t["alpha"] * t["table"][t["pos"]].transpose(1, 2),)


def m_mask_fill_chan(t, c):
    m = t["m"][:, None]
    return (t["x"] * (1.0 - m) + t["e"].reshape(1, -1, 1) * m,)


def m_add_masked(t, c):
    return (t["a"] + t["b"] * t["m"][:, None],)


def m_masked_l1(t, c):
    B, T, M = t["pred"].shape
    w = t["w"].reshape(B, T, 1)
    return (((t["pred"] - t["target"]).abs() * w).sum() / (w.sum() * M),)


def ssim_window(dtype):
    """11 x 11 Gaussian window, sigma 1.5, built in float32 as the reference builds it"""
    g = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().to(dtype)[None, None]


def m_ssim(t, c):
    B, T, M = t["pred"].shape
    a, b = t["pred"][:, None] + c["bias"], t["target"][:, None] + c["bias"]
    win = ssim_window(a.dtype)
    blur = lambda v: F.conv2d(v, win, padding=5)  # noqa: E731
    mu1, mu2 = blur(a), blur(b)
    s1, s2, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    w = t["w"].reshape(B, T, 1)
    return (((1.0 - ssim[:, 0]) * w).sum() / (w.sum() * M),)


def _fma32(a, b, acc):
    """fmaf on float32 arrays: the product is exact in float64, one rounding of the sum"""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _ssim_filter32(img, win):
    """csrc/train.hip, ssim_filter_kernel / ssim_bwd_kernel: one fmaf chain per pixel over the 121 taps, dy outer and dx inner, the tap
    weight fl(g[dy] g[dx]); cells outside the image hold 0"""
    B, H, W = img.shape
    padded = np.zeros((B, H + 10, W + 10), np.float32)
    padded[:, 5:5 + H, 5:5 + W] = img
    acc = np.zeros((B, H, W), np.float32)
    for dy in range(11):
        for dx in range(11):
            acc = _fma32(np.broadcast_to(win[dy, dx], acc.shape), padded[:, dy:dy + H, dx:dx + W], acc)
    return acc


def ssim_mirror(t, c, gout):
    """_SSIMLossFn in float32 in the kernels' documented order (csrc/train.hip: the window as fl(g_i g_j) of the fp32 Gaussian, the fmaf
    chains of the filter, ssim_map_kernel's association, set_scale_bcast's factor order, ssim_bwd_kernel's last line; the library is built
    with -ffp-contract=off).  The plain float32 torch expression is no mirror of it: the filtered second moments lose ~4 bits to
    E[x^2] - mu^2 at a bias of 6, and conv2d's sums land elsewhere within that loss than the kernel's fmaf chains.  -> (loss, dpred)"""
    f = np.float32
    pred, target, w = (t[k].detach().numpy().astype(f) for k in ("pred", "target", "w"))
    B, T, M = pred.shape
    g = np.array([math.exp(-(i - 5) ** 2 / (2.0 * 1.5 * 1.5)) for i in range(11)]).astype(f)
    s = f(0.0)
    for v in g:
        s = f(s + v)
    g = (g / s).astype(f)
    win = (g[:, None] * g[None, :]).astype(f)
    u, v = pred + f(c["bias"]), target + f(c["bias"])
    m1, m2 = _ssim_filter32(u, win), _ssim_filter32(v, win)
    q11, q22, q12 = _ssim_filter32(u * u, win), _ssim_filter32(v * v, win), _ssim_filter32(u * v, win)
    C1, C2 = f(0.0001), f(0.0009)
    v1, v2, cv = q11 - m1 * m1, q22 - m2 * m2, q12 - m1 * m2
    A1, A2 = f(2.0) * m1 * m2 + C1, f(2.0) * cv + C2
    B1, B2 = m1 * m1 + m2 * m2 + C1, v1 + v2 + C2
    ss = (A1 * A2) / (B1 * B2)
    wf = np.repeat(w.reshape(B, T, 1), M, 2)
    num = ((f(1.0) - ss) * wf).sum(dtype=f)
    den = f(w.sum(dtype=f) * f(M))
    dA1, dA2, dB1, dB2 = f(2.0) * m2, f(-2.0) * m2, f(2.0) * m1, f(-2.0) * m1
    d_mu1 = (dA1 * A2 + A1 * dA2) / (B1 * B2) - ss * (dB1 / B1 + dB2 / B2)
    d_s11 = -ss / B2
    d_s12 = f(2.0) * A1 / (B1 * B2)
    scale = f(-f(gout) / den)
    gm, g11, g12 = (_ssim_filter32((d * f(1.0)) * wf * scale, win) for d in (d_mu1, d_s11, d_s12))
    dimg = gm + f(2.0) * u * g11 + v * g12
    return torch.tensor(num / den, dtype=torch.float32), torch.from_numpy(dimg.astype(f))


def word_ids(txt, sil_ids=(1, 2, 3)):
    sil = torch.zeros_like(txt, dtype=torch.bool)
    for i in sil_ids:
        sil |= txt == i
    sil = sil.long()
    return (sil.cumsum(-1) * (1 - sil)).contiguous()


def m_dur_loss(t, c):
    dur, m2p, txt, wid = t["dur_pred"], t["mel2ph"], t["txt"], t["word_id"]
    B, Tt = txt.shape
    nonpad = (txt != 0).to(dur.dtype)
    dur_gt = (m2p[:, None, :] == torch.arange(1, Tt + 1)[None, :, None]).sum(-1).to(dur.dtype) * nonpad
    pd = ((torch.log(dur + 1) - torch.log(dur_gt + 1)) ** 2 * nonpad).sum() / nonpad.sum() * c["lam_p"]
    nw = int(wid.max()) + 1
    wp = torch.zeros(B, nw, dtype=dur.dtype).scatter_add(1, wid, dur)[:, 1:]
    wg = torch.zeros(B, nw, dtype=dur.dtype).scatter_add(1, wid, dur_gt)[:, 1:]
    wm = (wg > 0).to(dur.dtype)
    wd = ((torch.log(wp + 1) - torch.log(wg + 1)) ** 2 * wm).sum() / wm.sum() * c["lam_w"]
    return (pd, wd)


def m_pitch_loss(t, c):
    pp, f0, uv = t["pp"], t["f0"], t["uv"]  # pp [B, 2, T]: row 0 the f0 prediction, row 1 the voiced / unvoiced logit
    nonpad = (t["mel2ph"] != 0).to(pp.dtype)
    z = pp[:, 1]
    bce = torch.clamp(z, min=0) - z * uv + torch.log1p(torch.exp(-z.abs()))
    uvl = (bce * nonpad).sum() / nonpad.sum() * c["lam_uv"]
    nv = nonpad * (uv == 0).to(pp.dtype)
    f0l = ((pp[:, 0] - f0).abs() * nv).sum() / nv.sum() * c["lam_f0"]
    return (uvl, f0l)


MODELS = {
    "_Conv1dFn": m_conv, "_ActFn": m_act, "_LayerNormChFn": m_layernorm, "_PreLnFfnFn": m_preln_ffn, "_AddFn": m_add,
    "_EmbeddingFn": m_embedding, "_ExpandStatesFn": m_expand_states, "_AddChanMaskFn": m_add_chan_mask, "_TransposeFn": m_transpose,
    "_GateFn": m_gate, "_ResSkipFn": m_res_skip, "_DropoutFn": m_dropout, "_FanoutFn": m_fanout, "_GradScaleFn": m_grad_scale,
    "_SumLossesFn": m_sum_losses, "_AttnFn": m_attn, "_PreLnSelfAttnFn": m_preln_self_attn, "_PreLnCrossAttnFn": m_preln_cross_attn,
    "_PosAddFn": m_pos_add, "_MaskFillChanFn": m_mask_fill_chan, "_AddMaskedFn": m_add_masked, "_MaskedL1Fn": m_masked_l1,
    "_SSIMLossFn": m_ssim, "_DurLossFn": m_dur_loss, "_PitchLossFn": m_pitch_loss,
}

# nodes whose gradient test lives in another module: node -> (module, test, a name the test's source mentions)
SWEPT_ELSEWHERE = {
    "_StutterLossFn": ("test_gpu_stutter.py", "test_head_loss_kernel_matches_torch", "stutter_losses"),
    "_StepProjFn": ("test_gpu_training.py", "test_step_projections_of_all_layers_equal_the_per_layer_linears", "_StepProjFn"),
    "_DiffNetStackBf16Fn": ("test_gpu_bf16.py", "test_fused_bf16_layers_match_emulation", "_DiffNetStackBf16Fn"),
    # the layers of tests/golden/train_losses.npz through the node (diffnet.forward_train takes it under SET_AMD_WINO=2), every
    # gradient against the reference's own autograd; the detached-cond case of test_gpu_tape_branches.py names the node itself
    "_DiffNetStackFn": ("test_gpu_training.py", "test_training_losses_and_all_gradients_match_reference", "fused_stack"),
}


# =====================================================================================================================================
# operands
# =====================================================================================================================================
class Draw:
    """exact: integers in [-2, 2]; bounded: standard normals (times `s`)"""

    def __init__(self, mode, seed):
        self.mode, self.g = mode, torch.Generator().manual_seed(seed)

    def __call__(self, *shape, s=1.0):
        if self.mode == "exact":
            return torch.randint(-2, 3, shape, generator=self.g).float()
        return torch.randn(*shape, generator=self.g) * s

    def mask(self, B, T, keep=0.7):
        m = (torch.rand(B, T, generator=self.g) < keep).float()
        m[:, 0] = 1.0
        return m

    def ints(self, lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=self.g)


def o_conv(c, d):
    B, Cin, Cout, K, T = c["B"], c["Cin"], c["Cout"], c["K"], c["T"]
    s = 1.0 / math.sqrt(Cin * K)
    t = dict(x=d(B, Cin, T), w=d(Cout, Cin, K, s=s))
    if c.get("bias", True):
        t["b"] = d(Cout, s=0.1)
    if c.get("add"):
        t["add"] = d(B, Cin)
    if c.get("mask"):
        t["mask"] = d.mask(B, T)
    if c.get("res"):
        T_out = c.get("T_out", T + 2 * c["pad"] - c.get("dil", 1) * (K - 1))
        t["res"] = d(B, Cout, T_out)
        if c.get("res") == "flip":  # relu(z) + res and z of opposite sign wherever z != 0
            z = conv_z({k: v.double() for k, v in t.items()}, c)
            t["res"] = (-2.0 * z).float()
    return t


def o_ffn(c, d):
    B, C, Cm, K, T = c["B"], c["C"], c["Cmid"], c["K"], c["T"]
    t = dict(x=d(B, C, T), gamma=d(C), beta=d(C), w1=d(Cm, C, K, s=0.1), b1=d(Cm, s=0.1), w2=d(C, Cm, 1, s=0.1), b2=d(C, s=0.1))
    if c.get("mask"):
        t["mask"] = d.mask(B, T)
    return t


def o_attn_nodes(c, d):
    B, H, T = c["B"], c["H"], c["T"]
    s = 1.0 / math.sqrt(H)
    t = dict(x=d(B, H, T), gamma=d(H) * 0.3 + 1.0, beta=d(H, s=0.3), w_in=d(3 * H, H, 1, s=s), w_out=d(H, H, 1, s=s))
    Tk = T
    if "Tk" in c:
        Tk = c["Tk"]
        t["enc"] = d(B, H, Tk)
    if c.get("kpm"):
        t["kpm"] = _kpm(B, Tk)
    if c.get("mask"):
        t["mask"] = d.mask(B, T)
    return t


def _kpm(B, Tk):
    """padded key tails: utterance b pads its last b (Tk // (B + 1)) keys (the first pads none; none pads every key)"""
    kpm = torch.zeros(B, Tk)
    for b in range(B):
        n = b * (Tk // (B + 1))
        if n:
            kpm[b, Tk - n:] = 1.0
    return kpm


def o_attn(c, d):
    B, H, T = c["B"], c["H"], c["T"]
    Tk = c.get("Tk", T)
    t = dict(qkv=d(B, 3 * H, T)) if c["form"] == "self" else dict(q=d(B, H, T), kv=d(B, 2 * H, Tk))
    if c.get("kpm"):
        t["kpm"] = _kpm(B, Tk)
    return t


def mel2ph_rows(B, T, T_txt, g):
    """sorted mel2ph in [0, T_txt] with padded tails; the LAST utterance is all 0 when B > 1"""
    m = torch.sort(torch.randint(1, T_txt + 1, (B, T), generator=g), dim=1).values
    for b in range(B):
        m[b, T - (b * T) // (B + 2):] = 0
    if B > 1:
        m[B - 1] = 0
    return m


def o_losses(c, d):
    B, T, M = c["B"], c["T"], c["M"]
    pred = d(B, T, M, s=0.5) - 3.0
    target = torch.clamp(d(B, T, M, s=1.5) - 3.0, -6, 1.5)
    for b in range(1, B):
        target[b, T - (b * T) // (B + 1):] = 0
    w = (target.abs().sum(-1) != 0).float().reshape(-1)
    return dict(pred=pred, target=target, w=w)


def o_dur(c, d):
    B, T, Tt = c["B"], c["T"], c["T_txt"]
    txt = d.ints(1, 9, B, Tt)
    for b in range(B):
        txt[b, Tt - b:] = 0  # padded text tails
    m2p = torch.sort(d.ints(1, Tt + 1, B, T), dim=1).values
    m2p = torch.minimum(m2p, (txt != 0).sum(1, keepdim=True))
    m2p[:, T - 2:] = 0
    dur = torch.rand(B, Tt, generator=d.g) * 5
    return dict(dur_pred=dur, mel2ph=m2p, txt=txt, word_id=word_ids(txt))


def o_pitch(c, d):
    B, T = c["B"], c["T"]
    m2p = torch.sort(d.ints(1, 9, B, T), dim=1).values
    for b in range(B):
        m2p[b, T - (b * T) // (B + 1):] = 0  # padded tails; frame 0 is voiced speech in every utterance
    uv = (torch.rand(B, T, generator=d.g) < 0.4).float()
    uv[:, 0] = 0.0
    return dict(pp=d(B, 2, T), f0=d(B, T), uv=uv, mel2ph=m2p)


def _simple(shapes):
    """operands that are plain draws: name -> shape from the case"""
    return lambda c, d: {k: d(*f(c)) for k, f in shapes.items()}


BCT = lambda c: (c["B"], c["C"], c["T"])  # noqa: E731


def o_embedding(c, d):
    B, C, T, n = c["B"], c["C"], c["T"], c["rows"]
    idx = d.ints(0, n, B, T)
    idx[0, 0] = 0  # row 0 (the padding row of the padding_idx cases) is used at least once
    t = dict(idx=idx, table=d(n, C))
    if c.get("base"):
        t["base"] = d(B, C, T)
    return t


def o_expand(c, d):
    return dict(enc=d(c["B"], c["C"], c["T_txt"]), mel2ph=mel2ph_rows(c["B"], c["T"], c["T_txt"], d.g))


def o_acm(c, d):
    t = dict(x=d(*BCT(c)))
    if c.get("add"):
        t["add"] = d(c["B"], c["C"])
    if c.get("mask"):
        t["mask"] = d.mask(c["B"], c["T"])
    return t


def o_ln(c, d):
    t = dict(x=d(*BCT(c)), gamma=d(c["C"]), beta=d(c["C"]))
    if c.get("mask"):
        t["mask"] = d.mask(c["B"], c["T"])
    return t


def o_res_skip(c, d):
    t = dict(x=d(*BCT(c)), o=d(c["B"], 2 * c["C"], c["T"]))
    if c.get("skip"):
        t["skip"] = d(*BCT(c))
    return t


def o_pos_add(c, d):
    return dict(x=d(*BCT(c)), alpha=d(1) + 1.5, pos=d.ints(0, c["rows"], c["B"], c["T"]), table=d(c["rows"], c["C"]))


OPERANDS = {
    "_Conv1dFn": o_conv, "_ActFn": _simple(dict(z=lambda c: (c["n"],))), "_LayerNormChFn": o_ln, "_PreLnFfnFn": o_ffn,
    "_AddFn": _simple(dict(a=BCT, b=BCT)), "_EmbeddingFn": o_embedding, "_ExpandStatesFn": o_expand, "_AddChanMaskFn": o_acm,
    "_TransposeFn": _simple(dict(x=lambda c: c["shape"])), "_GateFn": _simple(dict(y=lambda c: (c["B"], 2 * c["C"], c["T"]))),
    "_ResSkipFn": o_res_skip, "_DropoutFn": _simple(dict(x=BCT)), "_FanoutFn": _simple(dict(x=BCT)), "_GradScaleFn": _simple(dict(x=BCT)),
    "_SumLossesFn": lambda c, d: {"v%d" % i: d() for i in range(c["n"])}, "_AttnFn": o_attn, "_PreLnSelfAttnFn": o_attn_nodes,
    "_PreLnCrossAttnFn": o_attn_nodes, "_PosAddFn": o_pos_add,
    "_MaskFillChanFn": lambda c, d: dict(x=d(*BCT(c)), e=d(1, 1, c["C"]), m=d.mask(c["B"], c["T"], 0.5)),
    "_AddMaskedFn": lambda c, d: dict(a=d(*BCT(c)), b=d(*BCT(c)), m=d.mask(c["B"], c["T"], 0.5)),
    "_MaskedL1Fn": o_losses, "_SSIMLossFn": o_losses, "_DurLossFn": o_dur, "_PitchLossFn": o_pitch,
}


# =====================================================================================================================================
# the case table
# =====================================================================================================================================
CASES = []


def case(name, node, mode, diff, nograd=(), absent=(), ups=None, **c):
    """diff: the operands that require grad in the all-wanted run; nograd: tuples of operands that do NOT require grad in further runs of
    the same case (each must come back None, the others bit-identical to the all-wanted run); absent: the optional operands this case
    leaves out; ups: the upstream gradient of each 0-d output."""
    CASES.append(dict(name=name, node=node, mode=mode, diff=tuple(diff), nograd=tuple(tuple(n) for n in nograd), absent=tuple(absent),
                      ups=ups, c=c))


def same(K, dil=1):
    return dil * (K - 1) // 2


CONV_ALL = ("x", "w", "b", "add", "res")
# every combination of needs_input_grad that _Conv1dFn.backward reads: each one off, dadd without dx, nothing but res, each one alone
CONV_NOGRAD = [("x",), ("w",), ("b",), ("add",), ("res",), ("x", "w", "b", "res"), ("x", "w", "b", "add"), ("w", "b", "add", "res"),
               ("x", "b", "add", "res"), ("x", "w", "add", "res"), ("x", "add"), ("w", "b")]

# ---- _Conv1dFn, exact: shapes x epilogue forms, each with and without res
case("conv_all_operands_b3_c7_t33_k3_dil2", "_Conv1dFn", "exact", CONV_ALL, nograd=CONV_NOGRAD, absent=("mask", "t_out"),
     B=3, Cin=7, Cout=32, K=3, dil=2, pad=2, T=33, add=True, res=True)
case("conv_t15_naive_wgrad", "_Conv1dFn", "exact", CONV_ALL, absent=("mask",), B=3, Cin=32, Cout=7, K=3, pad=1, T=15, add=True, res=True)
case("conv_t16_ordered_mfma_wgrad", "_Conv1dFn", "exact", CONV_ALL, absent=("mask",), B=3, Cin=32, Cout=7, K=3, pad=1, T=16, add=True,
     res=True)
case("conv_t1_c96", "_Conv1dFn", "exact", ("x", "w", "b"), absent=("chan_add", "res", "mask"), B=1, Cin=96, Cout=32, K=1, pad=0, T=1)
case("conv_t70_c96_k5", "_Conv1dFn", "exact", ("x", "w", "b"), absent=("chan_add", "res", "mask"), B=3, Cin=96, Cout=96, K=5, pad=2, T=70)
case("conv_no_bias_causal_t_out", "_Conv1dFn", "exact", ("x", "w"), absent=("bias", "chan_add", "res", "mask"), B=1, Cin=7, Cout=7, K=3,
     pad=2, T=33, T_out=33, bias=False)
for _res in (False, True):
    _r = "_res" if _res else ""
    _d = ("x", "w", "b") + (("res",) if _res else ())
    _a = ("chan_add",) + (() if _res else ("res",))
    _kw = dict(B=3, Cin=7, Cout=32, K=3, pad=1, T=33, res=_res)
    case("conv_epilogue_identity" + _r, "_Conv1dFn", "exact", _d, absent=_a + ("mask",), **_kw)
    case("conv_epilogue_alpha" + _r, "_Conv1dFn", "exact", _d, absent=_a + ("mask",), alpha=0.5, **_kw)
    case("conv_epilogue_mask" + _r, "_Conv1dFn", "exact", _d, absent=_a, mask=True, **_kw)
    case("conv_epilogue_pro_div" + _r, "_Conv1dFn", "exact", _d, absent=_a + ("mask",), pro="div", pro_param=2.0, **_kw)
    _kw["res"] = "flip" if _res else False
    case("conv_epilogue_relu" + _r, "_Conv1dFn", "exact", _d, absent=_a + ("mask",), act="relu", **_kw)
    case("conv_epilogue_relu_mask" + _r, "_Conv1dFn", "exact", _d, absent=_a, act="relu", mask=True, **_kw)
    case("conv_epilogue_relu_alpha" + _r, "_Conv1dFn", "exact", _d, absent=_a + ("mask",), act="relu", alpha=0.5, **_kw)
RELU_RES_CASE = "conv_epilogue_relu_res"
# ---- _Conv1dFn, bounded: the split activations (conv, then _ActFn, then the mask as a node of its own) and non-dyadic factors
for _act in ("gelu", "mish", "softplus", "tanh"):
    case("conv_split_%s_mask_alpha" % _act, "_Conv1dFn", "bounded", ("x", "w", "b", "add"), nograd=[("x",), ("add",)], absent=("res",),
         B=3, Cin=32, Cout=7, K=5, pad=2, T=33, add=True, mask=True, act=_act, alpha=f32f(5 ** -0.5))
case("conv_bounded_pro_div_alpha_res_mask", "_Conv1dFn", "bounded", CONV_ALL, B=3, Cin=96, Cout=32, K=3, dil=2, pad=2, T=70, add=True, res=True,
     mask=True, alpha=f32f(3 ** -0.5), pro="div", pro_param=f32f(math.sqrt(20.0)))
PRO_CASE = "conv_bounded_pro_div_alpha_res_mask"
case("conv_bounded_relu_pro_div", "_Conv1dFn", "bounded", ("x", "w", "b"), absent=("chan_add", "res", "mask"), B=1, Cin=32, Cout=32, K=1,
     pad=0, T=16, act="relu", pro="div", pro_param=f32f(math.sqrt(20.0)))
# the weight-gradient selection under set_compute_dtype("bf16") (T = 16: the convs themselves stay on the fp32 kernels)
BF16_WGRAD = {}
for _ci, _co in ((31, 32), (32, 31), (32, 32)):
    _n = "conv_wgrad_dtype_cin%d_cout%d" % (_ci, _co)
    BF16_WGRAD[_n] = _ci >= 32 and _co >= 32  # does the bf16 run take bf16 operands
    case(_n, "_Conv1dFn", "bounded", ("x", "w", "b"), absent=("chan_add", "res", "mask"), B=3, Cin=_ci, Cout=_co, K=1, pad=0, T=16)

# ---- the small nodes
for _act in ("gelu", "mish", "softplus", "tanh"):
    case("act_%s_n1000" % _act, "_ActFn", "bounded", ("z",), n=1000, act=_act)
case("layernorm_mask_b3_c7_t33", "_LayerNormChFn", "bounded", ("x", "gamma", "beta"), B=3, C=7, T=33, mask=True, eps=1e-5)
case("layernorm_no_mask_b1_c96_t70", "_LayerNormChFn", "bounded", ("x", "gamma", "beta"), absent=("mask",), B=1, C=96, T=70, eps=1e-5)
case("layernorm_c32_t1", "_LayerNormChFn", "bounded", ("x", "gamma", "beta"), absent=("mask",), B=3, C=32, T=1, eps=1e-5)
FFN_ALL = ("x", "gamma", "beta", "w1", "b1", "w2", "b2")
case("ffn_same_k3_mask", "_PreLnFfnFn", "bounded", FFN_ALL, absent=("drop",), B=3, C=32, Cmid=64, K=3, pad=1, T=33, mask=True,
     alpha=f32f(3 ** -0.5), act="gelu", eps=1e-5)
case("ffn_causal_k9_no_mask", "_PreLnFfnFn", "bounded", FFN_ALL, absent=("drop", "mask"), B=1, C=32, Cmid=64, K=9, pad=8, T=70,
     alpha=f32f(9 ** -0.5), act="gelu", eps=1e-5)
case("ffn_drop_offset_above_2_32_mask", "_PreLnFfnFn", "bounded", FFN_ALL, B=3, C=32, Cmid=64, K=3, pad=1, T=33, mask=True,
     alpha=f32f(3 ** -0.5), act="gelu", eps=1e-5, drop=(0.5, 1234567, (1 << 32) + 12345))
case("ffn_drop_no_mask_t16", "_PreLnFfnFn", "bounded", FFN_ALL, absent=("mask",), B=1, C=32, Cmid=64, K=9, pad=8, T=16,
     alpha=f32f(9 ** -0.5), act="gelu", eps=1e-5, drop=(0.5, 7, (1 << 33) + 1))
FFN_ALPHA_CASE = "ffn_same_k3_mask"
case("add_b3_c7_t33", "_AddFn", "exact", ("a", "b"), B=3, C=7, T=33)
case("embedding_base_scale2", "_EmbeddingFn", "exact", ("table", "base"), absent=("padding_idx",), B=3, C=7, T=33, rows=11, base=True,
     scale=2.0)
case("embedding_no_base_padding_idx0", "_EmbeddingFn", "exact", ("table",), absent=("base",), B=3, C=32, T=70, rows=11, scale=1.0,
     padding_idx=0)
case("embedding_no_base_no_padding_t1", "_EmbeddingFn", "exact", ("table",), absent=("base", "padding_idx"), B=1, C=96, T=1, rows=5, scale=0.5)
for _tt in (1, 14):
    case("expand_states_t_txt%d_last_row_all_0" % _tt, "_ExpandStatesFn", "exact", ("enc",), B=3, C=7, T=33, T_txt=_tt)
case("expand_states_b1_t1", "_ExpandStatesFn", "exact", ("enc",), B=1, C=32, T=1, T_txt=1)
case("add_chan_mask_both", "_AddChanMaskFn", "exact", ("x", "add"), nograd=[("add",), ("x",)], B=3, C=7, T=33, add=True, mask=True)
case("add_chan_mask_no_add", "_AddChanMaskFn", "exact", ("x",), absent=("add",), B=3, C=7, T=33, mask=True)
case("add_chan_mask_no_mask", "_AddChanMaskFn", "exact", ("x", "add"), absent=("mask",), B=1, C=96, T=70, add=True)
case("transpose_btc_to_bct", "_TransposeFn", "exact", ("x",), shape=(3, 33, 7), to_bct=True)
case("transpose_bct_to_btc", "_TransposeFn", "exact", ("x",), shape=(3, 7, 33), to_bct=False)
case("gate_b3_c7_t33", "_GateFn", "bounded", ("y",), B=3, C=7, T=33)
case("gate_b1_c96_t16", "_GateFn", "bounded", ("y",), B=1, C=96, T=16)
TWO_OUTPUT_UPS = ((1.0, 1.0), (3.0, 0.25), (0.0, 1.0))
for _u in TWO_OUTPUT_UPS:
    case("res_skip_ups_%g_%g" % _u, "_ResSkipFn", "bounded", ("x", "o", "skip"), B=3, C=7, T=33, skip=True, up_scale=_u)
case("res_skip_first_layer_no_skip_in", "_ResSkipFn", "bounded", ("x", "o"), absent=("skip_in",), B=1, C=32, T=70, up_scale=(3.0, 0.25))
case("dropout_p0.5_offset_above_2_32", "_DropoutFn", "exact", ("x",), B=3, C=7, T=33, p=0.5, seed=99, offset=(1 << 32) + 5)
for _n in (2, 3, 4):
    case("fanout_%d" % _n, "_FanoutFn", "exact", ("x",), B=3, C=7, T=33, n=_n)
case("grad_scale_2_pow_minus_3", "_GradScaleFn", "exact", ("x",), B=3, C=7, T=33, s=0.125)
case("sum_losses_6_terms", "_SumLossesFn", "exact", tuple("v%d" % i for i in range(6)), ups=(3.0,), n=6)

# ---- attention: head size 32 runs the fused kernels (and the three-launch form under SET_AMD_ATTN_FUSED=0), head size 7 the unfused only
for _form in ("self", "cross"):
    _diff = ("qkv",) if _form == "self" else ("q", "kv")
    _tk = {} if _form == "self" else dict(Tk=14)
    case("attn_%s_d32_kpm_want_p" % _form, "_AttnFn", "bounded", _diff, B=3, H=64, T=33, heads=2, form=_form, kpm=True, want_p=True,
         fill=float("-inf") if _form == "self" else -1e8, alpha=f32f(32 ** -0.5), **_tk)
    case("attn_%s_d32_no_kpm_no_p" % _form, "_AttnFn", "bounded", _diff, absent=("kpm", "want_p"), B=1, H=64, T=70, heads=2, form=_form,
         fill=float("-inf") if _form == "self" else -1e8, alpha=f32f(32 ** -0.5), **({} if _form == "self" else dict(Tk=1)))
case("attn_self_d7_unfused_only", "_AttnFn", "bounded", ("qkv",), absent=("kpm",), B=3, H=14, T=15, heads=2, form="self", want_p=True,
     fill=float("-inf"), alpha=f32f(7 ** -0.5))
SA_ALL = ("x", "gamma", "beta", "w_in", "w_out")
case("preln_self_attn_kpm_mask", "_PreLnSelfAttnFn", "bounded", SA_ALL, B=3, H=64, T=33, heads=2, kpm=True, mask=True,
     alpha=f32f(32 ** -0.5), eps=1e-5)
case("preln_self_attn_no_kpm_no_mask", "_PreLnSelfAttnFn", "bounded", SA_ALL, absent=("kpm", "mask"), B=1, H=64, T=16, heads=2,
     alpha=f32f(32 ** -0.5), eps=1e-5)
CA_ALL = ("x", "enc", "gamma", "beta", "w_in", "w_out")
case("preln_cross_attn_kpm_want_p", "_PreLnCrossAttnFn", "bounded", CA_ALL, nograd=[("enc",)], B=3, H=64, T=33, Tk=14, heads=2, kpm=True,
     want_p=True, alpha=f32f(32 ** -0.5), eps=1e-5)
case("preln_cross_attn_no_kpm_no_p", "_PreLnCrossAttnFn", "bounded", CA_ALL, absent=("kpm", "want_p"), B=1, H=64, T=16, Tk=16, heads=2,
     alpha=f32f(32 ** -0.5), eps=1e-5)
KV_CASE = "preln_cross_attn_kpm_want_p"
case("pos_add_b3_c7_t33", "_PosAddFn", "bounded", ("x", "alpha"), nograd=[("alpha",)], B=3, C=7, T=33, rows=40)
POS_CASE = "pos_add_b3_c7_t33"
case("mask_fill_chan_m80", "_MaskFillChanFn", "exact", ("e",), B=3, C=80, T=33)
case("mask_fill_chan_c7_t1", "_MaskFillChanFn", "exact", ("e",), B=1, C=7, T=1)
case("add_masked_b3_c7_t33", "_AddMaskedFn", "exact", ("a", "b"), nograd=[("a",)], B=3, C=7, T=33)

# ---- losses (M = 80)
case("masked_l1_b3_t33", "_MaskedL1Fn", "bounded", ("pred",), ups=(0.5,), B=3, T=33, M=80)
case("masked_l1_b1_t7", "_MaskedL1Fn", "bounded", ("pred",), ups=(1.0,), B=1, T=7, M=80)
case("ssim_t7_window_larger_than_image", "_SSIMLossFn", "bounded", ("pred",), ups=(0.5,), B=3, T=7, M=80, bias=6.0)
case("ssim_t33_off_tile_height", "_SSIMLossFn", "bounded", ("pred",), ups=(1.0,), B=1, T=33, M=80, bias=6.0)
for _u in TWO_OUTPUT_UPS:
    case("dur_loss_ups_%g_%g" % _u, "_DurLossFn", "bounded", ("dur_pred",), ups=_u, B=3, T=33, T_txt=14, lam_p=0.1, lam_w=1.0)
    case("pitch_loss_ups_%g_%g" % _u, "_PitchLossFn", "bounded", ("pp",), ups=_u, B=3, T=33, lam_uv=1.0, lam_f0=0.5)
case("pitch_loss_b1_t1", "_PitchLossFn", "bounded", ("pp",), ups=(3.0, 0.25), B=1, T=1, lam_uv=1.0, lam_f0=1.0)
SWAP_CASES = ("dur_loss_ups_3_0.25", "pitch_loss_ups_3_0.25", "res_skip_ups_3_0.25")

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the case a `needs_input_grad[i]` read of a backward is checked by: node -> {i: (case, operand)}; the inventory holds it to the source
NEEDS_INPUT_GRAD = {
    "_Conv1dFn": {0: "x", 1: "w", 2: "b", 3: "add", 4: "res"},
    "_AddChanMaskFn": {1: "add"}, "_PreLnCrossAttnFn": {1: "enc"}, "_PosAddFn": {1: "alpha"}, "_AddMaskedFn": {0: "a"},
}
# forward argument -> the operand name the cases use
ARG_NAMES = {"bias": "bias", "chan_add": "chan_add", "res": "res", "t_out": "t_out", "mask": "mask", "drop": "drop", "base": "base",
             "padding_idx": "padding_idx", "skip_in": "skip_in", "add": "add", "kpm": "kpm"}


# =====================================================================================================================================
# evaluation
# =====================================================================================================================================
_OPS, _REF = {}, {}


def operands(cs):
    """the case's operands (fp32 / int64 CPU tensors, by name): made once, shared, never changed"""
    if cs["name"] not in _OPS:
        c = cs["c"]
        seed = sum(ord(ch) for ch in cs["name"].rsplit("_ups_", 1)[0])  # (the same operands under every pair of upstream scalars)
        _OPS[cs["name"]] = OPERANDS[cs["node"]](c, Draw(cs["mode"], seed))
    return _OPS[cs["name"]]


def upstream(cs, outs):
    """one upstream gradient per differentiable output: the given scalars for 0-d outputs, else a draw of the output's shape (times the
    case's `up_scale` per output, so that the two outputs of a node never receive interchangeable gradients)"""
    d = Draw(cs["mode"], 4242 + len(cs["name"]))
    ups = []
    for i, o in enumerate(outs):
        if o.dim() == 0:
            ups.append(torch.tensor(cs["ups"][i], dtype=torch.float32))
        else:
            s = cs["c"].get("up_scale", (1.0,) * len(outs))[i]
            ups.append(d(*o.shape) * s)
    return ups


def n_diff_outputs(cs):
    """the outputs that carry a gradient (the attention probabilities do not)"""
    return 1 if cs["node"] in ("_AttnFn", "_PreLnCrossAttnFn") else None


def evaluate(cs, dtype, fault=None, ups=None):
    """-> (outputs, {operand: gradient}) of the model in `dtype` with the case's upstream gradients (or `ups`)"""
    t = {k: (v.detach().clone().to(dtype).requires_grad_(k in cs["diff"]) if v.is_floating_point() else v) for k, v in operands(cs).items()}
    c = dict(cs["c"], fault=fault) if fault else cs["c"]
    if cs["node"] == "_SSIMLossFn" and dtype == torch.float32:
        loss, dpred = ssim_mirror(t, c, float(cs["ups"][0]) if ups is None else float(ups[0]))
        return [loss], dict(pred=dpred)
    with torch.enable_grad():
        outs = MODELS[cs["node"]](t, c)
        nd = n_diff_outputs(cs) or len(outs)
        if ups is None:
            ups = upstream(cs, [o.detach() for o in outs[:nd]])
        loss = sum((o * u.to(dtype)).sum() for o, u in zip(outs[:nd], ups))
        grads = torch.autograd.grad(loss, [t[k] for k in cs["diff"]], allow_unused=True)
    return [o.detach() for o in outs], {k: (torch.zeros_like(t[k]) if g is None else g.detach()) for k, g in zip(cs["diff"], grads)}


def reference(cs):
    """-> dict(outs, grads: the float64 model; m_outs, m_grads: the float32 mirror; ups), computed once per case"""
    if cs["name"] not in _REF:
        outs, grads = evaluate(cs, F64)
        m_outs, m_grads = evaluate(cs, torch.float32)
        nd = n_diff_outputs(cs) or len(outs)
        _REF[cs["name"]] = dict(outs=outs, grads=grads, m_outs=m_outs, m_grads=m_grads, ups=upstream(cs, outs[:nd]))
    return _REF[cs["name"]]


def bar(model, mirror):
    return mirror_bar(model.numpy(), mirror.double().numpy())
