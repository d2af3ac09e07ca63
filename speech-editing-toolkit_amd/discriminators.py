"""HiFi-GAN's multi-period discriminator as the generator step uses it (modules/vocoder/hifigan/hifigan.py:154-223, 301-338;
tasks/vocoder/hifigan.py:26-50), on the GPU (csrc/sconv.hip):

    mpd = MultiPeriodDiscriminator().cuda()
    _, y_d_gs, fmap_rs, fmap_gs = mpd(y, y_)                   # y, y_: [B, 1, T] fp32; y_ = the generator's output
    a_p = generator_loss(y_d_gs) * hparams['lambda_adv']
    fm_f = feature_loss(fmap_rs, fmap_gs)
    (a_p + fm_f).backward()                                    # -> y_.grad

Built: the forward on both waveforms with every feature map, the three loss functions, and the gradient with respect to the generated
waveform.  Not built: gradients with respect to the discriminator's own weights (the discriminator step) -- the parameters are created
with requires_grad=False and one that requires grad raises under grad mode instead of silently getting none --, the conditional input
(use_cond) and spectral norm.

Layout: the reference folds [B, 1, T] into [B, 1, H, p] and runs (K, 1) Conv2d layers that never mix the p columns; here every (b, w)
column is a row of its own and a layer's activations are one [2 B p, C, H] buffer, the real signal's rows first.  A returned feature
map is `rows.view(B, p, C, H).permute(0, 2, 3, 1)`: the reference's [B, C, H, p] shape and values without a copy.  All six layers run
on set_sconv1d_fwd / set_sconv1d_dgrad (the stride-1 fifth conv and conv_post with s = 1: set_conv1d has no gate epilogue for the
backward, and one kernel pair keeps one summation order across the stack); the first layer reads the waveforms directly.

`y` is data: a `y` that requires grad raises.  There is no CPU fallback.

The multi-scale discriminator (hifigan.py:226-298, csrc/msd.hip) follows the same rules: `MultiScaleDiscriminator` / `DiscriminatorS`
below, with spectral norm for its first scale; the three loss functions take its [B, C, H] maps as they take the MPD's.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm, weight_norm

from . import ops
from .hifigan import _WNConv

LRELU_SLOPE = 0.1
PERIODS = (2, 3, 5, 7, 11)


class _WNConv2d(_WNConv):
    """The folded-weight cache of a weight-normed (K, 1) Conv2d: its [Cout, Cin, K, 1] weight is a [Cout, Cin, K] conv1d weight."""

    def conv_weight(self):
        w = self.folded()
        if self._cw is None:
            cout, cin, k, _one = w.shape
            self._cw = ops.ConvWeight((self._fold, "value"), cout, cin, k)
        return self._cw


def _rows_to_map(rows, B, p):
    """[B p, C, H] -> the reference's [B, C, H, p] (a view)."""
    _R, Cc, H = rows.shape
    return rows.view(B, p, Cc, H).permute(0, 2, 3, 1)


def _map_to_rows(g, B, p):
    """A gradient in [B, C, H, p] -> contiguous [B p, C, H] (no copy when it has the layout of the map it belongs to)."""
    t = g.permute(0, 3, 1, 2)
    if not t.is_contiguous():
        t = t.contiguous()
    return t.view(B * p, t.shape[2], t.shape[3])


class _DiscPFn(torch.autograd.Function):
    """One sub-discriminator on both signals.  Outputs: the generated score and six generated maps (differentiable in y_hat), then the
    real score and maps (not differentiable)."""

    @staticmethod
    def forward(ctx, y_hat, y, mod, sentinel):
        B, T = y_hat.shape
        p = mod.period
        convs = mod._layers()
        (cw0, b0, s0, pad0, _a0) = convs[0]
        maps = [ops.mpd_fold_conv_fwd(y, y_hat, cw0.raw(), b0, p, stride=s0, pad=pad0, slope=LRELU_SLOPE, sentinel=sentinel)]
        for cw, b, s, pad, act in convs[1:]:
            maps.append(ops.sconv1d_fwd(maps[-1], cw, b, stride=s, pad=pad, slope=LRELU_SLOPE if act else None, sentinel=sentinel))
        Rg = B * p
        gen = [m[Rg:] for m in maps]
        real = [m[:Rg] for m in maps]
        ctx.mod, ctx.sentinel, ctx.dims = mod, sentinel, (B, T, p)
        ctx.save_for_backward(*gen[:-1])
        outs_g = [_rows_to_map(m, B, p) for m in gen]
        outs_r = [_rows_to_map(m, B, p) for m in real]
        score_g, score_r = outs_g[-1].reshape(B, -1), outs_r[-1].reshape(B, -1)
        ctx.mark_non_differentiable(score_r, *outs_r)
        return (score_g, *outs_g, score_r, *outs_r)

    @staticmethod
    def backward(ctx, g_score, *rest):
        B, T, p = ctx.dims
        g_maps = list(rest[:6])
        if g_score is None and all(g is None for g in g_maps):
            return None, None, None, None
        saved = ctx.saved_tensors
        convs = ctx.mod._layers()
        adds = [None if g is None else _map_to_rows(g, B, p) for g in g_maps]
        H_last = saved[-1].shape[2] if len(saved) else None
        dz = adds[5]
        if g_score is not None:  # the score is the last map flattened in (h, w) order
            gs = g_score.reshape(B, -1, p).permute(0, 2, 1).reshape(B * p, 1, -1)
            dz = gs.contiguous() if dz is None else dz + gs
        if dz is None:
            H6 = ops.sconv_out_len(H_last, convs[5][0].K, convs[5][2], convs[5][3])
            dz = torch.zeros(B * p, 1, H6, dtype=torch.float32, device=saved[0].device)
        # top down: dz of layer i's input = gate(map i - 1) * (dgrad of layer i + the gradient arriving at map i - 1 from outside)
        for i in range(5, 0, -1):
            cw, _b, s, pad, _act = convs[i]
            f_in = saved[i - 1]
            dz = ops.sconv1d_dgrad(dz, cw, f_in.shape[2], stride=s, pad=pad, f_in=f_in, add=adds[i - 1], slope=LRELU_SLOPE, sentinel=ctx.sentinel)
        cw0, _b0, s0, pad0, _a0 = convs[0]
        g_wav = ops.mpd_fold_conv_bwd(dz, cw0.raw(), B, T, p, stride=s0, pad=pad0, sentinel=ctx.sentinel)
        return g_wav, None, None, None


class DiscriminatorP(nn.Module):
    """hifigan.py:154-196 with the reference's parameter names (convs.{i}.weight_g / weight_v / bias, conv_post.*; weight_v
    [Cout, Cin, K, 1]): a `model_disc['mpd']` checkpoint loads with strict=True.  `channels` is ours (narrow nets for tests).

    forward(y, y_hat) -> (score_r, score_g, fmap_r, fmap_g): scores [B, H p], maps [B, C, H, p] as the reference's, for the real and
    the generated waveform ([B, T] or [B, 1, T]); the generated outputs are differentiable in y_hat, the real ones detached."""

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False, use_cond=False, c_in=1, channels=(32, 128, 512, 1024, 1024)):
        super().__init__()
        if use_cond or use_spectral_norm or c_in != 1:
            raise NotImplementedError("DiscriminatorP is built without the conditional input (use_cond) and without spectral norm")
        if len(channels) != 5:
            raise ValueError("channels must name the five conv widths, got %r" % (channels,))
        self.period, self.kernel_size, self.stride = int(period), int(kernel_size), int(stride)
        chans = [1] + [int(c) for c in channels]
        # hifigan.py:167-171: padding (get_padding(5, 1), 0) = (2, 0) whatever the kernel size
        self.convs = nn.ModuleList([weight_norm(nn.Conv2d(chans[i], chans[i + 1], (kernel_size, 1), (stride if i < 4 else 1, 1), padding=(2, 0)))
                                    for i in range(5)])
        self.conv_post = weight_norm(nn.Conv2d(chans[5], 1, (3, 1), 1, padding=(1, 0)))
        for q in self.parameters():
            q.requires_grad_(False)
        self._wn = [_WNConv2d(m) for m in list(self.convs) + [self.conv_post]]

    def _layers(self):
        """[(ConvWeight, bias, stride, pad, leaky ReLU?)] of the six layers."""
        mods = list(self.convs) + [self.conv_post]
        return [(wn.conv_weight(), m.bias.data, m.stride[0], m.padding[0], i < 5) for i, (wn, m) in enumerate(zip(self._wn, mods))]

    def _check_weights(self):
        if torch.is_grad_enabled():
            for name, q in self.named_parameters():
                if q.requires_grad:
                    raise RuntimeError("%s requires grad: the discriminator's weight gradients are not built (only d/d y_hat is); "
                                       "keep its parameters at requires_grad=False" % name)

    def forward(self, y, y_hat, mel=None, sentinel=None):
        y2, yh2 = _check_waves(y, y_hat)
        self._check_weights()
        outs = _DiscPFn.apply(yh2, y2, self, sentinel)
        return outs[7], outs[0], list(outs[8:14]), list(outs[1:7])


def _check_waves(y, y_hat):
    for t, name in ((y, "y"), (y_hat, "y_hat")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("%s must live on the GPU: the discriminator has no CPU fallback" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if y.requires_grad:
        raise ValueError("y is data: the discriminator has no gradient with respect to it (pass y.detach())")
    if y.shape != y_hat.shape or y.dim() not in (2, 3) or (y.dim() == 3 and y.shape[1] != 1):
        raise ValueError("y and y_hat must be equal [B, T] or [B, 1, T], got %s and %s" % (tuple(y.shape), tuple(y_hat.shape)))
    B, T = y.shape[0], y.shape[-1]
    return y.reshape(B, T).contiguous(), y_hat.reshape(B, T).contiguous()


class _FanOut(torch.autograd.Function):
    """n aliases of the generated waveform; backward adds their gradients in list order: (((g0 + g1) + g2) + g3) + g4."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g.contiguous() for g in gs if g is not None]
        if not gs:
            return None, None
        tot = gs[0]
        for i in range(1, len(gs), 2):
            tot = ops.sum_div(tot, gs[i], gs[i + 1] if i + 1 < len(gs) else None)
        return tot, None


class MultiPeriodDiscriminator(nn.Module):
    """hifigan.py:199-223: DiscriminatorP at periods 2, 3, 5, 7, 11.  forward(y, y_hat, mel=None) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs),
    the reference's structure and shapes; y, y_hat: fp32 GPU [B, 1, T] (or [B, T]) with T > 11; `mel` is ignored."""

    def __init__(self, use_cond=False, c_in=1, channels=(32, 128, 512, 1024, 1024)):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(p, use_cond=use_cond, c_in=c_in, channels=channels) for p in PERIODS])

    def forward(self, y, y_hat, mel=None, sentinel=None):
        y2, yh2 = _check_waves(y, y_hat)
        n = len(self.discriminators)
        fan = _FanOut.apply(yh2, n) if torch.is_grad_enabled() and yh2.requires_grad else (yh2,) * n
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d, yh in zip(self.discriminators, fan):
            d._check_weights()
            outs = _DiscPFn.apply(yh, y2, d, sentinel)
            y_d_rs.append(outs[7])
            y_d_gs.append(outs[0])
            fmap_rs.append(list(outs[8:14]))
            fmap_gs.append(list(outs[1:7]))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs


# ---- the loss functions of hifigan.py:301-338: one launch pair forward, one launch backward ---------------------------------------------

class _MultiLoss(torch.autograd.Function):
    """loss[slot] = scale * sum over the slot's items, in list order, of mean(term); gradients for the `a` operands that ask for one."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        modes, slots, scale, n_slots = spec
        n = len(modes)
        a_list, b_list = tensors[:n], tensors[n:]
        table, chunks, _host = ops.multi_loss_items(a_list, b_list, modes, slots)
        loss = ops.multi_loss_fwd(table, n, chunks, scale, n_slots)
        ctx.spec = spec
        ctx.save_for_backward(*tensors)
        return tuple(loss[k].reshape(()) for k in range(n_slots))

    @staticmethod
    def backward(ctx, *gouts):
        modes, slots, scale, n_slots = ctx.spec
        n = len(modes)
        tensors = ctx.saved_tensors
        a_list, b_list = tensors[:n], tensors[n:]
        dev = a_list[0].device
        u = torch.stack([torch.zeros((), dtype=torch.float32, device=dev) if g is None else g.reshape(()).float() for g in gouts]).contiguous()
        grads = [torch.empty_strided(a.shape, a.stride(), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1 + i] else None
                 for i, a in enumerate(a_list)]
        if any(g is not None for g in grads):
            table, chunks, _host = ops.multi_loss_items(a_list, b_list, modes, slots, grads)
            ops.multi_loss_bwd(table, n, chunks, scale, u)
        return (None, *grads, *([None] * n))


def _multi_loss(a_list, b_list, modes, slots, scale, n_slots):
    if len(a_list) == 0:
        raise ValueError("a loss over an empty list")
    spec = (tuple(ops.LOSS_MODES[m] for m in modes), tuple(slots), float(scale), n_slots)
    return _MultiLoss.apply(spec, *a_list, *b_list)


def feature_loss(fmap_r, fmap_g):
    """hifigan.py:301-307: 2 * sum over every layer of every sub-discriminator of mean |r - g|.  Differentiable in the generated maps;
    the real maps are targets."""
    a = [gl for dg in fmap_g for gl in dg]
    b = [rl for dr in fmap_r for rl in dr]
    if len(a) != len(b):
        raise ValueError("feature_loss: %d generated maps against %d real ones" % (len(a), len(b)))
    return _multi_loss(a, b, ["l1"] * len(a), [0] * len(a), 2.0, 1)[0]


def generator_loss(disc_outputs):
    """hifigan.py:332-338: (1 / D) sum of mean (1 - dg)^2."""
    a = list(disc_outputs)
    return _multi_loss(a, [None] * len(a), ["sq1"] * len(a), [0] * len(a), 1.0 / max(len(a), 1), 1)[0]


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """hifigan.py:310-320: (r_losses, g_losses) = (sum mean (1 - dr)^2, sum mean dg^2) / len(disc_real_outputs)."""
    r, g = list(disc_real_outputs), list(disc_generated_outputs)
    if len(r) != len(g):
        raise ValueError("discriminator_loss: %d real outputs against %d generated ones" % (len(r), len(g)))
    a = r + g
    out = _multi_loss(a, [None] * len(a), ["sq1"] * len(r) + ["sq0"] * len(g), [0] * len(r) + [1] * len(g), 1.0 / max(len(r), 1), 2)
    return out[0], out[1]


# ---- the multi-scale discriminator (hifigan.py:226-298; csrc/msd.hip) -------------------------------------------------------------------
#
#     msd = MultiScaleDiscriminator().cuda()
#     _, y_d_gs, fmap_rs, fmap_gs = msd(y, y_)
#     a_s = generator_loss(y_d_gs) * hparams['lambda_adv'];  fm_s = feature_loss(fmap_rs, fmap_gs)
#
# Three DiscriminatorS see y, pool(y), pool(pool(y)), pool = AvgPool1d(4, 2, padding=1).  Activations are [2 B, C, H] rows, the real
# signal's first; a returned map is one half of them.  Layer 1 reads the waveforms (set_wave_conv_*), the grouped 41-tap layers run on
# set_gconv1d_*, the dense 5- and 3-tap layers at the end on set_sconv1d_*.  The first discriminator is spectrally normed: in eval() its
# weights are weight_orig / sigma with the stored u, v (folded once per weight version); in train() the reference calls it twice per
# forward and each call does one power iteration, so the real rows see the weights after the first and the generated rows those after
# the second -- the layers then run once per half with an image each, and weight_u / weight_v are updated in place as torch does.
# sigma is a constant of d / d y_hat; the backward uses the generated rows' weights.
MSD_CHANNELS = (128, 128, 256, 512, 1024, 1024, 1024)
MSD_GROUPS = (1, 4, 16, 16, 16, 16, 1)
_MSD_KERNELS = (15, 41, 41, 41, 41, 41, 5)
_MSD_STRIDES = (1, 2, 2, 4, 4, 1, 1)


class _SConv:
    """One conv of a DiscriminatorS: its geometry, the weight it runs with and the operand the kernels take (the raw weight for the
    first layer, a ConvWeight for a dense layer of at most 7 taps, a GroupedConvWeight otherwise)."""

    def __init__(self, mod, spectral, act):
        self.mod, self.spectral, self.act = mod, spectral, act
        self.K, self.stride, self.pad, self.groups = mod.kernel_size[0], mod.stride[0], mod.padding[0], mod.groups
        self.cout, self.cin = mod.out_channels, mod.in_channels
        self.kind = "wave" if self.cin == 1 else ("dense" if self.groups == 1 and self.K <= 7 else "grouped")
        self._slot = ops.CacheSlot()

    def _with_operand(self, W):
        W = W.contiguous()
        if self.kind == "wave":
            return W, W
        if self.kind == "dense":
            return W, ops.ConvWeight(W, self.cout, self.cin, self.K)
        return W, ops.GroupedConvWeight(W, self.cout, self.cin, self.K, self.groups)

    def _sigma_fold(self):
        m = self.mod
        w = m.weight_orig
        sigma = torch.dot(m.weight_u, torch.mv(w.reshape(w.shape[0], -1), m.weight_v))
        return w / sigma

    def fixed(self):
        """(weight, operand) of a weight-normed conv, or of a spectrally normed one in eval(): cached per weight version."""
        m = self.mod
        if self.spectral:
            key = ops.weights_key((m.weight_orig, m.weight_u, m.weight_v))
            return self._slot.get(key, lambda _: self._with_operand(self._sigma_fold().detach()))
        g, v = m.weight_g, m.weight_v
        return self._slot.get(ops.weights_key((g, v)), lambda _: self._with_operand(ops.weight_norm_fold(g.contiguous(), v.contiguous())))

    def power_step(self):
        """One power iteration of torch.nn.utils.spectral_norm on weight_u / weight_v in place, then (weight_orig / sigma, operand)."""
        m = self.mod
        with torch.no_grad():
            wm = m.weight_orig.reshape(m.weight_orig.shape[0], -1)
            m.weight_v.copy_(F.normalize(torch.mv(wm.t(), m.weight_u), dim=0, eps=1e-12))
            m.weight_u.copy_(F.normalize(torch.mv(wm, m.weight_v), dim=0, eps=1e-12))
            return self._with_operand(self._sigma_fold())

    def out_len(self, H):
        return (H + 2 * self.pad - self.K) // self.stride + 1 if H + 2 * self.pad >= self.K else 0


def _disc_s_run(convs, weights, a, b, sentinel):
    """The eight maps [R, C, H] of the rows of `a` (and of `b` behind them when given) under `weights` [(weight, operand)]."""
    c0, (w0, _op0) = convs[0], weights[0]
    maps = [ops.wave_conv_fwd(a, b, w0, c0.mod.bias.data, pad=c0.pad, slope=LRELU_SLOPE if c0.act else None, sentinel=sentinel)]
    for c, (_w, op) in zip(convs[1:], weights[1:]):
        run = ops.sconv1d_fwd if c.kind == "dense" else ops.gconv1d_fwd
        maps.append(run(maps[-1], op, c.mod.bias.data, stride=c.stride, pad=c.pad, slope=LRELU_SLOPE if c.act else None, sentinel=sentinel))
    return maps


class _DiscSFn(torch.autograd.Function):
    """One DiscriminatorS on both signals.  Outputs: the generated score and maps (differentiable in y_hat), then the real ones (not)."""

    @staticmethod
    def forward(ctx, y_hat, y, mod, sentinel):
        B, T = y_hat.shape
        convs = mod._convs
        n = len(convs)
        if mod.use_spectral_norm and mod.training:   # the reference's two calls: real first, then generated, one power iteration each
            w_real = [c.power_step() for c in convs]
            real = _disc_s_run(convs, w_real, y, None, sentinel)
            w_gen = [c.power_step() for c in convs]
            gen = _disc_s_run(convs, w_gen, y_hat, None, sentinel)
        else:
            w_gen = [c.fixed() for c in convs]
            maps = _disc_s_run(convs, w_gen, y, y_hat, sentinel)
            real, gen = [m[:B] for m in maps], [m[B:] for m in maps]
        ctx.convs, ctx.weights, ctx.sentinel, ctx.n = convs, w_gen, sentinel, n
        ctx.save_for_backward(*gen[:-1])
        score_g, score_r = gen[-1].reshape(B, -1), real[-1].reshape(B, -1)
        ctx.mark_non_differentiable(score_r, *real)
        return (score_g, *gen, score_r, *real)

    @staticmethod
    def backward(ctx, g_score, *rest):
        n = ctx.n
        g_maps = list(rest[:n])
        if g_score is None and all(g is None for g in g_maps):
            return None, None, None, None
        saved, convs, weights = ctx.saved_tensors, ctx.convs, ctx.weights
        B = saved[0].shape[0]
        adds = [None if g is None else g.contiguous() for g in g_maps]
        H_last = convs[-1].out_len(saved[-1].shape[2])
        dz = adds[-1]
        if g_score is not None:
            gs = g_score.reshape(B, 1, H_last)
            dz = gs.contiguous() if dz is None else dz + gs
        if dz is None:
            dz = torch.zeros(B, 1, H_last, dtype=torch.float32, device=saved[0].device)
        # top down: dz of layer i's input = gate(map i - 1) * (dgrad of layer i + the gradient arriving at map i - 1 from outside)
        for i in range(n - 1, 0, -1):
            c, f_in = convs[i], saved[i - 1]
            run = ops.sconv1d_dgrad if c.kind == "dense" else ops.gconv1d_dgrad
            dz = run(dz, weights[i][1], f_in.shape[2], stride=c.stride, pad=c.pad, f_in=f_in, add=adds[i - 1], slope=LRELU_SLOPE,
                     sentinel=ctx.sentinel)
        return ops.wave_conv_bwd(dz, weights[0][0], pad=convs[0].pad, sentinel=ctx.sentinel), None, None, None


class DiscriminatorS(nn.Module):
    """hifigan.py:226-259 with the reference's parameter and buffer names (convs.{i}.bias / weight_g / weight_v, or weight_orig /
    weight_u / weight_v under spectral norm; conv_post.*).  `channels` and `groups` are ours (narrow nets for tests).

    forward(y, y_hat) -> (score_r, score_g, fmap_r, fmap_g): scores [B, H], eight maps [B, C, H] each."""

    def __init__(self, use_spectral_norm=False, use_cond=False, upsample_rates=None, c_in=1, channels=MSD_CHANNELS, groups=MSD_GROUPS):
        super().__init__()
        if use_cond or c_in != 1:
            raise NotImplementedError("DiscriminatorS is built without the conditional input (use_cond)")
        if len(channels) != 7 or len(groups) != 7 or groups[0] != 1:
            raise ValueError("channels and groups must name the seven conv widths and group counts (the first conv has one group)")
        self.use_spectral_norm = bool(use_spectral_norm)
        norm_f = spectral_norm if self.use_spectral_norm else weight_norm
        chans = [1] + [int(c) for c in channels]
        self.convs = nn.ModuleList([norm_f(nn.Conv1d(chans[i], chans[i + 1], _MSD_KERNELS[i], _MSD_STRIDES[i], groups=int(groups[i]),
                                                     padding=(_MSD_KERNELS[i] - 1) // 2)) for i in range(7)])
        self.conv_post = norm_f(nn.Conv1d(chans[7], 1, 3, 1, padding=1))
        for q in self.parameters():
            q.requires_grad_(False)
        mods = list(self.convs) + [self.conv_post]
        self._convs = [_SConv(m, self.use_spectral_norm, i < 7) for i, m in enumerate(mods)]

    _check_weights = DiscriminatorP._check_weights

    def _check_length(self, T):
        H = T
        for i, c in enumerate(self._convs):
            H = c.out_len(H)
            if H < 1:
                raise ValueError("DiscriminatorS: %d samples leave layer %d without an output frame" % (T, i + 1))

    def forward(self, y, y_hat, mel=None, sentinel=None):
        y2, yh2 = _check_waves(y, y_hat)
        self._check_weights()
        self._check_length(y2.shape[1])
        n = len(self._convs)
        outs = _DiscSFn.apply(yh2, y2, self, sentinel)
        return outs[n + 1], outs[0], list(outs[n + 2:2 * n + 2]), list(outs[1:n + 1])


class _PoolStep(torch.autograd.Function):
    """x -> (an alias of x for this scale's discriminator, pool(x) for the next scale).  Backward: g_alias + pool^T(g_pooled) in one launch,
    so the three scales' gradients meet as g0 + pool^T(g1 + pool^T(g2))."""

    @staticmethod
    def forward(ctx, x, sentinel):
        ctx.set_materialize_grads(False)
        ctx.T, ctx.sentinel = x.shape[1], sentinel
        return x.view_as(x), ops.avgpool4s2_fwd(x, sentinel=sentinel)

    @staticmethod
    def backward(ctx, g_alias, g_pooled):
        if g_pooled is None:
            return g_alias, None
        return ops.avgpool4s2_bwd(g_pooled.contiguous(), ctx.T, add=None if g_alias is None else g_alias.contiguous(), sentinel=ctx.sentinel), None


class MultiScaleDiscriminator(nn.Module):
    """hifigan.py:262-298: a spectrally normed DiscriminatorS on the waveform and two weight-normed ones on its 4 / 2 average pools.
    forward(y, y_hat, mel=None) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs), the reference's structure and shapes; y, y_hat: fp32 GPU [B, 1, T]
    (or [B, T]); `mel` is ignored.  Needs no hparams (they only size the conditional net, which is not built)."""

    def __init__(self, use_cond=False, c_in=1, channels=MSD_CHANNELS, groups=MSD_GROUPS):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorS(use_spectral_norm=(i == 0), use_cond=use_cond, c_in=c_in, channels=channels, groups=groups)
                                             for i in range(3)])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=1), nn.AvgPool1d(4, 2, padding=1)])

    def forward(self, y, y_hat, mel=None, sentinel=None):
        y2, yh2 = _check_waves(y, y_hat)
        T, D = y2.shape[1], len(self.discriminators)
        for i, d in enumerate(self.discriminators):
            d._check_weights()
            if T < 2 and i:
                raise ValueError("MultiScaleDiscriminator: the pool of scale %d has no output sample" % i)
            T = T if i == 0 else ops.avgpool4s2_out_len(T)
            d._check_length(T)
        track = torch.is_grad_enabled() and yh2.requires_grad
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        n = len(self.discriminators[0]._convs)
        for i, d in enumerate(self.discriminators):
            if i + 1 < D:
                yh_i, yh_next = _PoolStep.apply(yh2, sentinel) if track else (yh2, ops.avgpool4s2_fwd(yh2, sentinel=sentinel))
                y_next = ops.avgpool4s2_fwd(y2, sentinel=sentinel)
            else:
                yh_i, yh_next, y_next = yh2, None, None
            outs = _DiscSFn.apply(yh_i, y2, d, sentinel)
            y_d_rs.append(outs[n + 1])
            y_d_gs.append(outs[0])
            fmap_rs.append(list(outs[n + 2:2 * n + 2]))
            fmap_gs.append(list(outs[1:n + 1]))
            y2, yh2 = y_next, yh_next
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs
