"""HiFi-GAN's multi-period discriminator as the generator step uses it (modules/vocoder/hifigan/hifigan.py:154-223, 301-338;
tasks/vocoder/hifigan.py:26-50), on the GPU (csrc/sconv.hip):

    mpd = MultiPeriodDiscriminator().cuda()
    _, y_d_gs, fmap_rs, fmap_gs = mpd(y, y_)                   # y, y_: [B, 1, T] fp32; y_ = the generator's output
    a_p = generator_loss(y_d_gs) * hparams['lambda_adv']
    fm_f = feature_loss(fmap_rs, fmap_gs)
    (a_p + fm_f).backward()                                    # -> y_.grad

Built: the forward on both waveforms with every feature map, the three loss functions, the gradient with respect to the generated
waveform, and -- after `trainable_()` -- the discriminator step (tasks/vocoder/hifigan.py:51-61, csrc/disc_wgrad.hip):

    mpd = MultiPeriodDiscriminator().cuda().trainable_()
    y_d_rs, y_d_gs, _, _ = mpd(y, y_.detach())
    r, f = discriminator_loss(y_d_rs, y_d_gs)
    (r + f).backward()                                         # -> .grad of every parameter; torch.optim.AdamW(mpd.parameters()).step()

Without `trainable_()` nothing changes: the parameters are created with requires_grad=False and one that requires grad raises under
grad mode instead of silently getting none.  With it the parameters are inputs of the autograd node, the real SCORE is differentiable
(the real MAPS stay targets, as feature_loss defines them), the backward runs the input-gradient chain over all 2 B (p) rows and after
each layer its weight / bias gradient and the backward of the weight-norm (or spectral-norm) fold; the waveform gradient is computed
only when y_hat requires grad, a frozen parameter costs no launch.  A gradient that reaches the generated maps while the weights are
trainable (feature_loss) flows into the weights through the generated rows and into y_hat as before.  Everything runs on the compute
stream (moving the weight gradients to the leaf stream is a follow-up).  Not built: the conditional input (use_cond) and spectral norm
for the MPD.

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


def _all_rows(g_real, g_gen, shape, like):
    """The gradient over all rows [real; generated] of a chain from the two halves' (either may be None: zeros)."""
    R, Cc, H = shape
    halves = [torch.zeros(R // 2, Cc, H, dtype=torch.float32, device=like.device) if g is None else g.reshape(R // 2, Cc, H) for g in (g_real, g_gen)]
    return torch.cat(halves, 0)


def _chain_bwd(descr, maps, dz, adds, want, to_first, sentinel):
    """The backward of layers n - 1 .. 1 of one chain over the rows of `maps`.  descr[i] = (dgrad, operand, K, stride, pad, groups);
    maps[i - 1]: the input of layer i; dz: the gradient at the last layer's output; adds[i - 1]: what arrives at map i - 1 from outside
    (or None); want[i] = (weight?, bias?).  Per layer the weight / bias gradient, then the input gradient -- the walk stops where
    nothing below wants one (`to_first`: the first layer does).  -> (dz at the first layer's pre-activation or None, [(dW, db)])."""
    n = len(descr)
    grads = [(None, None)] * n
    for i in range(n - 1, 0, -1):
        run, op, K, s, pad, groups = descr[i]
        f_in = maps[i - 1]
        wdw, wdb = want[i]
        if wdw or wdb:
            grads[i] = ops.gconv1d_wgrad(dz, f_in, K, stride=s, pad=pad, groups=groups, want_dw=wdw, want_db=wdb, sentinel=sentinel)
        if not (to_first or any(a or b for a, b in want[1:i])):
            return None, grads
        dz = run(dz, op, f_in.shape[2], stride=s, pad=pad, f_in=f_in, add=adds[i - 1], slope=LRELU_SLOPE, sentinel=sentinel)
    return dz, grads


class _DiscPFn(torch.autograd.Function):
    """One sub-discriminator on both signals.  Outputs: the generated score and six generated maps (differentiable in y_hat), then the
    real score and maps (not differentiable).  With the discriminator's parameters behind the four fixed inputs (trainable_): the
    real score is differentiable too and the backward also yields the parameters' gradients."""

    @staticmethod
    def forward(ctx, y_hat, y, mod, sentinel, *params):
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
        ctx.mod, ctx.sentinel, ctx.dims, ctx.n_params = mod, sentinel, (B, T, p), len(params)
        if params:
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(*maps[:-1], y, y_hat, *params)
        else:
            ctx.save_for_backward(*gen[:-1])
        outs_g = [_rows_to_map(m, B, p) for m in gen]
        outs_r = [_rows_to_map(m, B, p) for m in real]
        score_g, score_r = outs_g[-1].reshape(B, -1), outs_r[-1].reshape(B, -1)
        if params:
            ctx.mark_non_differentiable(*outs_r)
        else:
            ctx.mark_non_differentiable(score_r, *outs_r)
        return (score_g, *outs_g, score_r, *outs_r)

    @staticmethod
    def _backward_trainable(ctx, g_score, g_maps, g_score_r):
        """The discriminator step's backward: the dgrad chain over all 2 B p rows, each layer's weight / bias gradient from the same dz,
        the weight-norm fold's backward, and d / d y_hat only when it is asked for."""
        B, T, p = ctx.dims
        n_par = ctx.n_params
        none = (None,) * (4 + n_par)
        if g_score is None and g_score_r is None and all(g is None for g in g_maps):
            return none
        saved = ctx.saved_tensors
        maps, y, y_hat, params = saved[:5], saved[5], saved[6], saved[7:]
        need = ctx.needs_input_grad
        convs = ctx.mod._layers()
        Rg, dev = B * p, y.device
        H6 = ops.sconv_out_len(maps[4].shape[2], convs[5][0].K, convs[5][2], convs[5][3])

        def rows_of_score(g):
            return None if g is None else g.reshape(B, -1, p).permute(0, 2, 1).reshape(Rg, 1, -1)
        dz_g = None if g_maps[5] is None else _map_to_rows(g_maps[5], B, p)
        gs = rows_of_score(g_score)
        dz_g = gs if dz_g is None else (dz_g if gs is None else dz_g + gs)
        dz = _all_rows(rows_of_score(g_score_r), dz_g, (2 * Rg, 1, H6), y)
        adds = [None if g is None else _all_rows(None, _map_to_rows(g, B, p), tuple(maps[i].shape), y) for i, g in enumerate(g_maps[:5])]
        want = [(need[4 + 3 * i] or need[5 + 3 * i], need[6 + 3 * i]) for i in range(6)]
        descr = [None] + [(ops.sconv1d_dgrad, cw, cw.K, s, pad, 1) for cw, _b, s, pad, _act in convs[1:]]
        dz, grads = _chain_bwd(descr, maps, dz, adds, want, need[0] or any(want[0]), ctx.sentinel)
        cw0, _b0, s0, pad0, _a0 = convs[0]
        if any(want[0]):
            grads[0] = ops.mpd_fold_conv_wgrad(dz, y, y_hat, p, cw0.K, stride=s0, pad=pad0, want_dw=want[0][0], want_db=want[0][1], sentinel=ctx.sentinel)
        g_wav = ops.mpd_fold_conv_bwd(dz[Rg:], cw0.raw(), B, T, p, stride=s0, pad=pad0, sentinel=ctx.sentinel) if need[0] else None
        out = [g_wav, None, None, None]
        for i, (dw, db) in enumerate(grads):
            g, v = params[3 * i], params[3 * i + 1]
            dg, dv = (None, None) if dw is None else ops.weight_norm_fold_bwd(dw, g, v, want_dg=need[4 + 3 * i], want_dv=need[5 + 3 * i],
                                                                              sentinel=ctx.sentinel)
            out += [dg, dv, db]
        return tuple(out)

    @staticmethod
    def backward(ctx, g_score, *rest):
        B, T, p = ctx.dims
        g_maps = list(rest[:6])
        if ctx.n_params:
            return _DiscPFn._backward_trainable(ctx, g_score, g_maps, rest[6])
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
        self._trainable = False

    def trainable_(self, flag=True):
        """Opt in to (or out of) the discriminator step: the parameters require grad, become inputs of the autograd node and get
        `.grad` from a backward through the scores (real and generated); the real MAPS stay targets.  Without it nothing changes."""
        self._trainable = bool(flag)
        for q in self.parameters():
            q.requires_grad_(self._trainable)
        return self

    def _params(self):
        """The node's parameter inputs while trainable: (weight_g, weight_v, bias) per layer."""
        if not (self._trainable and torch.is_grad_enabled()):
            return ()
        return tuple(q for m in list(self.convs) + [self.conv_post] for q in (m.weight_g, m.weight_v, m.bias))

    def _layers(self):
        """[(ConvWeight, bias, stride, pad, leaky ReLU?)] of the six layers."""
        mods = list(self.convs) + [self.conv_post]
        return [(wn.conv_weight(), m.bias.data, m.stride[0], m.padding[0], i < 5) for i, (wn, m) in enumerate(zip(self._wn, mods))]

    def _check_weights(self):
        if torch.is_grad_enabled() and not self._trainable:
            for name, q in self.named_parameters():
                if q.requires_grad:
                    raise RuntimeError("%s requires grad: the discriminator's weight gradients are not built (only d/d y_hat is); "
                                       "keep its parameters at requires_grad=False" % name)

    def forward(self, y, y_hat, mel=None, sentinel=None):
        y2, yh2 = _check_waves(y, y_hat)
        self._check_weights()
        outs = _DiscPFn.apply(yh2, y2, self, sentinel, *self._params())
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


def _trainable_all(self, flag=True):
    """trainable_ of every sub-discriminator (see DiscriminatorP.trainable_)."""
    for d in self.discriminators:
        d.trainable_(flag)
    return self


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

    trainable_ = _trainable_all

    def forward(self, y, y_hat, mel=None, sentinel=None):
        y2, yh2 = _check_waves(y, y_hat)
        n = len(self.discriminators)
        fan = _FanOut.apply(yh2, n) if torch.is_grad_enabled() and yh2.requires_grad else (yh2,) * n
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d, yh in zip(self.discriminators, fan):
            d._check_weights()
            outs = _DiscPFn.apply(yh, y2, d, sentinel, *d._params())
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

    def _sigma(self):
        m = self.mod
        w = m.weight_orig
        return torch.dot(m.weight_u, torch.mv(w.reshape(w.shape[0], -1), m.weight_v))

    def _sigma_fold(self):
        return self.mod.weight_orig / self._sigma()

    def sn_state(self):
        """(u, v, sigma) as they stand, copied: what the spectral-norm fold's backward needs of the forward that just ran (the
        buffers move in place with the next power iteration)."""
        m = self.mod
        with torch.no_grad():
            return m.weight_u.clone(), m.weight_v.clone(), self._sigma().reshape(1)

    def params(self):
        """The autograd node's inputs for this conv: (weight_orig, bias) or (weight_g, weight_v, bias)."""
        m = self.mod
        return (m.weight_orig, m.bias) if self.spectral else (m.weight_g, m.weight_v, m.bias)

    def fold_bwd(self, dw, state, need, out, sentinel):
        """dW -> the gradients of this conv's weight parameters, in params() order.  Spectral norm: `state` = (u, v, sigma) of the
        forward; `out`: the back-projection so far (the other half's), to add to."""
        if dw is None:
            return [out] if self.spectral else [None, None]
        m = self.mod
        if self.spectral:
            u, v, sigma = state
            return [ops.spectral_norm_fold_bwd(dw, m.weight_orig.detach().contiguous(), u, v, sigma, out=out, accumulate=out is not None,
                                               sentinel=sentinel)]
        return list(ops.weight_norm_fold_bwd(dw, m.weight_g.detach().contiguous(), m.weight_v.detach().contiguous(), want_dg=need[0],
                                             want_dv=need[1], sentinel=sentinel))

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
    def forward(ctx, y_hat, y, mod, sentinel, *params):
        B, T = y_hat.shape
        convs = mod._convs
        n = len(convs)
        sn = mod.use_spectral_norm
        w_real = st_real = st_gen = maps = None
        if sn and mod.training:   # the reference's two calls: real first, then generated, one power iteration each
            w_real = [c.power_step() for c in convs]
            st_real = [c.sn_state() for c in convs] if params else None
            real = _disc_s_run(convs, w_real, y, None, sentinel)
            w_gen = [c.power_step() for c in convs]
            st_gen = [c.sn_state() for c in convs] if params else None
            gen = _disc_s_run(convs, w_gen, y_hat, None, sentinel)
        else:
            w_gen = [c.fixed() for c in convs]
            st_gen = [c.sn_state() for c in convs] if params and sn else None
            maps = _disc_s_run(convs, w_gen, y, y_hat, sentinel)
            real, gen = [m[:B] for m in maps], [m[B:] for m in maps]
        ctx.convs, ctx.weights, ctx.sentinel, ctx.n, ctx.n_params = convs, w_gen, sentinel, n, len(params)
        score_g, score_r = gen[-1].reshape(B, -1), real[-1].reshape(B, -1)
        if params:
            ctx.set_materialize_grads(False)
            ctx.halves, ctx.weights_real, ctx.states = maps is None, w_real, (st_real, st_gen)
            ctx.save_for_backward(*(real[:-1] + gen[:-1] if maps is None else maps[:-1]), y, y_hat, *params)
            ctx.mark_non_differentiable(*real)
        else:
            ctx.save_for_backward(*gen[:-1])
            ctx.mark_non_differentiable(score_r, *real)
        return (score_g, *gen, score_r, *real)

    @staticmethod
    def _backward_trainable(ctx, g_score, g_maps, g_score_r):
        """The discriminator step's backward.  One chain over all 2 B rows; a spectrally normed net in train() ran its halves with
        different weights and different u, v, so there the chain, the weight gradients and the fold's back-projection run per half and
        weight_orig.grad is the sum of the two back-projections, the real half's first."""
        n, n_par, convs, sentinel = ctx.n, ctx.n_params, ctx.convs, ctx.sentinel
        if g_score is None and g_score_r is None and all(g is None for g in g_maps):
            return (None,) * (4 + n_par)
        saved = ctx.saved_tensors
        n_maps = 2 * (n - 1) if ctx.halves else n - 1
        y, y_hat = saved[n_maps], saved[n_maps + 1]
        B = y.shape[0]
        need = ctx.needs_input_grad
        first, want = [], []
        at = 4
        for c in convs:
            k = len(c.params())
            first.append(at)
            want.append((any(need[at:at + k - 1]), need[at + k - 1]))
            at += k
        H_last = convs[-1].out_len(saved[n - 2].shape[2])
        dz_g = None if g_maps[-1] is None else g_maps[-1].contiguous()
        if g_score is not None:
            gs = g_score.reshape(B, 1, H_last)
            dz_g = gs.contiguous() if dz_g is None else dz_g + gs
        dz_r = None if g_score_r is None else g_score_r.reshape(B, 1, H_last).contiguous()
        adds_g = [None if g is None else g.contiguous() for g in g_maps[:-1]]

        def descr(weights):
            return [None] + [(ops.sconv1d_dgrad if c.kind == "dense" else ops.gconv1d_dgrad, w[1], c.K, c.stride, c.pad, c.groups)
                             for c, w in zip(convs[1:], weights[1:])]
        c0 = convs[0]
        g_wav = None
        runs = []   # per chain: ([(dW, db)], the forward's (u, v, sigma) per conv)
        if not ctx.halves:
            maps = saved[:n - 1]
            dz = _all_rows(dz_r, dz_g, (2 * B, 1, H_last), y)
            adds = [None if g is None else _all_rows(None, g, tuple(m.shape), y) for g, m in zip(adds_g, maps)]
            dz, grads = _chain_bwd(descr(ctx.weights), maps, dz, adds, want, need[0] or any(want[0]), sentinel)
            if any(want[0]):
                grads[0] = ops.wave_conv_wgrad(dz, y, y_hat, c0.K, pad=c0.pad, want_dw=want[0][0], want_db=want[0][1], sentinel=sentinel)
            if need[0]:
                g_wav = ops.wave_conv_bwd(dz[B:], ctx.weights[0][0], pad=c0.pad, sentinel=sentinel)
            runs.append((grads, ctx.states[1]))
        else:
            if dz_r is not None:
                dz, grads = _chain_bwd(descr(ctx.weights_real), saved[:n - 1], dz_r, [None] * (n - 1), want, any(want[0]), sentinel)
                if any(want[0]):
                    grads[0] = ops.wave_conv_wgrad(dz, y, None, c0.K, pad=c0.pad, want_dw=want[0][0], want_db=want[0][1], sentinel=sentinel)
                runs.append((grads, ctx.states[0]))
            if dz_g is not None or any(a is not None for a in adds_g):
                if dz_g is None:
                    dz_g = torch.zeros(B, 1, H_last, dtype=torch.float32, device=y.device)
                dz, grads = _chain_bwd(descr(ctx.weights), saved[n - 1:n_maps], dz_g, adds_g, want, need[0] or any(want[0]), sentinel)
                if any(want[0]):
                    grads[0] = ops.wave_conv_wgrad(dz, y_hat, None, c0.K, pad=c0.pad, want_dw=want[0][0], want_db=want[0][1], sentinel=sentinel)
                if need[0]:
                    g_wav = ops.wave_conv_bwd(dz, ctx.weights[0][0], pad=c0.pad, sentinel=sentinel)
                runs.append((grads, ctx.states[1]))
        out = [g_wav, None, None, None]
        for i, c in enumerate(convs):
            k = len(c.params())
            gw, gb = [None] * (k - 1), None
            for grads, states in runs:
                dw, db = grads[i]
                if dw is not None:
                    gw = c.fold_bwd(dw, states[i] if states else None, need[first[i]:first[i] + k - 1], gw[0], sentinel)
                if db is not None:
                    gb = db if gb is None else gb + db
            out += gw + [gb]
        return tuple(out)

    @staticmethod
    def backward(ctx, g_score, *rest):
        n = ctx.n
        g_maps = list(rest[:n])
        if ctx.n_params:
            return _DiscSFn._backward_trainable(ctx, g_score, g_maps, rest[n])
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
        self._trainable = False

    _check_weights = DiscriminatorP._check_weights
    trainable_ = DiscriminatorP.trainable_

    def _params(self):
        """The node's parameter inputs while trainable: per conv (weight_orig, bias) under spectral norm, else (weight_g, weight_v, bias)."""
        if not (self._trainable and torch.is_grad_enabled()):
            return ()
        return tuple(q for c in self._convs for q in c.params())

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
        outs = _DiscSFn.apply(yh2, y2, self, sentinel, *self._params())
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

    trainable_ = _trainable_all

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
            outs = _DiscSFn.apply(yh_i, y2, d, sentinel, *d._params())
            y_d_rs.append(outs[n + 1])
            y_d_gs.append(outs[0])
            fmap_rs.append(list(outs[n + 2:2 * n + 2]))
            fmap_gs.append(list(outs[1:n + 1]))
            y2, yh2 = y_next, yh_next
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs
