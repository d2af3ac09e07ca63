"""Differentiable versions of the ops in ops.py (same names / signatures), for the training path.

torch.autograd is used as the tape only: every forward AND backward below is a kernel of libset_amd.so
(include/set_amd.h, "Training" section).  Ops without gradients (masks, integer bookkeeping) are re-exported
from ops.py unchanged.
"""
import ctypes as C
import functools
import os

import torch

from . import _lib, leaf_stream, ops
from ._lib import SetAmdError  # noqa: E402
from ._lib import ACT, PRO, IMPL_NAIVE, check
from .ops import _p, _stream, _uniform_stride, ConvWeight

# no-gradient ops: identical to the inference path
abs_sum_mask = ops.abs_sum_mask
index_mask = ops.index_mask
masked_dur = ops.masked_dur
pitch_coarse = ops.pitch_coarse
mul_one_minus_mask = ops.mul_one_minus_mask
blend_mask = ops.blend_mask
sinusoid_embed = ops.sinusoid_embed
q_sample = ops.q_sample
randn = ops.randn
length_regulate = ops.length_regulate

L = _lib.lib


# --------------------------------------------------------------------------------------------------
# Gradient targets and step-scoped temporaries: the zero arena, where a parameter gradient goes, the per-stream scratch pools
# --------------------------------------------------------------------------------------------------
class _ZeroArena:
    """Zero-initialised gradient temporaries (split-K wgrad targets, bias sums, scatter-add targets) of one training
    step come out of ONE buffer cleared by ONE memset, instead of ~300 separate small fills per step (each a launch
    of a few microseconds on the critical stream).  Opened by FlatAdamW.zero_grad() and closed by FlatAdamW.step():
    only then is it safe, because the optimizer owns every .grad (views of its flat buffer), so autograd ADDS these
    temporaries into .grad and nothing keeps a reference past the step.  Outside such a step `_gzeros` is torch.zeros.
    Capacity follows the demand of the previous step.  One arena per owner (optimizer)."""

    def __init__(self):
        self.buf, self.off, self.need = None, 0, 0


_ARENAS = {}        # owner id -> _ZeroArena
_ACTIVE = [None]    # the arena of the optimisation step in progress (steps do not nest)


def zero_arena_begin(device, min_floats=0, owner=None):
    a = _ARENAS.setdefault(id(owner), _ZeroArena())
    want = max(int(min_floats), int(a.need * 1.05) + 4096)
    if a.buf is None or a.buf.device != device or a.buf.numel() < want:
        if a.buf is not None and a.buf.device == device:
            want = max(want, int(a.buf.numel() * 1.5))
        a.buf = torch.empty(want, dtype=torch.float32, device=device)
    a.buf.zero_()
    a.off, a.need = 0, 0
    _ACTIVE[0] = a


def zero_arena_end():
    _ACTIVE[0] = None


def _gzeros(shape, device):
    a = _ACTIVE[0]
    shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    n = 1
    for d in shape:
        n *= d
    if a is not None and a.buf.device == device:
        step = (n + 63) // 64 * 64  # 256-byte aligned slices
        a.need += step
        if a.off + step <= a.buf.numel():
            t = a.buf[a.off:a.off + n].view(shape)
            a.off += step
            return t
    return torch.zeros(shape, dtype=torch.float32, device=device)


def grad_sink(param):
    """The optimizer-owned .grad view to accumulate a parameter gradient into, or None when the gradient has to travel through
    autograd (no flat optimizer, first step, parameter used more than once).  Asking counts as a use of the parameter during the
    optimizer's first step (FlatAdamW.sink): once per parameter and backward node, never for a row slice of a parameter."""
    owner = getattr(param, "_flat_owner", None) if param is not None else None
    return owner.sink(param) if owner is not None else None


def _tape_tgt(param, dev, cw=None):
    """(accumulation target, gradient to hand to autograd or None when the kernel writes the optimizer's .grad view in place): THE rule
    of every backward node below -- the .grad view when the flat optimizer owns the parameter, else a zeroed temporary of its shape.
    cw: the ConvWeight the node's conv reads the parameter through; a row slice of a larger parameter (packed q / k / v projections)
    never goes in place (and does not ask for the sink)."""
    whole = cw is None or (cw.base == 0 and param.numel() == cw.Cout * cw.Cin * cw.K)
    sink = grad_sink(param) if whole else None
    if sink is not None:
        return sink, None
    tmp = _gzeros(param.shape, dev)
    return tmp, tmp


def _grouped_targets(params, dev):
    """Where the gradients of one parameter kind of all layers go: (base pointer, element stride between layers, what to hand to
    autograd per layer).  In place when the flat optimizer owns every one of them at a uniform stride (its layout is: each layer's
    parameters contiguous, in the same order); otherwise one zeroed [L, ...] temporary whose slices autograd accumulates."""
    sinks = [grad_sink(p_) for p_ in params]
    n = params[0].numel()
    if all(t is not None for t in sinks):
        step = _uniform_stride(sinks)
        if step is not None:
            return sinks[0].data_ptr(), step, [None] * len(params)
        # owned, but not at a uniform stride (never seen with FlatAdamW): through autograd like unowned parameters
    tmp = _gzeros(len(params) * n, dev).view(len(params), *params[0].shape)
    return tmp.data_ptr(), n, [tmp[l] for l in range(len(params))]


def _leaves(dev, rets, *operands):
    """The block in which the gradient kernels of some parameters are launched: on the leaf stream when EVERY target is written in place
    (rets: what _tape_tgt / _grouped_targets hand to autograd for them, None for a .grad view) -- the optimizer is then their next
    reader; else where they stand, on the compute stream.  operands: every tensor those kernels read (leaf_stream.py: held until they
    have run; one left out is a race between the two streams).  Nothing may be allocated inside."""
    for r in rets:
        if r is not None:
            return leaf_stream.leaf_work(dev, False)
    return leaf_stream.leaf_work(dev, True, *operands)


_DET_SCRATCH = {}  # (device, stream) -> per-block / per-slice partial results of the ordered reductions (reused: stream-ordered)
_WG_SCRATCH = {}  # (device, stream) -> slice-partial buffer of the ordered weight-gradient path (reused: stream-ordered)


def _scratch(pool, slack, device, n_floats):
    """The current stream's buffer of `pool` (reused in stream order, so every stream has its own), regrown (x 1.25 + slack) when it is
    smaller than n_floats."""
    key = (device, _stream().value)
    buf = pool.get(key)
    if buf is None or buf.numel() < n_floats:
        if buf is not None:
            leaf_stream.hold_until_join(buf)
        buf = torch.empty(int(n_floats * 1.25) + slack, dtype=torch.float32, device=device)
        pool[key] = buf
    return buf


_det_scratch = functools.partial(_scratch, _DET_SCRATCH, 4096)  # (device, n_floats)
_wg_scratch = functools.partial(_scratch, _WG_SCRATCH, 1024)


# --------------------------------------------------------------------------------------------------
# The steps most backward nodes share
# --------------------------------------------------------------------------------------------------
def channel_sum_(x, out, B, Cc, T):
    """out[c] += sum_{b,t} x[b][c][t], per-slice partials combined in slice order (deterministic)."""
    check(L().set_channel_sum_det(_p(x), _p(out), B, Cc, T, _p(_det_scratch(x.device, 2048 + Cc)), _stream()), "set_channel_sum_det")


def conv_wgrad(g, x, chan_add, dw, B, Cin, Cout, K, dil, pad, T, T_in, pro=0, pro_param=0.0, dw_ptr=None, dtype=None):
    """dW[co][ci][tap] += sum_{b,t} G[b][co][t] * P(X[b][ci][t + tap*dil - pad] + chan_add[b][ci]).  MFMA shapes go
    through set_conv1d_wgrad_det (per-slice partial sums reduced in slice order: bit-stable, no atomics) with bf16 or
    fp32 operands according to ops.compute_dtype(); tiny T uses the one-thread-per-weight kernel."""
    ptr = C.c_void_p(dw.data_ptr() if dw_ptr is None else dw_ptr)
    if T < 16:
        check(L().set_conv1d_wgrad(_p(g), _p(x), _p(chan_add), ptr, B, Cin, Cout, K, dil, pad, T, T_in, pro,
                                   float(pro_param), IMPL_NAIVE, _stream()), "set_conv1d_wgrad")
        return
    if dtype is not None:
        dt = dtype  # bf16 operands already in HBM (fused layer kernels)
    else:
        dt = _lib.DTYPE_BF16 if (ops.compute_dtype() == "bf16" and Cout >= 32 and Cin >= 32) else _lib.DTYPE_F32
    buf = _wg_scratch(g.device, L().set_conv1d_wgrad_scratch_floats(B, Cin, Cout, K, T, dt))
    check(L().set_conv1d_wgrad_det(_p(g), _p(x), _p(chan_add), ptr, B, Cin, Cout, K, dil, pad, T, T_in, pro,
                                   float(pro_param), dt, _p(buf), buf.numel(), _stream()), "set_conv1d_wgrad_det")


def conv_wgrad_grouped(g, x, chan_add, dw_ptr, groups, g_gs, x_gs, add_gs, dw_gs, B, Cin, Cout, K, dil, pad, T, T_in, dtype):
    """`groups` equal bf16 weight-gradient GEMMs (the same conv of every residual layer) in one launch + one ordered reduce;
    group q reads g + q g_gs, x + q x_gs, chan_add + q add_gs and adds into dw_ptr + q dw_gs (element strides)."""
    buf = _wg_scratch(g.device, L().set_conv1d_wgrad_grouped_scratch_floats(groups, B, Cin, Cout, K, T))
    check(L().set_conv1d_wgrad_det_grouped(_p(g), _p(x), _p(chan_add), C.c_void_p(dw_ptr), groups, g_gs, x_gs, add_gs, dw_gs, B, Cin,
                                           Cout, K, dil, pad, T, T_in, dtype, _p(buf), buf.numel(), _stream()),
          "set_conv1d_wgrad_det_grouped")


def _conv_leaves(g, x, chan_add, w, b, cw, B, Cin, Cout, K, dil, pad, T, T_in, pro=0, pro_param=0.0):
    """Weight gradient (w: the parameter; None: not wanted) and bias gradient (b likewise) of the conv y = W (*) P(x + chan_add) + b with
    output gradient g, as leaves.  cw: the ConvWeight the conv reads w through (plain [Cout,Cin,K] rows, possibly a row slice of a larger
    parameter), None: the whole parameter.  Returns what to hand to autograd for (w, b): None where the kernel wrote the optimizer's .grad
    view (autograd still fires the parameter's post-accumulate hook: bucket launch).  g may be the engine's own gradient buffer or a
    residual's gradient: held as an operand, it is not accumulated into in place (input_buffer.cpp: can_accumulate_inplace)."""
    dev = g.device
    t_w, r_w = _tape_tgt(w, dev, cw) if w is not None else (None, None)
    t_b, r_b = _tape_tgt(b, dev) if b is not None else (None, None)  # (a bias is never a slice: autograd takes a [Cout] gradient for a [Cout] input only)
    with _leaves(dev, (r_w, r_b), g, x, chan_add):
        if w is not None:
            conv_wgrad(g, x, chan_add, t_w, B, Cin, Cout, K, dil, pad, T, T_in, pro, pro_param,
                       dw_ptr=t_w.data_ptr() + (4 * cw.base if cw is not None else 0))
        if b is not None:
            channel_sum_(g, t_b, B, Cout, T)
    return r_w, r_b


def _conv_dgrad(g, cw, dil, pad, T_in, **kw):
    """Input gradient of a conv = convolution of G with W'[ci][co][tap] = W[co][ci][tap], taps at s + pad - tap*dil."""
    return ops.conv1d(g, cw.transposed(), None, dil=-dil, pad=-pad, T_iter=T_in, T_out=T_in, **kw)


def _masked_grad(dy, mask, alias=True):
    """dy * mask[b][t]: the gradient through a conv's masked identity epilogue (also the gradient of its residual input).  Without a
    mask that is dy itself (alias=False: a copy of it)."""
    if mask is None and alias:
        return dy
    g = torch.empty_like(dy)
    B, Cc, T = dy.shape
    check(L().set_conv_epilogue_bwd(_p(dy), None, _p(mask), _p(g), B, Cc, T, 0, 1.0, _stream()), "set_conv_epilogue_bwd")
    return g


def _row_sum(x):
    """[B, C] sums over t of x [B, C, T] (the gradient of a per-channel addend)."""
    B, Cc, T = x.shape
    out = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
    check(L().set_row_sum(_p(x), _p(out), B * Cc, T, 1.0, _stream()), "set_row_sum")
    return out


def _head_views(heads, *packed):
    """The (q, k, v) MatViews [B * heads, T, d] of one packed [B, 3H, T] tensor (qkv,) or of (q [B, H, T], kv [B, 2H, T])."""
    MV = ops.MatView
    if len(packed) == 1:
        qkv = packed[0]
        H = qkv.shape[1] // 3
        return MV.heads(qkv, heads, 0, H), MV.heads(qkv, heads, H, H), MV.heads(qkv, heads, 2 * H, H)
    q, kv = packed
    H = q.shape[1]
    return MV.heads(q, heads), MV.heads(kv, heads, 0, H), MV.heads(kv, heads, H, H)


# --------------------------------------------------------------------------------------------------
class _Conv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, chan_add, res, cw, dil, pad, pro, pro_param, act, alpha, mask, impl, t_out=None):
        assert not (act == "relu" and res is not None), "the backward gates ReLU on the saved output: conv1d() adds the residual as its own node"
        x = x.contiguous()
        y = ops.conv1d(x, cw, bias, dil=dil, pad=pad, pro=pro, pro_param=pro_param, act=act, alpha=alpha, res=res,
                       mask=mask, in_chan_add=chan_add, impl=impl, T_out=t_out)
        ctx.cw, ctx.cfg = cw, (dil, pad, pro, pro_param, act, alpha, impl)
        ctx.has = (bias is not None, chan_add is not None, res is not None)
        ctx.wparam, ctx.bparam = weight, bias  # the Parameter objects (gradient sinks of the flat optimizer)
        ctx.save_for_backward(x, chan_add, mask, y if act == "relu" else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, chan_add, mask, y = ctx.saved_tensors
        dil, pad, pro, pro_param, act, alpha, impl = ctx.cfg
        cw = ctx.cw
        has_bias, has_add, has_res = ctx.has
        dy = dy.contiguous()
        B, Cout, T = dy.shape
        Cin, T_in = x.shape[1], x.shape[2]
        if act == "none" and mask is None and alpha == 1.0:
            g = dy  # identity epilogue: no kernel, no copy (every DiffNet layer conv; 14 us x ~700 launches per step)
        else:
            g = torch.empty_like(dy)
            check(L().set_conv_epilogue_bwd(_p(dy), _p(y), _p(mask), _p(g), B, Cout, T, ACT[act], float(alpha), _stream()),
                  "set_conv_epilogue_bwd")
        dres = None
        if has_res and ctx.needs_input_grad[4]:
            dres = g if act == "none" and alpha == 1.0 else _masked_grad(dy, mask, alias=False)
        dx = dadd = None
        if ctx.needs_input_grad[0] or (has_add and ctx.needs_input_grad[3]):
            dx = _conv_dgrad(g, cw, dil, pad, T_in, alpha=(1.0 / pro_param) if pro == "div" else 1.0, impl=impl)
            if has_add and ctx.needs_input_grad[3]:
                dadd = _row_sum(dx)
        r_w = r_b = None
        want_w, want_b = ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        if want_w:
            assert cw.stap == 1 and cw.sci == cw.K and cw.sco == cw.Cin * cw.K, "plain conv layout"
        if want_w or want_b:
            r_w, r_b = _conv_leaves(g, x, chan_add, ctx.wparam if want_w else None, ctx.bparam if want_b else None, cw,
                                    B, Cin, Cout, cw.K, dil, pad, T, T_in, PRO[pro], pro_param)
        return (dx if ctx.needs_input_grad[0] else None, r_w, r_b, dadd, dres, None, None, None, None, None, None, None,
                None, None, None)


_SPLIT_ACTS = ("gelu", "mish", "softplus", "tanh")


def conv1d(x, weight, bias=None, *, dil=1, pad=0, pro="none", pro_param=0.0, act="none", act_param=0.0, alpha=1.0,
           res=None, mask=None, in_chan_add=None, out=None, accumulate=False, impl=None, T_iter=None, T_out=None,
           out_stride=1, out_off=0):
    """Differentiable set_conv1d (stride-1, plain [Cout,Cin,K] weights).  Activations other than ReLU run as a
    separate kernel so their pre-activation is available to the backward."""
    assert isinstance(weight, ConvWeight) and out is None and not accumulate and out_stride == 1 and out_off == 0
    assert pro in ("none", "div") and T_iter is None
    if act in _SPLIT_ACTS:
        assert res is None
        z = _Conv1dFn.apply(x, weight.raw(), bias, in_chan_add, None, weight, dil, pad, pro, pro_param, "none", alpha,
                            None, impl, T_out)
        y = activation(z, act, act_param)
        return add_chan_mask(y, None, mask) if mask is not None else y
    if act == "relu" and res is not None:
        # _Conv1dFn gates the ReLU on its saved output, which is relu(z) only while nothing is added to it: the residual (and the mask behind
        # it) run as nodes of their own.  Same operations in the same order as the fused epilogue (+ res, then * mask): the same bits.
        # No model combines the two (diffnet.py, fs.py), so no form a model uses gains a launch or a saved tensor.
        y = add(_Conv1dFn.apply(x, weight.raw(), bias, in_chan_add, None, weight, dil, pad, pro, pro_param, act, alpha, None,
                                impl, T_out), res)
        return add_chan_mask(y, None, mask) if mask is not None else y
    return _Conv1dFn.apply(x, weight.raw(), bias, in_chan_add, res, weight, dil, pad, pro, pro_param, act, alpha, mask,
                           impl, T_out)


class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, act, p):
        z = z.contiguous()
        y = torch.empty_like(z)
        check(L().set_act_fwd(_p(z), _p(y), z.numel(), ACT[act], float(p), _stream()), "set_act_fwd")
        ctx.save_for_backward(z)
        ctx.cfg = (act, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (z,) = ctx.saved_tensors
        act, p = ctx.cfg
        dy = dy.contiguous()
        dz = torch.empty_like(z)
        check(L().set_act_bwd(_p(z), _p(dy), _p(dz), z.numel(), ACT[act], float(p), _stream()), "set_act_bwd")
        return dz, None, None


def activation(z, act, p=0.0):
    return _ActFn.apply(z, act, p)


class _LayerNormChFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, mask, eps):
        x = x.contiguous()
        y = ops.layernorm_ch(x, gamma, beta, mask, eps)
        ctx.save_for_backward(x, gamma, mask)
        ctx.eps = eps
        ctx.gparam, ctx.bparam = gamma, beta
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mask = ctx.saved_tensors
        dy = dy.contiguous()
        B, Cc, T = x.shape
        dx = torch.empty_like(x)
        (dg, r_g), (db, r_b) = _tape_tgt(ctx.gparam, x.device), _tape_tgt(ctx.bparam, x.device)
        part = _det_scratch(x.device, L().set_layernorm_ch_bwd_scratch(B, Cc, T))  # per-block partial rows (reused: stream-ordered)
        check(L().set_layernorm_ch_bwd(_p(x), _p(gamma), _p(mask), _p(dy), _p(dx), _p(dg), _p(db), _p(part), B, Cc, T,
                                       float(ctx.eps), _stream()), "set_layernorm_ch_bwd")
        return dx, r_g, r_b, None, None


def layernorm_ch(x, gamma, beta, mask=None, eps=1e-5, out=None):
    return _LayerNormChFn.apply(x, gamma, beta, mask, eps)


class _PreLnFfnFn(torch.autograd.Function):
    """One tape node for the pre-LayerNorm feed-forward sub-block both models are built from (modules/commons/conv.py:24-65 ResidualBlock
    unit; modules/speech_editing/commons/transformer.py:76-113 + :619-652 TransformerFFNLayer inside Enc/DecSALayer):

        y = (x + W2 act(alpha (W1 (*) LN(x)) + alpha b1 ...) + b2) (* mask)      -- set_conv1d semantics: alpha scales conv + bias

    Forward = the four launches of the per-op tape (LN, conv k, activation on the saved pre-activation, 1x1 conv with the residual and the
    mask in its epilogue); backward = the same kernels in hand order.  What the single node saves: four autograd nodes per sub-block in
    each direction (17 sub-blocks per CampNet step, 8 per spec_denoiser step: the steps are bound by the host's enqueue time), the
    alpha-scaling launch (folded into the activation backward: set_act_bwd_scaled, same two roundings) and the `.contiguous()` /
    fan-out bookkeeping between them.  Gradients are bit-identical to the per-op tape's (tests: all-gradients goldens)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, w2, b2, cw1, cw2, dil, pad, alpha, act, act_param, eps, mask, t_out, drop=None):
        x = x.contiguous()
        h = ops.layernorm_ch(x, gamma, beta, None, eps)
        z = ops.conv1d(h, cw1, b1, dil=dil, pad=pad, alpha=alpha, T_out=t_out)
        f = torch.empty_like(z)
        check(L().set_act_fwd(_p(z), _p(f), z.numel(), ACT[act], float(act_param), _stream()), "set_act_fwd")
        if drop is None:
            y = ops.conv1d(f, cw2, b2, res=x, mask=mask)
        else:  # the branch through inverted dropout, then + x, * mask (conv.py:57-65)
            y = ops.residual_dropout(x, ops.conv1d(f, cw2, b2), mask, *drop)
        ctx.save_for_backward(x, gamma, mask, h, z, f)
        ctx.cws, ctx.cfg, ctx.drop = (cw1, cw2), (dil, pad, alpha, act, act_param, eps), drop
        ctx.params = (gamma, beta, w1, b1, w2, b2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mask, h, z, f = ctx.saved_tensors
        cw1, cw2 = ctx.cws
        dil, pad, alpha, act, act_param, eps = ctx.cfg
        p_gamma, p_beta, p_w1, p_b1, p_w2, p_b2 = ctx.params
        dy = dy.contiguous()
        B, Cc, T = dy.shape
        Cmid, T1, T_in = z.shape[1], z.shape[2], h.shape[2]
        # ---- second conv (1x1, + residual, * mask): G2 = dy * mask is also the residual's gradient
        if ctx.drop is not None:  # the branch's gradient is keep * G2 / (1 - p) (same Philox keys as the forward)
            g2, gb = torch.empty_like(dy), torch.empty_like(dy)
            p_, seed_, off_ = ctx.drop
            check(L().set_conv_epilogue_bwd_dropout(_p(dy), _p(mask), _p(g2), _p(gb), B, Cc, T, float(p_), int(seed_), int(off_),
                                                    _stream()), "set_conv_epilogue_bwd_dropout")
        else:
            g2 = gb = _masked_grad(dy, mask)
        df = _conv_dgrad(gb, cw2, 1, 0, T1)
        r_w2, r_b2 = _conv_leaves(gb, f, None, p_w2, p_b2, cw2, B, Cmid, Cc, 1, 1, 0, T, T1)
        # ---- activation backward with the first conv's alpha folded in: G1 = gradient of the raw conv + bias
        g1 = torch.empty_like(z)
        check(L().set_act_bwd_scaled(_p(z), _p(df), _p(g1), z.numel(), ACT[act], float(act_param), float(alpha), _stream()), "set_act_bwd_scaled")
        dh = _conv_dgrad(g1, cw1, dil, pad, T_in)
        r_w1, r_b1 = _conv_leaves(g1, h, None, p_w1, p_b1, cw1, B, Cc, Cmid, cw1.K, dil, pad, T1, T_in)
        # ---- LayerNorm backward, then the residual branch joins (same order as the fan-out node of the per-op tape: LN branch + residual)
        dxl, r_g, r_bt = _preln_tail(x, gamma, p_gamma, p_beta, dh, g2, eps)
        return (dxl, r_g, r_bt, r_w1, r_b1, r_w2, r_b2) + (None,) * 11


def preln_ffn(x, ln, cw1, b1, cw2, b2, *, dil=1, pad=0, alpha=1.0, act="gelu", act_param=0.0, mask=None, eps=1e-5, T_out=None,
              drop=None):
    """(x + conv1x1(act(alpha conv_k(LN(x))))) (* mask) as one tape node; ln = (gamma, beta).  SET_AMD_FUSED_NODES=0: the per-op tape
    (fan-out, LayerNorm, conv, activation, conv: five nodes) -- the cross-check of tests/test_gpu_training.py and the A/B of the bench.
    drop=(p, seed, offset): inverted dropout on the branch before the residual add, keep-mask of set_dropout keyed by (seed, offset,
    element index); the per-op form is then fan-out, LayerNorm, conv, activation, conv, dropout, add, mask."""
    if not _fused_nodes():
        x_ln, x_res = fanout(x, 2)
        h = layernorm_ch(x_ln, ln[0], ln[1], eps=eps)
        h = conv1d(h, cw1, b1, dil=dil, pad=pad, alpha=alpha, act=act, act_param=act_param, T_out=T_out)
        if drop is None:
            return conv1d(h, cw2, b2, res=x_res, mask=mask)
        y = add(x_res, dropout(conv1d(h, cw2, b2), *drop))
        return add_chan_mask(y, None, mask) if mask is not None else y
    return _PreLnFfnFn.apply(x, ln[0], ln[1], cw1.raw(), b1, cw2.raw(), b2, cw1, cw2, dil, pad, alpha, act, act_param, eps, mask, T_out,
                             None if drop is None else (float(drop[0]), int(drop[1]), int(drop[2])))


class _AddFn(torch.autograd.Function):
    """a + b on equal shapes (set_sum_scale); the gradient goes to both unchanged."""

    @staticmethod
    def forward(ctx, a, b):
        return ops.sum_div(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, d):
        return d, d


def add(a, b):
    return _AddFn.apply(a, b)


class _StutterLossFn(torch.autograd.Function):
    """StutterSpeech's head and losses as one tape node (csrc/stutter.hip): h [B,C,T] (post_net1 output) -> logits [B,T,3] = Linear(C, 3),
    ce = CrossEntropyLoss(ignore_index=2), focal = MultiFocalLoss (stutter_predictor.py:15-44, stutter_speech.py:97-99).  labels: int64
    [B,T] already remapped to {0: fluent, 1: stutter, 2: pad}.  The logits carry no gradient (they only feed the accuracy)."""

    @staticmethod
    def forward(ctx, h, w, b, labels):
        h = h.contiguous()
        B, Cc, T = h.shape
        dev = h.device
        ops._i(labels, "labels")
        assert labels.shape == (B, T), (tuple(labels.shape), (B, T))
        logits = torch.empty(B, T, 3, dtype=torch.float32, device=dev)
        stats = torch.empty(3, dtype=torch.float32, device=dev)
        scratch = _det_scratch(dev, L().set_stutter_head_scratch_floats(B, Cc, T))
        check(L().set_stutter_head_loss(_p(h), _p(w), _p(b), _p(labels), _p(logits), _p(stats), _p(scratch), B, Cc, T, _stream()),
              "set_stutter_head_loss")
        ctx.save_for_backward(h, w, logits, labels, stats)
        ctx.params = (w, b)
        ctx.mark_non_differentiable(logits)
        return logits, stats[0], stats[1]

    @staticmethod
    def backward(ctx, _dlogits, g_ce, g_focal):
        h, w, logits, labels, stats = ctx.saved_tensors
        p_w, p_b = ctx.params
        B, Cc, T = h.shape
        dev = h.device
        g_ce = None if g_ce is None else g_ce.contiguous()
        g_focal = None if g_focal is None else g_focal.contiguous()
        dh = torch.empty_like(h)
        part = torch.empty(L().set_stutter_head_scratch_floats(B, Cc, T), dtype=torch.float32, device=dev)  # own buffer: read on the leaf stream
        check(L().set_stutter_head_loss_bwd(_p(h), _p(w), _p(logits), _p(labels), _p(stats), _p(g_ce), _p(g_focal), _p(dh), None, None,
                                            _p(part), B, Cc, T, _stream()), "set_stutter_head_loss_bwd")
        (t_w, r_w), (t_b, r_b) = _tape_tgt(p_w, dev), _tape_tgt(p_b, dev)
        with _leaves(dev, (r_w, r_b), part):
            check(L().set_stutter_head_bwd_reduce(_p(part), _p(t_w), _p(t_b), B, Cc, T, _stream()), "set_stutter_head_bwd_reduce")
        return dh, r_w, r_b, None


def stutter_losses(h, w, b, labels):
    """(logits [B,T,3], ce, focal) of StutterSpeech's predictor head; see _StutterLossFn."""
    return _StutterLossFn.apply(h, w, b, labels)


class _EmbeddingFn(torch.autograd.Function):
    """out = (base or 0) + scale * table[idx]  written channel-major."""

    @staticmethod
    def forward(ctx, idx, table, base, scale, padding_idx):
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        if base is None:
            out = ops.embedding_bct(idx, table, scale=scale)
        else:
            out = ops.embedding_bct(idx, table, scale=scale, out=base.detach().clone(), accumulate=True)
        ctx.save_for_backward(idx)
        ctx.cfg = (tuple(table.shape), scale, base is not None)
        ctx.tparam = table
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        (n_rows, Cc), scale, has_base = ctx.cfg
        dout = dout.contiguous()
        B, T = idx.shape
        dtab, r_tab = _tape_tgt(ctx.tparam, dout.device)  # (a table that is a parameter used once: its gradient goes straight into .grad, on the leaf stream)
        # ordered scatter (no atomics): gradient rows transposed to [B][T][C], per-(utterance, segment) partial tables
        doutT = ops.bct_to_btc(dout)
        S = L().set_scatter_rows_segments(T)
        with _leaves(dout.device, (r_tab,), dout, doutT, idx):
            check(L().set_scatter_rows_det(_p(idx), _p(doutT), _p(dtab), B, T, Cc, n_rows, float(scale), ctx.padding_idx, 0,
                                           _p(_det_scratch(dout.device, B * S * n_rows * Cc)), _stream()), "set_scatter_rows_det")
        return None, r_tab, (dout if has_base else None), None, None


def embedding_bct(idx, table, scale=1.0, out=None, accumulate=False, padding_idx=None):
    return _EmbeddingFn.apply(idx, table, out if accumulate else None, scale, padding_idx)


class _ExpandStatesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, mel2ph):
        enc = enc.contiguous()
        ctx.save_for_backward(mel2ph)
        ctx.shape = tuple(enc.shape)
        return ops.expand_states(enc, mel2ph)

    @staticmethod
    def backward(ctx, dout):
        (mel2ph,) = ctx.saved_tensors
        B, Cc, T_txt = ctx.shape
        dout = dout.contiguous()
        T = mel2ph.shape[1]
        doutT = ops.bct_to_btc(dout)
        dencT = _gzeros((B, T_txt, Cc), dout.device)
        S = L().set_scatter_rows_segments(T)
        check(L().set_scatter_rows_det(_p(mel2ph), _p(doutT), _p(dencT), B, T, Cc, T_txt, 1.0, -1, 1,
                                       _p(_det_scratch(dout.device, B * S * T_txt * Cc)), _stream()), "set_scatter_rows_det")
        return ops.btc_to_bct(dencT), None


def expand_states(enc_bct, mel2ph):
    return _ExpandStatesFn.apply(enc_bct, mel2ph)


class _AddChanMaskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, add, mask):
        x = x.contiguous()
        ctx.save_for_backward(mask)
        ctx.has_add = add is not None
        return ops.add_chan_mask(x, add, mask)

    @staticmethod
    def backward(ctx, dout):
        (mask,) = ctx.saved_tensors
        dout = dout.contiguous()
        dx = ops.add_chan_mask(dout, None, mask) if mask is not None else dout
        return dx, (_row_sum(dx) if ctx.has_add and ctx.needs_input_grad[1] else None), None


def add_chan_mask(x, add=None, mask=None, out=None):
    return _AddChanMaskFn.apply(x, add, mask)


class _TransposeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, to_bct):
        ctx.to_bct = to_bct
        x = x.contiguous()
        return ops.btc_to_bct(x) if to_bct else ops.bct_to_btc(x)

    @staticmethod
    def backward(ctx, d):
        d = d.contiguous()
        return (ops.bct_to_btc(d) if ctx.to_bct else ops.btc_to_bct(d)), None


def btc_to_bct(x):
    return _TransposeFn.apply(x, True)


def bct_to_btc(x):
    return _TransposeFn.apply(x, False)


class _GateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        y = y.contiguous()
        ctx.save_for_backward(y)
        return ops.gate(y)

    @staticmethod
    def backward(ctx, dz):
        (y,) = ctx.saved_tensors
        dz = dz.contiguous()
        B, C2, T = y.shape
        dy = torch.empty_like(y)
        check(L().set_gate_bwd(_p(y), _p(dz), _p(dy), B, C2 // 2, T, _stream()), "set_gate_bwd")
        return dy


def gate(y):
    return _GateFn.apply(y)


class _ResSkipFn(torch.autograd.Function):
    """(x_out, skip_out) = ((x + o[:, :C]) / sqrt2, skip_in + o[:, C:])   (functional form of set_res_skip)."""

    @staticmethod
    def forward(ctx, x, o, skip_in):
        x, o = x.contiguous(), o.contiguous()
        first = skip_in is None
        skip = torch.empty_like(x) if first else skip_in.detach().clone()
        x_out = ops.res_skip(x, o, skip, first)
        ctx.first = first
        return x_out, skip

    @staticmethod
    def backward(ctx, dx_out, dskip):
        dx_out, dskip = dx_out.contiguous(), dskip.contiguous()
        B, Cc, T = dx_out.shape
        dx = torch.empty_like(dx_out)
        d_o = torch.empty(B, 2 * Cc, T, dtype=torch.float32, device=dx_out.device)
        check(L().set_res_skip_bwd(_p(dx_out), _p(dskip), _p(dx), _p(d_o), B, Cc, T, _stream()), "set_res_skip_bwd")
        return dx, d_o, (None if ctx.first else dskip)


def res_skip_fn(x, o, skip_in):
    return _ResSkipFn.apply(x, o, skip_in)


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(L().set_dropout(_p(x), _p(y), x.numel(), float(p), int(seed), int(offset), _stream()), "set_dropout")
        ctx.cfg = (p, seed, offset)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, offset = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(L().set_dropout(_p(dy), _p(dx), dy.numel(), float(p), int(seed), int(offset), _stream()), "set_dropout")
        return dx, None, None, None


def dropout(x, p, seed, offset=0):
    return _DropoutFn.apply(x, p, seed, offset) if p > 0 else x


class _FanoutFn(torch.autograd.Function):
    """n uses of one tensor: forward returns n aliases, backward sums the n gradients with set_sum_scale (so the
    fan-in accumulation is our kernel, not the autograd engine's elementwise add)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = n
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [g.contiguous() for g in grads if g is not None]
        acc = gs[0]
        k = 1
        while k < len(gs):
            acc = ops.sum_div(acc, gs[k], gs[k + 1] if k + 1 < len(gs) else None, 1.0)
            k += 2
        return acc, None


def fanout(x, n):
    return _FanoutFn.apply(x, n) if n > 1 else (x,)


class _GradScaleFn(torch.autograd.Function):
    """x.detach() + s * (x - x.detach())  (fs.py:144-145,167-169): identity forward, gradient scaled by s."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, d):
        d = d.contiguous()
        out = torch.empty_like(d)
        check(L().set_scale_bcast(_p(d), None, _p(out), d.numel(), 1, None, float(ctx.s), _stream()), "set_scale_bcast")
        return out, None


def grad_scale(x, s):
    return _GradScaleFn.apply(x, s) if s != 1 else x


# --------------------------------------------------------------------------------------------------
# DiffNet layer stack: fused forward (persistent Winograd kernel), hand-ordered backward
# --------------------------------------------------------------------------------------------------
class _DiffNetStackFn(torch.autograd.Function):
    """All L residual layers (diffnet.py:60-81,121-127) as ONE forward launch that also stores every layer's input x_l,
    pre-gate y_l and gated z_l; the backward walks the layers in reverse with the same kernels the per-op tape uses
    (res-skip / gate backward, conv dgrad = set_conv1d on the transposed weights, wgrad, channel / row sums).
    Inputs: hx [B,256,T], cond [B,H,T], dmat [B, L*256] (diffusion projections), then per layer
    (W_cond, b_cond, W_dil, b_dil, W_out, b_out).  Output: the skip sum [B,256,T] (the last layer's x is unused)."""

    @staticmethod
    def forward(ctx, dn, hx, cond, dmat, *params):
        L_, C_ = dn.n_layers, dn.C
        hx, cond, dmat = hx.contiguous(), cond.contiguous(), dmat.contiguous()
        B, _, T = hx.shape
        dev = hx.device
        layers = list(dn.residual_layers)
        condproj = torch.empty(B, L_ * 2 * C_, T, dtype=torch.float32, device=dev)
        for l, layer in enumerate(layers):
            ops.conv1d(cond, layer._w_cond, layer.conditioner_projection.bias, out=condproj[:, l * 2 * C_:(l + 1) * 2 * C_])
        x_all = torch.empty(L_ + 1, B, C_, T, dtype=torch.float32, device=dev)
        x_all[0].copy_(hx)
        y_all = torch.empty(L_, B, 2 * C_, T, dtype=torch.float32, device=dev)
        z_all = torch.empty(L_, B, C_, T, dtype=torch.float32, device=dev)
        skip = torch.empty(B, C_, T, dtype=torch.float32, device=dev)
        ws = ops.diffnet_stack(x_all[0], x_all[1], skip, condproj, dmat.data_ptr(), L_ * C_, 1, C_, dn.fused_packs(inference=False),
                               dn.dilation_cycle_length, x_all=x_all, save_y=y_all, save_z=z_all)
        ctx.dn, ctx.ws = dn, ws
        ctx.save_for_backward(cond, dmat, x_all, y_all, z_all)
        return skip

    @staticmethod
    def backward(ctx, dskip):
        dn = ctx.dn
        if int(ctx.ws[1]) != 0:  # (the forward's abort word; this read-back is the first host sync of the step)
            raise SetAmdError("set_diffnet_stack: a tile dependency wait of the training forward timed out")
        cond, dmat, x_all, y_all, z_all = ctx.saved_tensors
        L_, C_ = dn.n_layers, dn.C
        B, H, T = cond.shape
        dev = cond.device
        layers = list(dn.residual_layers)
        dskip = dskip.contiguous()
        need_cond = ctx.needs_input_grad[2]
        dcond = _gzeros(cond.shape, dev) if need_cond else None
        dd = torch.empty(B, L_ * C_, dtype=torch.float32, device=dev)
        dx = _gzeros((B, C_, T), dev)  # the last layer's x output feeds nothing
        grads = []
        for l in range(L_ - 1, -1, -1):
            layer = layers[l]
            dil = layer.dilation
            dxr = torch.empty_like(dx)
            d_o = torch.empty(B, 2 * C_, T, dtype=torch.float32, device=dev)
            check(L().set_res_skip_bwd(_p(dx), _p(dskip), _p(dxr), _p(d_o), B, C_, T, _stream()), "set_res_skip_bwd")
            out_p, cond_p, dil_p = layer.output_projection, layer.conditioner_projection, layer.dilated_conv
            (dw_out, r_wo), (db_out, r_bo), (dw_cond, r_wc), (db, r_bc), (db2, r_bd), (dw_dil, r_wd) = [
                _tape_tgt(p_, dev) for p_ in (out_p.weight, out_p.bias, cond_p.weight, cond_p.bias, dil_p.bias, dil_p.weight)]
            # output_projection (1x1, 256 -> 512)
            dz = _conv_dgrad(d_o, layer._w_out, 1, 0, T)
            # gate
            dy = torch.empty(B, 2 * C_, T, dtype=torch.float32, device=dev)
            check(L().set_gate_bwd(_p(y_all[l]), _p(dz), _p(dy), B, C_, T, _stream()), "set_gate_bwd")
            # conditioner_projection (1x1, H -> 512): y = ... + W_cond cond + b_cond
            if need_cond:
                _conv_dgrad(dy, layer._w_cond, 1, 0, T, out=dcond, accumulate=True)
            # dilated conv (k=3) on x_l + d_l
            dl = dmat[:, l * C_:(l + 1) * C_].contiguous()
            dxd = _conv_dgrad(dy, layer._w_dil, dil, dil, T)
            dd[:, l * C_:(l + 1) * C_] = _row_sum(dxd)
            dx = ops.sum_div(dxd, dxr)
            # the layer's six parameter gradients: leaves
            with _leaves(dev, (r_wo, r_bo, r_wc, r_bc, r_bd, r_wd), d_o, dy, z_all, cond, x_all, dl):
                conv_wgrad(d_o, z_all[l], None, dw_out, B, C_, 2 * C_, 1, 1, 0, T, T)
                channel_sum_(d_o, db_out, B, 2 * C_, T)
                conv_wgrad(dy, cond, None, dw_cond, B, H, 2 * C_, 1, 1, 0, T, T)
                channel_sum_(dy, db, B, 2 * C_, T)  # = db_cond = db_dil
                channel_sum_(dy, db2, B, 2 * C_, T)
                conv_wgrad(dy, x_all[l], dl, dw_dil, B, C_, 2 * C_, 3, dil, dil, T, T)
            grads.append((r_wc, r_bc, r_wd, r_bd, r_wo, r_bo))
        grads.reverse()
        flat = [g for tup in grads for g in tup]
        return (None, dx, dcond, dd, *flat)


class _SumLossesFn(torch.autograd.Function):
    """total = sum of the 0-d loss terms as ONE stack + ONE reduction (Python's sum() is an add launch per term, starting from 0, and an
    add / mul node per term on the way back); every term's gradient is the incoming one."""

    @staticmethod
    def forward(ctx, *vals):
        return torch.stack([v.reshape(()) for v in vals]).sum()

    @staticmethod
    def backward(ctx, g):
        return tuple(g for _ in ctx.needs_input_grad)


def sum_losses(vals):
    return _SumLossesFn.apply(*vals)


SWEEP_EVENTS = None  # bench.py sets a list: (start, end, launches) hipEvent pairs around the layer-backward sweep of every step


class _DiffNetStackBf16Fn(torch.autograd.Function):
    """All L residual layers with bf16 MFMA operands: one fused forward launch per layer that also saves the pre-gate y
    and the gated z in bf16, one fused backward launch per layer (d_o -> dz -> gate derivative -> dx, dcond, bias / step
    partial sums) and three weight-gradient GEMMs per layer on the saved bf16 operands (csrc/diffnet_bf16.hip).
    Same inputs / outputs as _DiffNetStackFn."""

    @staticmethod
    def forward(ctx, dn, hx, cond, dmat, *params):
        L_, C_ = dn.n_layers, dn.C
        hx, cond, dmat = hx.contiguous(), cond.contiguous(), dmat.contiguous()
        B, _, T = hx.shape
        dev = hx.device
        imgs, per = dn.bf16_layer_images(params)
        x_all = torch.empty(L_ + 1, B, C_, T, dtype=torch.float32, device=dev)
        x_all[0].copy_(hx)
        y16 = torch.empty(L_, B, 2 * C_, T, dtype=torch.bfloat16, device=dev)
        z16 = torch.empty(L_, B, C_, T, dtype=torch.bfloat16, device=dev)
        skip = torch.empty(B, C_, T, dtype=torch.float32, device=dev)
        a = _lib.SetDiffnetLayerBf16Args()
        a.skip, a.cond = skip.data_ptr(), cond.data_ptr()
        a.d_bs, a.d_cs = dmat.stride(0), 1
        a.B, a.T = B, T
        # per-layer addresses as integers (a tensor index or an nn.Module attribute per operand and layer cost ~0.4 ms of host time per step
        # in this loop and the backward sweep: the step is bound by the host's enqueue time)
        x0, sx = x_all.data_ptr(), 4 * B * C_ * T
        y0, z0, d0 = y16.data_ptr(), z16.data_ptr(), dmat.data_ptr()
        fn, st, ref = L().set_diffnet_layer_fwd_bf16, _stream(), C.byref(a)
        for l in range(L_):
            a.x_in, a.x_out = x0 + l * sx, x0 + (l + 1) * sx
            a.dstep = d0 + 4 * l * C_
            a.img, a.b_dil, a.b_cond, a.b_out, a.dil = per[l]
            a.y16, a.z16 = y0 + l * sx, z0 + l * (sx // 2)  # bf16 [B][2C][T] and [B][C][T]
            a.first = int(l == 0)
            check(fn(ref, st), "set_diffnet_layer_fwd_bf16")
        ctx.dn, ctx.imgs, ctx.per = dn, imgs, per
        ctx.save_for_backward(cond, dmat, x_all, y16, z16)
        return skip

    @staticmethod
    def backward(ctx, dskip):
        dn, per = ctx.dn, ctx.per
        cond, dmat, x_all, y16, z16 = ctx.saved_tensors
        L_, C_ = dn.n_layers, dn.C
        B, H, T = cond.shape
        dev = cond.device
        layers = list(dn.residual_layers)
        dskip = dskip.contiguous()
        dcond = torch.empty_like(cond)
        dd = torch.empty(B, L_ * C_, dtype=torch.float32, device=dev)
        # Weight gradients of ALL layers in three grouped launches after the sweep (dy / d_o of every layer are kept: 2 x L x 26 MB
        # at B = 32, T = 800) when the layers share one dilation; else three GEMMs per layer inside the sweep.
        grouped = len({layer.dilation for layer in layers}) == 1
        # the grouped form keeps dy / d_o of ALL layers alive (2 x L x B x 2C x T bf16: ~1 GB at L = 20, B = 32, T = 800, next to x_all,
        # y16, z16); beyond a budget (SET_AMD_GROUPED_WGRAD_MB, default 4096 MB -- 1.4 % of the 288 GB) it falls back to the per-layer form
        if grouped and 2 * L_ * B * 2 * C_ * T * 2 > float(os.environ.get("SET_AMD_GROUPED_WGRAD_MB", "4096")) * 2 ** 20:
            grouped = False
        n_slab = L_ if grouped else 1
        dy16_all = torch.empty(n_slab, B, 2 * C_, T, dtype=torch.bfloat16, device=dev)
        do16_all = torch.empty(n_slab, B, 2 * C_, T, dtype=torch.bfloat16, device=dev)
        dx = [torch.empty(B, C_, T, dtype=torch.float32, device=dev) for _ in range(2)]
        a = _lib.SetDiffnetLayerBf16BwdArgs()
        a.dskip, a.dcond = dskip.data_ptr(), dcond.data_ptr()
        a.B, a.T = B, T
        # measurement hook (bench.py): hipEvents that the sweep records around its diffnet_layer_bwd_bf16_kernel launches
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if SWEEP_EVENTS is not None else None
        sweep = _bf16_stack_bwd_grouped if grouped else _bf16_stack_bwd_per_layer
        cur, grads = sweep(a, layers, per, cond, dmat, x_all, y16, z16, dy16_all, do16_all, dx, dd, ev)
        need_cond = ctx.needs_input_grad[2]
        return (None, cur, dcond if need_cond else None, dd, *[g for tup in grads for g in tup])


def _sweep_done(ev, launches):
    if ev is not None:
        ev[1].record()
        SWEEP_EVENTS.append((ev[0], ev[1], launches))


def _bf16_stack_bwd_grouped(a, layers, per, cond, dmat, x_all, y16, z16, dy16_all, do16_all, dx, dd, ev):
    """The layers share one dilation: the sweep is L launches on integer addresses that keep dy / d_o and the per-tile partial sums
    (bias / step-offset gradients, L x ~2 MB at B = 32, T = 800) of EVERY layer; after it ONE launch reduces the partials and three
    grouped launches compute the weight gradients of all layers, instead of a 5 us reduce and three GEMMs per layer in the middle of the
    chain of layer kernels.  Returns (gradient w.r.t. the stack's input, per layer (W_cond, b_cond, W_dil, b_dil, W_out, b_out))."""
    L_, (B, H, T), C_, dev = len(layers), cond.shape, x_all.shape[2], cond.device
    dil = layers[0].dilation
    tiles = L().set_diffnet_layer_bwd_bf16_tiles(T, dil)
    pdbo_all = torch.empty(L_, B * tiles, 2 * C_, dtype=torch.float32, device=dev)
    pdby_all = torch.empty(L_, B * tiles, 2 * C_, dtype=torch.float32, device=dev)
    pdd_all = torch.empty(L_, B * tiles, C_, dtype=torch.float32, device=dev)
    if ev is not None:
        ev[0].record()
    # per-layer addresses as integers, the function, the stream and the byref bound once (see the forward)
    dy0, do0, y0, s16 = dy16_all.data_ptr(), do16_all.data_ptr(), y16.data_ptr(), 2 * B * 2 * C_ * T
    pb0, py0, pd0, sp = pdbo_all.data_ptr(), pdby_all.data_ptr(), pdd_all.data_ptr(), 4 * B * tiles * C_
    dxp = (dx[0].data_ptr(), dx[1].data_ptr())
    fn, st, ref = L().set_diffnet_layer_bwd_bf16, _stream(), C.byref(a)
    a.dil = dil
    curp = None  # gradient w.r.t. the current layer's x_out (None for the last layer: its x_out feeds nothing)
    for l in range(L_ - 1, -1, -1):
        a.dy16, a.do16, a.y16 = dy0 + l * s16, do0 + l * s16, y0 + l * s16
        a.dx_out, a.img, a.dx = curp, per[l][0], dxp[l & 1]
        a.part_dbo, a.part_dby, a.part_dd = pb0 + l * 2 * sp, py0 + l * 2 * sp, pd0 + l * sp
        a.dcond_first = int(l == L_ - 1)
        check(fn(ref, st), "set_diffnet_layer_bwd_bf16")
        curp = dxp[l & 1]
    _sweep_done(ev, L_)  # (nothing but the L layer launches lies between the events)
    n_act = B * 2 * C_ * T
    pb_o, sb_o, rb_o = _grouped_targets([ly.output_projection.bias for ly in layers], dev)
    pb_d, sb_d, rb_d = _grouped_targets([ly.dilated_conv.bias for ly in layers], dev)
    pb_c, sb_c, rb_c = _grouped_targets([ly.conditioner_projection.bias for ly in layers], dev)
    check(L().set_diffnet_layers_bwd_reduce(_p(pdbo_all), _p(pdby_all), _p(pdd_all), B, tiles, L_, C.c_void_p(pb_o), sb_o,
                                            C.c_void_p(pb_d), sb_d, C.c_void_p(pb_c), sb_c, _p(dd), dd.stride(0), C_, _stream()),
          "set_diffnet_layers_bwd_reduce")
    p_out, s_out, r_out = _grouped_targets([ly.output_projection.weight for ly in layers], dev)
    p_c, s_c, r_c = _grouped_targets([ly.conditioner_projection.weight for ly in layers], dev)
    p_d, s_d, r_d = _grouped_targets([ly.dilated_conv.weight for ly in layers], dev)
    dl_all = dmat.view(B, L_, C_).transpose(0, 1).contiguous()  # [L][B][C] step offsets (the conv's input is x + d)
    # written straight into .grad (every r_* entry None): leaves of the backward pass -- 2.3 ms of chip-filling GEMMs that run on the
    # leaf stream under the conditioner's backward (hundreds of 5-40 us kernels on a few dozen workgroups each)
    G16, GX16 = _lib.DTYPE_BF16_G16, _lib.DTYPE_BF16_G16_X16
    with _leaves(dev, r_out + r_c + r_d, do16_all, dy16_all, z16, cond, x_all, dl_all):
        conv_wgrad_grouped(do16_all, z16, None, p_out, L_, n_act, B * C_ * T, 0, s_out, B, C_, 2 * C_, 1, 1, 0, T, T, GX16)
        conv_wgrad_grouped(dy16_all, cond, None, p_c, L_, n_act, 0, 0, s_c, B, H, 2 * C_, 1, 1, 0, T, T, G16)
        conv_wgrad_grouped(dy16_all, x_all, dl_all, p_d, L_, n_act, B * C_ * T, B * C_, s_d, B, C_, 2 * C_, 3, dil, dil, T, T, G16)
    return dx[0], list(zip(r_c, rb_c, r_d, rb_d, r_out, rb_o))


def _bf16_wgrad(param, g, x, chan_add, *shape, dtype):
    """One layer weight gradient of the per-layer form, on the compute stream (the next layer's launch overwrites dy16 / do16)."""
    tgt, ret = _tape_tgt(param, g.device)
    conv_wgrad(g, x, chan_add, tgt, *shape, dtype=dtype)
    return ret


def _bf16_stack_bwd_per_layer(a, layers, per, cond, dmat, x_all, y16, z16, dy16_all, do16_all, dx, dd, ev):
    """Mixed dilations, or dy / d_o of all layers over the memory budget: one dy / d_o slab, and per layer the fused launch, one
    ordered reduce of its per-tile partials (bias / step-offset gradients) and three weight-gradient GEMMs.  Returns what
    _bf16_stack_bwd_grouped returns."""
    L_, (B, H, T), C_, dev = len(layers), cond.shape, x_all.shape[2], cond.device
    G16, GX16 = _lib.DTYPE_BF16_G16, _lib.DTYPE_BF16_G16_X16
    dy16, do16 = dy16_all[0], do16_all[0]
    a.dy16, a.do16 = dy16.data_ptr(), do16.data_ptr()
    grads = []
    cur = None  # gradient w.r.t. the current layer's x_out (None for the last layer: its x_out feeds nothing)
    if ev is not None:
        ev[0].record()
    for l in range(L_ - 1, -1, -1):
        layer = layers[l]
        dil = layer.dilation
        tiles = L().set_diffnet_layer_bwd_bf16_tiles(T, dil)
        pdbo = torch.empty(B * tiles, 2 * C_, dtype=torch.float32, device=dev)
        pdby = torch.empty(B * tiles, 2 * C_, dtype=torch.float32, device=dev)
        pdd = torch.empty(B * tiles, C_, dtype=torch.float32, device=dev)
        out = dx[l & 1]
        a.dx_out = None if cur is None else cur.data_ptr()
        a.y16, a.img, a.dx = y16[l].data_ptr(), per[l][0], out.data_ptr()
        a.part_dbo, a.part_dby, a.part_dd = pdbo.data_ptr(), pdby.data_ptr(), pdd.data_ptr()
        a.dil, a.dcond_first = dil, int(l == L_ - 1)
        check(L().set_diffnet_layer_bwd_bf16(C.byref(a), _stream()), "set_diffnet_layer_bwd_bf16")
        (t_out, db_out), (t_dil, db_dil), (t_cond, db_cond) = (
            _tape_tgt(m.bias, dev) for m in (layer.output_projection, layer.dilated_conv, layer.conditioner_projection))
        check(L().set_diffnet_layer_bwd_reduce(_p(pdbo), _p(pdby), _p(pdd), B, tiles, _p(t_out), _p(t_dil), _p(t_cond),
                                               dd.data_ptr() + 4 * l * C_, dd.stride(0), _stream()), "set_diffnet_layer_bwd_reduce")
        dw_out = _bf16_wgrad(layer.output_projection.weight, do16, z16[l], None, B, C_, 2 * C_, 1, 1, 0, T, T, dtype=GX16)
        dw_cond = _bf16_wgrad(layer.conditioner_projection.weight, dy16, cond, None, B, H, 2 * C_, 1, 1, 0, T, T, dtype=G16)
        dl = dmat[:, l * C_:(l + 1) * C_].contiguous()
        dw_dil = _bf16_wgrad(layer.dilated_conv.weight, dy16, x_all[l], dl, B, C_, 2 * C_, 3, dil, dil, T, T, dtype=G16)
        grads.append((dw_cond, db_cond, dw_dil, db_dil, dw_out, db_out))
        cur = out
    _sweep_done(ev, 4 * L_)
    grads.reverse()
    return cur, grads


class _StepProjFn(torch.autograd.Function):
    """dmat[n][l*C + co] = diffusion_projection_l(h)[co] for every residual layer l in one launch (diffnet.py:66,72); backward: one
    launch for the input gradient partials (+ their ordered sum) and one for all weight / bias gradients (csrc/train.hip)."""

    @staticmethod
    def forward(ctx, h, w_ls, b_ls, *params):
        L_ = len(params) // 2
        ws, bs = params[:L_], params[L_:]
        Cc, N = h.shape[1], h.shape[2]
        h = h.contiguous()
        out = torch.empty(N, L_ * Cc, dtype=torch.float32, device=h.device)
        check(L().set_step_proj_fwd(_p(h), _p(ws[0]), w_ls, _p(bs[0]), b_ls, _p(out), L_, Cc, N, _stream()), "set_step_proj_fwd")
        ctx.ws, ctx.bs, ctx.w_ls = ws, bs, w_ls
        ctx.save_for_backward(h)
        return out

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        ws, bs = ctx.ws, ctx.bs
        L_, Cc, N = len(ws), h.shape[1], h.shape[2]
        g = g.contiguous()
        dev = h.device
        p_w, s_w, r_w = _grouped_targets(list(ws), dev)
        p_b, s_b, r_b = _grouped_targets(list(bs), dev)
        dh = torch.empty_like(h)
        scratch = _det_scratch(dev, L().set_step_proj_bwd_scratch_floats(L_, Cc, N))
        check(L().set_step_proj_bwd_dh(_p(g), _p(ws[0]), ctx.w_ls, _p(dh), _p(scratch), L_, Cc, N, _stream()), "set_step_proj_bwd_dh")
        with _leaves(dev, r_w + r_b, h, g):
            check(L().set_step_proj_bwd_dw(_p(h), _p(g), C.c_void_p(p_w), s_w, C.c_void_p(p_b), s_b, L_, Cc, N, _stream()),
                  "set_step_proj_bwd_dw")
        return (dh, None, None, *r_w, *r_b)


def step_projections(dn, h):
    """[n, L*C] step offsets of all residual layers from the step embedding h [1, C, n]; None when the layers' parameters are not laid
    out at one stride (no flat optimizer and separately allocated tensors) or the shape is outside the kernel."""
    ws = [layer.diffusion_projection.weight for layer in dn.residual_layers]
    bs = [layer.diffusion_projection.bias for layer in dn.residual_layers]
    Cc, N = h.shape[1], h.shape[2]
    if h.shape[0] != 1 or Cc % 64 or N > 64 or Cc * (32 if N <= 32 else 64) > 16384:
        return None
    w_ls, b_ls = _uniform_stride(ws), _uniform_stride(bs)
    if w_ls is None or b_ls is None:
        return None
    return _StepProjFn.apply(h, w_ls, b_ls, *ws, *bs)


def diffnet_stack_train_bf16(dn, hx, cond, dmat):
    return _DiffNetStackBf16Fn.apply(dn, hx, cond, dmat, *dn.stack_params())


def diffnet_stack_train(dn, hx, cond, dmat):
    return _DiffNetStackFn.apply(dn, hx, cond, dmat, *dn.stack_params())


# --------------------------------------------------------------------------------------------------
# attention + the small CampNet ops
# --------------------------------------------------------------------------------------------------
def _attn_bwd(qv, kv, vv, p, do, dqv, dkv, dvv, heads, alpha):
    """Gradients of o = softmax(alpha q k^T) v into the views dqv / dkv / dvv (four strided batched GEMMs + one
    softmax backward)."""
    MV = ops.MatView
    dov = MV.heads(do, heads)
    dp = torch.empty_like(p)
    ops.bmm(dov, vv.t, MV.scores(dp))            # dP = dO V^T
    ops.bmm(MV.scores(p).t, dov, dvv)            # dV = P^T dO
    ds = ops.softmax_rows_bwd(p, dp)
    ops.bmm(MV.scores(ds), kv, dqv, alpha=alpha)   # dQ = alpha dS K
    ops.bmm(MV.scores(ds).t, qv, dkv, alpha=alpha)  # dK = alpha dS^T Q


class _AttnFn(torch.autograd.Function):
    """packed: (qkv [B, 3H, T],) -- self-attention on a packed in_proj output -- or (q [B, H, T], kv [B, 2H, Tk]) -> o [B, H, T] (+ p when
    asked); one gradient per packed tensor.  Default: the fused kernels -- the scores never reach HBM and the backward recomputes P from
    the saved log-sum-exp (csrc/attention_fused.hip); SET_AMD_ATTN_FUSED=0: bmm -> softmax -> bmm with the probabilities saved."""

    @staticmethod
    def forward(ctx, heads, kpm, fill, alpha, want_p, *packed):
        packed = tuple(t.contiguous() for t in packed)
        views = _head_views(heads, *packed)
        ctx.cfg = (heads, alpha, kpm, fill, len(packed))
        ctx.fused = ops.attention_fused_on(views[0].cols)  # (head size)
        if ctx.fused:
            o, lse, p = ops.attention_fused(*views, heads, kpm, fill, alpha, want_p)
            ctx.save_for_backward(*packed, o, lse)
        else:
            o, p = ops.attention_views(*views, heads, kpm, fill, alpha)
            ctx.save_for_backward(*packed, p)
        if p is None:
            p = packed[0].new_empty(0)
        ctx.mark_non_differentiable(p)
        return o, p

    @staticmethod
    def backward(ctx, do, _dp):
        heads, alpha, kpm, fill, n = ctx.cfg
        packed, rest = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        grads = tuple(torch.empty_like(t) for t in packed)
        views, dviews = _head_views(heads, *packed), _head_views(heads, *grads)
        if ctx.fused:
            ops.attention_fused_bwd(*views, *rest, do.contiguous(), *dviews, heads, kpm, fill, alpha)
        else:
            _attn_bwd(*views, rest[0], do.contiguous(), *dviews, heads, alpha)
        return (None,) * 5 + grads


def self_attention(qkv, heads, key_padding_mask=None, fill=float("-inf"), alpha=1.0, want_p=False):
    """(o, p): p is an empty tensor unless want_p (the fused kernels do not materialise the probabilities)."""
    return _AttnFn.apply(heads, key_padding_mask, fill, alpha, want_p, qkv)


def cross_attention(q, kv, heads, key_padding_mask=None, fill=-1e8, alpha=1.0, want_p=True):
    return _AttnFn.apply(heads, key_padding_mask, fill, alpha, want_p, q, kv)


def _preln_tail(x, gamma, p_gamma, p_beta, dh, g2, eps):
    """LayerNorm backward of a pre-LN sub-block, then the residual branch joins (LN branch + residual, the per-op tape's order)."""
    B, Cc, T = x.shape
    dxl = torch.empty_like(x)
    (t_g, r_g), (t_b, r_b) = _tape_tgt(p_gamma, x.device), _tape_tgt(p_beta, x.device)
    part = _det_scratch(x.device, L().set_layernorm_ch_bwd_scratch(B, Cc, T))
    check(L().set_layernorm_ch_bwd_add(_p(x), _p(gamma), None, _p(dh), _p(g2), _p(dxl), _p(t_g), _p(t_b), _p(part), B, Cc, T, float(eps),
                                       _stream()), "set_layernorm_ch_bwd_add")  # dx = LN gradient + residual gradient, one launch
    return dxl, r_g, r_b


class _PreLnSelfAttnFn(torch.autograd.Function):
    """One tape node for x + out_proj(self_attention(in_proj(LN(x)))) (* mask): the self-attention sub-block of Enc/DecSALayer
    (modules/speech_editing/commons/transformer.py:138-189,421-422,619-652; bias-free packed projections).  Same kernels as the per-op tape
    (LN, packed 1x1 in_proj, fused attention, 1x1 out_proj with the residual and the mask in its epilogue); fused attention kernels only."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w_in, w_out, cw_qkv, cw_out, heads, kpm, fill, alpha, mask, eps):
        x = x.contiguous()
        h = ops.layernorm_ch(x, gamma, beta, None, eps)
        qkv = ops.conv1d(h, cw_qkv)
        o, lse, _ = ops.attention_fused(*_head_views(heads, qkv), heads, kpm, fill, alpha, False)
        y = ops.conv1d(o, cw_out, None, res=x, mask=mask)
        ctx.save_for_backward(x, gamma, mask, kpm, h, qkv, o, lse)
        ctx.cfg, ctx.cws, ctx.params = (heads, fill, alpha, eps), (cw_qkv, cw_out), (gamma, beta, w_in, w_out)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mask, kpm, h, qkv, o, lse = ctx.saved_tensors
        heads, fill, alpha, eps = ctx.cfg
        cw_qkv, cw_out = ctx.cws
        p_gamma, p_beta, p_win, p_wout = ctx.params
        dy = dy.contiguous()
        B, H, T = dy.shape
        g2 = _masked_grad(dy, mask)
        do = _conv_dgrad(g2, cw_out, 1, 0, T)
        r_wo, _ = _conv_leaves(g2, o, None, p_wout, None, None, B, H, H, 1, 1, 0, T, T)
        dqkv = torch.empty_like(qkv)
        ops.attention_fused_bwd(*_head_views(heads, qkv), o, lse, do, *_head_views(heads, dqkv), heads, kpm, fill, alpha)
        dh = _conv_dgrad(dqkv, cw_qkv, 1, 0, T)
        r_wi, _ = _conv_leaves(dqkv, h, None, p_win, None, None, B, H, 3 * H, 1, 1, 0, T, T)
        dx, r_g, r_b = _preln_tail(x, gamma, p_gamma, p_beta, dh, g2, eps)
        return (dx, r_g, r_b, r_wi, r_wo) + (None,) * 8


class _PreLnCrossAttnFn(torch.autograd.Function):
    """One tape node for x + out_proj(attention(q = in_proj_q(LN(x)), k, v = in_proj_kv(enc))): the encoder-decoder attention sub-block of
    DecSALayer (transformer.py:283-410,531-609); returns (y, probabilities or an empty tensor).  The q rows and the k / v rows of the packed
    in_proj weight get ONE gradient (the per-op tape returns two full-size temporaries that autograd adds); fused attention kernels only."""

    @staticmethod
    def forward(ctx, x, enc, gamma, beta, w_in, w_out, cw_q, cw_kv, cw_out, heads, kpm, fill, alpha, want_p, eps):
        x, enc = x.contiguous(), enc.contiguous()
        h = ops.layernorm_ch(x, gamma, beta, None, eps)
        q = ops.conv1d(h, cw_q)
        kv = ops.conv1d(enc, cw_kv)
        o, lse, p = ops.attention_fused(*_head_views(heads, q, kv), heads, kpm, fill, alpha, want_p)
        y = ops.conv1d(o, cw_out, None, res=x)
        ctx.save_for_backward(x, enc, gamma, kpm, h, q, kv, o, lse)
        ctx.cfg, ctx.cws, ctx.params = (heads, fill, alpha, eps), (cw_q, cw_kv, cw_out), (gamma, beta, w_in, w_out)
        if p is None:
            p = x.new_empty(0)
        ctx.mark_non_differentiable(p)
        return y, p

    @staticmethod
    def backward(ctx, dy, _dp):
        x, enc, gamma, kpm, h, q, kv, o, lse = ctx.saved_tensors
        heads, fill, alpha, eps = ctx.cfg
        cw_q, cw_kv, cw_out = ctx.cws
        p_gamma, p_beta, p_win, p_wout = ctx.params
        g2 = dy.contiguous()
        B, H, T = g2.shape
        Tk = enc.shape[2]
        dev = g2.device
        do = _conv_dgrad(g2, cw_out, 1, 0, T)
        r_wo, _ = _conv_leaves(g2, o, None, p_wout, None, None, B, H, H, 1, 1, 0, T, T)
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        ops.attention_fused_bwd(*_head_views(heads, q, kv), o, lse, do, *_head_views(heads, dq, dkv), heads, kpm, fill, alpha)
        dh = _conv_dgrad(dq, cw_q, 1, 0, T)
        denc = _conv_dgrad(dkv, cw_kv, 1, 0, Tk) if ctx.needs_input_grad[1] else None
        # rows [0, H) of the packed weight from the queries, rows [H, 3H) from the keys / values: together the whole parameter, once
        t_wi, r_wi = _tape_tgt(p_win, dev)
        with _leaves(dev, (r_wi,), dq, dkv, h, enc):
            conv_wgrad(dq, h, None, t_wi, B, H, H, 1, 1, 0, T, T, dw_ptr=t_wi.data_ptr() + 4 * cw_q.base)
            conv_wgrad(dkv, enc, None, t_wi, B, H, 2 * H, 1, 1, 0, Tk, Tk, dw_ptr=t_wi.data_ptr() + 4 * cw_kv.base)
        dx, r_g, r_b = _preln_tail(x, gamma, p_gamma, p_beta, dh, g2, eps)
        return (dx, denc, r_g, r_b, r_wi, r_wo) + (None,) * 9


def _fused_nodes():
    return os.environ.get("SET_AMD_FUSED_NODES", "1") != "0"


def preln_self_attn(x, ln, attn, key_padding=None, mask=None, eps=1e-5):
    """x + self-attention(LayerNorm(x)) (* mask); attn: the module holding the packed projections (campnet.MultiheadAttention)."""
    if _fused_nodes() and ops.attention_fused_on(attn.embed_dim // attn.num_heads):
        return _PreLnSelfAttnFn.apply(x, ln[0], ln[1], attn._w_qkv.raw(), attn._w_out.raw(), attn._w_qkv, attn._w_out, attn.num_heads,
                                      key_padding, float("-inf"), attn.scaling, mask, eps)
    x_ln, x_res = fanout(x, 2)
    h = layernorm_ch(x_ln, ln[0], ln[1], eps=eps)
    qkv = conv1d(h, attn._w_qkv)
    o, _ = self_attention(qkv, attn.num_heads, key_padding, float("-inf"), attn.scaling)
    return conv1d(o, attn._w_out, res=x_res, mask=mask)


def preln_cross_attn(x, ln, attn, enc, enc_padding, want_p=True, eps=1e-5):
    """(x + encoder-decoder attention(LayerNorm(x), enc), probabilities [B, heads, T, T_txt] or an empty tensor)."""
    if _fused_nodes() and ops.attention_fused_on(attn.embed_dim // attn.num_heads):
        return _PreLnCrossAttnFn.apply(x, enc, ln[0], ln[1], attn._w_q.raw(), attn._w_out.raw(), attn._w_q, attn._w_kv, attn._w_out,
                                       attn.num_heads, enc_padding, -1e8, attn.scaling, want_p, eps)
    x_ln, x_res = fanout(x, 2)
    h = layernorm_ch(x_ln, ln[0], ln[1], eps=eps)
    q = conv1d(h, attn._w_q)
    kv = conv1d(enc, attn._w_kv)
    o, p = cross_attention(q, kv, attn.num_heads, enc_padding, -1e8, attn.scaling, want_p=want_p)
    return conv1d(o, attn._w_out, res=x_res), p


class _PosAddFn(torch.autograd.Function):
    """x + alpha * table[pos]   (transformer.py:795-796; alpha is the learnable pos_embed_alpha)."""

    @staticmethod
    def forward(ctx, x, alpha, pos, table):
        out = ops.embedding_bct(pos, table, scale=alpha.detach().reshape(1).contiguous(), out=x.clone(), accumulate=True)
        ctx.save_for_backward(pos, table)
        return out

    @staticmethod
    def backward(ctx, d):
        pos, table = ctx.saved_tensors
        dalpha = None
        if ctx.needs_input_grad[1]:
            pe = ops.embedding_bct(pos, table)
            prod = ops.blend_mask(torch.zeros_like(pe), pe, d.contiguous(), 1)  # pe * d elementwise
            dalpha = _sum(prod, arena=False).reshape(1)
        return d, dalpha, None, None


def pos_add(x, alpha, pos, table):
    return _PosAddFn.apply(x, alpha, pos, table)


class _MaskFillChanFn(torch.autograd.Function):
    """x*(1-m) + e[c]*m on [B,C,T]; x carries no gradient here (it is the input mel), e = mask_emb does."""

    @staticmethod
    def forward(ctx, x, e, m):
        ctx.save_for_backward(m)
        ctx.C = x.shape[1]
        return ops.mask_fill_chan(x, e.reshape(-1).contiguous(), m)

    @staticmethod
    def backward(ctx, d):
        (m,) = ctx.saved_tensors
        de = _gzeros(ctx.C, d.device)
        ops.masked_channel_sum(d.contiguous(), m, de)
        return None, de.reshape(1, 1, -1), None


def mask_fill_chan(x, e, m):
    return _MaskFillChanFn.apply(x, e, m)


class _AddMaskedFn(torch.autograd.Function):
    """a + b * m[b][t]  on [B,C,T]   (campnet.py:62,68: `mels*(1-mask) + coarse*mask`, `mel_coarse + fine*mask`)."""

    @staticmethod
    def forward(ctx, a, b, m):
        ctx.save_for_backward(m)
        return ops.sum_div(a.contiguous(), ops.add_chan_mask(b, None, m))

    @staticmethod
    def backward(ctx, d):
        (m,) = ctx.saved_tensors
        d = d.contiguous()
        return (d if ctx.needs_input_grad[0] else None), ops.add_chan_mask(d, None, m), None


def add_masked(a, b, m):
    return _AddMaskedFn.apply(a, b, m)


# --------------------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------------------
def frame_weights(target_btm):
    """weights_nonzero_speech(target)[..., 0]  -> [B*T]"""
    B, T, M = target_btm.shape
    w = torch.empty(B * T, dtype=torch.float32, device=target_btm.device)
    check(L().set_frame_weight(_p(target_btm.contiguous()), _p(w), B * T, M, _stream()), "set_frame_weight")
    return w


def _sum(x, w=None, inner=1, arena=True):
    # arena: the accumulator is a slice of the step's zero arena inside an optimisation step (no fill launch) -- for values consumed within the
    # step; a result handed to autograd as a gradient (which may keep it as .grad) owns its storage instead
    out = _gzeros(1, x.device) if arena else torch.zeros(1, dtype=torch.float32, device=x.device)
    check(L().set_weighted_sum_det(_p(x), _p(w), _p(out), x.numel(), inner, _p(_det_scratch(x.device, 1024)), _stream()),
          "set_weighted_sum_det")
    return out


class _MaskedL1Fn(torch.autograd.Function):
    """(|pred - target| * w).sum() / w_full.sum()   (speech_base.py:223-229; w broadcast over the mel axis)."""

    @staticmethod
    def forward(ctx, pred, target, w):
        pred, target = pred.contiguous(), target.contiguous()
        M = pred.shape[-1]
        absd = torch.empty_like(pred)
        check(L().set_l1_elem(_p(pred), _p(target), _p(absd), None, pred.numel(), _stream()), "set_l1_elem")
        num = _sum(absd, w, M)
        den = _sum(w) * float(M)
        ctx.save_for_backward(pred, target, w, den)
        return (num / den).reshape(())

    @staticmethod
    def backward(ctx, gout):
        pred, target, w, den = ctx.saved_tensors
        M = pred.shape[-1]
        sgn = torch.empty_like(pred)
        check(L().set_l1_elem(_p(pred), _p(target), None, _p(sgn), pred.numel(), _stream()), "set_l1_elem")
        scale = (gout.reshape(1) / den).contiguous()
        d = torch.empty_like(pred)
        check(L().set_scale_bcast(_p(sgn), _p(w), _p(d), pred.numel(), M, _p(scale), 1.0, _stream()), "set_scale_bcast")
        return d, None, None


def masked_l1(pred, target, w):
    return _MaskedL1Fn.apply(pred, target, w)


class _SSIMLossFn(torch.autograd.Function):
    """((1 - ssim_map(pred+bias, target+bias)) * w).sum() / w_full.sum()   (speech_base.py:247-257, ssim.py:24-44)."""

    @staticmethod
    def forward(ctx, pred, target, w, bias):
        B, T, M = pred.shape
        dev = pred.device
        img1, img2 = pred.contiguous(), target.contiguous()
        maps = [torch.empty(B, T, M, dtype=torch.float32, device=dev) for _ in range(5)]
        check(L().set_ssim_filter(_p(img1), _p(img2), float(bias), *[_p(m) for m in maps], B, T, M, _stream()), "set_ssim_filter")
        one_minus = torch.empty_like(pred)
        d = [torch.empty_like(pred) for _ in range(3)]
        check(L().set_ssim_map(*[_p(m) for m in maps], _p(one_minus), _p(d[0]), _p(d[1]), _p(d[2]), pred.numel(), _stream()),
              "set_ssim_map")
        num = _sum(one_minus, w, M)
        den = _sum(w) * float(M)
        ctx.save_for_backward(img1, img2, w, den, *d)
        ctx.bias = bias
        return (num / den).reshape(())

    @staticmethod
    def backward(ctx, gout):
        img1, img2, w, den, d0, d1, d2 = ctx.saved_tensors
        B, T, M = img1.shape
        scale = (-gout.reshape(1) / den).contiguous()  # d loss / d ssim = -w / den
        g = []
        for dk in (d0, d1, d2):
            t = torch.empty_like(dk)
            check(L().set_scale_bcast(_p(dk), _p(w), _p(t), dk.numel(), M, _p(scale), 1.0, _stream()), "set_scale_bcast")
            g.append(t)
        dimg = torch.empty_like(img1)
        check(L().set_ssim_bwd(_p(img1), _p(img2), float(ctx.bias), _p(g[0]), _p(g[1]), _p(g[2]), _p(dimg), B, T, M, _stream()),
              "set_ssim_bwd")
        return dimg, None, None, None


def ssim_loss(pred, target, w, bias=6.0):
    return _SSIMLossFn.apply(pred, target, w, bias)


class _DurLossFn(torch.autograd.Function):
    """returns (pdur, wdur) already multiplied by their lambdas (speech_editing_base.py:58-90)."""

    @staticmethod
    def forward(ctx, dur_pred, mel2ph, txt, word_id, n_words, lam_p, lam_w):
        dur_pred = dur_pred.contiguous()
        B, T_txt = dur_pred.shape
        T = mel2ph.shape[1]
        sums = _gzeros(4, dur_pred.device)
        check(L().set_dur_loss_sums_det(_p(dur_pred), _p(mel2ph), _p(txt), _p(word_id), _p(sums), B, T, T_txt, n_words,
                                        _p(_det_scratch(dur_pred.device, 4 * B)), _stream()), "set_dur_loss_sums_det")
        ctx.save_for_backward(dur_pred, mel2ph, txt, word_id, sums)
        ctx.cfg = (n_words, lam_p, lam_w)
        pd = sums[0] / sums[1] * lam_p
        wd = sums[2] / sums[3] * lam_w
        return pd, wd

    @staticmethod
    def backward(ctx, gp, gw):
        dur_pred, mel2ph, txt, word_id, sums = ctx.saved_tensors
        n_words, lam_p, lam_w = ctx.cfg
        B, T_txt = dur_pred.shape
        # both outputs normally receive the same upstream gradient (1.0 from the loss sum); handle them separately
        d = torch.empty_like(dur_pred)
        out = None
        for lam_a, lam_b, gg in ((lam_p, 0.0, gp), (0.0, lam_w, gw)):
            check(L().set_dur_loss(_p(dur_pred), _p(mel2ph), _p(txt), _p(word_id), _p(sums), _p(d), B, mel2ph.shape[1],
                                   T_txt, n_words, float(lam_a), float(lam_b), 1.0, _stream()), "set_dur_loss")
            term = torch.empty_like(d)
            check(L().set_scale_bcast(_p(d), None, _p(term), d.numel(), 1, _p(gg.reshape(1).contiguous()), 1.0, _stream()),
                  "set_scale_bcast")
            out = term if out is None else ops.sum_div(out, term, None, 1.0)
        return out, None, None, None, None, None, None


def dur_losses(dur_pred, mel2ph, txt, word_id, n_words, lam_p, lam_w):
    return _DurLossFn.apply(dur_pred, mel2ph, txt, word_id, n_words, lam_p, lam_w)


class _PitchLossFn(torch.autograd.Function):
    """returns (uv_loss, f0_loss) times their lambdas; pp is channel-major [B,2,T] (speech_editing_base.py:92-108)."""

    @staticmethod
    def forward(ctx, pp, f0, uv, mel2ph, lam_uv, lam_f0):
        pp = pp.contiguous()
        B, _, T = pp.shape
        sums = _gzeros(4, pp.device)
        check(L().set_pitch_loss_sums_det(_p(pp), _p(f0), _p(uv), _p(mel2ph), _p(sums), B, T,
                                          _p(_det_scratch(pp.device, 4 * ((B * T + 255) // 256))), _stream()),
              "set_pitch_loss_sums_det")
        ctx.save_for_backward(pp, f0, uv, mel2ph, sums)
        ctx.cfg = (lam_uv, lam_f0)
        return sums[0] / sums[1] * lam_uv, sums[2] / sums[3] * lam_f0

    @staticmethod
    def backward(ctx, g_uv, g_f0):
        pp, f0, uv, mel2ph, sums = ctx.saved_tensors
        lam_uv, lam_f0 = ctx.cfg
        B, _, T = pp.shape
        d = torch.empty_like(pp)
        check(L().set_pitch_loss(_p(pp), _p(f0), _p(uv), _p(mel2ph), _p(sums), _p(d), B, T, float(lam_uv),
                                 float(lam_f0), 1.0, _stream()), "set_pitch_loss")
        # rows carry independent upstream gradients: row 0 (f0) * g_f0, row 1 (uv) * g_uv
        gsc = torch.stack([g_f0.reshape(()), g_uv.reshape(())]).reshape(1, 2, 1).expand(B, 2, 1).contiguous().reshape(-1)
        out = torch.empty_like(d)
        check(L().set_scale_bcast(_p(d), _p(gsc), _p(out), d.numel(), T, None, 1.0, _stream()), "set_scale_bcast")
        return out, None, None, None, None, None


def pitch_losses(pp_bct, f0, uv, mel2ph, lam_uv, lam_f0):
    return _PitchLossFn.apply(pp_bct, f0, uv, mel2ph, lam_uv, lam_f0)


# --------------------------------------------------------------------------------------------------
# optimizer
# --------------------------------------------------------------------------------------------------
def grad_sumsq(flat_grad):
    out = torch.zeros(1, dtype=torch.float32, device=flat_grad.device)
    check(L().set_sumsq_det(_p(flat_grad), _p(out), flat_grad.numel(), _p(_det_scratch(flat_grad.device, 2048)), _stream()),
          "set_sumsq_det")
    return out


def adamw_step(flat_p, flat_g, m, v, lr, beta1, beta2, eps, weight_decay, step, sumsq=None, max_norm=0.0,
               grad_scale=1.0):
    check(L().set_adamw(_p(flat_p), _p(flat_g), _p(m), _p(v), flat_p.numel(), float(lr), float(beta1), float(beta2),
                        float(eps), float(weight_decay), int(step), _p(sumsq), float(max_norm), float(grad_scale),
                        _stream()), "set_adamw")
