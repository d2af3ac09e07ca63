"""Tensor-level wrappers over the C ABI (include/set_amd.h).

torch is used for device memory, the current HIP stream and parameter storage
only; every arithmetic op below is a kernel in libset_amd.so.  All tensors must
be fp32 (or int64 for indices), contiguous, on a HIP device.  Nothing here has a
CPU implementation: calling an op without the library / without a GPU raises.
"""
import collections
import ctypes as C
import math
import os
import typing

import torch

from . import _lib
from ._lib import (ACT, PRO, IMPL_BF16, IMPL_MFMA, IMPL_MFMA2, IMPL_NAIVE, SetConv1dArgs, SetDiffnetLayerArgs,
                   SetDiffLoopArgs, SetDiffnetStackArgs, check)

_DEFAULT_IMPL = os.environ.get("SET_AMD_CONV_IMPL", "auto")  # auto | naive | mfma
_WEIGHTS_EPOCH = 0  # bumped by in-place optimizer updates (they do not touch tensor version counters)


_COMPUTE_DTYPE = os.environ.get("SET_AMD_DTYPE", "f32")  # f32 | bf16: MFMA operand type of the conv / wgrad GEMMs


def set_compute_dtype(dtype):
    """'f32' (default; the parity path) or 'bf16': bf16 MFMA operands with fp32 accumulation, fp32 tensors in HBM and
    fp32 master weights (BASELINE configs[1]; what the reference gets from torch.autocast, trainer.py:325).  Applies to
    every conv / linear / weight-gradient GEMM large enough for the bf16 kernels; everything else is unchanged."""
    global _COMPUTE_DTYPE
    if dtype not in ("f32", "bf16"):
        raise ValueError("compute dtype must be 'f32' or 'bf16', got %r" % (dtype,))
    _COMPUTE_DTYPE = dtype


def compute_dtype():
    return _COMPUTE_DTYPE


def bump_weights_epoch():
    global _WEIGHTS_EPOCH
    _WEIGHTS_EPOCH += 1


def weights_key(tensors, *extra):
    """The key of everything cached from `tensors`: storage address and version counter of each tensor object (an in-place op, a
    load_state_dict copy or a new parameter object changes it; a `.data` view would carry a fresh counter), their device, the optimizer's
    weights epoch (its in-place kernels move no version counter) and the caller's `extra` settings.  A hit costs this one tuple and one
    compare: the bf16 training step looks up 100 - 170 weight images with it."""
    return (_WEIGHTS_EPOCH, tensors[0].device, extra, tuple([(t.data_ptr(), t._version) for t in tensors]))


class CacheSlot:
    """One cached value and the key it was built for.  `get(key, build)` returns the value while the key is unchanged, else stores
    `build(old_value)` (None at first; an image re-packed into the old storage reuses it).  `mark(key)`: the value was brought up to
    date for `key` elsewhere (the optimizer's one-launch re-packs)."""
    __slots__ = ("key", "value")

    def __init__(self):
        self.key = self.value = None

    def get(self, key, build):
        if key != self.key:
            self.value = build(self.value)
            self.key = key
        return self.value

    def mark(self, key):
        self.key = key


import weakref  # noqa: E402

_BF16_IMAGES = weakref.WeakSet()   # ConvWeights that hold a bf16 image (training rows, compute dtype bf16)
_F32_IMAGES = weakref.WeakSet()    # ConvWeights that hold an fp32 image (set_pack_conv_weight / _v2)
_PACK_TABLES = collections.OrderedDict()  # signature -> (device descriptor table, total elements, pinned host copy): the last few re-packs


def _repack_images(items):
    """Re-pack the images `items` -- (ConvWeight, _lib.IMG_* kind, slot, image, dil, CacheSlot) each -- from their master weights in ONE
    launch and mark them current for the present weights epoch; returns how many.  Images on another device than the first are left to
    the lazy path.  The descriptor table lives on the device and is built only when the set of images or their storage changes."""
    if not items:
        return 0
    ws = [it[0].raw() for it in items]
    dev = ws[0].device
    keep = [i for i, w in enumerate(ws) if w.device == dev and items[i][3].device == dev]
    # a deterministic order (the WeakSets' iteration order changes with the set of live images) and a small cache of tables: bucketed
    # ragged batches alternate between a few sets of used images (packed() vs packed_v2() by T) -- each set's table is built and uploaded
    # once, from pinned memory without a host sync
    order = sorted(range(len(keep)), key=lambda j: (items[keep[j]][3].data_ptr(), items[keep[j]][1], str(items[keep[j]][2])))
    items, ws = [items[keep[j]] for j in order], [ws[keep[j]] for j in order]
    sig = tuple((id(it[0]), it[1], it[2], w.data_ptr(), it[3].data_ptr()) for it, w in zip(items, ws))
    ent = _PACK_TABLES.get(sig)
    if ent is not None:
        _PACK_TABLES.move_to_end(sig)
    else:
        arr = (_lib.SetPackDesc * len(items))()
        start = 0
        for d, (cw, kind, slot, wp, dil, _), w in zip(arr, items, ws):
            d.w, d.wp = w.data_ptr(), wp.data_ptr()
            d.w_base, d.w_sco, d.w_sci, d.w_stap, d.start = cw.base, cw.sco, cw.sci, cw.stap, start
            d.Cout, d.Cin, d.K = cw.Cout, cw.Cin, cw.K
            n = _lib.lib().set_fill_pack_desc(C.byref(d), kind, int(dil))
            assert n == wp.numel(), (n, wp.numel(), kind)
            start += n
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        if dev.type == "cuda":
            host = host.pin_memory()
        ent = _PACK_TABLES[sig] = (host.to(dev, non_blocking=True), start, host)
        while len(_PACK_TABLES) > 8:
            _PACK_TABLES.popitem(last=False)
    check(_lib.lib().set_pack_conv_weights_batch(C.c_void_p(ent[0].data_ptr()), len(items), ent[1], _stream()), "set_pack_conv_weights_batch")
    for it, w in zip(items, ws):
        it[5].mark(weights_key((w,)))
    return len(items)


def repack_bf16_images():
    """Re-round EVERY live bf16 weight image from its fp32 master weight in ONE launch.  Called by the optimizer right after its step:
    the lazy per-weight check in `packed_bf16()` then finds nothing to do, instead of launching 100 - 170 tiny pack kernels (and
    allocating as many tensors) per training step."""
    return _repack_images([(cw, _lib.IMG_BF16, None, cw._img16.value, 0, cw._img16) for cw in _BF16_IMAGES if cw._img16.value is not None])


def repack_f32_images():
    """Re-pack every fp32 weight image USED since the last call in ONE launch (called by the optimizer right after its step, like
    repack_bf16_images): the lazy check in `packed()` / `packed_v2()` then finds nothing to do instead of launching ~150 pack kernels of
    ~5 us per fp32 training step (1.1 ms of the compute stream's 32 ms at B = 32, T = 800).  An image that was not used stays stale and
    is re-packed when it is next asked for.  Same kernel arithmetic (a copy into the image layout): same bits."""
    items = []
    for cw in _F32_IMAGES:
        if cw._used32 and cw._img32.value is not None:
            items.append((cw, _lib.IMG_F32, None, cw._img32.value, 0, cw._img32))
        for slot in cw._used2:
            ent = cw._img2.get(slot)
            if ent is not None:
                items.append((cw, _lib.IMG_F32_BIG, slot, *ent.value, ent))
        cw._used32 = False
        cw._used2 = set()
    return _repack_images(items)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


import threading  # noqa: E402

_STREAM_TLS = threading.local()  # .leaf: raw handle of the leaf stream while leaf_stream.leaf_work is open IN THIS THREAD (kernels only)


def _stream():
    """The current torch HIP stream of the current device as a raw handle.  (torch.cuda.current_stream() builds a Stream
    object through several Python layers -- ~10 us, once per kernel launch: ~3 ms of a 1,400-launch training step.)"""
    leaf = getattr(_STREAM_TLS, "leaf", None)
    if leaf is not None:
        return leaf
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """Device address of a tensor as a plain int (ctypes converts it for a `void *` parameter; wrapping it in c_void_p here cost 0.25 us per
    pointer, ~3,000 pointers per training step)."""
    return None if t is None else t.data_ptr()


def _uniform_stride(tensors):
    """Element stride between the (equal-shaped, contiguous fp32) tensors when they sit at one stride in memory, else None."""
    ptrs = [t.data_ptr() for t in tensors]
    n = tensors[0].numel()
    step = (ptrs[1] - ptrs[0]) if len(ptrs) > 1 else 4 * n
    if step % 4 or step < 4 * n or any(ptrs[i] != ptrs[0] + i * step for i in range(len(ptrs))):
        return None
    if any((not t.is_contiguous()) or t.dtype != torch.float32 for t in tensors):
        return None
    return step // 4


def _chk(t, dtype=torch.float32, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: the set_amd path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _f(t, name="tensor"):
    _chk(t, torch.float32, name)
    return t


def _fv(t, name="tensor"):
    """fp32 GPU tensor that may be a [B,C,T] view: only the last stride must be 1."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: the set_amd path has no CPU fallback" % name)
    if t.dtype != torch.float32 or t.dim() != 3 or t.stride(2) != 1:
        raise ValueError("%s must be an fp32 [B,C,T] tensor/view with unit last stride" % name)
    return t


def _i(t, name="index"):
    _chk(t, torch.int64, name)
    return t


# --------------------------------------------------------------------------
# weights: raw parameter + lazily packed MFMA image, re-packed when the parameter changes
# --------------------------------------------------------------------------
class ConvWeight:
    """Weight operand of set_conv1d.

    `w` is the raw tensor; (base, sco, sci, stap) address W[co][ci][tap] inside it, so the same class serves
    nn.Conv1d [Cout,Cin,K], nn.Linear [Cout,Cin] (K=1) and one polyphase branch of nn.ConvTranspose1d
    [Cin,Cout,k] (base=p, sco=k, sci=Cout*k, stap=u)."""

    def __init__(self, getter, Cout, Cin, K, base=0, sco=None, sci=None, stap=1):
        # `getter`: (owner, "attr.path") -- the weight is looked up on the owner at every use, so a deepcopy / pickle of
        # the model (EMA or teacher copies) follows its own parameters (a closure over the original module would keep
        # computing with the original's weights); a callable or a tensor is accepted too.
        self._getter = getter
        self.Cout, self.Cin, self.K = int(Cout), int(Cin), int(K)
        self.base = int(base)
        self.sco = int(sco if sco is not None else Cin * K)
        self.sci = int(sci if sci is not None else K)
        self.stap = int(stap)
        self._img32, self._img16, self._img_x2 = CacheSlot(), CacheSlot(), CacheSlot()
        self._img2 = {}  # big-tile images by LDS slot width: CacheSlot of (image, dil)
        self._used32, self._used2 = False, set()  # fp32 images asked for since the last repack_f32_images()

    def _resolve(self):
        g = self._getter
        if isinstance(g, tuple):
            obj = g[0]
            for name in g[1].split("."):
                # nn.Module.__getattr__ is the slow path of attribute lookup (three dict probes behind a failed normal lookup, ~0.6 us per
                # level, two levels per weight, several uses per conv): look into the module's own tables first
                d = getattr(obj, "__dict__", None)
                if d is None:
                    obj = getattr(obj, name)
                    continue
                sub = d.get("_modules")
                if sub is not None and name in sub:
                    obj = sub[name]
                    continue
                par = d.get("_parameters")
                if par is not None and name in par and par[name] is not None:
                    obj = par[name]
                    continue
                obj = getattr(obj, name)
            return obj
        return g() if callable(g) else g

    def raw(self):
        return _f(self._resolve(), "weight")

    def transposed(self):
        """W'[ci][co][tap] = W[co][ci][tap]: the weight operand of the input-gradient convolution."""
        if getattr(self, "_tr", None) is None:
            assert self.stap == 1
            self._tr = ConvWeight(self._getter, self.Cin, self.Cout, self.K, base=self.base, sco=self.sci, sci=self.sco,
                                  stap=1)
        return self._tr

    def _pack(self, w, wp, name, dtype, registry=None, mid=(), tail=()):
        """`set_pack_<name>` of the weight `w` into `wp` (None, or on another device: a new image).  An image re-packed in place is safe
        for the launches that read it before: they are earlier in stream order."""
        L = _lib.lib()
        if wp is None or wp.device != w.device:
            wp = torch.empty(getattr(L, "set_packed_%s_size" % name)(self.Cout, self.Cin, self.K), dtype=dtype, device=w.device)
        check(getattr(L, "set_pack_" + name)(_p(w), _p(wp), self.Cout, self.Cin, self.K, *mid, self.base, self.sco, self.sci, self.stap,
                                             *tail, _stream()), "set_pack_" + name)
        if registry is not None:
            registry.add(self)  # from now on the optimizer re-packs it in one launch with the others (repack_f32 / bf16_images)
        return wp

    def packed(self):
        w = self.raw()
        self._used32 = True
        return self._img32.get(weights_key((w,)), lambda wp: self._pack(w, wp, "conv_weight", torch.float32, _F32_IMAGES))

    def packed_bf16(self):
        """bf16 image for SET_IMPL_BF16 (re-rounded from the fp32 master weights whenever they change)."""
        w = self.raw()
        return self._img16.get(weights_key((w,)), lambda wp: self._pack(w, wp, "conv_weight_bf16", torch.bfloat16, _BF16_IMAGES))

    def packed_x2(self):
        """Two-piece fp16 image for SET_IMPL_F16X2 (re-split from the fp32 master weights whenever they change, into a new image)."""
        w = self.raw()
        return self._img_x2.get(weights_key((w,)), lambda _: self._pack(w, None, "conv_weight_x2", torch.float16, tail=(_x2_exponent(w),)))

    def packed_v2(self, dil):
        """Image for the big-tile kernel (depends on |dil| through the LDS chunking)."""
        w = self.raw()
        halo = (self.K - 1) * abs(dil)
        slot = 128 if (64 + halo) * 256 * 4 > 96 * 1024 else 256
        wp, _ = self._img2.setdefault(slot, CacheSlot()).get(weights_key((w,)), lambda old: (
            self._pack(w, old and old[0], "conv_weight_v2", torch.float32, _F32_IMAGES, mid=(int(dil),)), int(dil)))
        self._used2.add(slot)
        return wp


def _x2_exponent(w):
    """Power-of-two scale of a two-piece fp16 image: max |w| lands in [8, 16) (one host read-back per weight version)."""
    m = float(w.abs().max())
    return max(-60, min(60, 4 - math.frexp(m)[1])) if m > 0 and math.isfinite(m) else 0


def f16x2_eligible(T_iter, Cout, Cin, K, dil):
    """Shapes the two-piece fp16 conv kernel takes (and pays for): wide enough, receptive field <= 128 frames."""
    # (K = 1: two k-steps per 32-channel chunk between barriers -- measured slower than the fp32 kernel; not taken)
    return T_iter >= 64 and Cout >= 32 and Cin >= 32 and K >= 2 and Cin * K >= 96 and (K - 1) * abs(dil) <= 128


def conv_x2_range_flag(reset=True):
    """True if an activation left the fp16 range of the F16X2 splitting since the last reset (synchronises the device)."""
    v = C.c_int32(0)
    check(_lib.lib().set_conv_x2_range_flag(C.byref(v), int(bool(reset))), "set_conv_x2_range_flag")
    return bool(v.value)


def bf16_eligible(T_iter, Cout, Cin, K, dil, out_stride=1, out_off=0):
    """Shapes the bf16 kernels take: enough reduction depth and rows for a 64x64 wave tile to pay, stride-1 output."""
    return (T_iter >= 32 and Cout >= 32 and Cin * K >= 64 and out_stride == 1 and out_off == 0
            and (K - 1) * abs(dil) <= 128)


_AUTO_SPLIT = [False]


class split_convs:
    """with split_convs(): ...  -- inside, `auto` convolutions that are wide enough run on the two-piece fp16 kernel
    (SET_IMPL_F16X2: fp32-equivalent results on the 16-bit MFMA pipe).  The caller checks conv_x2_range_flag() afterwards and
    repeats the computation outside the scope if an activation left the fp16 range."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev, _AUTO_SPLIT[0] = _AUTO_SPLIT[0], self.on

    def __exit__(self, *exc):
        _AUTO_SPLIT[0] = self.prev


def _pick_impl(impl, T_iter, Cout=0, Cin=0, K=1, dil=1, out_stride=1, out_off=0, chan_add=False, plain=False, pad=0):
    impl = impl or _DEFAULT_IMPL
    if impl == "auto":
        if T_iter < 16:
            return "naive"
        # one or two output channels over a long sequence (HiFi-GAN conv_post): a streaming VALU kernel, not a GEMM
        if plain and Cout <= 2 and K <= 9 and dil == 1 and 0 <= pad <= 4 and K - pad <= 5 and out_stride == 1 and \
                T_iter >= 4096 and T_iter % 4 == 0 and _COMPUTE_DTYPE != "bf16":
            return "fewout"
        if _AUTO_SPLIT[0] and not chan_add and f16x2_eligible(T_iter, Cout, Cin, K, dil):
            return "f16x2"
        if _COMPUTE_DTYPE == "bf16" and bf16_eligible(T_iter, Cout, Cin, K, dil, out_stride, out_off):
            return "bf16"
        # big-tile kernel: measured (tools/conv_probe.py, profiles/r01_conv_probe.log) +2 % for the 3-tap convs with a
        # deep reduction (512 -> 256: the input-gradient convs of the DiffNet layers) on short sequences; the small-tile
        # kernel is equal or better everywhere else since its epilogue fetches its operands in batches and its main loop
        # is double-buffered (1x1 convs +3-12 %, 192 -> 192 k5 +10 %, 192 -> 384 k9 +45 %), and it balances better on
        # long sequences (HiFi-GAN)
        if Cout >= 192 and Cin >= 384 and K >= 3 and 32 <= T_iter <= 2048 and (K - 1) * abs(dil) <= 16:
            return "mfma2"
        return "mfma"
    return impl


def conv1d(x, weight, bias=None, *, dil=1, pad=0, pro="none", pro_param=0.0, act="none", act_param=0.0, alpha=1.0,
           res=None, mask=None, in_chan_add=None, out=None, accumulate=False, impl=None,
           T_iter=None, T_out=None, out_stride=1, out_off=0, out_div=0.0):
    """Generic fused conv (see SetConv1dArgs in set_amd.h).  x [B,Cin,T_in] -> out [B,Cout,T_out]."""
    _f(x, "x")
    assert isinstance(weight, ConvWeight)
    B, Cin, T_in = x.shape
    assert Cin == weight.Cin, (Cin, weight.Cin)
    if T_out is None:
        T_out = T_in + 2 * pad - dil * (weight.K - 1) if dil > 0 else T_in
    if T_iter is None:
        T_iter = T_out
    if out is None:
        out = torch.empty(B, weight.Cout, T_out, dtype=torch.float32, device=x.device)
    _fv(out, "out")
    plain = res is None and mask is None and in_chan_add is None and not accumulate and T_out == T_in and T_iter == T_out and \
        out.is_contiguous() and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    impl = _pick_impl(impl, T_iter, weight.Cout, Cin, weight.K, dil, out_stride, out_off, in_chan_add is not None, plain, pad)
    a = SetConv1dArgs()
    a.inp = x.data_ptr()
    if impl == "mfma2":
        a.w = weight.packed_v2(dil).data_ptr()
    elif impl == "bf16":
        a.w = weight.packed_bf16().data_ptr()
    elif impl == "f16x2":
        a.w = weight.packed_x2().data_ptr()
    else:  # "mfma": packed image; "naive" / "fewout": the raw weight
        a.w = (weight.packed() if impl == "mfma" else weight.raw()).data_ptr()
    a.bias = _f(bias, "bias").data_ptr() if bias is not None else None
    a.res = _fv(res, "res").data_ptr() if res is not None else None
    a.mask = _f(mask, "mask").data_ptr() if mask is not None else None
    a.in_chan_add = _f(in_chan_add, "in_chan_add").data_ptr() if in_chan_add is not None else None
    a.out = out.data_ptr()
    a.in_bs, a.in_cs = Cin * T_in, T_in
    a.out_bs, a.out_cs = out.stride(0), out.stride(1)
    if res is not None:
        a.res_bs, a.res_cs = res.stride(0), res.stride(1)
    a.w_base, a.w_sco, a.w_sci, a.w_stap = weight.base, weight.sco, weight.sci, weight.stap
    a.B, a.Cin, a.Cout, a.K, a.dil, a.pad = B, Cin, weight.Cout, weight.K, dil, pad
    a.T_in, a.T_iter, a.T_out, a.out_stride, a.out_off = T_in, T_iter, T_out, out_stride, out_off
    a.pro, a.act, a.accumulate = PRO[pro], ACT[act], int(bool(accumulate))
    a.impl = {"mfma": IMPL_MFMA, "mfma2": IMPL_MFMA2, "bf16": IMPL_BF16, "f16x2": _lib.IMPL_F16X2,
              "fewout": _lib.IMPL_FEWOUT}.get(impl, IMPL_NAIVE)
    a.pro_param, a.act_param, a.alpha = float(pro_param), float(act_param), float(alpha)
    a.out_div = float(out_div)
    assert not (out_div and not accumulate)
    if CONV_EVENTS is not None and impl in ("bf16", "mfma", "mfma2"):  # measurement hook (bench.py): hipEvents around every MFMA conv launch, keyed by shape
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(_lib.lib().set_conv1d(C.byref(a), _stream()), "set_conv1d")
        e1.record()
        CONV_EVENTS.append(((Cin, weight.Cout, weight.K, B, T_iter, impl), e0, e1))
        return out
    check(_lib.lib().set_conv1d(C.byref(a), _stream()), "set_conv1d")
    return out


CONV_EVENTS = None  # bench.py sets a list: ((Cin, Cout, K, B, T, impl), start, end) per bf16 / fp32 MFMA conv launch of the timed steps


def resblock_pair_eligible(C, K, dil, T):
    """Shapes the fused ResBlock-pair kernel takes while the split-operand scope is on (csrc/resblock_x2.hip)."""
    return bool(_AUTO_SPLIT[0]) and _DEFAULT_IMPL == "auto" and os.environ.get("SET_AMD_RESBLOCK_FUSED", "1") != "0" and \
        _lib.lib().set_resblock_pair_x2_supported(int(C), int(K), int(dil), int(T)) == 0


def resblock_pair(x, w1, b1, w2, b2, dil, *, slope=0.1, out=None, accumulate=False, out_div=0.0):
    """out = c2(lrelu(c1(lrelu(x)))) + x (+ out, / out_div): one iteration of HiFi-GAN's ResBlock1 loop (hifigan.py:51-58)
    as ONE launch on the two-piece fp16 operands; the intermediate never leaves LDS.  Bit-identical to the two conv1d
    launches with impl='f16x2'.  w1 / w2: ConvWeight [C, C, K]."""
    _f(x, "x")
    assert isinstance(w1, ConvWeight) and isinstance(w2, ConvWeight)
    B, Cc, T = x.shape
    assert (w1.Cout, w1.Cin, w2.Cout, w2.Cin) == (Cc, Cc, Cc, Cc) and w1.K == w2.K
    if out is None:
        out = torch.empty_like(x)
    _fv(out, "out")
    assert out.data_ptr() != x.data_ptr() and not (out_div and not accumulate)
    a = _lib.SetResblockPairArgs()
    a.x, a.out = x.data_ptr(), out.data_ptr()
    a.w1, a.w2 = w1.packed_x2().data_ptr(), w2.packed_x2().data_ptr()
    a.b1, a.b2 = _f(b1, "b1").data_ptr(), _f(b2, "b2").data_ptr()
    a.x_bs, a.x_cs, a.out_bs, a.out_cs = Cc * T, T, out.stride(0), out.stride(1)
    a.B, a.C, a.K, a.dil, a.T = B, Cc, w1.K, int(dil), T
    a.accumulate, a.slope, a.out_div = int(bool(accumulate)), float(slope), float(out_div)
    check(_lib.lib().set_resblock_pair_x2(C.byref(a), _stream()), "set_resblock_pair_x2")
    return out


def conv_transpose1d(x, w_getter, bias, Cin, Cout, k, stride, padding, *, pro="none", pro_param=0.0, impl=None,
                     cache=None):
    """nn.ConvTranspose1d as `stride` polyphase stride-1 convolutions (hifigan.py:114-115).
    out[co][n] = sum_ci sum_j Wt[ci][co][u*j+p] * in[ci][q-j],  n + P = u*q + p."""
    B, _, T_in = x.shape
    u, P = int(stride), int(padding)
    T_out = (T_in - 1) * u - 2 * P + k
    out = torch.empty(B, Cout, T_out, dtype=torch.float32, device=x.device)
    phases = cache if cache is not None else {}
    if impl is None and _AUTO_SPLIT[0] and Cin >= 32 and u * Cout >= 32 and T_in >= 64 and k >= u:
        # split-operand scope: every phase in one launch on the two-piece fp16 kernel (contiguous 16-byte stores)
        w = _f(ConvWeight(w_getter, Cout, Cin, k)._resolve(), "weight")

        def pack(_):
            wp = torch.empty(_lib.lib().set_packed_conv_transpose_x2_size(Cout, Cin, k, u), dtype=torch.float16, device=w.device)
            check(_lib.lib().set_pack_conv_transpose_x2(_p(w), _p(wp), Cout, Cin, k, u, _x2_exponent(w), _stream()),
                  "set_pack_conv_transpose_x2")
            return wp
        wp = phases.setdefault("x2", CacheSlot()).get(weights_key((w,)), pack)
        _f(x, "x")
        check(_lib.lib().set_conv_transpose1d_x2(_p(x), _p(wp), _p(bias) if bias is not None else None, _p(out), B, Cin, Cout, k,
                                                 u, P, T_in, PRO[pro], float(pro_param), _stream()), "set_conv_transpose1d_x2")
        return out
    for p in range(u):
        J = (k - p + u - 1) // u
        if J <= 0:
            continue
        if p not in phases:
            phases[p] = ConvWeight(w_getter, Cout, Cin, J, base=p, sco=k, sci=Cout * k, stap=u)
        conv1d(x, phases[p], bias, dil=-1, pad=0, pro=pro, pro_param=pro_param, out=out, impl=impl,
               T_iter=T_in + J - 1, T_out=T_out, out_stride=u, out_off=p - P)
    if k < u:  # output samples no tap reaches still carry the bias
        raise NotImplementedError("kernel_size < stride")
    return out


def weight_norm_fold(g, v):
    _f(g), _f(v)
    w = torch.empty_like(v)
    n0 = v.shape[0]
    check(_lib.lib().set_weight_norm_fold(_p(g), _p(v), _p(w), n0, v.numel() // n0, _stream()), "set_weight_norm_fold")
    return w


# --------------------------------------------------------------------------
# conditioner glue
# --------------------------------------------------------------------------
def layernorm_ch(x, gamma, beta, mask=None, eps=1e-5, out=None):
    _f(x), _f(gamma), _f(beta), _f(mask)
    B, Cc, T = x.shape
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().set_layernorm_ch(_p(x), _p(gamma), _p(beta), _p(mask), _p(out), B, Cc, T, float(eps), _stream()),
          "set_layernorm_ch")
    return out


def preln_ffn(x, ln, cw1, b1, cw2, b2, *, dil=1, pad=0, alpha=1.0, act="gelu", act_param=0.0, mask=None, eps=1e-5, T_out=None,
              drop=None):
    """Inference form of autograd_ops.preln_ffn: (x + conv1x1(act(alpha conv_k(LN(x))))) (* mask), the activation in the first conv's epilogue.
    drop=(p, seed, offset): the branch goes through inverted dropout before the residual add (set_residual_dropout)."""
    h = layernorm_ch(x, ln[0], ln[1], eps=eps)
    h = conv1d(h, cw1, b1, dil=dil, pad=pad, alpha=alpha, act=act, act_param=act_param, T_out=T_out)
    if drop is None:
        return conv1d(h, cw2, b2, res=x, mask=mask)
    return residual_dropout(x, conv1d(h, cw2, b2), mask, *drop)


def residual_dropout(x, z, mask, p, seed, offset=0):
    """(x + keep z/(1-p)) (* mask) on [B,C,T]; keep = set_dropout's decision for (seed, offset, element index)."""
    _f(x), _f(z), _f(mask)
    B, Cc, T = x.shape
    y = torch.empty_like(x)
    check(_lib.lib().set_residual_dropout(_p(x), _p(z), _p(mask), _p(y), B, Cc, T, float(p), int(seed), int(offset), _stream()),
          "set_residual_dropout")
    return y


def stutter_head(h, w, b):
    """Inference form of autograd_ops.stutter_losses: logits [B,T,3] = Linear(C, 3) over the frames of h [B,C,T] (no losses)."""
    _f(h), _f(w), _f(b)
    B, Cc, T = h.shape
    assert w.shape == (3, Cc) and b.shape == (3,), (tuple(w.shape), tuple(b.shape))
    logits = torch.empty(B, T, 3, dtype=torch.float32, device=h.device)
    check(_lib.lib().set_stutter_head_loss(_p(h), _p(w), _p(b), None, _p(logits), None, None, B, Cc, T, _stream()),
          "set_stutter_head_loss")
    return logits


def log_mel(wav, table, basis, lengths=None, *, n_fft, hop, n_mels, bin_lo, nbins, pad, reflect, clamp_input, mag_eps, floor, log_scale):
    """set_log_mel: wav [B,N] -> log-mel [B,T,n_mels] in one launch (melspec.LogMel prepares `table` / `basis`, the packed DFT table and
    filterbank images; `lengths` int64 [B] on the device or None).  Frames at or beyond a row's own count are 0.0."""
    _f(wav, "wav"), _f(table, "table"), _f(basis, "basis"), _i(lengths, "lengths")
    B, N = wav.shape
    T = 1 + (N + 2 * pad - n_fft) // hop
    mel = torch.empty(B, max(T, 0), n_mels, dtype=torch.float32, device=wav.device)
    a = _lib.SetLogMelArgs(wav=_p(wav), lengths=_p(lengths), table=_p(table), basis=_p(basis), mel=_p(mel), wav_bs=wav.stride(0),
                           log_scale=float(log_scale), B=B, N=N, T=T, n_fft=n_fft, hop=hop, n_mels=n_mels, bin_lo=bin_lo, nbins=nbins,
                           pad=pad, reflect=int(reflect), clamp_input=int(clamp_input), mag_eps=float(mag_eps), floor=float(floor))
    if table.numel() < _lib.lib().set_log_mel_table_size(n_fft, nbins) or basis.numel() < (nbins + 31) // 32 * 16 * 64 * 4:
        raise ValueError("log_mel: table / basis images are smaller than n_fft = %d, nbins = %d need" % (n_fft, nbins))
    check(_lib.lib().set_log_mel(C.byref(a), _stream()), "set_log_mel")
    return mel


def _buf(shape, device, sentinel):
    """An output or scratch buffer a kernel must write in full: uninitialised, or filled with `sentinel` (the tests pass NaN)."""
    t = torch.empty(shape, dtype=torch.float32, device=device)
    return t if sentinel is None else t.fill_(sentinel)


def mel_linear(wav, table, basis, *, n_fft, hop, n_mels, bin_lo, nbins, pad, reflect, clamp_input, mag_eps, sentinel=None):
    """set_mel_linear: wav [B,N] -> the filterbank product [B,T,n_mels] that set_log_mel takes the log of (same kernel body, same images)."""
    _f(wav, "wav"), _f(table, "table"), _f(basis, "basis")
    B, N = wav.shape
    T = 1 + (N + 2 * pad - n_fft) // hop
    mel = _buf((B, max(T, 0), n_mels), wav.device, sentinel)
    a = _lib.SetLogMelArgs(wav=_p(wav), lengths=None, table=_p(table), basis=_p(basis), mel=_p(mel), wav_bs=wav.stride(0), log_scale=1.0,
                           B=B, N=N, T=T, n_fft=n_fft, hop=hop, n_mels=n_mels, bin_lo=bin_lo, nbins=nbins, pad=pad, reflect=int(reflect),
                           clamp_input=int(clamp_input), mag_eps=float(mag_eps), floor=1.0)
    if table.numel() < _lib.lib().set_log_mel_table_size(n_fft, nbins) or basis.numel() < (nbins + 31) // 32 * 16 * 64 * 4:
        raise ValueError("mel_linear: table / basis images are smaller than n_fft = %d, nbins = %d need" % (n_fft, nbins))
    check(_lib.lib().set_mel_linear(C.byref(a), _stream()), "set_mel_linear")
    return mel


def mel_loss_fwd(mel_hat, mel_y, *, floor, log_scale, return_logs=False, sentinel=None):
    """set_mel_loss_fwd: the two linear mels [B,T,n_mels] -> (loss [1] = mean |L_hat - L_y|, g_mel = B T n_mels d loss / d mel_hat, L_hat, L_y);
    the two log-mels are None unless `return_logs`.  Two launches, no atomics, one summation order."""
    _f(mel_hat, "mel_hat"), _f(mel_y, "mel_y")
    if mel_hat.dim() != 3 or mel_hat.shape != mel_y.shape:
        raise ValueError("mel_loss_fwd: mel_hat and mel_y must be equal [B, T, n_mels], got %s and %s" % (tuple(mel_hat.shape), tuple(mel_y.shape)))
    B, T, M = mel_hat.shape
    dev = mel_hat.device
    g_mel, loss = _buf((B, T, M), dev, sentinel), _buf((1,), dev, sentinel)
    log_hat = _buf((B, T, M), dev, sentinel) if return_logs else None
    log_y = _buf((B, T, M), dev, sentinel) if return_logs else None
    part = _buf((_lib.lib().set_mel_loss_fwd_scratch_floats(B * T * M),), dev, sentinel)
    a = _lib.SetMelLossFwdArgs(mel_hat=_p(mel_hat), mel_y=_p(mel_y), g_mel=_p(g_mel), log_hat=_p(log_hat), log_y=_p(log_y), part=_p(part),
                               loss=_p(loss), log_scale=float(log_scale), B=B, T=T, n_mels=M, floor=float(floor))
    check(_lib.lib().set_mel_loss_fwd(C.byref(a), _stream()), "set_mel_loss_fwd")
    return loss, g_mel, log_hat, log_y


def mel_loss_bwd(wav, g_mel, table, basis_t, itable, *, n_fft, hop, n_mels, bin_lo, nbins, pad, mag_eps, count=1.0, sentinel=None):
    """set_mel_loss_bwd: the waveform [B,N] the linear mel was taken of and g_mel [B,T,n_mels] -> d/d wav [B,N] through filterbank,
    magnitude, windowed DFT, reflect padding and the input clamp, divided by `count` at the end (mel_loss_fwd's g_mel is count times the
    loss's gradient).  vocoder_losses.MelSpectrogramLoss prepares the images.  Three launches."""
    _f(wav, "wav"), _f(g_mel, "g_mel"), _f(table, "table"), _f(basis_t, "basis_t"), _f(itable, "itable")
    B, N = wav.shape
    T = 1 + (N + 2 * pad - n_fft) // hop
    if tuple(g_mel.shape) != (B, T, n_mels):
        raise ValueError("mel_loss_bwd: g_mel must be [%d, %d, %d], got %s" % (B, T, n_mels, tuple(g_mel.shape)))
    L = _lib.lib()
    nch = (nbins + 31) // 32
    if table.numel() < L.set_log_mel_table_size(n_fft, nbins) or itable.numel() < L.set_mel_idft_table_size(n_fft, nbins) \
            or basis_t.numel() < nch * 48 * 64:
        raise ValueError("mel_loss_bwd: table / basis_t / itable images are smaller than n_fft = %d, nbins = %d need" % (n_fft, nbins))
    dev = wav.device
    spec = _buf((max(L.set_mel_loss_bwd_spec_floats(B, T, nbins), 0),), dev, sentinel)
    g_pad, g_wav = _buf((B, (max(T, 0) + 3) * hop), dev, sentinel), _buf((B, N), dev, sentinel)
    a = _lib.SetMelLossBwdArgs(wav=_p(wav), table=_p(table), basis_t=_p(basis_t), itable=_p(itable), g_mel=_p(g_mel), spec=_p(spec),
                               g_pad=_p(g_pad), g_wav=_p(g_wav), wav_bs=wav.stride(0), B=B, N=N, T=T, n_fft=n_fft, hop=hop, n_mels=n_mels,
                               bin_lo=bin_lo, nbins=nbins, pad=pad, mag_eps=float(mag_eps), count=float(count))
    check(L.set_mel_loss_bwd(C.byref(a), _stream()), "set_mel_loss_bwd")
    return g_wav


def stft_geometries():
    """The (n_fft, hop, win) triples csrc/stft_loss.hip is compiled for."""
    L = _lib.lib()
    n = L.set_stft_geometries(None, 0)
    buf = (C.c_int32 * (3 * n))()
    L.set_stft_geometries(buf, n)
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]


_STFT_SIZE_KEYS = ("T", "table", "itable", "part", "mag", "spec", "g_pad", "Ts")


def stft_sizes(n_fft, hop, win, B, N):
    """set_stft_sizes as a dict: T, Ts and the element counts of table, itable, part (doubles), mag, spec, g_pad."""
    out = (C.c_int64 * 8)()
    check(_lib.lib().set_stft_sizes(n_fft, hop, win, B, N, out), "set_stft_sizes")
    return dict(zip(_STFT_SIZE_KEYS, out))


def _stft_args(x, y, table, n_fft, hop, win, what):
    _f(x, "x"), _f(table, "table")
    if y is not None:
        _f(y, "y")
        if y.shape != x.shape:
            raise ValueError("%s: x and y must be equal [B, N], got %s and %s" % (what, tuple(x.shape), tuple(y.shape)))
    if x.dim() != 2:
        raise ValueError("%s: x must be [B, N], got %s" % (what, tuple(x.shape)))
    B, N = x.shape
    sz = stft_sizes(n_fft, hop, win, B, N)
    if table.numel() < sz["table"]:
        raise ValueError("%s: the table image is smaller than (%d, %d, %d) needs" % (what, n_fft, hop, win))
    a = _lib.SetStftLossArgs(x=_p(x), y=_p(y), table=_p(table), x_bs=x.stride(0), y_bs=0 if y is None else y.stride(0), B=B, N=N, T=sz["T"],
                             n_fft=n_fft, hop=hop, win=win, scale=1.0)
    return a, sz


def stft_magnitude(x, table, *, n_fft, hop, win, sentinel=None):
    """set_stft_magnitude: x [B,N] -> sqrt(max(re^2 + im^2, 1e-7)) [B, T, n_fft/2 + 1] of the centred, reflect-padded STFT."""
    a, sz = _stft_args(x, None, table, n_fft, hop, win, "stft_magnitude")
    mag = _buf((x.shape[0], sz["T"], n_fft // 2 + 1), x.device, sentinel)
    a.mag = _p(mag)
    check(_lib.lib().set_stft_magnitude(C.byref(a), _stream()), "set_stft_magnitude")
    return mag


def stft_loss_fwd(x, y, table, *, n_fft, hop, win, which=1, keep=False, sentinel=None):
    """set_stft_loss_fwd: (loss [2] = spectral convergence and log-magnitude loss of one resolution, stats [6] float64 = D, G, count and
    the three sums, the kept magnitudes of the signal that is not differentiated or None).  `which`: 1 = y is differentiated, 0 = x."""
    a, sz = _stft_args(x, y, table, n_fft, hop, win, "stft_loss_fwd")
    dev = x.device
    loss = _buf((2,), dev, sentinel)
    stats = torch.empty(6, dtype=torch.float64, device=dev)
    part = torch.empty(sz["part"], dtype=torch.float64, device=dev)
    if sentinel is not None:
        stats.fill_(sentinel), part.fill_(sentinel)
    mag = _buf((sz["mag"],), dev, sentinel) if keep else None
    a.loss, a.stats, a.part, a.mag, a.which = _p(loss), _p(stats), _p(part), _p(mag), int(which)
    check(_lib.lib().set_stft_loss_fwd(C.byref(a), _stream()), "set_stft_loss_fwd")
    return loss, stats, mag


def stft_loss_bwd(x, y, table, itable, *, n_fft, hop, win, which=1, stats=None, u_sc=None, u_mag=None, scale=1.0, mag=None, g_m=None,
                  g_wav=None, sentinel=None, scratch=None):
    """set_stft_loss_bwd: the gradient [B,N] of scale (u_sc sc + u_mag mag) with respect to y (which = 1) or x (which = 0), written to a
    new tensor or ADDED to `g_wav`.  u_sc, u_mag: fp32 device tensors of one element; stats: stft_loss_fwd's; mag: its kept magnitudes
    (None: the other signal's DFT is computed again).  `g_m` [B,T,bins] replaces the loss's own magnitude gradient.  A dict `scratch`
    receives the two intermediate buffers (spec, g_pad) for inspection."""
    a, sz = _stft_args(x, y, table, n_fft, hop, win, "stft_loss_bwd")
    _f(itable, "itable")
    B, N = x.shape
    dev = x.device
    if itable.numel() < sz["itable"]:
        raise ValueError("stft_loss_bwd: the inverse table image is smaller than (%d, %d, %d) needs" % (n_fft, hop, win))
    if g_m is not None:
        _f(g_m, "g_m")
        if tuple(g_m.shape) != (B, sz["T"], n_fft // 2 + 1):
            raise ValueError("stft_loss_bwd: g_m must be [%d, %d, %d], got %s" % (B, sz["T"], n_fft // 2 + 1, tuple(g_m.shape)))
    else:
        _f(u_sc, "u_sc"), _f(u_mag, "u_mag")
        _chk(stats, torch.float64, "stats")
        if stats is None or u_sc is None or u_mag is None or stats.numel() < 6 or u_sc.numel() != 1 or u_mag.numel() != 1:
            raise ValueError("stft_loss_bwd: needs stats [6] and one-element u_sc, u_mag (or g_m)")
    if mag is not None and _f(mag, "mag").numel() < sz["mag"]:
        raise ValueError("stft_loss_bwd: the kept magnitudes are smaller than the forward writes")
    accumulate = g_wav is not None
    if accumulate:
        _f(g_wav, "g_wav")
        if tuple(g_wav.shape) != (B, N):
            raise ValueError("stft_loss_bwd: g_wav must be [%d, %d], got %s" % (B, N, tuple(g_wav.shape)))
    else:
        g_wav = _buf((B, N), dev, sentinel)
    spec, g_pad = _buf((sz["spec"],), dev, sentinel), _buf((sz["g_pad"],), dev, sentinel)
    a.itable, a.stats, a.u_sc, a.u_mag, a.g_m, a.mag = _p(itable), _p(stats), _p(u_sc), _p(u_mag), _p(g_m), _p(mag)
    a.spec, a.g_pad, a.g_wav, a.which, a.accumulate, a.scale = _p(spec), _p(g_pad), _p(g_wav), int(which), int(accumulate), float(scale)
    check(_lib.lib().set_stft_loss_bwd(C.byref(a), _stream()), "set_stft_loss_bwd")
    if scratch is not None:
        scratch.update(spec=spec, g_pad=g_pad)
    return g_wav


def _len_arg(lengths, B, name):
    _i(lengths, name)
    if lengths is not None and lengths.shape != (B,):
        raise ValueError("%s must be [%d], got %s" % (name, B, tuple(lengths.shape)))


def _out_arg(t, shape, dtype, ref, name):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=ref.device)
    _chk(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or t.device != ref.device:
        raise ValueError("%s must be %s on %s, got %s on %s" % (name, tuple(shape), ref.device, tuple(t.shape), t.device))
    return t


def mfcc(mel, table, lengths=None, take_log=False, out=None):
    """set_mfcc: mel [B,T,M] -> [B,T,K] against the DCT-II table [K,M] (metrics.dct_table); rows at or beyond `lengths` are +0.0."""
    _f(mel, "mel"), _f(table, "table")
    if mel.dim() != 3 or table.dim() != 2 or table.shape[1] != mel.shape[2]:
        raise ValueError("mfcc: mel must be [B,T,M] and table [K,M], got %s and %s" % (tuple(mel.shape), tuple(table.shape)))
    B, T, M = mel.shape
    K = table.shape[0]
    _len_arg(lengths, B, "lengths")
    out = _out_arg(out, (B, T, K), torch.float32, mel, "out")
    check(_lib.lib().set_mfcc(_p(mel), _p(lengths), _p(table), _p(out), B, T, M, K, int(bool(take_log)), _stream()), "set_mfcc")
    return out


def _pair_args(x, y, len_x, len_y, what):
    _f(x, "x"), _f(y, "y")
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("%s: x and y must be [B,Tx,K] and [B,Ty,K], got %s and %s" % (what, tuple(x.shape), tuple(y.shape)))
    if x.shape[2] != y.shape[2]:
        raise ValueError("%s: x has %d coefficients per frame, y has %d" % (what, x.shape[2], y.shape[2]))
    if y.device != x.device:
        raise ValueError("%s: x and y must be on one device" % what)
    _len_arg(len_x, x.shape[0], "len_x"), _len_arg(len_y, x.shape[0], "len_y")
    return x.shape[0], x.shape[1], y.shape[1], x.shape[2]


def dtw(x, y, len_x=None, len_y=None, dist=None, steps=None, dir=None):
    """set_dtw: the exact DTW of x [B,Tx,K] and y [B,Ty,K] under the euclidean cost -> (dist [B] fp32, steps [B] int32).  `dir`
    ([B,Tx,Ty] uint8, optional) receives the chosen predecessor of every cell inside [0, len_x) x [0, len_y) and is left as it was
    elsewhere.  `dist` / `steps`: optional output tensors."""
    B, Tx, Ty, K = _pair_args(x, y, len_x, len_y, "dtw")
    dist = _out_arg(dist, (B,), torch.float32, x, "dist")
    steps = _out_arg(steps, (B,), torch.int32, x, "steps")
    if dir is not None:
        _out_arg(dir, (B, Tx, Ty), torch.uint8, x, "dir")
    check(_lib.lib().set_dtw(_p(x), _p(y), _p(len_x), _p(len_y), _p(dist), _p(steps), _p(dir), B, Tx, Ty, K, _stream()), "set_dtw")
    return dist, steps


def dtw_path(dir, steps, len_x=None, len_y=None, path=None):
    """set_dtw_path: dir [B,Tx,Ty] uint8 and steps [B] int32 (both from `dtw`) -> path [B,Tx+Ty-1,2] int32, entries 0 .. steps[b]-1 of
    row b in path order from (0, 0); entries beyond are left as they were."""
    _chk(dir, torch.uint8, "dir"), _chk(steps, torch.int32, "steps")
    if dir.dim() != 3 or steps.shape != (dir.shape[0],):
        raise ValueError("dtw_path: dir must be [B,Tx,Ty] and steps [B], got %s and %s" % (tuple(dir.shape), tuple(steps.shape)))
    B, Tx, Ty = dir.shape
    _len_arg(len_x, B, "len_x"), _len_arg(len_y, B, "len_y")
    path = _out_arg(path, (B, Tx + Ty - 1, 2), torch.int32, dir, "path")
    check(_lib.lib().set_dtw_path(_p(dir), _p(len_x), _p(len_y), _p(steps), _p(path), B, Tx, Ty, _stream()), "set_dtw_path")
    return path


def zero_fill_dist(x, y, len_x=None, len_y=None):
    """set_zero_fill_dist: sum over t < max(len_x, len_y) of ||x_t - y_t||, the shorter side read as zeros -> [B] fp32."""
    B, Tx, Ty, K = _pair_args(x, y, len_x, len_y, "zero_fill_dist")
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    check(_lib.lib().set_zero_fill_dist(_p(x), _p(y), _p(len_x), _p(len_y), _p(out), B, Tx, Ty, K, _stream()), "set_zero_fill_dist")
    return out


def mcd_finish(num, steps, len_1, len_2, T1, T2):
    """set_mcd_finish: (mcd [B] fp32 = num / frames, penalty [B] fp32 = 2 - (len_1 + len_2) / frames, frames [B] int64), frames =
    `steps` (int32, from `dtw`) or, with steps None, max(len_1, len_2)."""
    _f(num, "num"), _chk(steps, torch.int32, "steps")
    B = num.shape[0]
    _len_arg(len_1, B, "len_1"), _len_arg(len_2, B, "len_2")
    mcd = torch.empty(B, dtype=torch.float32, device=num.device)
    penalty = torch.empty(B, dtype=torch.float32, device=num.device)
    frames = torch.empty(B, dtype=torch.int64, device=num.device)
    check(_lib.lib().set_mcd_finish(_p(num), _p(steps), _p(len_1), _p(len_2), _p(mcd), _p(penalty), _p(frames), B, int(T1), int(T2),
                                    _stream()), "set_mcd_finish")
    return mcd, penalty, frames


STOI_FRAME, STOI_HOP, STOI_SEG = 1024, 256, 30


def stoi_sizes(N):
    """(F_max, S, T) of waveforms of N samples (include/set_amd.h, the STOI block): energy frames at hop 512, samples of a compacted row,
    envelope frames at hop 256."""
    f_max = -(-(int(N) - STOI_FRAME) // (STOI_FRAME // 2)) if N > STOI_FRAME else 0
    return f_max, (STOI_FRAME // 2) * (f_max + 1), max(2 * (f_max - 1), 0)


def _stoi_wave_args(x, win, what):
    _f(x, "x"), _f(win, "win")
    if x.dim() != 2 or x.shape[1] <= STOI_FRAME or win.shape != (STOI_FRAME,):
        raise ValueError("%s: x must be [B,N] with N > %d and win [%d], got %s and %s" % (what, STOI_FRAME, STOI_FRAME, tuple(x.shape),
                                                                                         tuple(win.shape)))
    return x.shape[0], x.shape[1], stoi_sizes(x.shape[1])


def stoi_select(x, win, lengths=None, nrm=None, kept=None, K=None):
    """set_stoi_select: x [B,N] -> (kept [B,F_max] int32, K [B] int32, nrm [B,F_max] fp32): the frames of each row within 40 dB of its
    loudest, ascending in kept[b, :K[b]], and the frame norms nrm[b, :F_b]; entries beyond are left as they were."""
    B, N, (f_max, _, _) = _stoi_wave_args(x, win, "stoi_select")
    _len_arg(lengths, B, "lengths")
    nrm = _out_arg(nrm, (B, f_max), torch.float32, x, "nrm")
    kept = _out_arg(kept, (B, f_max), torch.int32, x, "kept")
    K = _out_arg(K, (B,), torch.int32, x, "K")
    check(_lib.lib().set_stoi_select(_p(x), x.stride(0), _p(lengths), _p(win), _p(nrm), _p(kept), _p(K), B, N, STOI_FRAME, _stream()),
          "set_stoi_select")
    return kept, K, nrm


def stoi_compact(x, y, win, kept, K, sil=None, sil_len=None):
    """set_stoi_compact: the overlap-add of the kept windowed frames of x and of y (both by x's list) -> (sil [2B,S], sil_len [2B] int64);
    row b is x's signal, row B + b is y's, and nothing at or beyond sil_len is written."""
    B, N, (f_max, S, _) = _stoi_wave_args(x, win, "stoi_compact")
    _f(y, "y"), _chk(kept, torch.int32, "kept"), _chk(K, torch.int32, "K")
    if y.shape != x.shape or y.device != x.device or kept.shape != (B, f_max) or K.shape != (B,):
        raise ValueError("stoi_compact: y must be %s, kept [%d,%d] and K [%d], got %s, %s and %s"
                         % (tuple(x.shape), B, f_max, B, tuple(y.shape), tuple(kept.shape), tuple(K.shape)))
    sil = _out_arg(sil, (2 * B, S), torch.float32, x, "sil")
    sil_len = _out_arg(sil_len, (2 * B,), torch.int64, x, "sil_len")
    check(_lib.lib().set_stoi_compact(_p(x), _p(y), x.stride(0), _p(win), _p(kept), _p(K), _p(sil), S, _p(sil_len), B, N, STOI_FRAME,
                                      _stream()), "set_stoi_compact")
    return sil, sil_len


def stoi_bands(sil, table, basis, lens=None, *, n_bands, bin_lo, nbins, tob=None):
    """set_stoi_bands: sil [R,S] -> band envelopes tob [R,T,n_bands], T = ceil((S - 1024) / 256); frames at or beyond a row's own count
    (from `lens`, int64 [R] samples) are +0.0.  `table` / `basis`: the packed DFT table and band matrix (metrics.stoi prepares them).
    S <= 1024 has no frame: an empty result and no launch."""
    _f(sil, "sil"), _f(table, "table"), _f(basis, "basis")
    if sil.dim() != 2:
        raise ValueError("stoi_bands: sil must be [R,S], got %s" % (tuple(sil.shape),))
    R, S = sil.shape
    _len_arg(lens, R, "lens")
    T = -(-(S - STOI_FRAME) // STOI_HOP) if S > STOI_FRAME else 0
    tob = _out_arg(tob, (R, T, n_bands), torch.float32, sil, "tob")
    if table.numel() < _lib.lib().set_log_mel_table_size(STOI_FRAME, nbins) or basis.numel() < (nbins + 31) // 32 * 16 * 64 * 4:
        raise ValueError("stoi_bands: table / basis images are smaller than nbins = %d needs" % nbins)
    if T > 0:
        check(_lib.lib().set_stoi_bands(_p(sil), sil.stride(0), _p(lens), _p(table), _p(basis), _p(tob), R, S, T, STOI_FRAME, STOI_HOP,
                                        n_bands, bin_lo, nbins, _stream()), "set_stoi_bands")
    return tob


def stoi_score(tob, lens=None, d=None, valid=None):
    """set_stoi_score: tob [2B,T,n_bands] (row b = clean, row B + b = degraded) -> (d [B] fp32, valid [B] bool).  `lens` int64 [B]:
    compacted samples per pair (stoi_compact's sil_len[:B]); a row of fewer than 30 frames has valid = False and d = NaN."""
    _f(tob, "tob")
    if tob.dim() != 3 or tob.shape[0] % 2:
        raise ValueError("stoi_score: tob must be [2B,T,n_bands], got %s" % (tuple(tob.shape),))
    B, T, n_bands = tob.shape[0] // 2, tob.shape[1], tob.shape[2]
    _len_arg(lens, B, "lens")
    d = _out_arg(d, (B,), torch.float32, tob, "d")
    valid = _out_arg(valid, (B,), torch.bool, tob, "valid")
    check(_lib.lib().set_stoi_score(_p(tob) if T else None, _p(lens), _p(d), _p(valid), B, T, n_bands, STOI_SEG, _stream()), "set_stoi_score")
    return d, valid


DB_FLOOR, DB_SCALE = 1e-10, 10.0 / math.log(10.0)  # librosa.power_to_db: 10 log10(max(amin, S)), ref = 1


def db_mel(wav, table, basis, lengths=None, *, n_mels, bin_lo, nbins, out=None):
    """set_db_mel: wav [B,N] -> 10 log10(max(1e-10, basis |STFT|^2)) [B,T,n_mels], T = 1 + N // 256, reflection padding of 512 (`table` /
    `basis`: the packed images of set_log_mel; `lengths` int64 [B] samples on the device or None).  A row of more than 512 samples has
    1 + len // 256 frames, a shorter one none; frames at or beyond a row's own count are +0.0."""
    _f(wav, "wav"), _f(table, "table"), _f(basis, "basis")
    if wav.dim() != 2 or wav.shape[1] <= 512:
        raise ValueError("db_mel: wav must be [B,N] with N > 512, got %s" % (tuple(wav.shape),))
    B, N = wav.shape
    _len_arg(lengths, B, "lengths")
    T = 1 + N // 256
    out = _out_arg(out, (B, T, n_mels), torch.float32, wav, "out")
    if table.numel() < _lib.lib().set_log_mel_table_size(1024, nbins) or basis.numel() < (nbins + 31) // 32 * 16 * 64 * 4:
        raise ValueError("db_mel: table / basis images are smaller than nbins = %d needs" % nbins)
    a = _lib.SetLogMelArgs(wav=_p(wav), lengths=_p(lengths), table=_p(table), basis=_p(basis), mel=_p(out),
                           wav_bs=wav.stride(0) if B > 1 else N,  # (a one-row tensor's stride is whatever its maker left there)
                           log_scale=DB_SCALE, B=B, N=N, T=T, n_fft=1024, hop=256, n_mels=n_mels, bin_lo=bin_lo, nbins=nbins, pad=512,
                           reflect=1, clamp_input=0, mag_eps=0.0, floor=DB_FLOOR)
    check(_lib.lib().set_db_mel(C.byref(a), _stream()), "set_db_mel")
    return out


def db_peak(db, frames=None, peak=None):
    """set_db_peak: db [B,T,M] -> peak [B], the maximum over the row's own frames (`frames` int64 [B] or None) and all bands; -inf for a
    row without frames."""
    _f(db, "db")
    if db.dim() != 3:
        raise ValueError("db_peak: db must be [B,T,M], got %s" % (tuple(db.shape),))
    B, T, M = db.shape
    _len_arg(frames, B, "frames")
    peak = _out_arg(peak, (B,), torch.float32, db, "peak")
    check(_lib.lib().set_db_peak(_p(db), _p(frames), _p(peak), B, T, M, _stream()), "set_db_peak")
    return peak


def db_mfcc(db, table, peak, frames=None, top_db=80.0, out=None):
    """set_db_mfcc: db [B,T,M], peak [B] -> [B,T,K] = table [K,M] (metrics.dct_ortho_table) applied to max(db, peak - top_db); rows at or
    beyond `frames` are +0.0."""
    _f(db, "db"), _f(table, "table"), _f(peak, "peak")
    if db.dim() != 3 or table.dim() != 2 or table.shape[1] != db.shape[2] or peak.shape != (db.shape[0],):
        raise ValueError("db_mfcc: db must be [B,T,M], table [K,M] and peak [B], got %s, %s and %s"
                         % (tuple(db.shape), tuple(table.shape), tuple(peak.shape)))
    B, T, M = db.shape
    K = table.shape[0]
    _len_arg(frames, B, "frames")
    out = _out_arg(out, (B, T, K), torch.float32, db, "out")
    check(_lib.lib().set_db_mfcc(_p(db), _p(frames), _p(peak), _p(table), _p(out), B, T, M, K, float(top_db), _stream()), "set_db_mfcc")
    return out


def coef_rms_dist(x, y, frames_x=None, frames_y=None, mcd=None, valid=None):
    """set_coef_rms_dist: x [B,Tx,K], y [B,Ty,K] -> (mcd [B] fp32, valid [B] bool): eval/mcd.py `cal_mcd(use_dtw=False)` per pair,
    mean_k(10 / ln 10 sqrt(2 sum_t (x - y)^2)) / T.  A pair of unequal frame counts, or without frames, has valid = False and mcd = NaN."""
    B, Tx, Ty, K = _pair_args(x, y, frames_x, frames_y, "coef_rms_dist")
    mcd = _out_arg(mcd, (B,), torch.float32, x, "mcd")
    valid = _out_arg(valid, (B,), torch.bool, x, "valid")
    check(_lib.lib().set_coef_rms_dist(_p(x), _p(y), _p(frames_x), _p(frames_y), _p(mcd), _p(valid), B, Tx, Ty, K, _stream()),
          "set_coef_rms_dist")
    return mcd, valid


def preln_self_attn(x, ln, attn, key_padding=None, mask=None, eps=1e-5):
    """Inference form of autograd_ops.preln_self_attn."""
    h = layernorm_ch(x, ln[0], ln[1], eps=eps)
    qkv = conv1d(h, attn._w_qkv)
    o, _ = self_attention(qkv, attn.num_heads, key_padding, float("-inf"), attn.scaling)
    return conv1d(o, attn._w_out, res=x, mask=mask)


def preln_cross_attn(x, ln, attn, enc, enc_padding, want_p=True, eps=1e-5):
    """Inference form of autograd_ops.preln_cross_attn: (x + attention, probabilities or None)."""
    h = layernorm_ch(x, ln[0], ln[1], eps=eps)
    q = conv1d(h, attn._w_q)
    kv = conv1d(enc, attn._w_kv)
    o, p = cross_attention(q, kv, attn.num_heads, enc_padding, -1e8, attn.scaling, want_p=want_p)
    return conv1d(o, attn._w_out, res=x), p


_VALIDATE = os.environ.get("SET_AMD_VALIDATE", "0") == "1"


def set_validate(on):
    """Host-side range checks of index tensors before the kernels that would otherwise clamp them (one device->host
    read per call: a debugging aid, off by default; `--validate` / `--debug` runs switch it on)."""
    global _VALIDATE
    _VALIDATE = bool(on)


def embedding_bct(idx, table, scale=1.0, out=None, accumulate=False, padding_idx=None):
    _i(idx), _f(table)
    B, T = idx.shape
    n_rows, Cc = table.shape
    if _VALIDATE and idx.numel() > 0:
        lo, hi = int(idx.min().item()), int(idx.max().item())
        if lo < 0 or hi >= n_rows:  # nn.Embedding raises here; the kernel clamps for memory safety only
            raise IndexError("embedding index out of range: [%d, %d] for a table of %d rows" % (lo, hi, n_rows))
    if out is None:
        assert not accumulate
        out = torch.empty(B, Cc, T, dtype=torch.float32, device=table.device)
    if isinstance(scale, torch.Tensor):  # a scale that lives on the device (a parameter): no host read
        check(_lib.lib().set_embedding_bct_dev_scale(_p(idx), _p(table), _p(_f(out)), B, T, Cc, n_rows, _p(_f(scale, "scale")),
                                                     int(bool(accumulate)), _stream()), "set_embedding_bct_dev_scale")
        return out
    check(_lib.lib().set_embedding_bct(_p(idx), _p(table), _p(_f(out)), B, T, Cc, n_rows, float(scale),
                                       int(bool(accumulate)), _stream()), "set_embedding_bct")
    return out


def abs_sum_mask(x):
    _f(x)
    B, Cc, T = x.shape
    m = torch.empty(B, T, dtype=torch.float32, device=x.device)
    check(_lib.lib().set_abs_sum_mask(_p(x), _p(m), B, Cc, T, _stream()), "set_abs_sum_mask")
    return m


def index_mask(idx):
    _i(idx)
    m = torch.empty(idx.shape, dtype=torch.float32, device=idx.device)
    check(_lib.lib().set_index_mask(_p(idx), _p(m), idx.numel(), _stream()), "set_index_mask")
    return m


def expand_states(enc_bct, mel2ph):
    _f(enc_bct), _i(mel2ph)
    B, Cc, T_txt = enc_bct.shape
    T = mel2ph.shape[1]
    out = torch.empty(B, Cc, T, dtype=torch.float32, device=enc_bct.device)
    check(_lib.lib().set_expand_states(_p(enc_bct), _p(mel2ph), _p(out), B, Cc, T_txt, T, _stream()),
          "set_expand_states")
    return out


def add_chan_mask(x, add=None, mask=None, out=None):
    _f(x), _f(add), _f(mask)
    B, Cc, T = x.shape
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().set_add_chan_mask(_p(x), _p(add), _p(mask), _p(out), B, Cc, T, _stream()), "set_add_chan_mask")
    return out


def masked_dur(mel2ph, tmask_bt, txt_tokens):
    _i(mel2ph), _f(tmask_bt), _i(txt_tokens)
    B, T = mel2ph.shape
    T_txt = txt_tokens.shape[1]
    out = torch.empty(B, T_txt, dtype=torch.int64, device=mel2ph.device)
    check(_lib.lib().set_masked_dur(_p(mel2ph), _p(tmask_bt), _p(txt_tokens), _p(out), B, T, T_txt, _stream()),
          "set_masked_dur")
    return out


def pitch_coarse(f0, uv, tmask=None, mel2ph_pad=None, uv_from_logit=False, want_denorm=True, want_coarse=True):
    _f(f0), _f(uv), _f(tmask), _i(mel2ph_pad)
    n = f0.numel()
    den = torch.empty_like(f0) if want_denorm else None
    co = torch.empty(f0.shape, dtype=torch.int64, device=f0.device) if want_coarse else None
    check(_lib.lib().set_pitch_coarse(_p(f0), _p(uv), _p(tmask), _p(mel2ph_pad), int(bool(uv_from_logit)), _p(den),
                                      _p(co), n, _stream()), "set_pitch_coarse")
    return den, co


def btc_to_bct(x):
    _f(x)
    B, T, Cc = x.shape
    out = torch.empty(B, Cc, T, dtype=torch.float32, device=x.device)
    check(_lib.lib().set_transpose_btc_to_bct(_p(x), _p(out), B, T, Cc, _stream()), "set_transpose_btc_to_bct")
    return out


def bct_to_btc(x):
    _f(x)
    B, Cc, T = x.shape
    out = torch.empty(B, T, Cc, dtype=torch.float32, device=x.device)
    check(_lib.lib().set_transpose_bct_to_btc(_p(x), _p(out), B, Cc, T, _stream()), "set_transpose_bct_to_btc")
    return out


def sum_div(a, b=None, c=None, div=1.0, out=None):
    _f(a), _f(b), _f(c)
    out = torch.empty_like(a) if out is None else out
    check(_lib.lib().set_sum_scale(_p(a), _p(b), _p(c), _p(out), float(div), a.numel(), _stream()), "set_sum_scale")
    return out


def blend_mask(a, b, m, inner):
    """a*(1-m) + b*m with m broadcast over `inner` trailing elements."""
    _f(a), _f(b), _f(m)
    out = torch.empty_like(a)
    check(_lib.lib().set_blend_mask(_p(a), _p(b), _p(m), _p(out), a.numel(), int(inner), _stream()), "set_blend_mask")
    return out


def mul_one_minus_mask(x, m, inner):
    _f(x), _f(m)
    out = torch.empty_like(x)
    check(_lib.lib().set_mul_one_minus_mask(_p(x), _p(m), _p(out), x.numel(), int(inner), _stream()),
          "set_mul_one_minus_mask")
    return out


def length_regulate(dur, txt_tokens):
    """nar_tts_modules.py:42-72.  Host reads max total length (the reference sizes a tensor the same way)."""
    _f(dur), _i(txt_tokens)
    B, T_txt = dur.shape
    total = torch.empty(B, dtype=torch.int64, device=dur.device)
    check(_lib.lib().set_dur_total(_p(dur), _p(txt_tokens), _p(total), B, T_txt, _stream()), "set_dur_total")
    T_out = int(total.max().item())
    out = torch.empty(B, max(T_out, 0), dtype=torch.int64, device=dur.device)
    if T_out > 0:
        check(_lib.lib().set_length_regulate(_p(dur), _p(txt_tokens), _p(out), B, T_txt, T_out, _stream()),
              "set_length_regulate")
    return out


# --------------------------------------------------------------------------
# DiffNet pieces
# --------------------------------------------------------------------------
def sinusoid_embed(t_float, dim):
    """-> [dim][n]"""
    _f(t_float)
    n = t_float.numel()
    out = torch.empty(dim, n, dtype=torch.float32, device=t_float.device)
    check(_lib.lib().set_sinusoid_embed(_p(t_float), _p(out), dim, n, _stream()), "set_sinusoid_embed")
    return out


def gate(y):
    _f(y)
    B, C2, T = y.shape
    z = torch.empty(B, C2 // 2, T, dtype=torch.float32, device=y.device)
    check(_lib.lib().set_gate(_p(y), _p(z), B, C2 // 2, T, _stream()), "set_gate")
    return z


def res_skip(x_in, o, skip, first):
    _f(x_in), _f(o), _f(skip)
    B, Cc, T = x_in.shape
    x_out = torch.empty_like(x_in)
    check(_lib.lib().set_res_skip(_p(x_in), _p(o), _p(x_out), _p(skip), B, Cc, T, int(bool(first)), _stream()),
          "set_res_skip")
    return x_out


def pack_diffnet_layer(w_dil, w_out, w1p=None, w2p=None):
    """Pack one layer; optionally into caller-provided slices of the contiguous [L][...] buffers."""
    _f(w_dil), _f(w_out)
    L = _lib.lib()
    if w1p is None:
        w1p = torch.empty(L.set_diffnet_w1p_size(), dtype=torch.float32, device=w_dil.device)
        w2p = torch.empty(L.set_diffnet_w2p_size(), dtype=torch.float32, device=w_dil.device)
    check(L.set_pack_diffnet_layer(_p(w_dil), _p(w_out), _p(_f(w1p)), _p(_f(w2p)), _stream()), "set_pack_diffnet_layer")
    return w1p, w2p


def pack_diffnet_layer_wino(w_dil, w_out, w1w, w2w):
    """Winograd F(2,3) images of one layer into slices of the contiguous [L][...] buffers."""
    _f(w_dil), _f(w_out), _f(w1w), _f(w2w)
    check(_lib.lib().set_pack_diffnet_layer_wino(_p(w_dil), _p(w_out), _p(w1w), _p(w2w), _stream()),
          "set_pack_diffnet_layer_wino")


def sync_ws_size(B, T):
    # the words of one stack (csrc/stack_queue.h: 16 + 2 B ceil(T / 32)) and the fixed words of set_diffusion_loop's utterance groups (8 at the most)
    return 160 + 2 * B * ((T + 31) // 32)


class SplitRangeError(_lib.SetAmdError):
    """An activation left the range of the fp16 operand splitting (the loop's output is not valid)."""


_SPLIT_MODE_OVERRIDE = [None]


def split_operand_mode():
    """Which splitting the throughput stack kernel uses: 2 = two fp16 pieces (three MFMA products per term), 3 = three bf16
    pieces (six products, fp32 range).  SET_AMD_SPLIT_OPERAND=bf16x3 / f16x2 overrides the default."""
    if _SPLIT_MODE_OVERRIDE[0] is not None:
        return _SPLIT_MODE_OVERRIDE[0]
    v = os.environ.get("SET_AMD_SPLIT_OPERAND", "f16x2").lower()
    if v not in ("f16x2", "bf16x3"):
        raise ValueError("SET_AMD_SPLIT_OPERAND must be f16x2 or bf16x3, not %r" % v)
    return 2 if v == "f16x2" else 3


class split_operand_mode_as:
    """with split_operand_mode_as(3): ...  -- pin the splitting for a block (the fallback of the reverse loop)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev, _SPLIT_MODE_OVERRIDE[0] = _SPLIT_MODE_OVERRIDE[0], self.mode

    def __exit__(self, *exc):
        _SPLIT_MODE_OVERRIDE[0] = self.prev


def _images_mask(have_wino, have_split, x3_mode):
    """The `images` bit mask of set_diffnet_stack_variant / _x3_winograd: which weight images the caller holds."""
    m = split_operand_mode() if x3_mode is None else int(x3_mode)
    return int(bool(have_wino)) | (2 if have_split else 0) | (4 if m == 3 else 0) | (8 if m == 2 else 0)


def stack_variant(B, T, dilation_cycle_length, have_wino=True, have_split=True, x3_mode=None):
    """0 / 1: direct kernel (64- / 32-frame tiles), 2: Winograd kernel, 3: row-split kernel (small batches), 4 / 5: split-operand
    kernel (3 x bf16 / 2 x fp16) -- what set_diffnet_stack would pick.  x3_mode: 0 (no split-operand images), 2, 3, or None =
    split_operand_mode()."""
    return int(_lib.lib().set_diffnet_stack_variant(int(B), int(T), int(dilation_cycle_length), _images_mask(have_wino, have_split, x3_mode)))


def stack_x3_winograd(B, T, dilation_cycle_length, have_wino=True, have_split=True, x3_mode=None):
    """Non-zero when variant 5 (two-piece fp16 split-operand kernel) runs GEMM 1 in its Winograd F(2,3) form for this shape (round 6,
    diffnet_stack_x3v_kernel): the number of 32-frame column blocks per tile -- 3 = 96-frame tiles (shapes with a tile chain for every CU),
    2 = 64-frame tiles; 0 = the direct form."""
    return int(_lib.lib().set_diffnet_stack_x3_winograd(int(B), int(T), int(dilation_cycle_length), _images_mask(have_wino, have_split, x3_mode)))


STACK_VARIANT_NAMES = {0: "diffnet_stack_kernel<2,4,2>", 1: "diffnet_stack_kernel<1,8,2>", 2: "diffnet_stack_wino_kernel",
                       3: "diffnet_stack_split_kernel", 4: "diffnet_stack_x3_kernel<SplitBf16x3>",
                       5: "diffnet_stack_x3_kernel<SplitF16x2>"}


class SplitOperandImages:
    """[L][n] 16-bit images of the split-operand stack kernel + the mode they were packed for."""

    def __init__(self, L, mode, device):
        self.mode = int(mode)
        n = int(_lib.lib().set_diffnet_layer_x3_image_size(self.mode))
        self.data = torch.empty(L, n, dtype=torch.int16, device=device)

    def pack(self, i, w_dil, w_out):
        """Layer i.  fp16 pieces: scale the weights by a power of two so that max |w| lands in [8, 16) (exact; undone on
        the accumulators by the kernel) -- one host read-back per layer and weight version."""
        _f(w_dil), _f(w_out)
        k1 = k2 = 0
        if self.mode == 2:
            import math
            m1, m2 = float(w_dil.abs().max()), float(w_out.abs().max())
            k1 = max(-60, min(60, 3 - math.frexp(m1)[1] + 1)) if m1 > 0 and math.isfinite(m1) else 0
            k2 = max(-60, min(60, 3 - math.frexp(m2)[1] + 1)) if m2 > 0 and math.isfinite(m2) else 0
        check(_lib.lib().set_pack_diffnet_layer_x3(_p(w_dil), _p(w_out), self.data[i].data_ptr(), self.mode, k1, k2, _stream()),
              "set_pack_diffnet_layer_x3")


def split_images(w1p_all, w2p_all):
    """Row-split images of the small-batch stack kernel from the packed layer images: the same values, one 32-row
    block per wave ([L][w][k-step][lane][rb] -> [L][4w + rb][k-step][lane])."""
    L = w1p_all.shape[0]
    return tuple(w.view(L, 4, -1, 64, 4).permute(0, 1, 4, 2, 3).contiguous().view(L, -1) for w in (w1p_all, w2p_all))


class StackImages(typing.NamedTuple):
    """The weight images of the DiffNet layer stack, each a contiguous [L][...] buffer (DiffNet.fused_packs() builds them; tests and probes
    build their own).  Which kernel reads which field (None = no such image: set_diffnet_stack picks among the kernels it has images for):
    w1p, w2p      packed fp32 images of the dilated conv / output projection (set_pack_diffnet_layer): the direct stack kernel (variants
                  0 / 1) and the per-layer kernels of the non-persistent reverse loop
    b_dil, b_out  [L, 512] biases: every kernel; b_dil.shape[0] is the number of layers of the launch
    w1w, w2w      Winograd F(2,3) images (set_pack_diffnet_layer_wino): the Winograd kernel (variant 2), also the training forward
    w1s, w2s      row-split images (split_images(w1p, w2p)): the small-batch row-split kernel (variant 3)
    wx3           SplitOperandImages: the split-operand kernel (variants 4 / 5, by wx3.mode)"""
    w1p: torch.Tensor
    w2p: torch.Tensor
    b_dil: torch.Tensor
    b_out: torch.Tensor
    w1w: typing.Optional[torch.Tensor] = None
    w2w: typing.Optional[torch.Tensor] = None
    w1s: typing.Optional[torch.Tensor] = None
    w2s: typing.Optional[torch.Tensor] = None
    wx3: typing.Optional[SplitOperandImages] = None


def _set_images(a, images, B, T, dcl, dev):
    """The image fields of a SetDiffnetStackArgs / SetDiffLoopArgs from a StackImages.  The row-split images and their z workspace go in
    only for shapes the row-split kernel (variant 3) is picked for; returns that workspace or None (the caller keeps it alive until the
    launch is enqueued; stream-ordered reuse is safe)."""
    if not isinstance(images, StackImages):
        raise TypeError("the layer stack takes its weight images as an ops.StackImages (fields by name), not %s: a bare tuple in the "
                        "wrong order would launch on the wrong image" % type(images).__name__)
    a.w1p_all, a.w2p_all = images.w1p.data_ptr(), images.w2p.data_ptr()
    a.b_dil_all, a.b_out_all = images.b_dil.data_ptr(), images.b_out.data_ptr()
    if images.w1w is not None:
        a.w1w_all, a.w2w_all = images.w1w.data_ptr(), images.w2w.data_ptr()
    x3 = images.wx3
    if x3 is not None:
        a.wx3_all, a.x3_mode = x3.data.data_ptr(), x3.mode
    if images.w1s is None or stack_variant(B, T, dcl, x3_mode=x3.mode if x3 is not None else 0) != 3:
        return None
    a.w1s_all, a.w2s_all = images.w1s.data_ptr(), images.w2s.data_ptr()
    z_ws = torch.empty(B * ((T + 31) // 32) * 256 * 32, dtype=torch.float32, device=dev)
    a.z_ws = z_ws.data_ptr()
    return z_ws


def diffnet_stack(xa, xb, skip, condproj, dstep_ptr, d_bs, d_cs, d_ls, images, dilation_cycle_length, sync_ws=None,
                  x_all=None, save_y=None, save_z=None, err_flag=None):
    """All L layers in one persistent launch.  condproj [B, L*512, T]; images: a StackImages (a bare tuple is a TypeError).
    Training forward (Winograd kernel only): x_all [L+1,B,256,T] (slab 0 = input) replaces the xa/xb ping-pong, save_y [L,B,512,T] /
    save_z [L,B,256,T] receive what the backward pass needs.
    Returns sync_ws (int32; [1] != 0 means a dependency wait timed out)."""
    B, Cc, T = xa.shape
    assert Cc == 256
    a = SetDiffnetStackArgs()  # (the images first: a bare tuple is refused before anything else is looked at)
    z_ws = _set_images(a, images, B, T, dilation_cycle_length, xa.device)  # noqa: F841 (kept alive until the launch is enqueued)
    _f(xa), _f(xb), _f(skip), _f(condproj)
    L = images.b_dil.shape[0]
    if sync_ws is None:
        sync_ws = torch.empty(sync_ws_size(B, T), dtype=torch.int32, device=xa.device)
    a.xa, a.xb, a.skip = xa.data_ptr(), xb.data_ptr(), skip.data_ptr()
    a.condproj, a.dstep = condproj.data_ptr(), dstep_ptr
    if x_all is not None:
        a.x_all, a.save_y, a.save_z = _f(x_all).data_ptr(), _f(save_y).data_ptr(), _f(save_z).data_ptr()
    if err_flag is not None:  # optional sticky int32 error word (1: a dependency wait timed out, 2: out of the fp16 split range)
        a.err_flag = err_flag.data_ptr()
    a.sync_ws = sync_ws.data_ptr()
    a.cp_bs, a.cp_ls = condproj.stride(0), 512 * T
    a.d_bs, a.d_cs, a.d_ls = int(d_bs), int(d_cs), int(d_ls)
    a.B, a.T, a.L, a.dilation_cycle_length = B, T, L, int(dilation_cycle_length)
    check(_lib.lib().set_diffnet_stack(C.byref(a), _stream()), "set_diffnet_stack")
    return sync_ws


def diffnet_layer(x_in, condproj, cp_bs, dstep, d_bs, d_cs, w1p, b_dil, w2p, b_out, x_out, skip, dil, first,
                  dbg_clock=None):
    _f(x_in), _f(x_out), _f(skip)
    B, Cc, T = x_in.shape
    assert Cc == 256
    a = SetDiffnetLayerArgs()
    a.x_in, a.condproj, a.dstep = x_in.data_ptr(), condproj, dstep
    a.w1p, a.b_dil, a.w2p, a.b_out = w1p.data_ptr(), b_dil.data_ptr(), w2p.data_ptr(), b_out.data_ptr()
    a.x_out, a.skip = x_out.data_ptr(), skip.data_ptr()
    a.cp_bs, a.d_bs, a.d_cs = int(cp_bs), int(d_bs), int(d_cs)
    a.B, a.T, a.dil, a.first = B, T, int(dil), int(bool(first))
    a.dbg_clock = dbg_clock.data_ptr() if dbg_clock is not None else None
    check(_lib.lib().set_diffnet_layer(C.byref(a), _stream()), "set_diffnet_layer")


def posterior_step(x0, x_t, coef4, eps=None, out=None, seed=0, offset=0):
    """coef4 [B,4] (or [1,4] shared by the batch)."""
    _f(x0), _f(x_t), _f(coef4), _f(eps)
    B = x0.shape[0]
    per_batch = x0.numel() // B
    out = x_t if out is None else out
    assert coef4.shape[0] in (1, B) and coef4.shape[-1] == 4
    coef_bs = 0 if coef4.shape[0] == 1 else 4
    check(_lib.lib().set_posterior_step(_p(x0), _p(x_t), _p(eps), _p(coef4), coef_bs, _p(out), B, per_batch, int(seed),
                                        int(offset), _stream()), "set_posterior_step")
    return out


def q_sample(x_start, eps, ab2, nonpad=None):
    _f(x_start), _f(eps), _f(ab2), _f(nonpad)
    B, M, T = x_start.shape[0], x_start.shape[-2], x_start.shape[-1]
    out = torch.empty_like(x_start)
    check(_lib.lib().set_q_sample(_p(x_start), _p(eps), _p(ab2), _p(nonpad), _p(out), B, M, T, _stream()),
          "set_q_sample")
    return out


def randn(shape, device, seed=0, offset=0):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(_lib.lib().set_randn(_p(out), out.numel(), int(seed), int(offset), _stream()), "set_randn")
    return out


def fanout(x, n):
    """Inference backend: n references to the same tensor."""
    return (x,) * n


def grad_scale(x, s):
    """Inference backend: identity (fs.py:144-145 only rescales gradients)."""
    return x


def dropout(x, p, seed, offset=0):
    """Inference backend: identity (eval mode)."""
    return x


def res_skip_fn(x, o, skip_in):
    """Functional form used by the shared layer code: returns (x_out, skip_out); skip_in None on the first layer."""
    first = skip_in is None
    skip = torch.empty_like(x) if first else skip_in
    return res_skip(x, o, skip, first), skip


def selftest_mfma():
    err = C.c_float(-1.0)
    check(_lib.lib().set_selftest_mfma(C.byref(err), _stream()), "set_selftest_mfma")
    return float(err.value)


def diffusion_loop(*, x, noise, seed, condproj, dstep, coef4, w_in, b_in, packs, w_skip, b_skip,
                   w_outp, b_outp, L, steps, dilation_cycle_length, want_layer_spans=False, n_groups=None,
                   persistent=None, bf16=None):
    """Enqueue the whole reverse loop (set_diffusion_loop).  x [B,M,T] is updated in place.
    packs: the layer stack's StackImages (DiffNet.fused_packs()).
    bf16 = dict(cond=[B,192,T] fp32, imgs=[L, n] bf16 layer images, b_cond=[L,512]): the opt-in bf16-operand loop
    (condproj is then unused and may be None)."""
    _f(x), _f(noise), _f(condproj), _f(dstep), _f(coef4)
    B, M, T = x.shape
    dev = x.device
    ws = [torch.empty(B, 256, T, dtype=torch.float32, device=dev) for _ in range(4)]
    ws_x0pred = torch.empty(B, M, T, dtype=torch.float32, device=dev)
    a = SetDiffLoopArgs()
    a.B, a.T, a.M, a.L, a.steps, a.dilation_cycle_length = B, T, M, L, steps, dilation_cycle_length
    a.x = x.data_ptr()
    a.noise = noise.data_ptr() if noise is not None else None
    a.seed = int(seed)
    a.condproj = condproj.data_ptr() if condproj is not None else None
    a.dstep, a.coef4 = dstep.data_ptr(), coef4.data_ptr()
    if bf16 is not None:
        a.cond, a.img16_all, a.b_cond_all = _f(bf16["cond"]).data_ptr(), bf16["imgs"].data_ptr(), _f(bf16["b_cond"]).data_ptr()
        # workspace of the several-layers-per-launch kernels (128-frame tiles: a block's private copy of its skip rows between the layers
        # of a group), sized for whatever group size the loop picks
        n_ws = max(_lib.lib().set_diffnet_layers_bf16_scratch_floats(B, T, 0, n, dilation_cycle_length) for n in range(2, 17)) \
            if dilation_cycle_length <= 2 else 0
        if n_ws > 0:
            bf16_ws = torch.empty(n_ws, dtype=torch.float32, device=dev)  # noqa: F841 (kept alive until the loop is enqueued: stream-ordered free)
            a.bf16_ws, a.bf16_ws_floats = bf16_ws.data_ptr(), n_ws
    a.w_in_p, a.b_in = w_in.packed().data_ptr(), b_in.data_ptr()
    z_ws = _set_images(a, packs, B, T, dilation_cycle_length, dev)  # noqa: F841 (kept alive until the loop is enqueued)
    a.persistent = int(default_persistent() if persistent is None else bool(persistent))
    sync_ws = torch.empty(sync_ws_size(B, T), dtype=torch.int32, device=dev)
    a.sync_ws = sync_ws.data_ptr()
    err = torch.zeros(1, dtype=torch.int32, device=dev)  # sticky: a dependency wait of the persistent kernel gave up
    a.err_flag = err.data_ptr()
    bf16_bx2 = bf16 is not None and split_operand_mode() == 2  # the opt-in bf16 loop: its layers are bf16, its step boundary fp32-equivalent
    use_bx2 = ((a.wx3_all and a.x3_mode == 2) or bf16_bx2) and M <= 96 and os.environ.get("SET_AMD_BOUNDARY_X2", "1") != "0"
    if use_bx2:
        # the fused step boundary on the same two-piece fp16 operands
        a.w_skip_x2, a.w_outp_x2, a.w_in_x2 = (w.packed_x2().data_ptr() for w in (w_skip, w_outp, w_in))
    a.w_skip_p, a.b_skip = w_skip.packed().data_ptr(), b_skip.data_ptr()
    a.w_outp_p, a.b_outp = w_outp.packed().data_ptr(), b_outp.data_ptr()
    a.ws_x0, a.ws_x1, a.ws_skip, a.ws_h = (w.data_ptr() for w in ws)
    a.ws_x0pred = ws_x0pred.data_ptr()
    a.ws_q4 = 1  # the workspaces are ours: the library may keep them in the channel-quad layout (SetDiffLoopArgs.ws_q4)
    a.n_groups = default_groups(B, T) if n_groups is None else int(n_groups)
    spans, loop_ms = None, None
    if want_layer_spans:
        spans = (C.c_float * steps)()
        a.layer_span_ms = C.cast(spans, C.POINTER(C.c_float))
        loop_ms = C.c_float(0.0)
        a.loop_ms = C.pointer(loop_ms)
    check(_lib.lib().set_diffusion_loop(C.byref(a), _stream()), "set_diffusion_loop")
    # one 4-byte read-back per reverse loop; fail loudly, never return garbage.  The range word can be raised by the persistent stack kernel
    # AND by the split-operand step boundary, which the bf16 loop takes whether or not `persistent` is set
    if a.persistent or use_bx2:
        code = int(err.item())
        if code == 2:
            raise SplitRangeError("set_diffusion_loop: an activation of magnitude >= 32768 is outside the range of the fp16 "
                                  "operand splitting; set SET_AMD_SPLIT_OPERAND=bf16x3 (fp32 range) or SET_AMD_X3=0")
        if code != 0:
            raise _lib.SetAmdError("set_diffusion_loop: a tile dependency wait of the persistent layer-stack kernel timed out")
    # the group chains are joined back into the current stream, so stream-ordered reuse of these buffers is safe
    if spans is None:
        return None
    return {"layer_span_ms": list(spans), "loop_ms": float(loop_ms.value), "n_groups": int(a.n_groups),
            "persistent": int(a.persistent)}


def default_persistent():
    """SET_AMD_PERSISTENT=0/1 overrides; default: persistent layer-stack kernel."""
    return os.environ.get("SET_AMD_PERSISTENT", "1") != "0"


def default_groups(B, T):
    """Utterance groups for the reverse loop (callers may pass groups= themselves).  Measured on MI355X (profiles/): more than
    one group is slower -- kernels from different streams are placed on the same CUs first, so the per-CU imbalance
    of a 416-block launch gets worse, not better -- hence 1.  Grouping never changes results."""
    return 1


# --------------------------------------------------------------------------
# attention building blocks (CampNet rows)
# --------------------------------------------------------------------------
class MatView:
    """A batch of matrices inside a tensor: element (bo, bi, r, c) at  offset + bo*bo_s + bi*bi_s + r*rs + c*cs
    (in floats).  `.t` swaps rows and columns.  Heads of a [B, heads*d, T] activation: MatView.heads(x, heads)."""

    def __init__(self, tensor, n_outer, n_inner, rows, cols, bo_s, bi_s, rs, cs, offset=0):
        self.tensor = _f(tensor)
        self.n_outer, self.n_inner, self.rows, self.cols = int(n_outer), int(n_inner), int(rows), int(cols)
        self.bo_s, self.bi_s, self.rs, self.cs, self.offset = int(bo_s), int(bi_s), int(rs), int(cs), int(offset)

    @property
    def t(self):
        return MatView(self.tensor, self.n_outer, self.n_inner, self.cols, self.rows, self.bo_s, self.bi_s, self.cs,
                       self.rs, self.offset)

    @staticmethod
    def heads(x, heads, chan0=0, width=None):
        """Channels [chan0, chan0+width) of x [B, C, T] (contiguous) split into heads -> per (b, h) the matrix
        [T, d]: rows = frames, cols = head channels.  (q / k / v are channel slices of one packed projection.)"""
        B, Ctot, T = x.shape
        H = Ctot - chan0 if width is None else width
        d = H // heads
        assert x.is_contiguous() and d * heads == H and chan0 + H <= Ctot
        return MatView(x, B, heads, T, d, Ctot * T, d * T, 1, T, offset=chan0 * T)

    @staticmethod
    def scores(s):
        """s [B, heads, Tq, Tk] (contiguous) -> per (b, h) the matrix [Tq, Tk]."""
        B, h, Tq, Tk = s.shape
        assert s.is_contiguous()
        return MatView(s, B, h, Tq, Tk, h * Tq * Tk, Tq * Tk, Tk, 1)

    def ptr(self):
        return self.tensor.data_ptr() + 4 * self.offset


def bmm(a, b, c, alpha=1.0, accumulate=False):
    """c = alpha * a @ b (+ c) on MatViews.  When c is column-major the transposed problem is run so that the
    stores stay coalesced (c^T = b^T a^T)."""
    assert a.cols == b.rows and a.rows == c.rows and b.cols == c.cols
    assert (a.n_outer, a.n_inner) == (b.n_outer, b.n_inner) == (c.n_outer, c.n_inner)
    if c.rs == 1 and c.cs != 1:
        a, b, c = b.t, a.t, c.t
    g = _lib.SetBmmArgs()
    g.A, g.B, g.C = a.ptr(), b.ptr(), c.ptr()
    g.a_bo, g.a_bi, g.a_ms, g.a_ks = a.bo_s, a.bi_s, a.rs, a.cs
    g.b_bo, g.b_bi, g.b_ks, g.b_ns = b.bo_s, b.bi_s, b.rs, b.cs
    g.c_bo, g.c_bi, g.c_ms, g.c_ns = c.bo_s, c.bi_s, c.rs, c.cs
    g.n_outer, g.n_inner, g.M, g.N, g.K = c.n_outer, c.n_inner, c.rows, c.cols, a.cols
    g.alpha, g.accumulate = float(alpha), int(bool(accumulate))
    check(_lib.lib().set_bmm(C.byref(g), _stream()), "set_bmm")
    return c.tensor


def softmax_rows(x, key_padding_mask=None, rows_per_batch=1, fill=float("-inf"), out=None):
    """softmax over the last dim of a contiguous tensor; kpm [B, cols] fp32 (1 = pad), B = rows / rows_per_batch."""
    _f(x), _f(key_padding_mask)
    cols = x.shape[-1]
    rows = x.numel() // cols
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().set_softmax_rows(_p(x), _p(key_padding_mask), _p(out), rows, cols, int(rows_per_batch), float(fill),
                                      _stream()), "set_softmax_rows")
    return out


def softmax_rows_bwd(p, dp):
    _f(p), _f(dp)
    cols = p.shape[-1]
    ds = torch.empty_like(p)
    check(_lib.lib().set_softmax_rows_bwd(_p(p), _p(dp), _p(ds), p.numel() // cols, cols, _stream()), "set_softmax_rows_bwd")
    return ds


def make_positions(tokens=None, x_bct=None):
    """int64 [B,T]: 1,2,3.. over the non-zero tokens (or the non-zero entries of channel 0 of x_bct), 0 elsewhere."""
    if tokens is not None:
        _i(tokens)
        B, T = tokens.shape
        pos = torch.empty(B, T, dtype=torch.int64, device=tokens.device)
        check(_lib.lib().set_make_positions(_p(tokens), None, 0, _p(pos), B, T, _stream()), "set_make_positions")
    else:
        _f(x_bct)
        B, Cc, T = x_bct.shape
        pos = torch.empty(B, T, dtype=torch.int64, device=x_bct.device)
        check(_lib.lib().set_make_positions(None, _p(x_bct), Cc * T, _p(pos), B, T, _stream()), "set_make_positions")
    return pos


def head_mean(p):
    """p [B, heads, ...] -> mean over heads [B, ...]."""
    _f(p)
    B, h = p.shape[:2]
    out = torch.empty((B,) + tuple(p.shape[2:]), dtype=torch.float32, device=p.device)
    check(_lib.lib().set_head_mean(_p(p), _p(out), B, h, out.numel() // B, _stream()), "set_head_mean")
    return out


def mask_fill_chan(x, e, m):
    """x [B,C,T]*(1-m[B,T]) + e[C]*m"""
    _f(x), _f(e), _f(m)
    B, Cc, T = x.shape
    out = torch.empty_like(x)
    check(_lib.lib().set_mask_fill_chan(_p(x), _p(e), _p(m), _p(out), B, Cc, T, _stream()), "set_mask_fill_chan")
    return out


def masked_channel_sum(d, m, out):
    _f(d), _f(m), _f(out)
    B, Cc, T = d.shape
    check(_lib.lib().set_masked_channel_sum(_p(d), _p(m), _p(out), B, Cc, T, _stream()), "set_masked_channel_sum")
    return out


def attention_fused_on(head_dim=None):
    """The fused attention kernels (csrc/attention_fused.hip) are the default for the head sizes they are instantiated for (32, 64,
    96: the shipped 192 / 2 config and its neighbours); any other head size, or SET_AMD_ATTN_FUSED=0, runs the three-launch
    bmm -> softmax -> bmm composition (any head size; also the cross-check of the tests)."""
    if head_dim is not None and int(head_dim) not in (32, 64, 96):
        return False
    return os.environ.get("SET_AMD_ATTN_FUSED", "1") != "0"


def _attn_args(qv, kv, vv, o, lse, heads, key_padding_mask, fill, alpha, p=None):
    d = qv.cols
    assert qv.rs == 1 and kv.rs == 1 and vv.rs == 1 and kv.cols == d and vv.cols == d and kv.rows == vv.rows
    assert qv.bi_s == d * qv.cs and kv.bi_s == d * kv.cs and vv.bi_s == d * vv.cs  # heads = consecutive channel slices
    a = _lib.SetAttnArgs()
    a.q, a.k, a.v = qv.ptr(), kv.ptr(), vv.ptr()
    a.o, a.lse = o.data_ptr(), lse.data_ptr()
    a.p = p.data_ptr() if p is not None else None
    a.kpm = _f(key_padding_mask, "key_padding_mask").data_ptr() if key_padding_mask is not None else None
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = qv.bo_s, kv.bo_s, vv.bo_s, o.stride(0)
    a.q_cs, a.k_cs, a.v_cs, a.o_cs = qv.cs, kv.cs, vv.cs, o.stride(1)
    a.B, a.heads, a.head_dim, a.Tq, a.Tk = qv.n_outer, heads, d, qv.rows, kv.rows
    a.scale, a.fill = float(alpha), float(fill)
    a.bf16 = int(_COMPUTE_DTYPE == "bf16")
    return a


def attention_fused(qv, kv, vv, heads, key_padding_mask=None, fill=float("-inf"), alpha=1.0, want_p=False):
    """o = softmax(alpha q k^T (+ mask)) v per head in ONE launch (scores never in HBM): returns (o [B,H,Tq], lse
    [B,heads,2,Tq] = row max and sum of the softmax, p [B,heads,Tq,Tk] or None).  q / k / v: MatView.heads views."""
    B, Tq, Tk, d = qv.n_outer, qv.rows, kv.rows, qv.cols
    dev = qv.tensor.device
    o = torch.empty(B, heads * d, Tq, dtype=torch.float32, device=dev)
    lse = torch.empty(B, heads, 2, Tq, dtype=torch.float32, device=dev)  # row max m, sum l (log-sum-exp = m + log l)
    p = torch.empty(B, heads, Tq, Tk, dtype=torch.float32, device=dev) if want_p else None
    a = _attn_args(qv, kv, vv, o, lse, heads, key_padding_mask, fill, alpha, p)
    check(_lib.lib().set_attention(C.byref(a), _stream()), "set_attention")
    return o, lse, p


def attention_fused_bwd(qv, kv, vv, o, lse, do, dqv, dkv, dvv, heads, key_padding_mask=None, fill=float("-inf"), alpha=1.0):
    """Gradients of attention_fused into the views dqv / dkv / dvv (two launches, P recomputed from lse)."""
    g = _lib.SetAttnBwdArgs()
    g.fwd = _attn_args(qv, kv, vv, o, lse, heads, key_padding_mask, fill, alpha)
    _f(do, "do")
    assert do.shape == o.shape and do.stride() == o.stride()
    delta = torch.empty(lse.shape[0], lse.shape[1], lse.shape[3], dtype=torch.float32, device=lse.device)
    g.d_o, g.delta = do.data_ptr(), delta.data_ptr()
    g.dq, g.dk, g.dv = dqv.ptr(), dkv.ptr(), dvv.ptr()
    g.dq_bs, g.dk_bs, g.dv_bs = dqv.bo_s, dkv.bo_s, dvv.bo_s
    g.dq_cs, g.dk_cs, g.dv_cs = dqv.cs, dkv.cs, dvv.cs
    check(_lib.lib().set_attention_bwd(C.byref(g), _stream()), "set_attention_bwd")


def attention_views(qv, kv, vv, heads, key_padding_mask=None, fill=float("-inf"), alpha=1.0):
    """o = softmax(alpha * q k^T (+mask)) v per head; q/k/v given as MatView.heads views.  Returns (o [B,H,Tq]
    contiguous, p [B,heads,Tq,Tk])."""
    B, Tq, Tk, d = qv.n_outer, qv.rows, kv.rows, qv.cols
    dev = qv.tensor.device
    s = torch.empty(B, heads, Tq, Tk, dtype=torch.float32, device=dev)
    bmm(qv, kv.t, MatView.scores(s), alpha=alpha)
    p = softmax_rows(s, key_padding_mask, heads * Tq, fill, out=s)
    o = torch.empty(B, heads * d, Tq, dtype=torch.float32, device=dev)
    bmm(MatView.scores(p), vv, MatView.heads(o, heads))
    return o, p


def self_attention(qkv, heads, key_padding_mask=None, fill=float("-inf"), alpha=1.0, want_p=False):
    """qkv [B, 3H, T] = packed in_proj output (transformer.py:421-422) -> (o [B,H,T], p or None)."""
    H = qkv.shape[1] // 3
    views = (MatView.heads(qkv, heads, 0, H), MatView.heads(qkv, heads, H, H), MatView.heads(qkv, heads, 2 * H, H))
    if attention_fused_on(H // heads):
        o, _, p = attention_fused(*views, heads, key_padding_mask, fill, alpha, want_p)
        return o, p
    return attention_views(*views, heads, key_padding_mask, fill, alpha)


def cross_attention(q, kv, heads, key_padding_mask=None, fill=-1e8, alpha=1.0, want_p=True):
    """q [B,H,Tq], kv [B,2H,Tk] (in_proj_k / in_proj_v of the encoder output, transformer.py:433-451)."""
    H = q.shape[1]
    views = (MatView.heads(q, heads), MatView.heads(kv, heads, 0, H), MatView.heads(kv, heads, H, H))
    if attention_fused_on(H // heads):
        o, _, p = attention_fused(*views, heads, key_padding_mask, fill, alpha, want_p)
        return o, p
    return attention_views(*views, heads, key_padding_mask, fill, alpha)


def pos_add(x, alpha, pos, table):
    """x + alpha * table[pos]  (transformer.py:795-796)"""
    return embedding_bct(pos, table, scale=alpha.detach().reshape(1).contiguous(), out=x.clone(), accumulate=True)


def add_masked(a, b, m):
    """a + b * m[b][t] on [B,C,T]"""
    return sum_div(a.contiguous(), add_chan_mask(b, None, m))


# --------------------------------------------------------------------------
# multi-period discriminator (csrc/sconv.hip): strided convs on [R][C][H] rows, the folded first layer, the list losses
# --------------------------------------------------------------------------
def sconv_out_len(H_in, K, stride, pad):
    """H_out = (H_in + 2 pad - K) // stride + 1 (set_sconv1d_out_len; raises outside 1 <= K <= 7, 1 <= stride <= 4, 0 <= pad < K)."""
    n = _lib.lib().set_sconv1d_out_len(int(H_in), int(K), int(stride), int(pad))
    if n < 0:
        check(n, "set_sconv1d_out_len")
    return n


def _rows3(t, name):
    _f(t, name)
    if t.dim() != 3:
        raise ValueError("%s must be a contiguous [R, C, H] tensor, got %s" % (name, tuple(t.shape)))
    return t


def sconv1d_fwd(x, weight, bias=None, *, stride, pad, slope=None, sentinel=None):
    """set_sconv1d_fwd: x [R,Cin,H_in] -> act(conv(x) + bias) [R,Cout,H_out]; `slope` None: no activation, else leaky ReLU."""
    _rows3(x, "x"), _f(bias, "bias")
    R, Cin, H_in = x.shape
    if Cin != weight.Cin:
        raise ValueError("sconv1d_fwd: x has %d channels, the weight takes %d" % (Cin, weight.Cin))
    H_out = sconv_out_len(H_in, weight.K, stride, pad)
    out = _buf((R, weight.Cout, H_out), x.device, sentinel)
    check(_lib.lib().set_sconv1d_fwd(_p(x), _p(weight.packed()), _p(bias), _p(out), R, Cin, weight.Cout, H_in, weight.K, int(stride), int(pad),
                                     int(slope is not None), float(slope or 0.0), _stream()), "set_sconv1d_fwd")
    return out


def sconv1d_dgrad(dz_out, weight, H_in, *, stride, pad, f_in=None, add=None, slope=0.0, sentinel=None):
    """set_sconv1d_dgrad: dz_out [R,Cout,H_out] -> gate(f_in) * (add + conv^T(dz_out)) [R,Cin,H_in]; `weight` is the FORWARD layer's
    ConvWeight (its transposed image is packed here); f_in / add: [R,Cin,H_in] or None."""
    _rows3(dz_out, "dz_out")
    R, Cout, H_out = dz_out.shape
    if Cout != weight.Cout or H_out != sconv_out_len(H_in, weight.K, stride, pad):
        raise ValueError("sconv1d_dgrad: dz_out %s does not belong to a (%d -> %d, K = %d, stride %d, pad %d) layer on %d frames"
                         % (tuple(dz_out.shape), weight.Cin, weight.Cout, weight.K, stride, pad, H_in))
    for t, name in ((f_in, "f_in"), (add, "add")):
        if t is not None and tuple(_rows3(t, name).shape) != (R, weight.Cin, H_in):
            raise ValueError("sconv1d_dgrad: %s must be [%d, %d, %d], got %s" % (name, R, weight.Cin, H_in, tuple(t.shape)))
    dz_in = _buf((R, weight.Cin, H_in), dz_out.device, sentinel)
    check(_lib.lib().set_sconv1d_dgrad(_p(dz_out), _p(weight.transposed().packed()), _p(f_in), _p(add), _p(dz_in), R, weight.Cin, Cout, int(H_in),
                                       weight.K, int(stride), int(pad), float(slope), _stream()), "set_sconv1d_dgrad")
    return dz_in


def mpd_fold_conv_fwd(y, y_hat, w, bias, period, *, stride, pad, slope=None, sentinel=None):
    """set_mpd_fold_conv_fwd: y, y_hat [B,T] -> the first layer's map [2 B p, C, H_out] (real rows first); w: the raw weight [C, K]
    (any contiguous shape of C K elements with C first)."""
    _f(y, "y"), _f(y_hat, "y_hat"), _f(w, "w"), _f(bias, "bias")
    if y.dim() != 2 or y.shape != y_hat.shape:
        raise ValueError("mpd_fold_conv_fwd: y and y_hat must be equal [B, T], got %s and %s" % (tuple(y.shape), tuple(y_hat.shape)))
    B, T = y.shape
    Cc = w.shape[0]
    K = w.numel() // Cc
    if T <= period:
        raise ValueError("mpd_fold_conv_fwd: the reflect pad of period %d needs more than %d samples, got %d" % (period, period, T))
    H_out = sconv_out_len((T + period - 1) // period, K, stride, pad)
    out = _buf((2 * B * period, Cc, H_out), y.device, sentinel)
    check(_lib.lib().set_mpd_fold_conv_fwd(_p(y), _p(y_hat), _p(w), _p(bias), _p(out), B, T, int(period), Cc, K, int(stride), int(pad),
                                           int(slope is not None), float(slope or 0.0), _stream()), "set_mpd_fold_conv_fwd")
    return out


def mpd_fold_conv_bwd(dz, w, B, T, period, *, stride, pad, sentinel=None):
    """set_mpd_fold_conv_bwd: dz [B p, C, H_out] (generated rows) -> d/d y_hat [B, T]."""
    _rows3(dz, "dz"), _f(w, "w")
    Cc = w.shape[0]
    K = w.numel() // Cc
    H_out = sconv_out_len((T + period - 1) // period, K, stride, pad)
    if tuple(dz.shape) != (B * period, Cc, H_out):
        raise ValueError("mpd_fold_conv_bwd: dz must be [%d, %d, %d], got %s" % (B * period, Cc, H_out, tuple(dz.shape)))
    g_wav = _buf((B, T), dz.device, sentinel)
    check(_lib.lib().set_mpd_fold_conv_bwd(_p(dz), _p(w), _p(g_wav), B, T, int(period), Cc, K, int(stride), int(pad), _stream()),
          "set_mpd_fold_conv_bwd")
    return g_wav


LOSS_MODES = dict(l1=0, sq1=1, sq0=2)
MULTI_LOSS_WORDS, MULTI_LOSS_CHUNK = 18, 2048


def _loss_dims(a, b):
    """(extents, a strides, b strides) of an item, four each: size-1 dims dropped, the rest ordered by a's stride (largest first, the
    tensor's own order among equals) and merged wherever both operands allow -- a dense tensor and a target of the same layout become one
    run in memory order.  More than four dims left, or an `a` that overlaps itself, is refused."""
    dims = [(n, sa, (b.stride(i) if b is not None else 0)) for i, (n, sa) in enumerate(zip(a.shape, a.stride())) if n != 1]
    if any(sa == 0 for _n, sa, _sb in dims):
        raise ValueError("a loss operand must not overlap itself (an expanded dim): the gradient has its layout")
    dims.sort(key=lambda d: -d[1])
    merged = []
    for n, sa, sb in dims:
        if merged and merged[-1][1] == n * sa and merged[-1][2] == n * sb:
            m = merged[-1]
            merged[-1] = (m[0] * n, sa, sb)
        else:
            merged.append((n, sa, sb))
    if len(merged) > 4:
        raise ValueError("a loss operand pair of shape %s needs more than four strided dims" % (tuple(a.shape),))
    merged = [(1, 0, 0)] * (4 - len(merged)) + merged
    return [m[0] for m in merged], [m[1] for m in merged], [m[2] for m in merged]


def multi_loss_items(a_list, b_list, modes, slots, grads=None):
    """The device table of set_multi_loss_fwd / _bwd for the operand pairs (b None for the squared forms) -> (table [n, 18] int64 on the
    device, total_chunks).  `grads`: per item the gradient buffer (a's strides) or None."""
    import numpy as np
    rows, chunk0 = [], 0
    for i, (a, b, mode, slot) in enumerate(zip(a_list, b_list, modes, slots)):
        _chk_loss_operand(a, "a")
        if mode == LOSS_MODES["l1"]:
            _chk_loss_operand(b, "b")
            if b.shape != a.shape or b.device != a.device:
                raise ValueError("loss operands must have equal shapes on one device, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
        else:
            b = None
        if a.numel() == 0:
            raise ValueError("a loss operand has no elements")
        e, sa, sb = _loss_dims(a, b)
        g = grads[i] if grads is not None else None
        rows.append([a.data_ptr(), b.data_ptr() if b is not None else 0, g.data_ptr() if g is not None else 0, mode] + e + sa + sb + [chunk0, slot])
        chunk0 += (a.numel() + MULTI_LOSS_CHUNK - 1) // MULTI_LOSS_CHUNK
    host = torch.from_numpy(np.asarray(rows, dtype=np.int64).reshape(len(rows), MULTI_LOSS_WORDS))
    dev = a_list[0].device
    if dev.type == "cuda":
        host = host.pin_memory()
    return host.to(dev, non_blocking=True), chunk0, host


def _chk_loss_operand(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("loss operand %s must live on the GPU: the set_amd path has no CPU fallback" % name)
    if t.dtype != torch.float32:
        raise TypeError("loss operand %s must be float32, got %s" % (name, t.dtype))


def multi_loss_fwd(table, n_items, total_chunks, scale, n_slots, sentinel=None):
    """set_multi_loss_fwd -> loss [n_slots] fp32 on the device."""
    part = torch.empty(total_chunks, dtype=torch.float64, device=table.device)
    if sentinel is not None:
        part.fill_(sentinel)
    loss = _buf((n_slots,), table.device, sentinel)
    check(_lib.lib().set_multi_loss_fwd(_p(table), n_items, total_chunks, float(scale), n_slots, _p(part), _p(loss), _stream()), "set_multi_loss_fwd")
    return loss


def multi_loss_bwd(table, n_items, total_chunks, scale, u):
    """set_multi_loss_bwd: writes the gradient buffers the table names; u [n_slots] fp32 on the device."""
    _f(u, "u")
    check(_lib.lib().set_multi_loss_bwd(_p(table), n_items, total_chunks, float(scale), _p(u), _stream()), "set_multi_loss_bwd")


# --------------------------------------------------------------------------
# multi-scale discriminator (csrc/msd.hip): grouped convs with up to 41 taps, the first layer from the waveforms, the 4 / 2 average pool
# --------------------------------------------------------------------------
GCONV_KMAX, WAVE_CONV_KMAX = 41, 15
GCONV_TILES = (128, 64)   # frames per block when a group's rows (Cout / g forward, Cin / g dgrad) fit one 32-row block / need more


def gconv_tile(rows_per_group):
    """Output frames (forward) or, times the stride, input frames (dgrad) of one block (set_gconv1d_tile)."""
    n = _lib.lib().set_gconv1d_tile(int(rows_per_group))
    if n < 0:
        check(n, "set_gconv1d_tile")
    return n


def gconv_out_len(H_in, K, stride, pad):
    """H_out = (H_in + 2 pad - K) // stride + 1 (set_gconv1d_out_len; raises outside 1 <= K <= 41, 1 <= stride <= 4, 0 <= pad < K)."""
    n = _lib.lib().set_gconv1d_out_len(int(H_in), int(K), int(stride), int(pad))
    if n < 0:
        check(n, "set_gconv1d_out_len")
    return n


class GroupedConvWeight:
    """Weight operand of set_gconv1d_fwd / _dgrad: W [Cout, Cin / groups, K].  Group g is the dense conv weight W[g Cout/G : (g + 1) Cout/G];
    its image is what set_pack_conv_weight makes of it (the one layout, the one pack kernel), written into slot g of one buffer -- and
    likewise the transposed weights for the input gradient.  `getter` as ConvWeight's; the images follow the weight's storage and version."""

    def __init__(self, getter, Cout, Cin, K, groups):
        if Cout % groups or Cin % groups:
            raise ValueError("groups = %d must divide Cin = %d and Cout = %d" % (groups, Cin, Cout))
        self.Cout, self.Cin, self.K, self.groups = int(Cout), int(Cin), int(K), int(groups)
        self._src = ConvWeight(getter, Cout, Cin // groups, K)   # resolves the weight; never packed as a whole
        self._fwd, self._tr = CacheSlot(), CacheSlot()

    def raw(self):
        return self._src.raw()

    def _pack(self, w, wp, transposed):
        L = _lib.lib()
        cog, cig, K = self.Cout // self.groups, self.Cin // self.groups, self.K
        rows, red = (cig, cog) if transposed else (cog, cig)
        slot = L.set_packed_conv_weight_size(rows, red, K)
        if wp is None or wp.device != w.device:
            wp = torch.empty(self.groups * slot, dtype=torch.float32, device=w.device)
        sco, sci = (K, cig * K) if transposed else (cig * K, K)
        for g in range(self.groups):
            check(L.set_pack_conv_weight(_p(w), wp.data_ptr() + 4 * g * slot, rows, red, K, g * cog * cig * K, sco, sci, 1, _stream()),
                  "set_pack_conv_weight")
        return wp

    def packed(self):
        w = self.raw()
        return self._fwd.get(weights_key((w,)), lambda wp: self._pack(w, wp, False))

    def packed_transposed(self):
        w = self.raw()
        return self._tr.get(weights_key((w,)), lambda wp: self._pack(w, wp, True))


def gconv1d_fwd(x, weight, bias=None, *, stride, pad, slope=None, sentinel=None):
    """set_gconv1d_fwd: x [R,Cin,H_in] -> act(grouped conv(x) + bias) [R,Cout,H_out]; `slope` None: no activation, else leaky ReLU."""
    _rows3(x, "x"), _f(bias, "bias")
    R, Cin, H_in = x.shape
    if Cin != weight.Cin:
        raise ValueError("gconv1d_fwd: x has %d channels, the weight takes %d" % (Cin, weight.Cin))
    H_out = gconv_out_len(H_in, weight.K, stride, pad)
    if H_out < 1:
        raise ValueError("gconv1d_fwd: %d frames give no output frame at K = %d, stride %d, pad %d" % (H_in, weight.K, stride, pad))
    out = _buf((R, weight.Cout, H_out), x.device, sentinel)
    check(_lib.lib().set_gconv1d_fwd(_p(x), _p(weight.packed()), _p(bias), _p(out), R, Cin, weight.Cout, weight.groups, H_in, weight.K, int(stride),
                                     int(pad), int(slope is not None), float(slope or 0.0), _stream()), "set_gconv1d_fwd")
    return out


def gconv1d_dgrad(dz_out, weight, H_in, *, stride, pad, f_in=None, add=None, slope=0.0, sentinel=None):
    """set_gconv1d_dgrad: dz_out [R,Cout,H_out] -> gate(f_in) * (add + conv^T(dz_out)) [R,Cin,H_in]; f_in / add: [R,Cin,H_in] or None."""
    _rows3(dz_out, "dz_out")
    R, Cout, H_out = dz_out.shape
    if Cout != weight.Cout or H_out != gconv_out_len(H_in, weight.K, stride, pad):
        raise ValueError("gconv1d_dgrad: dz_out %s does not belong to a (%d -> %d, K = %d, stride %d, pad %d, groups %d) layer on %d frames"
                         % (tuple(dz_out.shape), weight.Cin, weight.Cout, weight.K, stride, pad, weight.groups, H_in))
    for t, name in ((f_in, "f_in"), (add, "add")):
        if t is not None and tuple(_rows3(t, name).shape) != (R, weight.Cin, H_in):
            raise ValueError("gconv1d_dgrad: %s must be [%d, %d, %d], got %s" % (name, R, weight.Cin, H_in, tuple(t.shape)))
    dz_in = _buf((R, weight.Cin, H_in), dz_out.device, sentinel)
    check(_lib.lib().set_gconv1d_dgrad(_p(dz_out), _p(weight.packed_transposed()), _p(f_in), _p(add), _p(dz_in), R, weight.Cin, Cout, weight.groups,
                                       int(H_in), weight.K, int(stride), int(pad), float(slope), _stream()), "set_gconv1d_dgrad")
    return dz_in


def wave_conv_fwd(y, y_hat, w, bias, *, pad, slope=None, sentinel=None):
    """set_wave_conv_fwd: y, y_hat [B,T] -> the first layer's map [2 B, C, T] (real rows first); w: the raw weight [C, 1, K] or [C, K].
    y_hat None: the map of y alone [B, C, T]."""
    _f(y, "y"), _f(y_hat, "y_hat"), _f(w, "w"), _f(bias, "bias")
    if y.dim() != 2 or (y_hat is not None and y.shape != y_hat.shape):
        raise ValueError("wave_conv_fwd: y and y_hat must be equal [B, T], got %s and %s" % (tuple(y.shape), tuple(y_hat.shape)))
    B, T = y.shape
    Cc = w.shape[0]
    K = w.numel() // Cc
    out = _buf(((1 if y_hat is None else 2) * B, Cc, T), y.device, sentinel)
    check(_lib.lib().set_wave_conv_fwd(_p(y), _p(y_hat), _p(w), _p(bias), _p(out), B, T, Cc, K, int(pad), int(slope is not None), float(slope or 0.0),
                                       _stream()), "set_wave_conv_fwd")
    return out


def wave_conv_bwd(dz, w, *, pad, sentinel=None):
    """set_wave_conv_bwd: dz [B, C, T] (generated rows) -> d/d y_hat [B, T]."""
    _rows3(dz, "dz"), _f(w, "w")
    B, Cc, T = dz.shape
    if w.shape[0] != Cc:
        raise ValueError("wave_conv_bwd: dz has %d channels, the weight %d" % (Cc, w.shape[0]))
    g_wav = _buf((B, T), dz.device, sentinel)
    check(_lib.lib().set_wave_conv_bwd(_p(dz), _p(w), _p(g_wav), B, T, Cc, w.numel() // Cc, int(pad), _stream()), "set_wave_conv_bwd")
    return g_wav


def avgpool4s2_out_len(T):
    return _lib.lib().set_avgpool4s2_out_len(int(T))


def avgpool4s2_fwd(x, sentinel=None):
    """set_avgpool4s2_fwd: AvgPool1d(4, 2, padding=1) on x [B, T] -> [B, (T - 2) // 2 + 1]."""
    _f(x, "x")
    if x.dim() != 2 or x.shape[1] < 2:
        raise ValueError("avgpool4s2_fwd: x must be [B, T] with T >= 2, got %s" % (tuple(x.shape),))
    B, T = x.shape
    out = _buf((B, avgpool4s2_out_len(T)), x.device, sentinel)
    check(_lib.lib().set_avgpool4s2_fwd(_p(x), _p(out), B, T, _stream()), "set_avgpool4s2_fwd")
    return out


def avgpool4s2_bwd(g_out, T, add=None, sentinel=None):
    """set_avgpool4s2_bwd: g_out [B, T_out] -> add + pool^T(g_out) [B, T]."""
    _f(g_out, "g_out"), _f(add, "add")
    B = g_out.shape[0]
    if g_out.dim() != 2 or T < 2 or g_out.shape[1] != avgpool4s2_out_len(T) or (add is not None and tuple(add.shape) != (B, T)):
        raise ValueError("avgpool4s2_bwd: g_out %s (and add) do not belong to a pool of %d samples" % (tuple(g_out.shape), T))
    g_in = _buf((B, T), g_out.device, sentinel)
    check(_lib.lib().set_avgpool4s2_bwd(_p(g_out), _p(add), _p(g_in), B, int(T), _stream()), "set_avgpool4s2_bwd")
    return g_in


# --------------------------------------------------------------------------
# the discriminator step (csrc/disc_wgrad.hip): weight and bias gradients of the discriminators' convs, the backward of the norm folds
# --------------------------------------------------------------------------
GCONV_WGRAD_CHUNK, GCONV_WGRAD_COLS, GCONV_WGRAD_MAX_SLICES, FIRST_WGRAD_MAX_SLICES = 32, 128, 64, 64


def gconv_wgrad_plan(R, Cin, Cout, groups, H_in, K, stride, pad, n_cu=0):
    """The number of reduction slices set_gconv1d_wgrad takes at `slices` = 0 (set_gconv1d_wgrad_plan); n_cu 0: the current device's."""
    n = _lib.lib().set_gconv1d_wgrad_plan(int(R), int(Cin), int(Cout), int(groups), int(H_in), int(K), int(stride), int(pad), int(n_cu))
    if n < 0:
        check(n, "set_gconv1d_wgrad_plan")
    return n


def _grad_out(t, shape, dev, accumulate, sentinel, name):
    """The buffer a gradient is written to (new, `sentinel`-filled for the tests) or added to (`t`, which accumulate requires)."""
    if t is None:
        if accumulate:
            raise ValueError("%s: accumulate needs the tensor to add to" % name)
        return _buf(shape, dev, sentinel)
    _f(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def gconv1d_wgrad(dz, x, K, *, stride, pad, groups=1, want_dw=True, want_db=False, dw=None, db=None, accumulate=False, slices=0, sentinel=None):
    """set_gconv1d_wgrad: dz [R,Cout,H_out], x [R,Cin,H_in] -> (dW [Cout, Cin / groups, K] or None, db [Cout] or None).  `dw` / `db`:
    tensors to write or, with accumulate, to add to.  slices 0: the plan's."""
    _rows3(dz, "dz"), _rows3(x, "x")
    R, Cout, H_out = dz.shape
    _R, Cin, H_in = x.shape
    K, groups = int(K), int(groups)
    if _R != R or Cin % groups or Cout % groups or not 1 <= K <= GCONV_KMAX or H_out != gconv_out_len(H_in, K, stride, pad):
        raise ValueError("gconv1d_wgrad: dz %s and x %s do not belong to one (K = %d, stride %d, pad %d, groups %d) layer"
                         % (tuple(dz.shape), tuple(x.shape), K, stride, pad, groups))
    if not (want_dw or want_db):
        return None, None
    L = _lib.lib()
    dev = dz.device
    dw = _grad_out(dw, (Cout, Cin // groups, K), dev, accumulate, sentinel, "dw") if want_dw else None
    db = _grad_out(db, (Cout,), dev, accumulate, sentinel, "db") if want_db else None
    scratch, n = None, 0
    if want_dw:
        if slices == 0:
            slices = gconv_wgrad_plan(R, Cin, Cout, groups, H_in, K, stride, pad)
        if slices != 1 or accumulate:
            n = L.set_gconv1d_wgrad_scratch_floats(R, Cin, Cout, groups, H_in, K, int(stride), int(pad), int(slices))
            if n < 0:
                check(n, "set_gconv1d_wgrad_scratch_floats")
            scratch = _buf((n,), dev, sentinel)
    check(L.set_gconv1d_wgrad(_p(dz), _p(x), _p(dw), _p(db), R, Cin, Cout, groups, H_in, K, int(stride), int(pad), int(bool(accumulate)), int(slices),
                              _p(scratch), n, _stream()), "set_gconv1d_wgrad")
    return dw, db


def _first_part(Cc, K, slices, dev, sentinel):
    n = _lib.lib().set_first_conv_wgrad_part_doubles(int(Cc), int(K), int(slices))
    if n < 0:
        check(n, "set_first_conv_wgrad_part_doubles")
    part = torch.empty(n, dtype=torch.float64, device=dev)
    return (part if sentinel is None else part.fill_(sentinel)), n


def mpd_fold_conv_wgrad(dz, y, y_hat, period, K, *, stride, pad, want_dw=True, want_db=True, dw=None, db=None, accumulate=False, slices=0,
                        sentinel=None):
    """set_mpd_fold_conv_wgrad: dz [2 B p, C, H_out] (all rows), y, y_hat [B, T] -> (dW [C, K] or None, db [C] or None)."""
    _rows3(dz, "dz"), _f(y, "y"), _f(y_hat, "y_hat")
    if y.dim() != 2 or y.shape != y_hat.shape:
        raise ValueError("mpd_fold_conv_wgrad: y and y_hat must be equal [B, T], got %s and %s" % (tuple(y.shape), tuple(y_hat.shape)))
    B, T = y.shape
    R, Cc, H_out = dz.shape
    if T <= period or R != 2 * B * period or H_out != sconv_out_len((T + period - 1) // period, K, stride, pad):
        raise ValueError("mpd_fold_conv_wgrad: dz %s does not belong to period %d on %s" % (tuple(dz.shape), period, tuple(y.shape)))
    if not (want_dw or want_db):
        return None, None
    dw = _grad_out(dw, (Cc, K), dz.device, accumulate, sentinel, "dw") if want_dw else None
    db = _grad_out(db, (Cc,), dz.device, accumulate, sentinel, "db") if want_db else None
    part, n = _first_part(Cc, K, slices, dz.device, sentinel)
    check(_lib.lib().set_mpd_fold_conv_wgrad(_p(dz), _p(y), _p(y_hat), _p(dw), _p(db), B, T, int(period), Cc, int(K), int(stride), int(pad),
                                             int(bool(accumulate)), int(slices), _p(part), n, _stream()), "set_mpd_fold_conv_wgrad")
    return dw, db


def wave_conv_wgrad(dz, y, y_hat, K, *, pad, want_dw=True, want_db=True, dw=None, db=None, accumulate=False, slices=0, sentinel=None):
    """set_wave_conv_wgrad: dz [2 B, C, T] (all rows; [B, C, T] with y_hat None), y, y_hat [B, T] -> (dW [C, K] or None, db [C] or None)."""
    _rows3(dz, "dz"), _f(y, "y"), _f(y_hat, "y_hat")
    B, T = y.shape
    R, Cc, H = dz.shape
    if y.dim() != 2 or (y_hat is not None and y_hat.shape != y.shape) or R != (1 if y_hat is None else 2) * B or H != T:
        raise ValueError("wave_conv_wgrad: dz %s does not belong to waveforms %s" % (tuple(dz.shape), tuple(y.shape)))
    if not (want_dw or want_db):
        return None, None
    dw = _grad_out(dw, (Cc, K), dz.device, accumulate, sentinel, "dw") if want_dw else None
    db = _grad_out(db, (Cc,), dz.device, accumulate, sentinel, "db") if want_db else None
    part, n = _first_part(Cc, K, slices, dz.device, sentinel)
    check(_lib.lib().set_wave_conv_wgrad(_p(dz), _p(y), _p(y_hat), _p(dw), _p(db), B, T, Cc, int(K), int(pad), int(bool(accumulate)), int(slices),
                                         _p(part), n, _stream()), "set_wave_conv_wgrad")
    return dw, db


def weight_norm_fold_bwd(dw, g, v, *, want_dg=True, want_dv=True, sentinel=None):
    """set_weight_norm_fold_bwd: dW (v's shape), g, v -> (dg (g's shape) or None, dv or None)."""
    _f(dw, "dw"), _f(g, "g"), _f(v, "v")
    n0 = v.shape[0]
    if dw.numel() != v.numel() or g.numel() != n0:
        raise ValueError("weight_norm_fold_bwd: dW %s, g %s, v %s" % (tuple(dw.shape), tuple(g.shape), tuple(v.shape)))
    if not (want_dg or want_dv):
        return None, None
    dg = _buf(tuple(g.shape), v.device, sentinel) if want_dg else None
    dv = _buf(tuple(v.shape), v.device, sentinel) if want_dv else None
    check(_lib.lib().set_weight_norm_fold_bwd(_p(dw), _p(g), _p(v), _p(dg), _p(dv), n0, v.numel() // n0, 0, _stream()), "set_weight_norm_fold_bwd")
    return dg, dv


def spectral_norm_fold_bwd(dw, w_orig, u, v, sigma, *, out=None, accumulate=False, sentinel=None):
    """set_spectral_norm_fold_bwd: dW, weight_orig [n0, ...], u [n0], v [inner], sigma (a device scalar) -> d weight_orig (written to
    or, with accumulate, added to `out`)."""
    _f(dw, "dw"), _f(w_orig, "w_orig"), _f(u, "u"), _f(v, "v"), _f(sigma, "sigma")
    n0 = w_orig.shape[0]
    inner = w_orig.numel() // n0
    if dw.numel() != w_orig.numel() or u.numel() != n0 or v.numel() != inner or sigma.numel() != 1:
        raise ValueError("spectral_norm_fold_bwd: dW %s, weight_orig %s, u %s, v %s" % (tuple(dw.shape), tuple(w_orig.shape), tuple(u.shape), tuple(v.shape)))
    out = _grad_out(out, tuple(w_orig.shape), w_orig.device, accumulate, sentinel, "out")
    part = torch.empty(n0, dtype=torch.float64, device=w_orig.device)
    if sentinel is not None:
        part.fill_(sentinel)
    check(_lib.lib().set_spectral_norm_fold_bwd(_p(dw), _p(w_orig), _p(u), _p(v), _p(sigma), _p(out), n0, inner, int(bool(accumulate)), _p(part), _stream()),
          "set_spectral_norm_fold_bwd")
    return out
