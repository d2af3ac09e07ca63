"""GPU branch sweep of the bf16 DiffNet layer kernels (csrc/diffnet_bf16.hip): the pack kernel, the per-layer forward in both
instantiations, the two layer-group kernels, the backward and the three ordered reductions.  ONE raw ABI call per case against the
model of tests/test_diffnet_bf16_reference.py, which also holds the case tables (each case names the branch it reaches; CPU tests pin
that against Python mirrors of the launch code) and asserts every condition this file stands on.

  exact      integer-grid operands with rounding probes, a saturated gate (forward) / a class-coded y16 (backward): every partial sum
             in any order is an fp32 number (budgets asserted on the CPU), so every output must equal the model BIT FOR BIT.
  bounded    operands of Gaussian magnitude at two scales, an unsaturated gate, stage by stage: y16, z16 and dy16 must lie in the set of
             bf16 numbers RNE can return on the model's interval (summation bound, gate slack; at most 5 % of the elements have a choice,
             asserted on the CPU); x_out and skip are held to the summation bound of the model's GEMM 2 fed with the kernel's OWN z16, dx,
             dcond, part_dby and part_dd to that of the model fed with the kernel's own dy16; d_o16 bit for bit.
  identical  Gaussian operands: what the ABI promises to be bit-identical is compared bit for bit -- the inference form of the per-layer
             forward with the training form, a layer group with `nl` per-layer launches on the same images.
Every output (fp32 tensors, bf16 tensors, the part_* arrays, the scratch, the image) is a view inside a larger sentinel-filled buffer
and the WHOLE buffer is compared: the model's written set against the model, everything else against the sentinel.  Inputs are
checked unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_bf16_reference import bf16_value, q4, rne_bf16_bits
from test_conv_reference import gamma
from test_diffnet_bf16_reference import (BWD, BWD_REFUSED, E_INVALID, FC, FH, FWD, FWD_REFUSED, LAYERS, LAYERS_REFUSED, N_IMG, RED_COLS, RED_ROWS,
                                         ROWS_RG, bwd_tiles, int_partials, layer_image, layers_launch, layers_plan, layers_scratch_written,
                                         layers_scratch_floats, make_backward_exact, make_forward_exact, pack_weights, SCALES, backward_from_dy,
                                         forward_gemm2, in_set, make_backward_bounded, make_forward_bounded, q4_unpack)

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
IMG_SENTINEL = 0x5A5A
GUARD = 64  # elements either side of every view (128 bytes of bf16: views stay 16-byte aligned)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_ALIVE = []  # device tensors whose raw address went to a launch


@pytest.fixture(autouse=True)
def _keep_launch_operands():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more is started on this GPU
        pytest.exit("device error after a sweep case, the session ends here: %s" % e, returncode=3)
    _ALIVE.clear()


def _L():
    from set_amd import _lib
    return _lib.lib()


def _s():
    from set_amd.ops import _stream
    return _stream()


def _line(family, name, mode, frac=0.0):
    print("DIFFNETBF16SWEEP family=%s case=%s mode=%s worst_fraction_of_bar=%.4f" % (family, name, mode, frac))


class Buf:
    """A view of n elements inside a sentinel-filled device buffer.  kind "f32" (sentinel -7777) or "u16" (0x5A5A); init: what the view
    holds before the call (a tensor / array, "nan", or None: the sentinel)."""

    def __init__(self, dev, kind, n, init=None):
        self.kind, self.n = kind, n
        if kind == "f32":
            host = torch.full((n + 2 * GUARD,), SENTINEL)
            if isinstance(init, str):
                host[GUARD:GUARD + n] = float("nan")
            elif init is not None:
                host[GUARD:GUARD + n] = init.reshape(-1).float()
        else:
            a = np.full(n + 2 * GUARD, IMG_SENTINEL, dtype=np.uint16)
            if init is not None:
                a[GUARD:GUARD + n] = np.asarray(init, dtype=np.uint16).reshape(-1)
            host = torch.from_numpy(a.view(np.int16).copy())
        self.before = host.clone()
        self.d = host.to(dev)
        _ALIVE.append(self.d)
        self.ptr = self.d.data_ptr() + GUARD * (4 if kind == "f32" else 2)

    def bits(self):
        h = self.d.cpu()
        return h.view(torch.int32) if self.kind == "f32" else h

    def view(self):
        return self.d.cpu()[GUARD:GUARD + self.n]

    def want_bits(self, want=None):
        """The whole buffer as it must be after the call: `want` (None: what the view held before) inside the untouched guards."""
        w = self.before.clone()
        if want is not None:
            if self.kind == "f32":
                w[GUARD:GUARD + self.n] = want.reshape(-1).float()
            else:
                w[GUARD:GUARD + self.n] = torch.from_numpy(np.asarray(want, dtype=np.uint16).reshape(-1).view(np.int16).copy())
        return w.view(torch.int32) if self.kind == "f32" else w

    def check(self, what, want=None, either_zero=False):
        """either_zero (bf16 only): where the model holds +0 a -0 passes too."""
        got, w = self.bits(), self.want_bits(want)
        if either_zero:
            got = torch.where((got == -32768) & (w == 0), torch.zeros_like(got), got)
        bad = (got != w).nonzero().flatten()
        assert bad.numel() == 0, (what, "first differing buffer elements (view starts at %d)" % GUARD, bad[:8].tolist(),
                                  self.d.cpu()[bad[:8]].tolist(), (self.want_bits(want).view(torch.float32) if self.kind == "f32" else w)[bad[:8]].tolist())


def _within(buf, what, want, bar):
    """fp32 buffer: the guards bit for bit, every element of the view within its bar (a NaN is outside any bar).  Returns the worst
    fraction of the bar."""
    h = buf.d.cpu()
    assert bool((h[:GUARD] == SENTINEL).all() and (h[GUARD + buf.n:] == SENTINEL).all()), (what, "guards")
    d = (h[GUARD:GUARD + buf.n].double() - want.reshape(-1)).abs()
    bar = bar.reshape(-1)
    bad = (~(d <= bar)).nonzero().flatten()
    assert bad.numel() == 0, (what, bad.numel(), bad[:6].tolist(), h[GUARD:GUARD + buf.n][bad[:6]].tolist(), want.reshape(-1)[bad[:6]].tolist(), bar[bad[:6]].tolist())
    return float((d / (bar + 1e-300))[bar > 0].max()) if bool((bar > 0).any()) else 0.0


def _in_sets(buf, what, B, Cc, T, lo_v, hi_v):
    """bf16 buffer (quad layout): the guards, and every element of the view inside its admissible set.  Returns the [B][C][T] bits."""
    h = buf.d.cpu().numpy().view(np.uint16)
    assert (h[:GUARD] == IMG_SENTINEL).all() and (h[GUARD + buf.n:] == IMG_SENTINEL).all(), (what, "guards")
    bits = q4_unpack(h[GUARD:GUARD + buf.n], B, Cc, T)
    ok = in_set(bits, lo_v, hi_v)
    bad = (~ok).nonzero()
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:6].tolist(), bf16_value(bits)[~ok][:6].tolist(), lo_v[~ok][:6].tolist(), hi_v[~ok][:6].tolist())
    return bits


def _ro(dev, t):
    """A read-only fp32 operand on the device; returns (device tensor, host copy)."""
    h = t.detach().float().contiguous().clone()
    d = h.to(dev)
    _ALIVE.append(d)
    return d, h


def _unchanged(pairs):
    for d, h in pairs:
        assert torch.equal(d.cpu().view(torch.int32) if d.dtype == torch.float32 else d.cpu(), h.view(torch.int32) if h.dtype == torch.float32 else h)


def _dstep(dev, d, d_bs, d_cs, layers=1, d_ls=0):
    """d [layers][B][256] at layer * d_ls + b * d_bs + c * d_cs inside a buffer of 99s."""
    d = d.reshape(layers, -1, FC)
    B = d.shape[1]
    n = (layers - 1) * d_ls + (B - 1) * d_bs + (FC - 1) * d_cs + 1
    h = torch.full((n,), 99.0)
    h.as_strided((layers, B, FC), (d_ls, d_bs, d_cs)).copy_(d)
    return _ro(dev, h)


def _pack_one(dev, Wd, Wc, Wo):
    """set_pack_diffnet_layer_bf16 into a guarded buffer, compared whole with the image model."""
    ws = [_ro(dev, w) for w in (Wd, Wc, Wo)]
    img = Buf(dev, "u16", N_IMG)
    assert _L().set_pack_diffnet_layer_bf16(ws[0][0].data_ptr(), ws[1][0].data_ptr(), ws[2][0].data_ptr(), img.ptr, _s()) == 0
    torch.cuda.synchronize()
    img.check("packed image", layer_image(Wd, Wc, Wo))
    _unchanged(ws)
    img.before = img.d.cpu().clone()  # from here on the image is an input: check() without `want` compares with this
    return img


# ------------------------------------------------------------------------------------------------------------------------
# gate preconditions, host mirrors
# ------------------------------------------------------------------------------------------------------------------------
GATE_POINTS = [((40.0, 40.0), 1.0), ((40.0, -40.0), -1.0), ((20.0, 12.0), 1.0), ((20.0, -12.0), -1.0), ((0.0, 0.0), 0.0), ((0.0, 40.0), 0.5),
               ((0.0, -40.0), -0.5)]


def _fwd_args(B, T, dil, first, x, xo, skip, cond, dstep, d_bs, d_cs, img, bd, bc, bo, y16=None, z16=None):
    from set_amd import _lib
    a = _lib.SetDiffnetLayerBf16Args()
    a.x_in, a.x_out, a.skip, a.cond, a.dstep, a.img = x, xo, skip, cond, dstep, img
    a.b_dil, a.b_cond, a.b_out, a.y16, a.z16 = bd, bc, bo, y16, z16
    a.d_bs, a.d_cs, a.B, a.T, a.dil, a.first = d_bs, d_cs, B, T, dil, first
    return a


def test_gate_preconditions(dev):
    """What the exact modes stand on: with zero weights the training-form forward puts y at the biases; at the points the exact modes
    use -- (+40, +-40), (+20, +-12), (0, 0), (0, +-40) -- the device's sigmoid(y_g) tanh(y_f) must round to +-1, +-1, 0, +-1/2 bit for bit
    (sigmoid(0) = 1/2 and tanh(0) = 0 are what the class-coded backward cases assume of the same two device functions)."""
    B, T = 1, 130
    g = torch.Generator().manual_seed(5)
    z = torch.zeros
    img = _pack_one(dev, z(512, FC, 3), z(512, FH), z(512, FC))
    pt = torch.arange(FC) % len(GATE_POINTS)
    bdil = torch.cat([torch.tensor([GATE_POINTS[i][0][0] for i in pt]), torch.tensor([GATE_POINTS[i][0][1] for i in pt])])
    x, cond = torch.randn(B, FC, T, generator=g), torch.randn(B, FH, T, generator=g)
    ops = [_ro(dev, t) for t in (x, cond, bdil, z(512), z(512))]
    ds = _dstep(dev, torch.randn(B, FC, generator=g), FC, 1)
    xo, sk = Buf(dev, "f32", B * FC * T), Buf(dev, "f32", B * FC * T, "nan")
    y16, z16 = Buf(dev, "u16", B * 512 * T), Buf(dev, "u16", B * FC * T)
    a = _fwd_args(B, T, 1, 1, ops[0][0].data_ptr(), xo.ptr, sk.ptr, ops[1][0].data_ptr(), ds[0].data_ptr(), FC, 1, img.ptr, ops[2][0].data_ptr(),
                  ops[3][0].data_ptr(), ops[4][0].data_ptr(), y16.ptr, z16.ptr)
    assert _L().set_diffnet_layer_fwd_bf16(C.byref(a), _s()) == 0
    torch.cuda.synchronize()
    want_z = torch.tensor([GATE_POINTS[i][1] for i in pt])[None, :, None].expand(B, FC, T)
    got = bf16_value(q4_unpack(z16.view().numpy().view(np.uint16), B, FC, T))
    for i, (pnt, wz) in enumerate(GATE_POINTS):
        print("GATEPRECONDITION y=(%g, %g) z16=%s want %g" % (pnt[0], pnt[1], sorted(set(got[:, pt == i].reshape(-1).tolist())), wz))
    y16.check("y16 = the biases", q4(rne_bf16_bits(bdil[None, :, None].expand(B, 512, T).contiguous())))
    z16.check("z16 at the gate points", q4(rne_bf16_bits(want_z.contiguous())))
    sk.check("skip = 0 (zero weights and biases, first)", torch.zeros(B, FC, T))
    xo.check("x_out = x / sqrt 2", torch.from_numpy(x.numpy() * np.float32(0.70710678118654752440)))
    _line("gate", "preconditions", "exact")


def test_host_mirrors_equal_the_library(dev, monkeypatch):
    """The four callable mirrors against the library's own answers."""
    L = _L()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert L.set_diffnet_layer_bf16_image_size() == N_IMG
    for T in (1, 5, 111, 112, 113, 126, 127, 253, 400):
        for dil in (1, 2, 4, 8):
            assert L.set_diffnet_layer_bwd_bf16_tiles(T, dil) == bwd_tiles(T, dil)
    for env in (None, "64", "128", "96"):
        if env is None:
            monkeypatch.delenv("SET_AMD_BF16_FUSE_TILE", raising=False)
        else:
            monkeypatch.setenv("SET_AMD_BF16_FUSE_TILE", env)
        for B, T in ((1, 100), (3, 400), (32, 800), (4, 800), (64, 800)):
            for L_ in (1, 3, 5, 10, 20):
                for dcl in (1, 2, 3, 4):
                    assert L.set_diffnet_layers_bf16_plan(B, T, L_, dcl) == layers_plan(B, T, L_, dcl, env, n_cu), (env, B, T, L_, dcl)
    for B, T in ((1, 1), (2, 60), (3, 400), (32, 800)):
        for dcl in (1, 2, 3, 4):
            for nl in range(1, 18):
                for l0 in (0, 1, 3):
                    assert L.set_diffnet_layers_bf16_scratch_floats(B, T, l0, nl, dcl) == layers_scratch_floats(B, T, l0, nl, dcl), (B, T, l0, nl, dcl)
    assert L.set_diffnet_layers_bf16_scratch_floats(0, 1, 0, 1, 1) == 0 and L.set_diffnet_layers_bf16_scratch_floats(1, 1, -1, 1, 1) == 0


# ------------------------------------------------------------------------------------------------------------------------
# pack
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_pack_writes_the_modelled_image_and_nothing_else(dev, seed):
    _pack_one(dev, *pack_weights(seed))
    _line("pack", "single_seed%d" % seed, "exact")


@pytest.mark.parametrize("L_", [1, 3])
def test_pack_layers_equals_single_packs_at_flat_optimizer_strides(dev, L_):
    """Layer q reads w* + q * its stride (strides larger than the tensors, 99s in the gaps) and writes image q."""
    ws = [pack_weights(10 + q) for q in range(L_)]
    sizes, strides = (512 * FC * 3, 512 * FH, 512 * FC), (512 * FC * 3 + 17, 512 * FH + 4, 512 * FC + 129)
    flats = []
    for j in range(3):
        h = torch.full(((L_ - 1) * strides[j] + sizes[j],), 99.0)
        for q in range(L_):
            h[q * strides[j]:q * strides[j] + sizes[j]] = ws[q][j].reshape(-1)
        flats.append(_ro(dev, h))
    img = Buf(dev, "u16", L_ * N_IMG)
    rc = _L().set_pack_diffnet_layers_bf16(flats[0][0].data_ptr(), flats[1][0].data_ptr(), flats[2][0].data_ptr(), strides[0], strides[1], strides[2],
                                           img.ptr, L_, _s())
    assert rc == 0
    torch.cuda.synchronize()
    img.check("images of %d layers" % L_, np.concatenate([layer_image(*w) for w in ws]))
    _unchanged(flats)
    _line("pack", "layers_L%d" % L_, "exact")


def test_pack_refusals(dev):
    img = Buf(dev, "u16", 64)
    w, _ = _ro(dev, torch.zeros(8))
    assert _L().set_pack_diffnet_layer_bf16(None, w.data_ptr(), w.data_ptr(), img.ptr, _s()) == E_INVALID
    assert _L().set_pack_diffnet_layers_bf16(w.data_ptr(), w.data_ptr(), w.data_ptr(), 0, 0, 0, img.ptr, 0, _s()) == E_INVALID
    torch.cuda.synchronize()
    img.check("image of a refused pack")


# ------------------------------------------------------------------------------------------------------------------------
# per-layer forward
# ------------------------------------------------------------------------------------------------------------------------
def _forward(dev, o, img, train, skip0):
    """One set_diffnet_layer_fwd_bf16 call on fresh buffers.  skip0: the tensor the skip view holds before the call, or "nan"."""
    B, T = o["B"], o["T"]
    ops = [_ro(dev, o[k]) for k in ("x", "cond", "bd", "bc", "bo")]
    ds = _dstep(dev, o["d"], o["d_bs"], o["d_cs"])
    xo, sk = Buf(dev, "f32", B * FC * T), Buf(dev, "f32", B * FC * T, skip0)
    y16 = Buf(dev, "u16", B * 512 * T) if train else None
    z16 = Buf(dev, "u16", B * FC * T) if train else None
    a = _fwd_args(B, T, o["dil"], o["first"], ops[0][0].data_ptr(), xo.ptr, sk.ptr, ops[1][0].data_ptr(), ds[0].data_ptr(), o["d_bs"], o["d_cs"],
                  img.ptr, ops[2][0].data_ptr(), ops[3][0].data_ptr(), ops[4][0].data_ptr(), y16.ptr if train else None, z16.ptr if train else None)
    assert _L().set_diffnet_layer_fwd_bf16(C.byref(a), _s()) == 0
    torch.cuda.synchronize()
    _unchanged(ops + [ds])
    img.check("image after the launch")
    return xo, sk, y16, z16


@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_layer_forward_exact(dev, c):
    """Both instantiations against the exact model: x_out, skip, and (training form) y16 and z16 bit for bit, the buffers whole.
    first = 1 runs over a NaN-filled skip: a NaN that reaches an output is a finding."""
    o = make_forward_exact(c)
    img = _pack_one(dev, o["Wd"], o["Wc"], o["Wo"])
    skip0 = "nan" if c["first"] else o["skip0"]
    for train in (True, False):
        xo, sk, y16, z16 = _forward(dev, o, img, train, skip0)
        what = "%s %s" % (c["name"], "train" if train else "infer")
        if train:
            y16.check(what + " y16", q4(o["y16"]))
            z16.check(what + " z16", q4(o["z16"]))
        xo.check(what + " x_out", o["x_out"])
        sk.check(what + " skip", o["skip"])
        _line("layer_fwd_%s_%s" % ("train" if train else "infer", "_".join(c["branch"])), c["name"], "exact")


@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_layer_forward_bounded(dev, c):
    """Stage by stage at both scales: y16 and z16 inside their admissible sets, x_out and skip within the summation bound of the model's
    GEMM 2 on the kernel's own z16; then the inference form on the same operands: x_out and skip bit for bit those of the training form."""
    B, T = c["B"], c["T"]
    worst = 0.0
    for k in range(len(SCALES)):
        o = make_forward_bounded(c, k)
        img = _pack_one(dev, o["Wd"], o["Wc"], o["Wo"])
        skip0 = "nan" if c["first"] else o["skip0"]
        xo, sk, y16, z16 = _forward(dev, o, img, True, skip0)
        what = "%s/%d" % (c["name"], k)
        ybits = _in_sets(y16, what + " y16", B, 512, T, o["y_lo"], o["y_hi"])
        zbits = _in_sets(z16, what + " z16", B, FC, T, o["z_lo"], o["z_hi"])
        flips = int((ybits != rne_bf16_bits(o["y"].float())).sum())
        x_w, x_bar, s_w, s_bar = forward_gemm2(o, zbits)
        fx, fs = _within(xo, what + " x_out", x_w, x_bar), _within(sk, what + " skip", s_w, s_bar)
        print("%s: y16 differs from RNE(model y) in %d of %d elements; x_out %.3f, skip %.3f of the bar" % (what, flips, ybits.size, fx, fs))
        worst = max(worst, fx, fs)
        xo_i, sk_i, _, _ = _forward(dev, o, img, False, skip0)
        for name, a, b in (("x_out", xo, xo_i), ("skip", sk, sk_i)):
            bad = (a.bits() != b.bits()).nonzero().flatten()
            assert bad.numel() == 0, (what, name, "inference form differs from the training form, first buffer element", bad[:4].tolist())
    _line("layer_fwd_" + "_".join(c["branch"]), c["name"], "bounded", worst)


def _gauss_layer(g, scale=1.0):
    return dict(Wd=torch.randn(512, FC, 3, generator=g) * 0.03 * scale, Wc=torch.randn(512, FH, generator=g) * 0.05 * scale,
                Wo=torch.randn(512, FC, generator=g) * 0.05 * scale, bd=torch.randn(512, generator=g) * 0.1, bc=torch.randn(512, generator=g) * 0.1,
                bo=torch.randn(512, generator=g) * 0.1)


@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_inference_form_equals_training_form_bit_for_bit(dev, c):
    """Gaussian operands, an unsaturated gate: the two instantiations share every instruction that feeds x_out and skip."""
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]))
    B, T = c["B"], c["T"]
    o = dict(c, **_gauss_layer(g))
    o.update(x=torch.randn(B, FC, T, generator=g), cond=torch.randn(B, FH, T, generator=g), d=torch.randn(B, FC, generator=g) * 0.3,
             skip0=torch.randn(B, FC, T, generator=g))
    img = _pack_one(dev, o["Wd"], o["Wc"], o["Wo"])
    skip0 = "nan" if c["first"] else o["skip0"]
    xo_t, sk_t, y16, z16 = _forward(dev, o, img, True, skip0)
    xo_i, sk_i, _, _ = _forward(dev, o, img, False, skip0)
    for what, a, b in (("x_out", xo_t, xo_i), ("skip", sk_t, sk_i)):
        bad = (a.bits() != b.bits()).nonzero().flatten()
        assert bad.numel() == 0, (c["name"], what, "first differing buffer element", bad[:4].tolist(), a.d.cpu()[bad[:4]].tolist(), b.d.cpu()[bad[:4]].tolist())
        assert bool(torch.isfinite(a.view()).all())
        guards = torch.cat([a.d.cpu()[:GUARD], a.d.cpu()[-GUARD:]])
        assert bool((guards == SENTINEL).all())
    for b16 in (y16, z16):
        h = b16.d.cpu().numpy().view(np.uint16)
        assert (h[:GUARD] == IMG_SENTINEL).all() and (h[-GUARD:] == IMG_SENTINEL).all()
        assert bool(torch.isfinite(bf16_value(h[GUARD:-GUARD])).all())
    _line("layer_fwd_infer_vs_train", c["name"], "identical")


@pytest.mark.parametrize("name,kw", FWD_REFUSED, ids=[n for n, _ in FWD_REFUSED])
def test_layer_forward_refusals_write_nothing(dev, name, kw):
    B, T = 1, 40
    bufs = [Buf(dev, "f32", B * FC * T) for _ in range(2)] + [Buf(dev, "u16", B * 512 * T), Buf(dev, "u16", B * FC * T)]
    r, _ = _ro(dev, torch.zeros(B * FC * T + 1024))
    img = Buf(dev, "u16", N_IMG, np.zeros(N_IMG, dtype=np.uint16))
    a = _fwd_args(kw.get("B", B), kw.get("T", T), kw.get("dil", 1), 0, r.data_ptr(), bufs[0].ptr, bufs[1].ptr, r.data_ptr(), r.data_ptr(), FC, 1, img.ptr,
                  r.data_ptr(), r.data_ptr(), r.data_ptr(), None if kw.get("one_of_y_z") == "z" else bufs[2].ptr,
                  None if kw.get("one_of_y_z") == "y" else bufs[3].ptr)
    assert _L().set_diffnet_layer_fwd_bf16(C.byref(a), _s()) == E_INVALID, name
    torch.cuda.synchronize()
    for b in bufs:
        b.check(name)


# ------------------------------------------------------------------------------------------------------------------------
# layer groups
# ------------------------------------------------------------------------------------------------------------------------
def _layers_args(c, x, xo, skip, cond, dstep, d_ls, img, bd, bc, bo, scratch, scratch_floats):
    from set_amd import _lib
    a = _lib.SetDiffnetLayersBf16Args()
    a.x_in, a.x_out, a.skip, a.cond, a.dstep, a.img = x, xo, skip, cond, dstep, img
    a.b_dil, a.b_cond, a.b_out, a.scratch, a.scratch_floats = bd, bc, bo, scratch, scratch_floats
    a.d_bs, a.d_cs, a.d_ls = FC * c["d_cs"] + c["d_pad"], c["d_cs"], d_ls
    a.B, a.T, a.l0, a.nl, a.dilation_cycle_length, a.first = c["B"], c["T"], c["l0"], c["nl"], c["dcl"], c["first"]
    return a


def _set_tile_env(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("SET_AMD_BF16_FUSE_TILE", raising=False)
    else:
        monkeypatch.setenv("SET_AMD_BF16_FUSE_TILE", env)


@pytest.mark.parametrize("c", LAYERS, ids=[c["name"] for c in LAYERS])
def test_layer_group_equals_per_layer_launches_bit_for_bit(dev, monkeypatch, c):
    """set_diffnet_layers_fwd_bf16 promises x and the skip sum bit-identical to nl set_diffnet_layer_fwd_bf16 launches: both run here on
    the same images (packed by ONE set_pack_diffnet_layers_bf16 launch), the same Gaussian operands and a dstep counted from layer 0 of
    the network.  The scratch is exactly set_diffnet_layers_bf16_scratch_floats long inside sentinels; 64-frame tiles leave it alone."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    r = layers_launch(c, n_cu)
    assert r["rc"] == 0 and r["branch"] == c["branch"]
    B, T, l0, nl, dcl = c["B"], c["T"], c["l0"], c["nl"], c["dcl"]
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]))
    lay = [_gauss_layer(g) for _ in range(nl)]
    cat = lambda k: _ro(dev, torch.stack([l[k] for l in lay]))
    wd, wc, wo, bd, bc, bo = (cat(k) for k in ("Wd", "Wc", "Wo", "bd", "bc", "bo"))
    img = Buf(dev, "u16", nl * N_IMG)
    assert _L().set_pack_diffnet_layers_bf16(wd[0].data_ptr(), wc[0].data_ptr(), wo[0].data_ptr(), 512 * FC * 3, 512 * FH, 512 * FC, img.ptr, nl, _s()) == 0
    x0, cond = _ro(dev, torch.randn(B, FC, T, generator=g)), _ro(dev, torch.randn(B, FH, T, generator=g))
    skip0 = "nan" if c["first"] else torch.randn(B, FC, T, generator=g)
    d_bs, d_cs = FC * c["d_cs"] + c["d_pad"], c["d_cs"]
    d_ls = B * d_bs + c["d_lpad"]
    ds = _dstep(dev, torch.randn(l0 + nl, B, FC, generator=g) * 0.3, d_bs, d_cs, l0 + nl, d_ls)
    torch.cuda.synchronize()
    img.before = img.d.cpu().clone()
    # ---- nl per-layer launches
    cur, sk_ref = x0[0], Buf(dev, "f32", B * FC * T, skip0)
    for m in range(nl):
        nxt = Buf(dev, "f32", B * FC * T)
        a = _fwd_args(B, T, 1 << ((l0 + m) % dcl), int(bool(c["first"]) and m == 0), cur.data_ptr() if torch.is_tensor(cur) else cur.ptr, nxt.ptr, sk_ref.ptr,
                      cond[0].data_ptr(), ds[0].data_ptr() + 4 * (l0 + m) * d_ls, d_bs, d_cs, img.ptr + 2 * m * N_IMG, bd[0].data_ptr() + 4 * 512 * m,
                      bc[0].data_ptr() + 4 * 512 * m, bo[0].data_ptr() + 4 * 512 * m)
        assert _L().set_diffnet_layer_fwd_bf16(C.byref(a), _s()) == 0
        cur = nxt
    x_ref = cur
    # ---- one launch
    n_ws = _L().set_diffnet_layers_bf16_scratch_floats(B, T, l0, nl, dcl)
    assert n_ws == layers_scratch_floats(B, T, l0, nl, dcl) >= max(r["need"], 1)
    ws = Buf(dev, "f32", n_ws)
    xo, sk = Buf(dev, "f32", B * FC * T), Buf(dev, "f32", B * FC * T, skip0)
    _set_tile_env(monkeypatch, c["env"])
    a = _layers_args(c, x0[0].data_ptr(), xo.ptr, sk.ptr, cond[0].data_ptr(), ds[0].data_ptr(), d_ls, img.ptr, bd[0].data_ptr(), bc[0].data_ptr(),
                     bo[0].data_ptr(), ws.ptr, n_ws)
    assert _L().set_diffnet_layers_fwd_bf16(C.byref(a), _s()) == 0
    torch.cuda.synchronize()
    for what, got, ref in (("x", xo, x_ref), ("skip", sk, sk_ref)):
        bad = (got.bits() != ref.bits()).nonzero().flatten()
        assert bad.numel() == 0, (c["name"], what, "first differing buffer elements (view starts at %d, frame = (i - %d) %% T)" % (GUARD, GUARD),
                                  bad[:8].tolist(), got.d.cpu()[bad[:8]].tolist(), ref.d.cpu()[bad[:8]].tolist())
        assert bool(torch.isfinite(got.view()).all())
        h = got.d.cpu()
        assert bool((h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all())
    h = ws.d.cpu()
    assert bool((h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all()), "scratch guards"
    if r["tile"] == 64:
        ws.check("scratch of a 64-frame launch")
    else:
        assert bool((h[GUARD + r["need"]:] == SENTINEL).all()), "scratch beyond what the launch asks for"
        used, written = h[GUARD:GUARD + r["need"]].numpy(), layers_scratch_written(c, r)
        assert not (used[~written] != SENTINEL).any(), ("scratch written outside the modelled set", np.nonzero((used != SENTINEL) & ~written)[0][:8].tolist())
        assert not (used[written] == SENTINEL).any() and np.isfinite(used[written]).all(), "scratch: a parked skip row is missing"
    _unchanged([x0, cond, ds, wd, wc, wo, bd, bc, bo])
    img.check("images after the launches")
    _line("layers_t%d_%s" % c["branch"], c["name"], "identical")


@pytest.mark.parametrize("row", LAYERS_REFUSED, ids=[r[0] for r in LAYERS_REFUSED])
def test_layer_group_refusals_write_nothing(dev, monkeypatch, row):
    name, kw, code, why = row
    c = dict(B=1, T=40, l0=0, first=1, d_cs=1, d_pad=0)
    c.update(kw)
    B, T = c["B"], c["T"]
    n_ws = max(layers_scratch_floats(B, T, 0, 2, 1), 64)
    ws, xo, sk = Buf(dev, "f32", n_ws), Buf(dev, "f32", B * FC * T), Buf(dev, "f32", B * FC * T)
    r, _ = _ro(dev, torch.zeros(17 * 1024))
    img = Buf(dev, "u16", 17 * N_IMG, np.zeros(17 * N_IMG, dtype=np.uint16))  # (sized for 17 layers, should a form be admitted after all)
    _set_tile_env(monkeypatch, c["env"])
    short = 1 if c.get("scratch_short") else 0
    if short:
        assert layers_launch(dict(c, scratch_short=False))["need"] == n_ws
    a = _layers_args(c, r.data_ptr(), r.data_ptr() if c.get("alias") else xo.ptr, sk.ptr, r.data_ptr(), r.data_ptr(), FC, img.ptr, r.data_ptr(), r.data_ptr(),
                     r.data_ptr(), ws.ptr, n_ws - short)
    assert _L().set_diffnet_layers_fwd_bf16(C.byref(a), _s()) == code, name
    torch.cuda.synchronize()
    for b in (ws, xo, sk, img):
        b.check(name)


# ------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------
def _bwd_args(B, T, dil, dcond_first, dxo, dskip, y16, img, dx, dy16, do16, dcond, pdbo, pdby, pdd):
    from set_amd import _lib
    a = _lib.SetDiffnetLayerBf16BwdArgs()
    a.dx_out, a.dskip, a.y16, a.img, a.dx, a.dy16, a.do16, a.dcond = dxo, dskip, y16, img, dx, dy16, do16, dcond
    a.part_dbo, a.part_dby, a.part_dd = pdbo, pdby, pdd
    a.B, a.T, a.dil, a.dcond_first = B, T, dil, dcond_first
    return a


DX_FORMS = {}


@pytest.mark.parametrize("c", BWD, ids=[c["name"] for c in BWD])
def test_layer_backward_exact(dev, c):
    """Stands on test_gate_preconditions (sigmoid(0) = 1/2, tanh(0) = 0, sigmoid(40) = 1, tanh(+-40) = +-1 on the device): with the
    class-coded y16 the gate derivative is 0, +-1/4 or 1/2 and every sum is exact, so d_o16, dy16, dcond, the three partial-sum arrays
    (tiles per utterance = set_diffnet_layer_bwd_bf16_tiles, the rows of a tile partly beyond T included) and dx must equal the model
    bit for bit.  dx = dxd + dx_out * RSQRT2 may be one fused or two rounded operations: either is accepted for the whole tensor and
    printed; with dx_out = NULL there is only one.  dcond_first = 1 runs over a NaN-filled dcond."""
    o = make_backward_exact(c)
    B, T, dil = c["B"], c["T"], c["dil"]
    tiles = _L().set_diffnet_layer_bwd_bf16_tiles(T, dil)
    assert tiles == bwd_tiles(T, dil)
    img = _pack_one(dev, o["Wd"], o["Wc"], o["Wo"])
    ins = [_ro(dev, o["dskip"])] + ([_ro(dev, o["dxo"])] if c["dxo"] else [])
    y16 = Buf(dev, "u16", B * 512 * T, q4(o["y16"]))
    dx, dy16, do16 = Buf(dev, "f32", B * FC * T), Buf(dev, "u16", B * 512 * T), Buf(dev, "u16", B * 512 * T)
    dcond = Buf(dev, "f32", B * FH * T, "nan" if c["dcond_first"] else o["dcond0"])
    pdbo, pdby, pdd = Buf(dev, "f32", B * tiles * 512), Buf(dev, "f32", B * tiles * 512), Buf(dev, "f32", B * tiles * FC)
    a = _bwd_args(B, T, dil, c["dcond_first"], ins[1][0].data_ptr() if c["dxo"] else None, ins[0][0].data_ptr(), y16.ptr, img.ptr, dx.ptr, dy16.ptr,
                  do16.ptr, dcond.ptr, pdbo.ptr, pdby.ptr, pdd.ptr)
    assert _L().set_diffnet_layer_bwd_bf16(C.byref(a), _s()) == 0
    torch.cuda.synchronize()
    _unchanged(ins)
    y16.check("y16 is an input")
    img.check("image after the launch")
    # dx_out = NULL: the first 256 channels of d_o are zeros of either sign (the kernel multiplies the dskip rows it loads in their place by 0.0f)
    do16.check(c["name"] + " do16", q4(o["do16"]), either_zero=not c["dxo"])
    dy16.check(c["name"] + " dy16", q4(o["dy16"]))
    pdbo.check(c["name"] + " part_dbo", o["part_dbo"])
    pdby.check(c["name"] + " part_dby", o["part_dby"])
    dcond.check(c["name"] + " dcond", o["dcond"])
    pdd.check(c["name"] + " part_dd", o["part_dd"])
    got = dx.bits()
    form = "separate" if torch.equal(got, dx.want_bits(o["dx_sep"])) else "fused" if torch.equal(got, dx.want_bits(o["dx_fma"])) else None
    if form is None:
        dx.check(c["name"] + " dx (neither evaluation; shown against the separately rounded one)", o["dx_sep"])
    if c["dxo"] and not torch.equal(o["dx_sep"], o["dx_fma"]):
        DX_FORMS[c["name"]] = form
        print("DXEVALUATION case=%s dx = dxd + dx_out * RSQRT2 is evaluated %s" % (c["name"], form))
        assert len(set(DX_FORMS.values())) == 1, DX_FORMS  # one build, one evaluation
    _line("layer_bwd_" + "_".join(c["branch"]), c["name"], "exact")


@pytest.mark.parametrize("c", BWD, ids=[c["name"] for c in BWD])
def test_layer_backward_bounded(dev, c):
    """Stage by stage at both scales: d_o16 bit for bit, dy16 inside its admissible set, dx, dcond, part_dby and part_dd within the
    summation bounds of the model fed with the kernel's own dy16, part_dbo within that of the model's d_o16."""
    B, T, dil = c["B"], c["T"], c["dil"]
    tiles = bwd_tiles(T, dil)
    worst = 0.0
    for k in range(len(SCALES)):
        o = make_backward_bounded(c, k)
        img = _pack_one(dev, o["Wd"], o["Wc"], o["Wo"])
        ins = [_ro(dev, o["dskip"])] + ([_ro(dev, o["dxo"])] if c["dxo"] else [])
        y16 = Buf(dev, "u16", B * 512 * T, q4(o["y16"]))
        dx, dy16, do16 = Buf(dev, "f32", B * FC * T), Buf(dev, "u16", B * 512 * T), Buf(dev, "u16", B * 512 * T)
        dcond = Buf(dev, "f32", B * FH * T, "nan" if c["dcond_first"] else o["dcond0"])
        parts = dict(part_dbo=Buf(dev, "f32", B * tiles * 512), part_dby=Buf(dev, "f32", B * tiles * 512), part_dd=Buf(dev, "f32", B * tiles * FC))
        a = _bwd_args(B, T, dil, c["dcond_first"], ins[1][0].data_ptr() if c["dxo"] else None, ins[0][0].data_ptr(), y16.ptr, img.ptr, dx.ptr, dy16.ptr,
                      do16.ptr, dcond.ptr, parts["part_dbo"].ptr, parts["part_dby"].ptr, parts["part_dd"].ptr)
        assert _L().set_diffnet_layer_bwd_bf16(C.byref(a), _s()) == 0
        torch.cuda.synchronize()
        _unchanged(ins)
        y16.check("y16 is an input")
        img.check("image after the launch")
        what = "%s/%d" % (c["name"], k)
        do16.check(what + " do16", q4(o["do16"]), either_zero=not c["dxo"])
        dybits = _in_sets(dy16, what + " dy16", B, 512, T, o["dy_lo"], o["dy_hi"])
        w = backward_from_dy(o, dybits)
        fr = {n: _within(b, what + " " + n, *w[n]) for n, b in dict(parts, dx=dx, dcond=dcond).items()}
        print(what, " ".join("%s %.3f" % kv for kv in sorted(fr.items())))
        worst = max(worst, *fr.values())
    _line("layer_bwd_" + "_".join(c["branch"]), c["name"], "bounded", worst)


@pytest.mark.parametrize("name,kw", BWD_REFUSED, ids=[n for n, _ in BWD_REFUSED])
def test_layer_backward_refusals_write_nothing(dev, name, kw):
    B, T = 1, 40
    r, _ = _ro(dev, torch.zeros(B * 512 * T))
    img = Buf(dev, "u16", N_IMG, np.zeros(N_IMG, dtype=np.uint16))
    outs = dict(dx=Buf(dev, "f32", B * FC * T), dy16=Buf(dev, "u16", B * 512 * T), do16=Buf(dev, "u16", B * 512 * T), dcond=Buf(dev, "f32", B * FH * T),
                part_dbo=Buf(dev, "f32", 512), part_dby=Buf(dev, "f32", 512), part_dd=Buf(dev, "f32", FC))
    p = {k: v.ptr for k, v in outs.items()}
    p.update(dskip=r.data_ptr(), y16=r.data_ptr())
    if kw.get("missing"):
        p[kw["missing"]] = None
    a = _bwd_args(B, T, kw.get("dil", 1), 0, r.data_ptr(), p["dskip"], p["y16"], img.ptr, p["dx"], p["dy16"], p["do16"], p["dcond"], p["part_dbo"],
                  p["part_dby"], p["part_dd"])
    assert _L().set_diffnet_layer_bwd_bf16(C.byref(a), _s()) == E_INVALID, name
    torch.cuda.synchronize()
    for b in outs.values():
        b.check(name)


# ------------------------------------------------------------------------------------------------------------------------
# reductions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", RED_ROWS)
def test_partial_rows_sum_is_exact_on_integers(dev, rows):
    """out[g][j] (+)= scale * sum_r part[(g rows + r) cols + j]: integer partials, power-of-two scales, bit for bit against float64."""
    for cols in RED_COLS:
        for groups, acc, scale in ((1, 0, 0.5), (3, 1, 2.0), (3, 0, 1.0), (1, 1, 0.25)):
            part = int_partials(rows * 1000 + cols + groups, (groups, rows, cols))
            pd = _ro(dev, part)
            old = int_partials(7 + cols, (groups, cols), 8)
            out = Buf(dev, "f32", groups * cols, old)
            assert _L().set_partial_rows_sum(pd[0].data_ptr(), out.ptr, groups, rows, cols, acc, scale, _s()) == 0
            torch.cuda.synchronize()
            out.check("rows %d cols %d groups %d acc %d" % (rows, cols, groups, acc), part.double().sum(1) * scale + (old.double() if acc else 0.0))
            _unchanged([pd])
    _line("partial_rows_sum", "rows%d" % rows, "exact")


def _reduce_case(dev, B, tiles, L_, single, gauss=False, seed=0):
    """One set_diffnet_layer(s)_bwd_reduce call; returns the target buffers, their float64 models and the sums of magnitudes."""
    g = torch.Generator().manual_seed(seed)
    mk = (lambda shape: torch.randn(shape, generator=g)) if gauss else (lambda shape: torch.randint(-64, 65, shape, generator=g).float())
    pdbo, pdby, pdd = mk((L_, B * tiles, 512)), mk((L_, B * tiles, 512)), mk((L_, B, tiles, FC))
    ps = [_ro(dev, t) for t in (pdbo, pdby, pdd)]
    s_out, s_dil, s_cond, dd_ls = (0, 0, 0, 0) if single else (512 + 40, 512 + 1, 1024, FC + 2)
    dd_bs = FC + 9 if single else L_ * dd_ls + 5
    tg = []
    for s in (s_out, s_dil, s_cond):
        old = mk(((L_ - 1) * s + 512,))
        tg.append((Buf(dev, "f32", old.numel(), old), old, s))
    dd_old = mk(((L_ - 1) * dd_ls + (B - 1) * dd_bs + FC,))
    dd = Buf(dev, "f32", dd_old.numel(), dd_old)
    if single:
        rc = _L().set_diffnet_layer_bwd_reduce(ps[0][0].data_ptr(), ps[1][0].data_ptr(), ps[2][0].data_ptr(), B, tiles, tg[0][0].ptr, tg[1][0].ptr,
                                               tg[2][0].ptr, dd.ptr, dd_bs, _s())
    else:
        rc = _L().set_diffnet_layers_bwd_reduce(ps[0][0].data_ptr(), ps[1][0].data_ptr(), ps[2][0].data_ptr(), B, tiles, L_, tg[0][0].ptr, s_out,
                                                tg[1][0].ptr, s_dil, tg[2][0].ptr, s_cond, dd.ptr, dd_bs, dd_ls, _s())
    assert rc == 0
    torch.cuda.synchronize()
    _unchanged(ps)
    wants, mags = [], []
    for (buf, old, s), part in zip(tg, (pdbo, pdby, pdby)):  # db_* ACCUMULATE
        w, m = old.double().clone(), old.double().abs()
        for q in range(L_):
            w[q * s:q * s + 512] += part[q].double().sum(0)
            m[q * s:q * s + 512] += part[q].double().abs().sum(0)
        wants.append(w)
        mags.append(m)
    w, m = dd_old.double().clone(), torch.zeros(dd_old.numel(), dtype=torch.float64)
    for q in range(L_):
        for b in range(B):  # dd is WRITTEN
            w[q * dd_ls + b * dd_bs:q * dd_ls + b * dd_bs + FC] = pdd[q, b].double().sum(0)
            m[q * dd_ls + b * dd_bs:q * dd_ls + b * dd_bs + FC] = pdd[q, b].double().abs().sum(0)
    return [t[0] for t in tg] + [dd], wants + [w], mags + [m]


@pytest.mark.parametrize("tiles", RED_ROWS)
def test_layer_bwd_reduce_is_exact_on_integers(dev, tiles):
    """db_out, db_dil, db_cond ACCUMULATE onto non-zero targets, dd is WRITTEN over non-zero values; nothing else in the buffers changes.
    One layer (both entry points) and L = 3 with target strides larger than 512 and a dd_ls stride."""
    for B in (1, 3):
        for L_, single in ((1, True), (1, False), (3, False)):
            bufs, wants, _ = _reduce_case(dev, B, tiles, L_, single, seed=tiles * 10 + B)
            for i, (b, w) in enumerate(zip(bufs, wants)):
                b.check("tiles %d B %d L %d single %d target %d" % (tiles, B, L_, single, i), w)
    _line("layer_bwd_reduce", "tiles%d" % tiles, "exact")


def test_reductions_on_gaussians_are_within_the_ordered_sum_bound_and_bit_stable(dev):
    worst = 0.0
    for single, L_ in ((True, 1), (False, 3)):
        runs = []
        for _ in range(2):
            bufs, wants, mags = _reduce_case(dev, 3, 37, L_, single, gauss=True, seed=3)
            runs.append([b.bits().clone() for b in bufs])
            for b, w, m in zip(bufs, wants, mags):
                got = b.d.cpu()[GUARD:GUARD + b.n].double()
                bar = gamma(3 * 37 + ROWS_RG + 4) * m  # rows of one chain + the chain and group sums + the accumulate
                d = (got - w).abs()
                assert bool((d <= bar).all()), float((d / (bar + 1e-300)).max())
                worst = max(worst, float((d / (bar + 1e-300))[bar > 0].max()))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
    g = torch.Generator().manual_seed(4)
    part = torch.randn(3, 37, 200, generator=g)
    pd, old = _ro(dev, part), torch.randn(3, 200, generator=g)
    outs = []
    for _ in range(2):
        out = Buf(dev, "f32", 600, old)
        assert _L().set_partial_rows_sum(pd[0].data_ptr(), out.ptr, 3, 37, 200, 1, 0.7, _s()) == 0
        torch.cuda.synchronize()
        outs.append(out.bits().clone())
        want = part.double().sum(1) * float(np.float32(0.7)) + old.double()
        bar = gamma(37 + ROWS_RG + 6) * (part.double().abs().sum(1) * 0.7 + old.double().abs())
        d = (out.view().double().reshape(3, 200) - want).abs()
        assert bool((d <= bar).all())
        worst = max(worst, float((d / bar).max()))
    assert torch.equal(outs[0], outs[1])
    _line("reductions", "gaussian", "bounded", worst)
