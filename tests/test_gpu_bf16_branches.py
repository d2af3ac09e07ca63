"""GPU branch sweep of the bf16-operand conv family (csrc/bf16.hip): the forward / input-gradient kernels behind set_conv1d with
impl = SET_IMPL_BF16 (the one-shot 1x1 kernels, the staged kernel in both stage shapes, both tile shapes, both tap-group sizes and
both input staging forms), the weight-gradient kernels behind set_conv1d_wgrad_det / set_conv1d_wgrad_det_grouped (one tap per
block, three taps in three copies / one copy, all taps; the ordered reduce) and the two pack kernels.  ONE raw ABI call per case
against the float64 model of tests/test_bf16_reference.py, which also holds the case tables: each case names the kernel instance
it reaches and the C condition it satisfies, and CPU tests pin that against Python mirrors of the launch code.

Two assertions per case:
  exact    rounding probes (10 significant bits in one operand, small integers in the other; power-of-two parameters): every partial
           sum in any order is an fp32 number (budget asserted on the CPU), so the kernel must equal the model BIT FOR BIT -- which
           pins the rounding contract (prologue in fp32, then one round-to-nearest-even) besides every index, chunk walk and tap offset.
  bounded  Gaussian operands at two scales; every element within conv_bound() evaluated on the rounded operands (the derived bar of
           the fp32 sweeps: the products are exact in fp32, what is left is fp32 summation).
out, res, dW, the scratch and the packed image are views inside larger sentinel-filled buffers; the WHOLE buffer is compared: the
model's written set against the model, everything else against what was there.  Inputs are checked unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_bf16_reference import (DTYPE_CODE, FWD, GROUPED, PACK, REFUSED, SCALES, WGRAD, make_forward, make_wgrad, mfma_exactness_case,
                                 pack_bf16_image, pack_operands, q4, up, wgrad_bf16_branch, wgrad_slice_models)
from test_conv_reference import gamma, weight_view

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
IMG_SENTINEL = 0x5A5A
E_UNSUPPORTED, E_INVALID = -2, -1
PRO_CODE = {"none": 0, "lrelu": 1, "div": 2}
GUARD = 64


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_ALIVE = []  # device tensors whose raw address went to a launch


@pytest.fixture(autouse=True)
def _keep_launch_operands():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _p(t, byte_off=0):
    if t is None:
        return None
    _ALIVE.append(t)
    return t.data_ptr() + byte_off


def _L():
    from set_amd import _lib
    return _lib.lib()


def _s():
    from set_amd.ops import _stream
    return _stream()


def _u16(dev, arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint16).view(np.int16).copy()).to(dev)


def _line(family, name, mode, frac):
    print("BF16SWEEP family=%s case=%s mode=%s worst_fraction_of_bar=%.4f" % (family, name, mode, frac))


# ------------------------------------------------------------------------------------------------------------------------
# pack
# ------------------------------------------------------------------------------------------------------------------------
def _pack(dev, wd, addr, Cout, Cin, K, W_view):
    """set_pack_conv_weight_bf16 into a guarded buffer, compared whole with the model; returns (buffer, byte offset of the image)."""
    size = _L().set_packed_conv_weight_bf16_size(Cout, Cin, K)
    want = np.full(size + 2 * GUARD, IMG_SENTINEL, dtype=np.uint16)
    want[GUARD:GUARD + size] = pack_bf16_image(W_view, Cout, Cin, K, size)
    buf = _u16(dev, np.full(size + 2 * GUARD, IMG_SENTINEL, dtype=np.uint16))
    rc = _L().set_pack_conv_weight_bf16(_p(wd), _p(buf, 2 * GUARD), Cout, Cin, K, addr["base"], addr["sco"], addr["sci"], addr["stap"], _s())
    assert rc == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("packed image", bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    return buf, 2 * GUARD


_PACK_IDS = ["%d_%d_%d_%s" % (c[0], c[1], c[2], c[3] if isinstance(c[3], str) else "phase") for c in PACK]


@pytest.mark.parametrize("case", PACK, ids=_PACK_IDS)
def test_pack_kernel_writes_the_modelled_image_and_nothing_else(dev, case):
    Cout, Cin, K, _ = case
    store, addr = pack_operands(case)
    wd = store.to(dev)
    _pack(dev, wd, addr, Cout, Cin, K, weight_view(store, Cout, Cin, K, **addr))
    assert torch.equal(wd.cpu(), store)


def test_batch_pack_writes_the_same_images(dev):
    from set_amd import _lib
    arr = (_lib.SetPackDesc * len(PACK))()
    bufs, wants, keep, start = [], [], [], 0
    for d, case in zip(arr, PACK):
        Cout, Cin, K, _ = case
        store, addr = pack_operands(case, seed=1)
        wd = store.to(dev)
        size = _L().set_packed_conv_weight_bf16_size(Cout, Cin, K)
        want = np.full(size + 2 * GUARD, IMG_SENTINEL, dtype=np.uint16)
        want[GUARD:GUARD + size] = pack_bf16_image(weight_view(store, Cout, Cin, K, **addr), Cout, Cin, K, size)
        buf = _u16(dev, np.full(size + 2 * GUARD, IMG_SENTINEL, dtype=np.uint16))
        d.w, d.wp = _p(wd), _p(buf, 2 * GUARD)
        d.w_base, d.w_sco, d.w_sci, d.w_stap, d.start = addr["base"], addr["sco"], addr["sci"], addr["stap"], start
        d.Cout, d.Cin, d.K = Cout, Cin, K
        assert _L().set_fill_pack_desc(C.byref(d), _lib.IMG_BF16, 0) == size and (d.CoutP, d.CinP) == (up(Cout, 128), up(Cin, 32))
        start += size
        bufs.append(buf)
        wants.append(want)
        keep.append((wd, store))
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    assert _L().set_pack_conv_weights_batch(C.c_void_p(_p(raw)), len(PACK), start, _s()) == 0
    torch.cuda.synchronize()
    for buf, want, (wd, store), case in zip(bufs, wants, keep, PACK):
        assert np.array_equal(buf.cpu().numpy().view(np.uint16), want), case
        assert torch.equal(wd.cpu(), store)


def test_one_table_mixes_the_three_image_kinds(dev):
    """set_pack_conv_weights_batch over ONE table that holds an fp32 small-tile, an fp32 big-tile and a bf16 image (4- and 2-byte elements
    behind one `start` search, in elements): each image bit-equal to what its per-image entry writes, nothing written outside the images
    (both go into poisoned buffers with guards on either side, compared whole)."""
    from set_amd import _lib
    L, g, guard = _L(), torch.Generator().manual_seed(9), 256  # guard bytes
    bf = min((c for c in PACK if c[0] % 128 or c[1] % 32), key=lambda c: L.set_packed_conv_weight_bf16_size(*c[:3]))  # smallest ragged one
    bf_store, bf_addr = pack_operands(bf, seed=2)
    cases = [  # kind, Cout, Cin, K, dil, raw weight, addressing, bytes per element
        (_lib.IMG_F32, 7, 20, 3, 0, torch.randn(7, 20, 3, generator=g), dict(base=0, sco=60, sci=3, stap=1), 4),
        (_lib.IMG_F32_BIG, 130, 100, 3, -17, torch.randn(100, 130, 3, generator=g), dict(base=0, sco=3, sci=130 * 3, stap=1), 4),  # transposed
        (_lib.IMG_BF16, bf[0], bf[1], bf[2], 0, bf_store, bf_addr, 2),
    ]
    arr = (_lib.SetPackDesc * len(cases))()
    pairs, start = [], 0
    for d, (kind, Cout, Cin, K, dil, w, addr, esz) in zip(arr, cases):
        wd = w.to(dev)
        d.w, d.w_base, d.w_sco, d.w_sci, d.w_stap, d.start = _p(wd), addr["base"], addr["sco"], addr["sci"], addr["stap"], start
        d.Cout, d.Cin, d.K = Cout, Cin, K
        n = L.set_fill_pack_desc(C.byref(d), kind, dil)
        assert n > 0
        got, ref = (torch.full((n * esz + 2 * guard,), 0x5A, dtype=torch.uint8, device=dev) for _ in range(2))
        d.wp = _p(got, guard)
        a = (addr["base"], addr["sco"], addr["sci"], addr["stap"], _s())
        if kind == _lib.IMG_F32:
            assert L.set_packed_conv_weight_size(Cout, Cin, K) == n and L.set_pack_conv_weight(_p(wd), _p(ref, guard), Cout, Cin, K, *a) == 0
        elif kind == _lib.IMG_F32_BIG:
            assert L.set_packed_conv_weight_v2_size(Cout, Cin, K) == n and L.set_pack_conv_weight_v2(_p(wd), _p(ref, guard), Cout, Cin, K, dil, *a) == 0
        else:
            assert L.set_packed_conv_weight_bf16_size(Cout, Cin, K) == n and L.set_pack_conv_weight_bf16(_p(wd), _p(ref, guard), Cout, Cin, K, *a) == 0
        pairs.append((got, ref, n * esz, kind))
        start += n
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    assert L.set_pack_conv_weights_batch(C.c_void_p(_p(raw)), len(cases), start, _s()) == 0
    torch.cuda.synchronize()
    for got, ref, nbytes, kind in pairs:
        for buf in (got, ref):  # guards untouched, the image written (a zero-padded image of nonzero weights is not the poison)
            assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + nbytes:] == 0x5A).all()), kind
            assert not bool((buf[guard:guard + nbytes] == 0x5A).all()), kind
        assert torch.equal(got, ref), kind


# ------------------------------------------------------------------------------------------------------------------------
# forward / input gradient
# ------------------------------------------------------------------------------------------------------------------------
def _run_forward(o, dev, monkeypatch):
    """One set_conv1d(impl = SET_IMPL_BF16) call on fresh device copies; returns the whole out buffer."""
    from set_amd import _lib
    if o["units"] is None:
        monkeypatch.delenv("SET_AMD_CONV_BF16_UNITS", raising=False)
    else:
        monkeypatch.setenv("SET_AMD_CONV_BF16_UNITS", o["units"])
    B, Cin, T_in = o["x"].shape
    Cout, K = o["Cout"], o["K"]
    bs, cs, off = o["x_emb"] if o["x_emb"] is not None else (Cin * T_in, T_in, 0)
    x_buf = torch.full((GUARD + off + (B - 1) * bs + (Cin - 1) * cs + T_in + GUARD,), 99.0)  # 99 around the view: a read outside it shows
    x_buf.as_strided((B, Cin, T_in), (bs, cs, 1), GUARD + off).copy_(o["x"])
    xd = x_buf.to(dev)
    add_buf = add_d = None
    if o["add_t"] is not None:
        add_buf = torch.full((4 + o["add_off"] + B * Cin + 4,), 99.0)
        add_buf[4 + o["add_off"]:4 + o["add_off"] + B * Cin] = o["add_t"].reshape(-1)
        add_d = add_buf.to(dev)
    wd = o["wstore"].to(dev)
    img, img_off = _pack(dev, wd, o["waddr"], Cout, Cin, K, o["W"])
    t = lambda v: None if v is None else v.to(dev)
    bias, mask = t(o["bias_t"]), t(o["mask_t"])
    out_buf, res_buf = o["out_buf"].to(dev), t(o["res_buf"])
    out = o["out_view"](out_buf)
    res = None if res_buf is None else o["res_view"](res_buf)
    kw = o["kw"]
    a = _lib.SetConv1dArgs()
    a.inp = _p(xd, 4 * (GUARD + off))
    a.w = _p(img, img_off)
    a.bias, a.mask = _p(bias), _p(mask)
    a.in_chan_add = None if add_d is None else _p(add_d, 4 * (4 + o["add_off"]))
    _ALIVE.extend([out_buf, res_buf])
    a.out = out.data_ptr()
    a.res = None if res is None else res.data_ptr()
    a.in_bs, a.in_cs = bs, cs
    a.out_bs, a.out_cs = out.stride(0), out.stride(1)
    if res is not None:
        a.res_bs, a.res_cs = res.stride(0), res.stride(1)
    wa = o["waddr"]
    a.w_base, a.w_sco, a.w_sci, a.w_stap = wa["base"], wa["sco"], wa["sci"], wa["stap"]
    a.B, a.Cin, a.Cout, a.K, a.dil, a.pad = B, Cin, Cout, K, kw["dil"], kw["pad"]
    a.T_in, a.T_iter, a.T_out, a.out_stride, a.out_off = T_in, kw["T_iter"], kw["T_out"], 1, 0
    a.pro, a.act, a.accumulate, a.impl = _lib.PRO[o["pro"]], _lib.ACT[kw["act"]], int(kw["accumulate"]), _lib.IMPL_BF16
    a.pro_param, a.act_param, a.alpha, a.out_div = o["pro_param"], kw["act_param"], kw["alpha"], kw["out_div"]
    _lib.check(_L().set_conv1d(C.byref(a), _s()), "set_conv1d")
    torch.cuda.synchronize()
    # operands are read-only
    assert torch.equal(xd.cpu(), x_buf) and torch.equal(wd.cpu(), o["wstore"])
    assert add_d is None or torch.equal(add_d.cpu(), add_buf)
    assert res_buf is None or torch.equal(res_buf.cpu(), o["res_buf"])
    assert bias is None or torch.equal(bias.cpu(), o["bias_t"])
    assert mask is None or torch.equal(mask.cpu(), o["mask_t"])
    return out_buf.cpu()


def _compare(name, family, mode, got, want, bar):
    d = (got.double() - want).abs()
    bad = (~(d <= bar)).nonzero().flatten()  # (a NaN is outside any bar)
    frac = float((d / (bar + 1e-300))[bar > 0].max()) if bool((bar > 0).any()) else 0.0
    print("%s: max |d| %.3e, %d of %d buffer elements outside" % (name, float(d.max()), bad.numel(), d.numel()))
    _line(family, name, mode, frac)
    assert bad.numel() == 0, (name, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert bool(torch.isfinite(got).all())


FWD_RUNS = [(i, c, mode) for i, c in enumerate(FWD) for mode in c["modes"]]


@pytest.mark.parametrize("i,c,mode", FWD_RUNS, ids=["%s-%s" % (c["name"], mode) for _, c, mode in FWD_RUNS])
def test_conv_bf16_forward_branch(dev, monkeypatch, i, c, mode):
    for scale in ((0,) if mode == "exact" else range(len(SCALES))):
        o = make_forward(c, mode, scale, i)
        assert 0 < o["written"] <= c["B"] * c["Cout"] * c["T_out"]
        got = _run_forward(o, dev, monkeypatch)
        # exact: the bar is zero everywhere; bounded: zero outside the model's written set
        _compare("%s/%d" % (c["name"], scale), "conv_" + "_".join(str(v) for v in c["branch"]), mode, got, o["want"], o["bar"])


def test_bf16_mfma_adds_exact_products_and_the_accumulator_without_loss(dev, monkeypatch):
    """What the exact mode rests on: v_mfma_f32_32x32x16_bf16 returns the exact sum whenever every partial result is an fp32 number.
    The deciding case (tests/test_bf16_reference.py, mfma_exactness_case): one product of one granule, of either sign, against
    2^24 - 2 granules -- inside one MFMA, in the next MFMA of the stage, in the next stage."""
    x, W, want = mfma_exactness_case()
    c = dict(FWD[0], name="mfma_exact", B=1, Cin=64, Cout=8, K=3, dil=1, pad=1, T_in=8, T_out=8, T_iter=8)
    o = dict(c, x=x, add_t=None, wstore=W, W=W, waddr=dict(base=0, sco=192, sci=3, stap=1), bias_t=None, mask_t=None, res_buf=None,
             res_view=None, out_buf=torch.full((8 * 8 + 2 * GUARD,), SENTINEL), units=None, add_off=0, x_emb=None, pro="none", pro_param=0.0,
             kw=dict(dil=1, pad=1, T_iter=8, T_out=8, act="none", act_param=0.0, alpha=1.0, accumulate=False, out_div=0.0))
    o["out_view"] = lambda b: b.as_strided((1, 8, 8), (64, 8, 1), GUARD)
    got = _run_forward(o, dev, monkeypatch)
    rows = o["out_view"](got)[0].double()
    print("rows (frame 3):", rows[:, 3].tolist(), "want", want.tolist())
    assert torch.equal(rows, want[:, None].expand(8, 8))
    assert bool((got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("name,kw", REFUSED, ids=[n for n, _ in REFUSED])
def test_conv_bf16_refuses_what_it_cannot_run_and_leaves_out_alone(dev, name, kw):
    """set_conv1d_bf16_dispatch: halo > 128, out_stride != 1, out_off != 0 -> SET_E_UNSUPPORTED before any launch."""
    from set_amd import _lib
    B, Cin, Cout, T = 1, 64, 64, 300
    K = kw["K"]
    x = torch.ones(B * Cin * T + 4096, device=dev)
    w = torch.zeros(_L().set_packed_conv_weight_bf16_size(Cout, Cin, K) // 2 + 64, device=dev)  # (2 bf16 per float)
    out = torch.full((B * Cout * T * 2 + 4096,), SENTINEL, device=dev)
    a = _lib.SetConv1dArgs()
    a.inp, a.w, a.out = _p(x), _p(w), _p(out)
    a.in_bs, a.in_cs, a.out_bs, a.out_cs = Cin * T, T, Cout * T * 2, T * 2
    a.B, a.Cin, a.Cout, a.K, a.dil, a.pad = B, Cin, Cout, K, kw["dil"], kw["pad"]
    a.T_in, a.T_iter, a.T_out, a.out_stride, a.out_off = T, T, T * 2, kw.get("out_stride", 1), kw.get("out_off", 0)
    a.impl, a.alpha = _lib.IMPL_BF16, 1.0
    assert _L().set_conv1d(C.byref(a), _s()) == E_UNSUPPORTED, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------------
def _operand(dev, op, bits):
    """Device storage of one group's operand: fp32 [B][C][T] as it is, bf16 bits through the channel-quad interleave."""
    return _u16(dev, q4(op.numpy().astype(np.uint16))) if bits else op.contiguous().reshape(-1).to(dev)


def _wgrad_call(o, dev, monkeypatch, *, grouped=False, group=None, short=0, twice=False):
    """One call (grouped: set_conv1d_wgrad_det_grouped over all groups; else set_conv1d_wgrad_det on group `group`).  Returns the whole dW
    buffer, the whole scratch buffer, (dw offset, dw group stride, scratch offset, floats the call must write, floats asked for), rc."""
    if o["units3"] is None:
        monkeypatch.delenv("SET_AMD_WGRAD3_UNITS", raising=False)
    else:
        monkeypatch.setenv("SET_AMD_WGRAD3_UNITS", o["units3"])
    B, Cin, Cout, K, T, T_in, dt = o["B"], o["Cin"], o["Cout"], o["K"], o["T"], o["T_in"], o["dtype"]
    G = o["groups"] if grouped else 1
    qs = list(range(G)) if grouped else [group or 0]
    n = Cout * Cin * K
    L = _L()
    gd = torch.cat([_operand(dev, o["g"][q], dt != "bf16") for q in qs])
    x_shared = bool(o.get("x_shared"))
    xd = torch.cat([_operand(dev, o["x"][q], dt == "gx16") for q in (qs[:1] if x_shared else qs)])
    has_add = o["adds"][qs[0]] is not None
    ad = torch.cat([o["adds"][q].reshape(-1) for q in qs]).to(dev) if has_add else None
    host = [t.cpu().clone() for t in (gd, xd)] + ([ad.cpu().clone()] if has_add else [])
    dw_gs = n + 37  # sentinels between the groups' targets
    dw_buf = torch.full((GUARD + G * dw_gs + GUARD,), SENTINEL)
    for j, q in enumerate(qs):
        dw_buf[GUARD + j * dw_gs:GUARD + j * dw_gs + n] = o["dw0"][q].reshape(-1)
    dwd = dw_buf.to(dev)
    need = L.set_conv1d_wgrad_grouped_scratch_floats(G, B, Cin, Cout, K, T) if grouped else \
        L.set_conv1d_wgrad_scratch_floats(B, Cin, Cout, K, T, DTYPE_CODE[dt])
    (_, _), S = wgrad_bf16_branch(o, G)
    scratch = torch.full((GUARD + need + GUARD,), SENTINEL, device=dev)
    for _ in range(2 if twice else 1):
        if grouped:
            rc = L.set_conv1d_wgrad_det_grouped(_p(gd), _p(xd), _p(ad), _p(dwd, 4 * GUARD), G, B * Cout * T, 0 if x_shared else B * Cin * T_in, B * Cin,
                                                dw_gs, B, Cin, Cout, K, o["dil"], o["pad"], T, T_in, DTYPE_CODE[dt], _p(scratch, 4 * GUARD),
                                                need - short, _s())
        else:
            rc = L.set_conv1d_wgrad_det(_p(gd), _p(xd), _p(ad), _p(dwd, 4 * GUARD), B, Cin, Cout, K, o["dil"], o["pad"], T, T_in, PRO_CODE[o["pro"]],
                                        o["pp"], DTYPE_CODE[dt], _p(scratch, 4 * GUARD), need - short, _s())
    torch.cuda.synchronize()
    for dv, hv in zip([gd, xd] + ([ad] if has_add else []), host):  # operands are read-only
        assert torch.equal(dv.cpu(), hv)
    return dwd.cpu(), scratch.cpu(), (GUARD, dw_gs, GUARD, G * S * n, need), rc


def _check_wgrad(o, mode, dw_buf, sc_buf, lay, qs, family, name, times=1, slices=True):
    """The whole dW buffer and the whole scratch buffer against the model."""
    off, dw_gs, s_off, written, need = lay
    B, T, n = o["B"], o["T"], o["Cout"] * o["Cin"] * o["K"]
    S = written // (n * len(qs))
    want = torch.full(dw_buf.shape, SENTINEL, dtype=torch.float64)
    bar = torch.zeros_like(want)
    for j, q in enumerate(qs):
        sl = slice(off + j * dw_gs, off + j * dw_gs + n)
        want[sl] = (o["dw0"][q].double() + times * o["dw"][q]).reshape(-1)
        if mode != "exact":
            bar[sl] = (gamma(B * T + S + 4) * (o["A"][q] + o["dw0"][q].double().abs())).reshape(-1)
    _compare(name, family, mode, dw_buf, want, bar)
    # scratch: partial[group][slice][Cout][Cin][K] from the start of the view; the rest of what the size function asked for, and the guards, untouched
    assert bool((sc_buf[:s_off] == SENTINEL).all()) and bool((sc_buf[s_off + written:] == SENTINEL).all()), "scratch outside the partial tiles"
    parts = sc_buf[s_off:s_off + written].double().reshape(len(qs), S, n)
    assert bool(torch.isfinite(parts).all())
    for j, q in enumerate(qs):
        if mode == "exact":
            if slices:
                model = wgrad_slice_models(o, q).reshape(S, n)
                bad = (parts[j] != model).nonzero()
                assert bad.shape[0] == 0, ("partial tiles", name, q, bad[:6].tolist())
            else:
                assert torch.equal(parts[j].sum(0), o["dw"][q].reshape(-1))
        else:
            d = (parts[j].sum(0) - o["dw"][q].reshape(-1)).abs()
            assert bool((d <= gamma(B * T + S + 4) * o["A"][q].reshape(-1)).all()), ("sum of the partial tiles", name, q)


def _family(branch):
    return "%s_%s" % (branch[0], "_".join(str(int(v)) if isinstance(v, bool) else str(v) for v in branch[1]))


WGRAD_RUNS = [(i, c, mode) for i, c in enumerate(WGRAD) for mode in ("exact", "bounded")]


@pytest.mark.parametrize("i,c,mode", WGRAD_RUNS, ids=["%s-%s" % (c["name"], mode) for _, c, mode in WGRAD_RUNS])
def test_wgrad_bf16_branch(dev, monkeypatch, i, c, mode):
    for scale in ((0,) if mode == "exact" or c["heavy"] else range(len(SCALES))):
        o = make_wgrad(c, mode, scale, i)
        dw_buf, sc_buf, lay, rc = _wgrad_call(o, dev, monkeypatch)
        assert rc == 0
        _check_wgrad(o, mode, dw_buf, sc_buf, lay, [0], _family(c["branch"]), "%s/%d" % (c["name"], scale))


@pytest.mark.parametrize("name", ["w3u_dil1", "wt_k5_same", "w_gx16_xu"])
def test_wgrad_bf16_adds_to_what_dw_holds_and_a_second_call_adds_again(dev, monkeypatch, name):
    i, c = next((i, c) for i, c in enumerate(WGRAD) if c["name"] == name)
    o = make_wgrad(c, "exact", 0, i)
    assert 2 * o["budget"] < 2 ** 24 and float(o["dw0"].abs().max()) > 0
    dw_buf, sc_buf, lay, rc = _wgrad_call(o, dev, monkeypatch, twice=True)
    assert rc == 0
    _check_wgrad(o, "exact", dw_buf, sc_buf, lay, [0], _family(c["branch"]), name + "/twice", times=2, slices=False)


GROUPED_RUNS = [(c, mode) for c in GROUPED for mode in ("exact", "bounded")]


@pytest.mark.parametrize("c,mode", GROUPED_RUNS, ids=["%s-%s" % (c["name"], mode) for c, mode in GROUPED_RUNS])
def test_grouped_wgrad_equals_the_model_and_the_single_calls(dev, monkeypatch, c, mode):
    """One launch over the groups (dW targets dw_gs apart, sentinels between them) against the model, and against one
    set_conv1d_wgrad_det call per group: bit for bit in exact mode; in bounded mode the two entry points plan different slice counts
    (another summation order), so both are held to the bar."""
    G = c["groups"]
    for scale in ((0,) if mode == "exact" else range(len(SCALES))):
        o = make_wgrad(c, mode, scale, GROUPED.index(c), groups=G)
        dw_buf, sc_buf, lay, rc = _wgrad_call(o, dev, monkeypatch, grouped=True)
        assert rc == 0
        _check_wgrad(o, mode, dw_buf, sc_buf, lay, list(range(G)), "grouped_" + _family(c["branch"]), "%s/%d" % (c["name"], scale))
        n = c["Cout"] * c["Cin"] * c["K"]
        for q in range(G):
            o1 = dict(o, groups=1)
            one_buf, one_sc, one_lay, rc = _wgrad_call(o1, dev, monkeypatch, group=q)
            assert rc == 0
            _check_wgrad(o1, mode, one_buf, one_sc, one_lay, [q], "single_" + _family(wgrad_bf16_branch(c)[0]), "%s/%d/group%d" % (c["name"], scale, q))
            if mode == "exact":
                assert torch.equal(one_buf[lay[0]:lay[0] + n], dw_buf[lay[0] + q * lay[1]:lay[0] + q * lay[1] + n])


WGRAD_REFUSED = [
    # name, dtype, Cin, Cout, add, pro, floats short of the scratch size, return code
    ("g16_Cout_mod4", "g16", 40, 70, False, "none", 0, E_UNSUPPORTED),
    ("gx16_Cin_mod4", "gx16", 42, 72, False, "none", 0, E_UNSUPPORTED),
    ("gx16_chan_add", "gx16", 40, 72, True, "none", 0, E_INVALID),
    ("gx16_prologue", "gx16", 40, 72, False, "lrelu", 0, E_INVALID),
    ("scratch_one_float_short", "bf16", 40, 72, False, "none", 1, E_INVALID),
]


@pytest.mark.parametrize("row", WGRAD_REFUSED, ids=[r[0] for r in WGRAD_REFUSED])
def test_wgrad_bf16_refusals_leave_dw_and_scratch_alone(dev, row):
    name, dt, Cin, Cout, add, pro, short, code = row
    B, K, T = 2, 1, 72
    L = _L()
    gd = torch.ones(B * up(Cout, 4) * T, device=dev)  # (large enough for either operand type, should a kernel be launched after all)
    xd = torch.ones(B * up(Cin, 4) * T, device=dev)
    ad = torch.ones(B * Cin, device=dev) if add else None
    dw = torch.full((Cout * Cin * K + 2 * GUARD,), SENTINEL, device=dev)
    need = L.set_conv1d_wgrad_scratch_floats(B, Cin, Cout, K, T, DTYPE_CODE[dt])
    scratch = torch.full((need + 2 * GUARD,), SENTINEL, device=dev)
    rc = L.set_conv1d_wgrad_det(_p(gd), _p(xd), _p(ad), _p(dw, 4 * GUARD), B, Cin, Cout, K, 1, 0, T, T, PRO_CODE[pro], 0.375, DTYPE_CODE[dt],
                                _p(scratch, 4 * GUARD), need - short, _s())
    torch.cuda.synchronize()
    assert rc == code, name
    assert bool((dw == SENTINEL).all()) and bool((scratch == SENTINEL).all())
