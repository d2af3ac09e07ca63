"""The discriminator step on the GPU (csrc/disc_wgrad.hip, set_amd.discriminators with trainable_) against the float64 models of
tests/disc_step_models.py.

Raw calls write into sentinel-filled guarded buffers (tests/raw_abi.py); the modules run with NaN-filled outputs and scratch.  Integer
cases are compared bit for bit (every product and sum is exact; +0 and -0 are one value); Gaussian cases within BAR_FACTOR times the
float32 mirror's error.  Every test prints the largest error / bar ratio of its stages (`-s` shows them;
profiles/disc_step_gpu_accuracy.log is that output)."""
import numpy as np
import pytest
import torch

import disc_step_models as DM
import mpd_models as PM
import msd_models as SM
from raw_abi import L, Sent, bits, check, stream, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
E_INVALID = -1


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def same_bits(got, want):
    got, want = np.asarray(got, np.float32) + np.float32(0), np.asarray(want, np.float32) + np.float32(0)
    return got.shape == want.shape and bool((bits(got) == bits(want)).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def raw_wgrad(dz, x, G, K, s, pad, slices=0, old=None, want_dw=True, want_db=True, off=0):
    """set_gconv1d_wgrad into guarded buffers; `old` = (dW, db) to accumulate into.  -> (dW or None, db or None)."""
    R, Cout, _Ho = dz.shape
    Cin, H = x.shape[1:]
    dw = Sent((Cout, Cin // G, K), DEV, off=off) if want_dw else None
    db = Sent((Cout,), DEV, off=1 - off) if want_db else None
    if old is not None:
        for buf, a in zip((dw, db), old):
            if buf is not None:
                buf.fill(a)
    n = L().set_gconv1d_wgrad_scratch_floats(R, Cin, Cout, G, H, K, s, pad, slices)
    assert n > 0
    scratch = Sent((n,), DEV, off=off)
    dzd, xd = to_dev(dz, DEV), to_dev(x, DEV)
    check(L().set_gconv1d_wgrad(dzd.data_ptr(), xd.data_ptr(), None if dw is None else dw.ptr, None if db is None else db.ptr, R, Cin, Cout, G, H, K, s,
                                pad, int(old is not None), slices, scratch.ptr, n, stream()), "set_gconv1d_wgrad")
    scratch.get()                                    # nothing written around the scratch
    return (None if dw is None else dw.get()), (None if db is None else db.get())


# ---- the weight gradient, integer operands: bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", DM.WGRAD_TRIPLES, ids=lambda t: "%dto%dx%d" % t)
def test_wgrad_integer_cases_bit_for_bit(triple):
    cases = [c for c in DM.wgrad_cases() if c[:3] == triple]
    assert len(cases) >= 8
    for n, (cig, cog, G, K, s, pad, H, R, slices, acc, use_db) in enumerate(cases):
        rng = np.random.default_rng(1000 * cig + 10 * cog + n)
        Ho = DM.out_len(H, K, s, pad)
        x = DM.int_array(rng, (R, cig * G, H), DM.INT_X)
        dz = DM.int_array(rng, (R, cog * G, Ho), DM.INT_X)
        old = (DM.int_array(rng, (cog * G, cig, K), 64), DM.int_array(rng, (cog * G,), 64)) if acc else None
        want_w, want_b = DM.gconv_wgrad(dz.astype(np.float64), x.astype(np.float64), K, s, pad, G)
        if acc:
            want_w, want_b = want_w + old[0], want_b + old[1]
        got_w, got_b = raw_wgrad(dz, x, G, K, s, pad, slices, old, want_db=use_db, off=n % 2)
        tag = (cig, cog, G, K, s, pad, H, R, slices, acc, use_db)
        assert same_bits(got_w, want_w), ("dW", tag)
        assert got_b is None or same_bits(got_b, want_b), ("db", tag)
    # db alone (no weight gradient wanted)
    _w, got_b = raw_wgrad(dz, x, G, K, s, pad, 0, None, want_dw=False)
    assert _w is None and same_bits(got_b, DM.gconv_wgrad(dz.astype(np.float64), x.astype(np.float64), K, s, pad, G)[1])


@pytest.mark.parametrize("cin,cout,G,K,s", DM.MSD_PAIRS + DM.MPD_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("H", [64, 77])
def test_wgrad_gaussian_within_the_mirror_bar(cin, cout, G, K, s, H):
    rng = np.random.default_rng(cin + cout + H + s)
    R, pad = 2, (K - 1) // 2
    x = rng.standard_normal((R, cin, H)).astype(np.float32)
    dz = rng.standard_normal((R, cout, DM.out_len(H, K, s, pad))).astype(np.float32)
    want_w, want_b = DM.gconv_wgrad(dz.astype(np.float64), x.astype(np.float64), K, s, pad, G)
    planned = L().set_gconv1d_wgrad_plan(R, cin, cout, G, H, K, s, pad, 0)
    for slices, forced in ((planned, 0), (2, 2)):
        mir_w, mir_b = DM.gconv_wgrad_mirror(dz, x, K, s, pad, G, slices)
        bar_w, bar_b = DM.bar(want_w, mir_w), DM.bar(want_b, mir_b)
        got_w, got_b = raw_wgrad(dz, x, G, K, s, pad, forced)
        err_w, err_b = float(np.abs(got_w - want_w).max()), float(np.abs(got_b - want_b).max())
        print("wgrad %4d -> %4d g %2d K %2d s %d H %2d slices %d: dW err %.3e bar %.3e ratio %.3f; db err %.3e bar %.3e ratio %.3f"
              % (cin, cout, G, K, s, H, slices, err_w, bar_w, err_w / bar_w, err_b, bar_b, err_b / bar_b))
        assert 0 < bar_w < 1e-3 and err_w <= bar_w and 0 < bar_b < 1e-4 and err_b <= bar_b


def test_wgrad_is_bit_reproducible_and_planned_slices_reach_the_reduce():
    """A shape whose plan takes several slices on this device: two runs agree bit for bit and with the mirror's bar."""
    rng = np.random.default_rng(3)
    R, cin, cout, G, K, s, pad, H = 6, 8, 16, 1, 5, 1, 2, 200
    slices = L().set_gconv1d_wgrad_plan(R, cin, cout, G, H, K, s, pad, 0)
    assert slices > 1
    x = rng.standard_normal((R, cin, H)).astype(np.float32)
    dz = rng.standard_normal((R, cout, H)).astype(np.float32)
    a, b = raw_wgrad(dz, x, G, K, s, pad), raw_wgrad(dz, x, G, K, s, pad, off=1)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    want, _ = DM.gconv_wgrad(dz.astype(np.float64), x.astype(np.float64), K, s, pad, G)
    bar = DM.bar(want, DM.gconv_wgrad_mirror(dz, x, K, s, pad, G, slices)[0])
    assert float(np.abs(a[0] - want).max()) <= bar


# ---- the first layers ----------------------------------------------------------------------------------------------------------------------
def raw_first(fold, dz, y, y_hat, p, K, s, pad, slices, old, want_dw=True, want_db=True, off=0):
    B, T = y.shape
    Cc = dz.shape[1]
    dw = Sent((Cc, K), DEV, off=off) if want_dw else None
    db = Sent((Cc,), DEV, off=1 - off) if want_db else None
    if old is not None:
        for buf, a in zip((dw, db), old):
            if buf is not None:
                buf.fill(a)
    n = L().set_first_conv_wgrad_part_doubles(Cc, K, slices)
    part = torch.full((n + 16,), NAN, dtype=torch.float64, device=DEV)
    dzd, yd = to_dev(dz, DEV), to_dev(y, DEV)
    yhd = None if y_hat is None else to_dev(y_hat, DEV)
    args = (dzd.data_ptr(), yd.data_ptr(), ptr(yhd), None if dw is None else dw.ptr, None if db is None else db.ptr, B, T)
    tail = (int(old is not None), slices, part.data_ptr(), n, stream())
    if fold:
        check(L().set_mpd_fold_conv_wgrad(*args, p, Cc, K, s, pad, *tail), "set_mpd_fold_conv_wgrad")
    else:
        check(L().set_wave_conv_wgrad(*args, Cc, K, pad, *tail), "set_wave_conv_wgrad")
    assert bool(torch.isnan(part[n:]).all())
    return (None if dw is None else dw.get()), (None if db is None else db.get())


@pytest.mark.parametrize("p", PM.PERIODS)
def test_first_layer_wgrads_integer_cases_bit_for_bit(p):
    n = 0
    for T in (p + 1, 23, 64, 97, 10 * p):                 # T % p != 0 (the mirror region is read) and T % p == 0
        for K, s, pad in ((5, 3, 2), (15, 1, 7), (3, 2, 0)):
            rng = np.random.default_rng(100 * T + K + p)
            B, Cc = 2, (6, 33)[n % 2]
            H = -(-T // p)
            Ho = DM.out_len(H, K, s, pad)
            if Ho < 1:
                continue
            y, y_hat = DM.int_array(rng, (B, T), DM.INT_X), DM.int_array(rng, (B, T), DM.INT_X)
            dz = DM.int_array(rng, (2 * B * p, Cc, Ho), DM.INT_X)
            old = (DM.int_array(rng, (Cc, K), 64), DM.int_array(rng, (Cc,), 64)) if n % 2 else None
            want_w, want_b = DM.fold_wgrad(dz.astype(np.float64), y, y_hat, p, K, s, pad)
            if old is not None:
                want_w, want_b = want_w + old[0], want_b + old[1]
            got_w, got_b = raw_first(True, dz, y, y_hat, p, K, s, pad, (0, 1, 3, 7)[n % 4], old, want_dw=n % 5 != 4, want_db=n % 3 != 2, off=n % 2)
            assert got_w is None or same_bits(got_w, want_w), ("fold dW", p, T, K, s, pad)
            assert got_b is None or same_bits(got_b, want_b), ("fold db", p, T, K, s, pad)
            n += 1
    assert n >= 10
    # the MSD's first layer: both signals, and one signal alone (what a spectrally normed net in train() runs)
    for T, K in ((14, 15), (15, 15), (65, 15), (200, 7), (333, 1)):
        rng = np.random.default_rng(T + K)
        B, Cc, pad = 2, 12, (K - 1) // 2
        y, y_hat = DM.int_array(rng, (B, T), DM.INT_X), DM.int_array(rng, (B, T), DM.INT_X)
        dz = DM.int_array(rng, (2 * B, Cc, T), DM.INT_X)
        want_w, want_b = DM.wave_wgrad(dz.astype(np.float64), np.concatenate([y, y_hat]), K, pad)
        got_w, got_b = raw_first(False, dz, y, y_hat, 1, K, 1, pad, (0, 2)[T % 2], None)
        assert same_bits(got_w, want_w) and same_bits(got_b, want_b), ("wave", T, K)
        want_w, want_b = DM.wave_wgrad(dz[B:].astype(np.float64), y_hat, K, pad)
        got_w, got_b = raw_first(False, dz[B:], y_hat, None, 1, K, 1, pad, 3, None, off=1)
        assert same_bits(got_w, want_w) and same_bits(got_b, want_b), ("wave alone", T, K)


def test_first_layer_wgrads_gaussian_within_the_bar():
    rng = np.random.default_rng(21)
    B, T, Cc = 2, 333, 32
    y, y_hat = PM.waves(22, B, T)
    for p in (3, 11):
        K, s, pad = 5, 3, 2
        dz = rng.standard_normal((2 * B * p, Cc, DM.out_len(-(-T // p), K, s, pad))).astype(np.float32)
        want_w, want_b = DM.fold_wgrad(dz.astype(np.float64), y, y_hat, p, K, s, pad)
        got_w, got_b = raw_first(True, dz, y, y_hat, p, K, s, pad, 0, None)
        bar_w, bar_b = DM.bar(want_w, DM._r32(want_w)), DM.bar(want_b, DM._r32(want_b))
        err_w, err_b = float(np.abs(got_w - want_w).max()), float(np.abs(got_b - want_b).max())
        print("fold wgrad p %2d: dW err %.3e bar %.3e ratio %.3f; db ratio %.3f" % (p, err_w, bar_w, err_w / bar_w, err_b / bar_b))
        assert 0 < bar_w and err_w <= bar_w and 0 < bar_b and err_b <= bar_b
    dz = rng.standard_normal((2 * B, Cc, T)).astype(np.float32)
    want_w, want_b = DM.wave_wgrad(dz.astype(np.float64), np.concatenate([y, y_hat]), 15, 7)
    got_w, got_b = raw_first(False, dz, y, y_hat, 1, 15, 1, 7, 0, None)
    bar_w, bar_b = DM.bar(want_w, DM._r32(want_w)), DM.bar(want_b, DM._r32(want_b))
    err_w, err_b = float(np.abs(got_w - want_w).max()), float(np.abs(got_b - want_b).max())
    print("wave wgrad: dW err %.3e bar %.3e ratio %.3f; db ratio %.3f" % (err_w, bar_w, err_w / bar_w, err_b / bar_b))
    assert 0 < bar_w and err_w <= bar_w and 0 < bar_b and err_b <= bar_b


# ---- the fold backwards ----------------------------------------------------------------------------------------------------------------------
def raw_wn_bwd(dw, g, v, want_dg=True, want_dv=True):
    n0 = v.shape[0]
    dg = Sent(g.shape, DEV, off=1) if want_dg else None
    dv = Sent(v.shape, DEV) if want_dv else None
    d, gd, vd = to_dev(dw, DEV), to_dev(g, DEV), to_dev(v, DEV)
    check(L().set_weight_norm_fold_bwd(d.data_ptr(), gd.data_ptr(), vd.data_ptr(), None if dg is None else dg.ptr, None if dv is None else dv.ptr, n0,
                                       v.size // n0, 0, stream()), "set_weight_norm_fold_bwd")
    return (None if dg is None else dg.get()), (None if dv is None else dv.get())


def raw_sn_bwd(dw, W, u, v, sigma, old=None):
    n0 = W.shape[0]
    out = Sent(W.shape, DEV, off=1)
    if old is not None:
        out.fill(old)
    part = torch.full((n0,), NAN, dtype=torch.float64, device=DEV)
    d, Wd, ud, vd, sd = (to_dev(a, DEV) for a in (dw, W, u, v, np.asarray([sigma], np.float32)))
    check(L().set_spectral_norm_fold_bwd(d.data_ptr(), Wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), sd.data_ptr(), out.ptr, n0, W.size // n0,
                                         int(old is not None), part.data_ptr(), stream()), "set_spectral_norm_fold_bwd")
    return out.get()


def test_fold_backwards_exact_on_power_of_two_norms_and_within_the_bar():
    rng = np.random.default_rng(8)
    for shape in ((5, 4, 4), (33, 16, 4, 1), (300, 1, 16), (2, 8, 41 * 2)):            # inner 16, 64, 16, 656
        n0 = shape[0]
        inner = int(np.prod(shape[1:]))
        v = rng.choice([-1.0, 1.0], size=shape).astype(np.float32)
        if inner not in (16, 64):                                                   # 16 entries of +-2, the rest 0: norm 8
            v[:] = 0
            v.reshape(n0, -1)[:, rng.permutation(inner)[:16]] = 2
        v *= np.float32(2.0) ** rng.integers(-1, 3, size=(n0,) + (1,) * (len(shape) - 1))
        g = (np.float32(2.0) ** rng.integers(-2, 3, size=(n0,) + (1,) * (len(shape) - 1))).astype(np.float32) * rng.choice([-1, 1, 3], size=(n0,) + (1,) * (len(shape) - 1))
        g = g.astype(np.float32)
        dw = DM.int_array(rng, shape, 8)
        dg, dv = DM.wn_fold_bwd(dw.astype(np.float64), g.astype(np.float64), v.astype(np.float64))
        got_g, got_v = raw_wn_bwd(dw, g, v)
        assert same_bits(got_g, dg) and same_bits(got_v, dv), shape
        only_g, none_v = raw_wn_bwd(dw, g, v, want_dv=False)
        assert none_v is None and same_bits(only_g, dg)
    # Gaussian: the quotients are not exact; the kernel works in double and rounds once, as the mirror does
    shape = (72, 40, 5, 1)
    v, dw = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal((72, 1, 1, 1))).astype(np.float32)
    dg, dv = DM.wn_fold_bwd(dw.astype(np.float64), g.astype(np.float64), v.astype(np.float64))
    got_g, got_v = raw_wn_bwd(dw, g, v)
    rg, rv = np.abs(got_g - dg).max() / DM.bar(dg, DM._r32(dg)), np.abs(got_v - dv).max() / DM.bar(dv, DM._r32(dv))
    print("weight-norm fold backward: dg err / bar %.3f, dv err / bar %.3f" % (rg, rv))
    assert rg <= 1 and rv <= 1
    # spectral norm: integer W, u, v with sigma = u^T W v a power of two
    for n0, rest in ((6, (3, 5)), (300, (1, 15)), (40, (10, 41))):
        inner = int(np.prod(rest))
        W = DM.int_array(rng, (n0,) + rest, 3)
        u, vv = DM.int_array(rng, (n0,), 2), DM.int_array(rng, (inner,), 2)
        u[0] = vv[0] = 1
        W.reshape(n0, -1)[0, 0] = 0
        W.reshape(n0, -1)[0, 0] = 4096 - float(u.astype(np.float64) @ (W.reshape(n0, -1).astype(np.float64) @ vv.astype(np.float64)))
        sigma = float(SM.sn_sigma(W.astype(np.float64), u.astype(np.float64), vv.astype(np.float64)))
        assert sigma == 4096.0
        dw = DM.int_array(rng, (n0,) + rest, 8)
        want = DM.sn_fold_bwd(dw.astype(np.float64), W.astype(np.float64), u.astype(np.float64), vv.astype(np.float64))
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)      # the case is exact in float32
        assert same_bits(raw_sn_bwd(dw, W, u, vv, sigma), want), (n0, rest)
        old = DM.int_array(rng, (n0,) + rest, 8) / np.float32(4096.0 * 4096.0) * 1024
        assert same_bits(raw_sn_bwd(dw, W, u, vv, sigma, old), (want + old).astype(np.float32)), ("accumulate", n0, rest)
    W = rng.standard_normal((72, 40, 5)).astype(np.float32)
    u, vv = rng.standard_normal(72).astype(np.float32), rng.standard_normal(200).astype(np.float32)
    dw = rng.standard_normal(W.shape).astype(np.float32)
    sigma = np.float32(SM.sn_sigma(W.astype(np.float64), u.astype(np.float64), vv.astype(np.float64)))
    s64 = float(sigma)
    n0 = 72
    d2 = dw.astype(np.float64).reshape(n0, -1)
    want = ((d2 - (d2 * W.astype(np.float64).reshape(n0, -1)).sum() / s64 * np.outer(u.astype(np.float64), vv.astype(np.float64))) / s64).reshape(W.shape)
    got = raw_sn_bwd(dw, W, u, vv, sigma)
    r = np.abs(got - want).max() / DM.bar(want, DM._r32(want))
    print("spectral-norm fold backward: err / bar %.3f" % r)
    assert r <= 1


# ---- the modules, end to end -----------------------------------------------------------------------------------------------------------------
_MODULES = {}


def _module(case, trainable=True):
    from set_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    kind, _B, _T, train, _sw, _sy = DM.E2E[case]
    if kind not in _MODULES:
        _MODULES[kind] = (MultiPeriodDiscriminator(channels=PM.NARROW) if kind == "mpd" else
                          MultiScaleDiscriminator(channels=DM.MSD_NARROW, groups=DM.MSD_NARROW_GROUPS)).to(DEV)
    net = _MODULES[kind]
    state = DM.e2e_inputs(case)[0]
    with torch.no_grad():
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    net.trainable_(trainable)
    for q in net.parameters():
        q.grad = None
    return net.train(train)


def _forward(case, net, yh_grad=False):
    from set_amd.discriminators import discriminator_loss
    _state, y, y_hat = DM.e2e_inputs(case)
    yd, yh = to_dev(y, DEV).unsqueeze(1), to_dev(y_hat, DEV).unsqueeze(1)
    if yh_grad:
        yh.requires_grad_()
    rs, gs, fr, fg = net(yd, yh, sentinel=NAN)
    r, f = discriminator_loss(rs, gs)
    return yh, rs, gs, fr, fg, r, f


def _gpu_gates(case, fr, fg):
    """The gate values the GPU took on its own maps, in the shape the step models take them, and the flat (real, generated) lists."""
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    if DM.E2E[case][0] == "mpd":
        real = [[PM.map_to_rows(n(m)) for m in maps[:5]] for maps in fr]
        gen = [[PM.map_to_rows(n(m)) for m in maps[:5]] for maps in fg]
        gates = [[DM.gate_of(np.concatenate([a, b]), PM.SLOPE).astype(np.float64) for a, b in zip(r, g)] for r, g in zip(real, gen)]
    else:
        real, gen = [[n(m) for m in maps[:7]] for maps in fr], [[n(m) for m in maps[:7]] for maps in fg]
        gates = [([DM.gate_of(a, PM.SLOPE).astype(np.float64) for a in r], [DM.gate_of(a, PM.SLOPE).astype(np.float64) for a in g]) for r, g in zip(real, gen)]
    return gates, [a for r in real for a in r], [a for g in gen for a in g]


@pytest.mark.parametrize("case", list(DM.E2E))
def test_step_end_to_end_against_the_model(case):
    fw, mi, bars = DM.e2e_forward(case), DM.e2e_forward(case, np.float32), DM.load_bars(case)
    net = _module(case)
    names = [k for k, _q in net.named_parameters()]
    params = [q for _k, q in net.named_parameters()]
    assert all(q.requires_grad for q in params)
    _yh, rs, gs, fr, fg, r, f = _forward(case, net)
    assert all(s.requires_grad for s in rs + gs) and not any(m.requires_grad for d in fr for m in d)
    # the GPU's gate decisions differ from the model's only where the model itself is undecided, and rarely
    gates, got_r, got_g = _gpu_gates(case, fr, fg)
    flips = entries = 0
    for got, ops64, ops32 in zip((got_r, got_g), DM.gate_operands(fw, case), DM.gate_operands(mi, case)):
        for a, m64, und in zip(got, ops64, DM.undecided(ops64, ops32)):
            differ = DM.gate_of(a, PM.SLOPE) != DM.gate_of(m64, PM.SLOPE)
            assert not (differ & ~und).any()
            flips, entries = flips + int(differ.sum()), entries + differ.size
    assert flips <= DM.UNDECIDED_CAP * entries, (flips, entries)
    worst = 0.0
    for k, (u_r, u_f) in enumerate(DM.U_PAIRS):
        total = r * u_r + f * u_f
        g1 = torch.autograd.grad(total, params, retain_graph=True)
        g2 = torch.autograd.grad(total, params, retain_graph=True)
        want = DM.e2e_step(fw, case, u_r, u_f, gates=gates)
        order = list(want)                                                   # the order of the recorded bars
        assert set(order) == set(names) and len(order) == len(names)
        gbars = DM.grad_bars(bars, k)
        for name, q, a, b in zip(names, params, g1, g2):
            assert a is not None and tuple(a.shape) == tuple(q.shape) and torch.equal(a, b) and bool(torch.isfinite(a).all()), name
            err = float(np.abs(a.cpu().numpy().astype(np.float64) - want[name].reshape(tuple(q.shape))).max())
            ratio = err / gbars[order.index(name)]
            if ratio > 0.5:
                print("  %s u %d: %d entries, |grad| max %.3e, err %.3e, err / bar %.3f" % (name, k, q.numel(), np.abs(want[name]).max(), err, ratio))
            worst = max(worst, ratio)
    print("disc step %-15s gate flips %d of %d; worst parameter-gradient err / bar %.3f" % (case, flips, entries, worst))
    assert worst <= 1.0
    # .backward(): a second one accumulates to exactly twice
    (r + f).backward(retain_graph=True)
    first = [q.grad.clone() for q in params]
    (r + f).backward()
    assert all(torch.equal(q.grad, 2 * a) for q, a in zip(params, first))
    # a second run from restored buffers gives the same bits
    net = _module(case)
    _yh, _rs, _gs, _fr, _fg, r2, f2 = _forward(case, net)
    (r2 + f2).backward()
    assert torch.equal(r, r2) and torch.equal(f, f2)
    assert all(torch.equal(q.grad, a) for q, a in zip(net.parameters(), first))


@pytest.mark.parametrize("case", ["mpd_333", "msd_333_eval", "msd_333_train"])
def test_frozen_parameters_get_none_and_launch_nothing(case, monkeypatch):
    from set_amd import ops
    net = _module(case)
    calls = dict(wgrad=0, dgrad=0, first=0, fold=0)

    def counted(name, key):
        fn = getattr(ops, name)

        def run(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        monkeypatch.setattr(ops, name, run)
    for name, key in (("gconv1d_wgrad", "wgrad"), ("sconv1d_dgrad", "dgrad"), ("gconv1d_dgrad", "dgrad"), ("mpd_fold_conv_wgrad", "first"),
                      ("wave_conv_wgrad", "first"), ("weight_norm_fold_bwd", "fold"), ("spectral_norm_fold_bwd", "fold")):
        counted(name, key)
    live = [k for k, _q in net.named_parameters() if ".conv_post." in k and not k.endswith("bias")]
    for k, q in net.named_parameters():
        q.requires_grad_(k in live)
    _yh, _rs, _gs, _fr, _fg, r, f = _forward(case, net)
    (r + f).backward()
    D = len(net.discriminators)
    halves = 1 if case.endswith("train") else 0            # the spectrally normed scale in train(): one chain per half
    assert calls == dict(wgrad=D + halves, dgrad=0, first=0, fold=D + halves), calls
    for k, q in net.named_parameters():
        assert (q.grad is not None) == (k in live), k
    # the live gradients are those of the fully trainable step, bit for bit
    full = _module(case)
    _yh, _rs, _gs, _fr, _fg, r, f = _forward(case, full)
    (r + f).backward()
    want = dict((k, q.grad) for k, q in full.named_parameters())
    net2 = _module(case)
    for k, q in net2.named_parameters():
        q.requires_grad_(k in live)
    _yh, _rs, _gs, _fr, _fg, r, f = _forward(case, net2)
    (r + f).backward()
    assert all(torch.equal(q.grad, want[k]) for k, q in net2.named_parameters() if k in live)


@pytest.mark.parametrize("case", ["mpd_333", "msd_333_train"])
def test_generated_waveform_gradient_together_with_trainable_weights(case):
    """y_hat.requires_grad with trainable weights: the parameters' gradients do not move, and d / d y_hat is bit for bit what the
    frozen (generator-side) path gives for the same loss."""
    net = _module(case)
    _yh, _rs, _gs, _fr, _fg, r, f = _forward(case, net)
    (r + f).backward()
    want = [q.grad.clone() for q in net.parameters()]
    net = _module(case)
    yh, _rs, _gs, _fr, _fg, r, f = _forward(case, net, yh_grad=True)
    (r + f).backward()
    assert all(torch.equal(q.grad, a) for q, a in zip(net.parameters(), want))
    g_train = yh.grad.clone()
    assert float(g_train.abs().max()) > 0
    net = _module(case, trainable=False)
    yh, rs, _gs, _fr, _fg, r, f = _forward(case, net, yh_grad=True)
    assert not any(s.requires_grad for s in rs)
    (r + f).backward()
    assert torch.equal(yh.grad, g_train)


@pytest.mark.parametrize("case", ["mpd_333", "msd_333_eval"])
def test_an_optimizer_step_invalidates_the_folded_weights(case):
    net = _module(case)
    _yh, _rs, gs0, _fr, _fg, r, f = _forward(case, net)
    (r + f).backward()
    torch.optim.SGD(net.parameters(), lr=0.5).step()
    with torch.no_grad():
        _yh, rs, gs, _fr, _fg, _r, _f = _forward(case, net)
    state = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    _state, y, y_hat = DM.e2e_inputs(case)
    kind = DM.E2E[case][0]
    fwd = (lambda **kw: PM.mpd_forward(y, y_hat, state, **kw)) if kind == "mpd" else \
        (lambda **kw: SM.msd_forward(y, y_hat, state, DM.MSD_NARROW_GROUPS, False, **kw))
    fw, mi = fwd(), fwd(dtype=np.float32, chain=True)
    worst = moved = 0.0
    for i in range(len(gs)):
        for got, key, old in ((gs[i], "scores_g", gs0[i]), (rs[i], "scores_r", None)):
            bar = DM.bar(fw[key][i], mi[key][i])
            worst = max(worst, float(np.abs(got.cpu().numpy() - fw[key][i]).max()) / bar)
            if old is not None:
                moved = max(moved, float((got - old.detach()).abs().max()) / bar)
    print("%s after one SGD step: score err / bar %.3f; the step moved the scores by %.0f bars" % (case, worst, moved))
    assert worst <= 1.0 and moved > 100


def test_trainable_false_restores_the_frozen_behaviour():
    for case in ("mpd_333", "msd_333_eval"):
        net = _module(case)
        net.trainable_(False)
        assert not any(q.requires_grad for q in net.parameters())
        _yh, rs, gs, fr, _fg, _r, _f = _forward(case, net, yh_grad=True)
        assert not any(s.requires_grad for s in rs) and all(s.requires_grad for s in gs) and not any(m.requires_grad for d in fr for m in d)
        next(net.parameters()).requires_grad_(True)
        with pytest.raises(RuntimeError, match="weight gradients are not built"):
            _forward(case, net)
        net.trainable_(True)
        _yh, rs, _gs, _fr, _fg, _r, _f = _forward(case, net)
        assert all(s.requires_grad for s in rs)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x = torch.zeros(2 * 8 * 40 + 64, device=DEV)
    p, n = x.data_ptr(), 4096
    s = torch.zeros(n, device=DEV)
    d = torch.zeros(n, dtype=torch.float64, device=DEV)

    def wg(dz=p, xx=p, dw=p, db=None, R=2, Cin=8, Cout=8, G=1, H=40, K=5, st=1, pad=2, acc=0, slices=2, scratch=s.data_ptr(), floats=n):
        return L().set_gconv1d_wgrad(dz, xx, dw, db, R, Cin, Cout, G, H, K, st, pad, acc, slices, scratch, floats, stream())
    assert wg() == 0
    for kw in (dict(K=DM.KMAX + 1, pad=2), dict(K=0), dict(st=5), dict(st=0), dict(G=3), dict(G=0), dict(pad=5), dict(slices=DM.MAX_SLICES + 1),
               dict(slices=-1), dict(floats=2 * 8 * 8 * 5 - 1), dict(scratch=None), dict(dz=None), dict(xx=None), dict(dw=None, db=None), dict(acc=2),
               dict(H=2, pad=0)):
        assert wg(**kw) == E_INVALID, kw
    assert wg(slices=1, scratch=None, floats=0) == 0                 # one slice, no accumulate: the scratch is not read
    assert wg(slices=1, acc=1, scratch=None, floats=0) == E_INVALID
    torch.cuda.synchronize()
    first = lambda **kw: L().set_mpd_fold_conv_wgrad(*[kw.get(k, v) for k, v in (("dz", p), ("y", p), ("y_hat", p), ("dw", p), ("db", None), ("B", 1), ("T", 40),  # noqa: E731
                                                                               ("p", 2), ("C", 4), ("K", 5), ("s", 3), ("pad", 2), ("acc", 0), ("slices", 2),
                                                                               ("part", d.data_ptr()), ("n", n))], stream())
    assert first() == 0
    for kw in (dict(K=16), dict(s=5), dict(T=2), dict(y_hat=None), dict(part=None), dict(n=2 * 4 * 6 - 1), dict(dw=None), dict(slices=DM.FIRST_MAX_SLICES + 1)):
        assert first(**kw) == E_INVALID, kw
    assert L().set_wave_conv_wgrad(p, p, None, p, None, 1, 40, 4, 15, 7, 0, 1, d.data_ptr(), n, stream()) == 0
    assert L().set_wave_conv_wgrad(p, p, None, p, None, 1, 40, 4, 15, 6, 0, 1, d.data_ptr(), n, stream()) == E_INVALID
    assert L().set_weight_norm_fold_bwd(p, p, p, None, None, 4, 10, 0, stream()) == E_INVALID
    assert L().set_weight_norm_fold_bwd(None, p, p, p, p, 4, 10, 0, stream()) == E_INVALID
    assert L().set_spectral_norm_fold_bwd(p, p, p, p, None, p, 4, 10, 0, d.data_ptr(), stream()) == E_INVALID
    assert L().set_spectral_norm_fold_bwd(p, p, p, p, p, p, 4, 10, 0, None, stream()) == E_INVALID
    torch.cuda.synchronize()
