"""CPU checks of the multi-resolution STFT loss's float64 model (msstft_models.py) and of the conditions the GPU tests
(test_gpu_msstft.py) stand on: the model against torch's own stft + autograd in float64 for both argument positions, the argument order
of the task, its gradient against finite differences of its loss, the frame, pad and fold rules, the kernel images' element maps, the
documented summation order, the clamp's exact fixtures, and -- per fixture -- the bars derived from a float32 mirror and the share of
entries whose sign / clamp decision is within four of the mirror's errors."""
import math

import numpy as np
import pytest

import msstft_models as SM
from msstft_models import CLAMP, GEOS


@pytest.fixture(scope="module")
def M():
    import set_amd  # noqa: F401
    from set_amd import melspec
    return melspec


@pytest.mark.parametrize("which", [1, 0])
def test_model_matches_torch_stft_and_autograd_in_float64(which):
    """Same float32 inputs, unrounded float64 window / twiddles on both sides.  Bound: a DFT sum has at most 1200 terms, so its rounding
    error is at most 1200 u sum|terms| with u = 2^-53; against the result that is a factor sum|terms| / |result|, ~sqrt(1200) = 35 for
    these noise-like frames and at most ~1e3 at their smallest bins: 1200 * 1e3 * 1.1e-16 ~ 1.3e-10 relative on a magnitude, which ln and
    1 / m pass on one to one.  The losses, O(1) numbers, and the gradient relative to its largest element are held to 1e-9."""
    x, y = SM.pair(2, 3000, seed=3)
    tabs = [SM.table64(g) for g in GEOS]
    for u in SM.UPSTREAMS:
        sc, mg, grad, _ = SM.loss_and_grad(x, y, GEOS, which, u, np.float64, tables=tabs)
        tsc, tmg, tg = SM.torch_loss_and_grad(x, y, GEOS, which, u)
        rel = np.abs(grad - tg).max() / np.abs(tg).max()
        print("which=%d u=%s: sc %.12f (torch %.12f), mag %.12f (torch %.12f); max |d grad| / max |grad| = %.3e" % (which, u, sc, tsc, mg, tmg, rel))
        assert abs(sc - tsc) <= 1e-9 and abs(mg - tmg) <= 1e-9
        assert rel <= 1e-9


def test_argument_order_of_the_task():
    """HifiGanTask calls stft_loss(y, y_): real first, generated second.  Swapping the arguments changes sc (its denominator is the second
    argument's norm) and leaves mag unchanged (|a - b| = |b - a|)."""
    x, y = SM.pair(1, 3000, seed=4)
    sc, mg, _, _ = SM.loss_and_grad(x, y, GEOS, 1)
    sc2, mg2, _, _ = SM.loss_and_grad(y, x, GEOS, 1)
    tsc, tmg, _ = SM.torch_loss_and_grad(x, y)
    tsc2, tmg2, _ = SM.torch_loss_and_grad(y, x)
    assert mg == mg2 and tmg == tmg2
    assert abs(sc - sc2) > 1e-6 * sc and abs(tsc - tsc2) > 1e-6 * tsc
    assert abs(sc - tsc) <= 1e-9 and abs(sc2 - tsc2) <= 1e-9


@pytest.mark.parametrize("which", [1, 0])
def test_gradient_matches_central_differences_of_the_models_own_loss(which):
    """h = 1e-5 along unit directions: truncation ~ h^2 |f'''|, rounding ~ u |loss| / h = 1e-11; held to 1e-5 of the gradient's norm.  No
    sign or clamp decision changes within the step (asserted), so the loss is smooth on it."""
    x, y = (v.astype(np.float64) for v in SM.pair(1, 2000, seed=7))
    u = (1.0, 0.7)
    _, _, grad, parts = SM.loss_and_grad(x, y, GEOS, which, u)
    rng = np.random.default_rng(0)
    h = 1e-5

    def value(a, b):
        sc, mg, _, p = SM.loss_and_grad(a, b, GEOS, which, u)
        for q, q0 in zip(p, parts):
            assert np.array_equal(np.sign(q["ym"] - q["xm"]), np.sign(q0["ym"] - q0["xm"]))
            assert np.array_equal(q["yp"] >= CLAMP, q0["yp"] >= CLAMP) and np.array_equal(q["xp"] >= CLAMP, q0["xp"] >= CLAMP)
        return u[0] * sc + u[1] * mg

    for _ in range(2):
        v = rng.standard_normal(x.shape)
        v /= np.linalg.norm(v)
        fd = (value(x, y + h * v) - value(x, y - h * v)) / (2 * h) if which == 1 else (value(x + h * v, y) - value(x - h * v, y)) / (2 * h)
        an = float((grad * v).sum())
        print("which=%d: finite difference %.9e, analytic %.9e" % (which, fd, an))
        assert abs(fd - an) <= 1e-5 * np.linalg.norm(grad)


def test_frame_and_pad_rules(M):
    import torch
    for geo in GEOS:
        for n in (geo[0] // 2 + 1, 1100, 3199, 3200, 7680, 15359, 15377):
            if n <= geo[0] // 2:
                continue
            T = torch.stft(torch.zeros(1, n, dtype=torch.float64), geo[0], geo[1], geo[2], torch.hann_window(geo[2], dtype=torch.float64),
                           return_complex=True).shape[-1]
            assert SM.n_frames(n, geo) == T == 1 + n // geo[1]
        with pytest.raises(ValueError):
            SM.pad_index(geo[0] // 2, geo[0] // 2)                        # N <= pad: reflect padding needs more samples
        idx = SM.pad_index(geo[0] // 2 + 1, geo[0] // 2)
        assert idx[0] == geo[0] // 2 and idx[-1] == 0 and idx[geo[0] // 2] == 0
    # the tile edges the GPU shapes are chosen for
    assert SM.n_frames(3199, GEOS[2]) == 64 and SM.n_frames(3200, GEOS[2]) == 65
    assert SM.n_frames(7680, GEOS[0]) == 65 and SM.n_frames(15359, GEOS[1]) == 64 and SM.n_frames(15377, GEOS[1]) == 65
    # the window: torch's periodic Hann, centred in fft_size
    for geo in GEOS:
        w = M.hann_padded(geo[0], geo[2])
        lf = SM.left(geo)
        assert np.allclose(w[lf:lf + geo[2]], torch.hann_window(geo[2], dtype=torch.float64).numpy(), atol=1e-15)
        assert not w[:lf].any() and not w[lf + geo[2]:].any() and lf % geo[1] != 0


@pytest.mark.parametrize("n,pad", [(1100, 1024), (1025, 1024), (3000, 512), (700, 256)])
def test_fold_gather_form_equals_the_scatter_by_the_pad_index(n, pad):
    rng = np.random.default_rng(n)
    g_p = rng.integers(-1000, 1000, n + 2 * pad).astype(np.float64)       # integers: both orders of addition are exact
    want = np.zeros(n)
    np.add.at(want, SM.pad_index(n, pad), g_p)
    assert np.array_equal(SM.fold(g_p, n, pad), want)
    hits = SM.fold(np.ones(n + 2 * pad), n, pad)
    if n == 1100:                                                          # both mirrors land on samples 75 .. 1024
        assert np.all(hits[75:1025] == 3) and np.all(hits[1:75] == 2) and np.all(hits[1025:1099] == 2) and hits[0] == 1 and hits[1099] == 1


@pytest.mark.parametrize("geo", GEOS)
def test_packers_element_maps(M, geo):
    n_fft, hop, win = geo
    nb, lf = SM.nbins(geo), SM.left(geo)
    table = M.dft_table(n_fft, win, 0, nb)
    img = M.pack_stft_table(table, win)
    nch = (nb + 31) // 32
    assert img.shape == (nch, win // 2, 64, 2)
    assert np.array_equal(M.unpack_stft_table(img, nb, n_fft), table)
    rng = np.random.default_rng(1)
    for _ in range(200):
        ch, s, lane, e = rng.integers(nch), rng.integers(win // 2), rng.integers(64), rng.integers(2)
        f = 32 * ch + (lane & 31)
        want = table[e, f, lf + 2 * s + (lane >> 5)] if f < nb else 0.0
        assert img[ch, s, lane, e] == want
    Q, rbt, NW = M.stft_idft_layout(hop, win)
    assert (Q, rbt, NW) == {120: (5, 4, 4), 240: (5, 8, 8), 50: (5, 2, 4)}[hop]
    it = M.pack_stft_idft_table(table, hop, win)
    assert it.shape == (nch, NW, 32 * Q, 64)
    for _ in range(400):
        ch, wave, kk, lane = rng.integers(nch), rng.integers(NW), rng.integers(32 * Q), rng.integers(64)
        q, part, s = kk >> 5, (kk >> 4) & 1, kk & 15
        f = 32 * ch + 2 * s + (lane >> 5)
        c = 32 * (wave if rbt >= 4 else (wave >> 1)) + (lane & 31)
        want = table[part, f, lf + hop * q + c] if (f < nb and c < hop and hop * q + c < win) else 0.0
        assert it[ch, wave, kk, lane] == want
    # every (part, bin, window sample) is in the inverse image exactly as often as waves share its row block
    assert np.isclose(np.abs(it).sum(dtype=np.float64), (2 if rbt == 2 else 1) * np.abs(table).sum(dtype=np.float64), rtol=1e-12)


def test_summation_order_restated():
    """The documented order on the mirror's magnitudes: the same numbers as a plain double sum to a few ulps, entries beyond the last
    frame and the last bin add nothing, and the order is what it says (a literal walk of one block's lanes)."""
    geo = GEOS[2]
    d = SM.derived(1, 3200, 2)
    xm, ym = d["p32"]["xm"], d["p32"]["ym"]                               # T = 65: two tiles, the second with one live frame
    sd, sg, sl, sc, mg = SM.fwd_sums_restated(xm, ym, geo)
    dd = (ym - xm).astype(np.float32).astype(np.float64)
    l = np.abs(SM.log_of(ym, np.float32) - SM.log_of(xm, np.float32)).astype(np.float32).astype(np.float64)
    for got, ent in ((sd, dd * dd), (sg, ym.astype(np.float64) ** 2), (sl, l)):
        assert abs(got - math.fsum(ent.ravel())) <= 1e-13 * math.fsum(ent.ravel())
    assert sc == np.float32(math.sqrt(sd) / math.sqrt(sg)) and mg == np.float32(sl / xm.size)
    # block (z = 1, b = 0, tile = 0), wave 2 = chunk 6: lane (h, j) walks cb, then r
    ent = ym.astype(np.float64) ** 2
    lanes = np.zeros(64)
    for h in range(2):
        for j in range(32):
            s = 0.0
            for cb in range(2):
                for r in range(16):
                    s += ent[0, 32 * cb + j, 32 * 6 + (r & 3) + 8 * (r >> 2) + 4 * h]
            lanes[32 * h + j] = s
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ o]
    only = np.zeros_like(ym)
    only[0, :64, 192:224] = ym[0, :64, 192:224]
    with np.errstate(divide="ignore", invalid="ignore"):                   # (the logs of the zeros: S_l is not looked at)
        assert SM.fwd_sums_restated(np.zeros_like(ym), only, geo)[1] == lanes[0]


@pytest.mark.parametrize("B,n", SM.CASES)
def test_bars_and_undecided_share(B, n):
    for gi, geo in enumerate(GEOS):
        d = SM.derived(B, n, gi)
        print("B=%d N=%d %s: bars %s; undecided share x %.2e y %.2e; min power %.2e" % (
            B, n, geo, " ".join("%s %.3e" % kv for kv in sorted(d["bars"].items())), d["share"][0], d["share"][1], d["min_power"]))
        assert all(v > 0 and np.isfinite(v) for v in d["bars"].values())
        assert max(d["share"]) <= SM.UNDECIDED_CAP
    for which in (1, 0):
        dg = SM.derived_grad(B, n, which)
        print("B=%d N=%d which=%d: gradient bars %s, loss bars sc %.3e mag %.3e; max |g_sc| %.3e max |g_mag| %.3e" % (
            B, n, which, " ".join("%s %.3e" % (u, SM.grad_bar(dg, u)) for u in SM.UPSTREAMS), dg["bar_sc"], dg["bar_mag"],
            np.abs(dg["g_sc"]).max(), np.abs(dg["g_mag"]).max()))
        # (the log-magnitude term divides by m^2: at the fixtures' smallest bins the float32 spectrum's error is a per cent of m, and
        # the mirror's gradient error is ~1e-3 of the largest element -- the bar follows the mirror, whatever it is)
        assert 0 < dg["e_sc"] < np.abs(dg["g_sc"]).max() and 0 < dg["e_mag"] < np.abs(dg["g_mag"]).max()


def test_clamp_fixtures_have_their_properties():
    """Each exact fixture, with a margin of 4 x the mirror's error: what the GPU test asserts exactly must not hang on a rounding."""
    n = 8192
    fx = SM.clamp_fixtures(n)
    for gi, geo in enumerate(GEOS):
        # zeros: the frames inside the stretch have power exactly 0 in the model and in the mirror (every term is a product with 0.0)
        x, y, _ = fx["zeros"]
        sil = SM.silent_frames(n, geo)
        assert len(sil) >= 2
        for dt in (np.float64, np.float32):
            re, im = SM.spectrum(y, geo, dt)
            assert not re[0, sil].any() and not im[0, sil].any()
        # quiet: every power of both signals, plus 4 mirror errors, is below the clamp
        for name, sigs in (("quiet", (0, 1)), ("mixed", (1,))):
            for k in sigs:
                w = fx[name][k]
                p64 = SM.magnitude(*SM.spectrum(w, geo, np.float64), np.float64)[1]
                p32 = SM.magnitude(*SM.spectrum(w, geo, np.float32), np.float32)[1]
                assert p64.max() + 4 * np.abs(p32 - p64).max() < CLAMP, (name, geo, p64.max())
        # mixed: the loud signal is above the clamp nearly everywhere, so both losses are far from 0
        p = SM.resolution(fx["mixed"][0], fx["mixed"][1], geo, np.float64)
        assert p["sc"] > 1.0 and p["mag"] > 1.0
    for name in ("quiet", "mixed"):
        x, y, which = fx[name]
        sc, mg, g, _ = SM.loss_and_grad(x, y, GEOS, which)
        assert not g.any()
        assert (sc == 0 and mg == 0) if name == "quiet" else (sc > 1 and mg > 1)
    x, y, which = fx["zeros"]
    _, _, g, _ = SM.loss_and_grad(x, y, GEOS, which)
    lo, hi = SM.ZERO_STRETCH[0] + 1200, SM.ZERO_STRETCH[1] - 1200
    assert hi > lo and not g[0, lo:hi].any() and g[0, :SM.ZERO_STRETCH[0]].all()
