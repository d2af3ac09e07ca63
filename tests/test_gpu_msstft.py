"""GPU checks of the multi-resolution STFT loss and its waveform gradient (csrc/stft_loss.hip through set_amd.vocoder_losses), stage by
stage and end to end, against the float64 model of msstft_models.py.  The bars are 4 x the error of a float32 mirror of the same matrix
form (derived and printed per fixture; test_msstft_reference.py asserts the conditions they stand on).  Every output and scratch buffer
starts as NaN, so an element a kernel leaves out shows.  Shapes: the smallest at which a tile, a mirror or a hop edge can go wrong."""
import numpy as np
import pytest
import torch

import msstft_models as SM
from msstft_models import CLAMP, GEOS

pytestmark = pytest.mark.gpu
NAN = float("nan")
MEASURED = {}


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _grad_mode():
    """The module differentiates: whatever grad mode an earlier test module left behind, these tests run with it enabled."""
    with torch.enable_grad():
        yield


_FN = {}


def _fn(key="all", **kw):
    from set_amd.vocoder_losses import MultiResolutionSTFTLoss, STFTLoss
    k = (key, tuple(sorted(kw.items())))
    if k not in _FN:
        _FN[k] = MultiResolutionSTFTLoss(**kw) if key == "all" else STFTLoss(*GEOS[key], **kw)
    return _FN[k]


def _note(key, err, bar):
    MEASURED[key] = max(MEASURED.get(key, (0.0, 0.0)), (err / bar if bar else 0.0, err))
    assert err <= bar, (key, err, bar)


def _t(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _geo(geo):
    return dict(n_fft=geo[0], hop=geo[1], win=geo[2])


@pytest.mark.parametrize("B,n", SM.CASES)
def test_stage_by_stage(dev, B, n):
    from set_amd import ops
    from set_amd.vocoder_losses import stft_magnitude
    for gi, geo in enumerate(GEOS):
        d = SM.derived(B, n, gi)
        bars, p = d["bars"], d["p64"]
        x, y = _t(d["x"], dev), _t(d["y"], dev)
        table, itable = _fn(gi)._tables(dev)[0]
        # stage 1: the magnitudes
        xm, ym = stft_magnitude(x, *geo, sentinel=NAN).cpu().numpy(), stft_magnitude(y, *geo, sentinel=NAN).cpu().numpy()
        assert xm.shape == p["xm"].shape and np.isfinite(xm).all() and np.isfinite(ym).all()
        e_mag = float(max(np.abs(xm - p["xm"]).max(), np.abs(ym - p["ym"]).max()))
        # stage 2: the finished sums, bit for bit the documented order applied to the GPU's own magnitudes
        for which in (1, 0):
            loss, stats, kept = ops.stft_loss_fwd(x, y, table, which=which, keep=True, sentinel=NAN, **_geo(geo))
            st = stats.cpu().numpy()
            sd, sg, sl, sc, mg = SM.fwd_sums_restated(xm, ym, geo)
            assert np.array_equal(st[3:6].view(np.uint64), np.array([sd, sg, sl]).view(np.uint64)), (st[3:6], sd, sg, sl)
            assert st[0] == np.sqrt(sd) and st[1] == np.sqrt(sg) and st[2] == xm.size
            assert np.array_equal(loss.cpu().numpy().view(np.uint32), np.array([sc, mg], dtype=np.float32).view(np.uint32))
            # the kept magnitudes: the other signal's, [B][chunks x 32][Ts], the bits of stage 1
            T, nb = xm.shape[1], xm.shape[2]
            sz = ops.stft_sizes(*geo, B, n)
            kp = kept.cpu().numpy().reshape(B, -1, sz["Ts"])
            assert np.isfinite(kp).all() and np.array_equal(kp[:, :nb, :T].transpose(0, 2, 1), xm if which == 1 else ym)
        e_sc, e_lm = abs(float(sc) - float(p["sc"])), abs(float(mg) - float(p["mag"]))
        # stage 3..5: the spectral backward on a given g_m, the inverse and the fold
        scratch = {}
        gm = _t(d["g_given"], dev)
        g_wav = ops.stft_loss_bwd(y, y, table, itable, which=1, g_m=gm, sentinel=NAN, scratch=scratch, **_geo(geo))
        s = scratch["spec"].cpu().numpy().reshape(B, 2, -1, sz["Ts"])
        assert np.isfinite(s).all() and np.isfinite(scratch["g_pad"].cpu().numpy()).all()
        assert not s[:, :, nb:].any() and not s[:, :, :, T:].any()           # bins and frames that do not exist: exactly 0
        e_spec = float(max(np.abs(s[:, 0, :nb, :T].transpose(0, 2, 1) - d["spec_given"][0]).max(),
                           np.abs(s[:, 1, :nb, :T].transpose(0, 2, 1) - d["spec_given"][1]).max()))
        gw = g_wav.cpu().numpy()
        assert np.isfinite(gw).all() and gw.shape == (B, n)
        e_w = float(np.abs(gw - d["gw_given"]).max())
        # added to an existing gradient instead of written: one fp32 addition per sample
        acc = torch.ones(B, n, device=dev)
        ops.stft_loss_bwd(y, y, table, itable, which=1, g_m=gm, g_wav=acc, sentinel=NAN, **_geo(geo))
        assert torch.equal(acc, 1.0 + g_wav)
        print("B=%d N=%d %s: magnitude %.3e (bar %.3e), sc %.3e (%.3e), mag %.3e (%.3e), g_re/g_im of a given g_m %.3e (%.3e), g_wav %.3e (%.3e)" % (
            B, n, geo, e_mag, bars["mag"], e_sc, bars["sc"], e_lm, bars["lmag"], e_spec, bars["spec"], e_w, bars["g_wav"]))
        _note("magnitude", e_mag, bars["mag"])
        _note("sc (one resolution)", e_sc, bars["sc"])
        _note("mag (one resolution)", e_lm, bars["lmag"])
        _note("g_re / g_im given g_m", e_spec, bars["spec"])
        _note("g_wav given g_m", e_w, bars["g_wav"])


def _run(fn, x, y, which, **kw):
    a, b = x.clone(), y.clone()
    (b if which == 1 else a).requires_grad_(True)
    sc, mg = fn(a, b, sentinel=NAN, **kw)
    return (b if which == 1 else a), sc, mg


def _model_with_gpu_choices(B, n, which, u, dev):
    """The float64 gradient with the GPU's own sign / clamp choice at the undecided entries (both are admissible there), the model's
    everywhere else.  The GPU's choices are read off its own magnitudes: sign(m - r), and m > sqrt(1e-7) for a power at or above the clamp."""
    from set_amd.vocoder_losses import stft_magnitude
    x, y = SM.pair(B, n)
    signs, passed, share = [], [], 0.0
    for gi, geo in enumerate(GEOS):
        und = SM.derived(B, n, gi)["undecided"][which]
        share = max(share, float(und.mean()))
        xm, ym = stft_magnitude(_t(x, dev), *geo).cpu().numpy(), stft_magnitude(_t(y, dev), *geo).cpu().numpy()
        m, r = (ym, xm) if which == 1 else (xm, ym)
        signs.append(np.where(und, np.sign(m.astype(np.float64) - r), np.nan))
        passed.append(np.where(und, (m > np.sqrt(np.float32(CLAMP))).astype(np.int64), -1))
    assert share <= SM.UNDECIDED_CAP
    return SM.loss_and_grad(x, y, GEOS, which, u, np.float64, signs=signs, passed=passed)[2], share


@pytest.mark.parametrize("which", [1, 0])
@pytest.mark.parametrize("B,n", SM.CASES)
def test_end_to_end(dev, B, n, which):
    fn = _fn()
    dg = SM.derived_grad(B, n, which)
    x, y = (_t(v, dev) for v in SM.pair(B, n))
    a, sc, mg = _run(fn, x, y, which)
    assert sc.shape == () and mg.shape == () and sc.requires_grad and mg.requires_grad
    _note("sc (end to end)", abs(float(sc.detach()) - dg["sc"]), dg["bar_sc"])
    _note("mag (end to end)", abs(float(mg.detach()) - dg["mag"]), dg["bar_mag"])
    (sc + mg).backward(retain_graph=True)
    g = a.grad.clone()
    assert g.shape == (B, n) and torch.isfinite(g).all()
    ref, share = _model_with_gpu_choices(B, n, which, (1.0, 1.0), dev)
    err = float(np.abs(g.cpu().numpy() - ref).max())
    print("B=%d N=%d which=%d: sc %.3e (bar %.3e), mag %.3e (%.3e), gradient %.3e (bar %.3e), max |gradient| %.3e, undecided %.2e" % (
        B, n, which, abs(float(sc.detach()) - dg["sc"]), dg["bar_sc"], abs(float(mg.detach()) - dg["mag"]), dg["bar_mag"], err,
        SM.grad_bar(dg, (1.0, 1.0)), np.abs(ref).max(), share))
    _note("gradient (end to end, u = 1, 1)", err, SM.grad_bar(dg, (1.0, 1.0)))
    # a second backward: the same bits
    a.grad = None
    (sc + mg).backward()
    assert torch.equal(a.grad, g)
    # a second forward + backward: the same bits
    a2, sc2, mg2 = _run(fn, x, y, which)
    (sc2 + mg2).backward()
    assert torch.equal(sc2, sc) and torch.equal(mg2, mg) and torch.equal(a2.grad, g)
    # recomputing the other signal's spectrum in backward instead of keeping its magnitudes: the same bits
    a5, sc5, mg5 = _run(_fn(recompute=True), x, y, which)
    (sc5 + mg5).backward()
    assert torch.equal(sc5, sc) and torch.equal(mg5, mg) and torch.equal(a5.grad, g)
    # unequal upstream scalars, combined on the device
    u = SM.UPSTREAMS[1]
    a3, sc3, mg3 = _run(fn, x, y, which)
    (u[0] * sc3 + u[1] * mg3).backward()
    ref3, _ = _model_with_gpu_choices(B, n, which, u, dev)
    _note("gradient (end to end, u = 45, 0.5)", float(np.abs(a3.grad.cpu().numpy() - ref3).max()), SM.grad_bar(dg, u))
    # [B, 1, N] in, [B, 1, N] out
    a4, sc4, mg4 = _run(fn, x[:, None, :], y[:, None, :], which)
    (sc4 + mg4).backward()
    assert a4.grad.shape == (B, 1, n) and torch.equal(a4.grad[:, 0], g) and torch.equal(sc4, sc) and torch.equal(mg4, mg)


@pytest.mark.parametrize("B,n", [c for c in SM.CASES if c[0] > 1])
def test_batch_rows_have_the_bits_of_the_row_alone(dev, B, n):
    """The magnitudes only: the losses and the gradient couple the rows through D, G and count (include/set_amd.h)."""
    from set_amd.vocoder_losses import stft_magnitude
    y = _t(SM.pair(B, n)[1], dev)
    for geo in GEOS:
        full = stft_magnitude(y, *geo, sentinel=NAN)
        for r in range(B):
            assert torch.equal(stft_magnitude(y[r:r + 1], *geo, sentinel=NAN)[0], full[r])


def test_exact_cases(dev):
    fn = _fn()
    n = 8192
    fx = SM.clamp_fixtures(n)
    # equal inputs: sc == 0, mag == 0, an all-zero gradient
    w = _t(SM.pair(2, 3000)[1], dev)
    for which in (1, 0):
        a, sc, mg = _run(fn, w, w, which)
        (sc + mg).backward()
        assert float(sc.detach()) == 0.0 and float(mg.detach()) == 0.0 and torch.isfinite(a.grad).all() and not a.grad.cpu().numpy().any()
    # quiet: every power of both signals is below the clamp: losses exactly 0, gradient exactly 0
    x, y, which = fx["quiet"]
    a, sc, mg = _run(fn, _t(x, dev), _t(y, dev), which)
    (sc + mg).backward()
    assert float(sc.detach()) == 0.0 and float(mg.detach()) == 0.0 and torch.isfinite(a.grad).all() and not a.grad.cpu().numpy().any()
    # mixed: a quiet differentiated signal against a loud one: non-zero losses, a gradient that is exactly zero
    x, y, which = fx["mixed"]
    a, sc, mg = _run(fn, _t(x, dev), _t(y, dev), which)
    (sc + mg).backward()
    assert float(sc.detach()) > 1.0 and float(mg.detach()) > 1.0 and torch.isfinite(a.grad).all() and not a.grad.cpu().numpy().any()
    # zeros: a stretch of exact zeros in both signals: under silent frames only the gradient is exactly 0, and non-zero before the stretch
    x, y, which = fx["zeros"]
    a, sc, mg = _run(fn, _t(x, dev), _t(y, dev), which)
    (sc + mg).backward()
    g = a.grad.cpu().numpy()
    lo, hi = SM.ZERO_STRETCH[0] + 1200, SM.ZERO_STRETCH[1] - 1200
    assert np.isfinite(g).all() and not g[0, lo:hi].any() and g[0, :SM.ZERO_STRETCH[0]].all()
    from set_amd.vocoder_losses import stft_magnitude
    for geo in GEOS:
        m = stft_magnitude(_t(y, dev), *geo, sentinel=NAN).cpu().numpy()
        assert np.all(m[0, SM.silent_frames(n, geo)] == np.sqrt(np.float32(CLAMP)))


def test_refusals(dev):
    from set_amd.vocoder_losses import MultiResolutionSTFTLoss, STFTLoss, stft_magnitude
    fn = _fn()
    z = torch.zeros(2, 4096, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(z.cpu(), z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(z, z.cpu())
    with pytest.raises(TypeError):
        fn(z.double(), z)
    with pytest.raises(TypeError):
        fn(z, z.double())
    with pytest.raises(ValueError):
        fn(z, z[:1])
    with pytest.raises(ValueError):
        fn(z[:, None, None], z[:, None, None])
    with pytest.raises(ValueError, match="reflect padding"):
        fn(z[:, :1024], z[:, :1024])                                       # N <= max(fft_size) / 2
    sc, mg = fn(z[:, :1025], z[:, :1025])
    assert float(sc) == 0.0 and float(mg) == 0.0
    assert float(STFTLoss(512, 50, 240)(z[:, :257], z[:, :257])[0]) == 0.0  # one resolution: its own pad
    with pytest.raises(ValueError, match="both require grad"):
        fn(z.clone().requires_grad_(True), z.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"compiled geometries.*\(1024, 120, 600\).*\(2048, 240, 1200\).*\(512, 50, 240\)"):
        STFTLoss(1024, 128, 600)
    with pytest.raises(ValueError, match="compiled geometries"):
        MultiResolutionSTFTLoss([1024, 2048, 512], [128, 240, 50], [600, 1200, 240])
    with pytest.raises(ValueError, match="hann_window"):
        MultiResolutionSTFTLoss(window="hamming_window")
    with pytest.raises(ValueError, match="hann_window"):
        STFTLoss(1024, 120, 600, "hamming_window")
    with pytest.raises(ValueError):
        stft_magnitude(z, 1024, 128, 600)
    # the C entries' own refusals
    from set_amd import ops
    from set_amd._lib import SetAmdError
    table, itable = fn._tables(dev)[0]
    with pytest.raises(SetAmdError, match="set_stft_sizes"):
        ops.stft_sizes(1024, 128, 600, 2, 4096)
    with pytest.raises(SetAmdError, match="set_stft_magnitude"):
        ops.stft_magnitude(z[:, :512].contiguous(), table, n_fft=1024, hop=120, win=600)
    a = z.clone().requires_grad_(True)
    with torch.no_grad():
        assert not fn(z, a)[0].requires_grad
    assert not fn(z, z)[0].requires_grad


def test_report_measured_errors():
    """Printed last: the largest error seen per quantity, as a share of its bar (profiles/ms_stft_gpu_accuracy.log quotes them)."""
    for k, (share, err) in sorted(MEASURED.items()):
        print("measured %s: %.3e at %.2f of its bar" % (k, err, share))
    assert all(share <= 1.0 for share, _ in MEASURED.values())
