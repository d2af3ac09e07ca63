"""GPU checks of the mel-cepstral distortion path (csrc/mcd.hip through set_amd.metrics and set_amd.ops) against the float64 models of
mcd_models.py.

`set_dtw` is checked bit for bit on integer grids (every cost, sum and compare is exact in fp32: test_mcd_reference.py asserts it of the
same cases) at the strip, column-block and ring edges of the shipped kernel (256-row strips, 64-column blocks, a 320-column ring, K padded
to 40 or 64), and on real-valued inputs whose every decision along the optimal path keeps a margin of 4 x the derived error bound (same
file), where the path must be the model's and `dist` within the bound.  Shapes are the smallest at which each edge can go wrong."""
import math

import numpy as np
import pytest
import torch

import mcd_models as MM

pytestmark = pytest.mark.gpu

SENT_U8, SENT_I32, SENT_F32 = 0xA5, -777, -12345.0
HP = {"fft_size": 1024, "win_size": 1024, "hop_size": 256, "audio_num_mel_bins": 80, "audio_sample_rate": 22050, "fmin": 55, "fmax": 7600}


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def MT():
    import set_amd  # noqa: F401
    from set_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def ops():
    import set_amd  # noqa: F401
    from set_amd import ops
    return ops


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _single(MT, dev, x, y):
    """One pair through metrics.dtw with the path: (dist fp32 scalar, steps, path [steps, 2], the rest of the path buffer)."""
    dist, steps, path, count = MT.dtw(_t(x, dev), _t(y, dev), return_path=True)
    assert dist.shape == () and steps.shape == () and path.shape == (len(x) + len(y) - 1, 2) and int(count) == int(steps)
    p = path.cpu().numpy()
    return dist.cpu().numpy(), int(steps), p[:int(steps)], p[int(steps):]


# ---- set_dtw, exact ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MM.exact_cases(), ids=lambda c: "%dx%d-K%d-g%s" % c[:4])
def test_dtw_integer_grids_bit_for_bit(MT, ops, dev, case):
    lx, ly, K, grid, off, seed = case
    x, y = MM.grid_pair(lx, ly, K, grid, off, seed)
    m = MM.dtw(x, y)
    dist, steps, path, rest = _single(MT, dev, x, y)
    assert dist.dtype == np.float32 and float(dist) == float(m["dist"]), (float(dist), float(m["dist"]))
    assert steps == m["steps"] == len(m["path"])
    assert np.array_equal(path, m["path"]) and not rest.any()
    dir_ = torch.full((1, lx, ly), SENT_U8, dtype=torch.uint8, device=dev)
    d2, s2 = ops.dtw(_t(x, dev)[None], _t(y, dev)[None], dir=dir_)
    assert np.array_equal(dir_[0].cpu().numpy(), m["dir"])
    assert float(d2[0]) == float(dist) and int(s2[0]) == steps
    d3, s3 = MT.dtw(_t(x, dev), _t(y, dev))  # without the path: the same numbers
    assert float(d3) == float(dist) and int(s3) == steps


def test_dtw_ragged_batch_in_sentinel_buffers(ops, dev):
    """B = 5 with mixed lengths inside Tx = 513, Ty = 300.  Inputs beyond a row's length are NaN (a read shows); the outputs are views
    inside sentinel-filled buffers compared whole (nothing outside the live rectangle or beyond `count` is written); each row equals the
    same pair run alone; two runs are bit-identical."""
    B, Tx, Ty, K = 5, 513, 300, 39
    lens_x, lens_y = [513, 257, 1, 256, 300], [300, 64, 300, 1, 65]
    x = np.full((B, Tx, K), np.nan, dtype=np.float32)
    y = np.full((B, Ty, K), np.nan, dtype=np.float32)
    models = []
    for b in range(B):
        xb, yb = MM.grid_pair(lens_x[b], lens_y[b], K, ("34", "122", "236")[b % 3], 7 * b, seed=50 + b)
        x[b, :lens_x[b]], y[b, :lens_y[b]] = xb, yb
        models.append(MM.dtw(xb, yb))
    xd, yd = _t(x, dev), _t(y, dev)
    lx, ly = torch.tensor(lens_x, device=dev), torch.tensor(lens_y, device=dev)
    P = Tx + Ty - 1

    def run():
        big = dict(dist=torch.full((B + 2,), SENT_F32, device=dev), steps=torch.full((B + 2,), SENT_I32, dtype=torch.int32, device=dev),
                   dir=torch.full((B + 2, Tx, Ty), SENT_U8, dtype=torch.uint8, device=dev),
                   path=torch.full((B + 2, P, 2), SENT_I32, dtype=torch.int32, device=dev))
        dist, steps = ops.dtw(xd, yd, lx, ly, dist=big["dist"][1:B + 1], steps=big["steps"][1:B + 1], dir=big["dir"][1:B + 1])
        ops.dtw_path(big["dir"][1:B + 1], steps, lx, ly, path=big["path"][1:B + 1])
        return {k: v.cpu().numpy() for k, v in big.items()}

    got, again = run(), run()
    want = dict(dist=np.full(B + 2, SENT_F32, dtype=np.float32), steps=np.full(B + 2, SENT_I32, dtype=np.int32),
                dir=np.full((B + 2, Tx, Ty), SENT_U8, dtype=np.uint8), path=np.full((B + 2, P, 2), SENT_I32, dtype=np.int32))
    for b, m in enumerate(models):
        want["dist"][1 + b], want["steps"][1 + b] = m["dist"], m["steps"]
        want["dir"][1 + b, :lens_x[b], :lens_y[b]] = m["dir"]
        want["path"][1 + b, :m["steps"]] = m["path"]
    for k in want:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    for b in range(B):  # the same pair alone, in buffers of its own size
        d, s = ops.dtw(_t(x[b:b + 1, :lens_x[b]], dev), _t(y[b:b + 1, :lens_y[b]], dev))
        assert d.cpu().numpy().view(np.uint32)[0] == got["dist"].view(np.uint32)[1 + b] and int(s[0]) == got["steps"][1 + b]


# ---- set_dtw, real-valued ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MM.REAL_CASES, ids=lambda c: "%dx%d-K%d" % c[:3])
def test_dtw_real_valued_path_is_the_models_and_dist_within_the_bound(MT, dev, case):
    lx, ly, K, seed, kind = case
    x, y = MM.real_pair(lx, ly, K, seed, kind)
    m = MM.dtw(x, y)
    dist, steps, path, rest = _single(MT, dev, x, y)
    bound = MM.dist_rel_bound(lx, ly, K)  # (lx + ly + K + 2) 2^-24
    err = abs(float(dist) - float(m["dist"])) / float(m["dist"])
    print("set_dtw %dx%d K=%d (%s): dist %.6f, model %.6f, relative error %.3e, bound %.3e, steps %d"
          % (lx, ly, K, kind, float(dist), float(m["dist"]), err, bound, steps))
    assert steps == m["steps"] and np.array_equal(path, m["path"]) and not rest.any()
    assert err <= bound, (err, bound)


# ---- set_mfcc ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(80, 39), (96, 64), (80, 64), (96, 39)])
@pytest.mark.parametrize("take_log", [False, True])
def test_mfcc_against_the_model(MT, dev, M, K, take_log):
    B, T, lens = 3, 37, [37, 16, 5]  # 16-frame blocks: a whole row, exactly one block, less than one
    rng = np.random.default_rng(M + K)
    mel = rng.standard_normal((B, T, M)) - 3.0
    if take_log:
        mel = 10.0 ** mel
    mel = mel.astype(np.float32)
    feed = mel.copy()
    for b, n in enumerate(lens):
        feed[b, n:] = np.nan  # never read
    out = MT.mfcc(_t(feed, dev), lens, n_mfcc=K, take_log=take_log).cpu().numpy()
    assert out.shape == (B, T, K) and out.dtype == np.float32
    worst = 0.0
    for b, n in enumerate(lens):
        x = mel[b, :n].astype(np.float64)
        want = MM.mfcc(x, K, take_log)
        bar = MM.mfcc_bar(np.log10(x) if take_log else x, M)[:, None]  # (M + 2) 2^-24 sum_n |x_n| per coefficient of a frame
        err = np.abs(out[b, :n].astype(np.float64) - want)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (b, float((err / bar).max()))
        assert not out[b, n:].any() and not np.signbit(out[b, n:]).any()  # exactly +0.0
    print("set_mfcc M=%d K=%d take_log=%d: max error / bar = %.3f" % (M, K, take_log, worst))
    full = MT.mfcc(_t(mel, dev), n_mfcc=K, take_log=take_log)
    one = MT.mfcc(_t(mel[1], dev), n_mfcc=K, take_log=take_log)  # [T, M] -> [T, K]
    assert one.shape == (T, K) and torch.equal(one, full[1]) and torch.equal(full[1, :16], _t(out[1, :16], dev))


# ---- mel_mcd / wav_mcd end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_dtw", [True, False])
def test_mel_mcd_against_the_model(MT, dev, use_dtw):
    """Derived relative tolerance on mcd at K = 39, M = 80, lengths up to 120, log-mels of magnitude ~3 (sum_n |x_n| up to ~270):
    the distance bound ((120 + 97 + 41) 2^-24 = 1.5e-5 with DTW, (41 + 1 + 8) 2^-24 = 3.0e-6 without) + 2 sqrt(39) bar / mean cost
    (bar = 82 x 2^-24 x ~270 = 1.3e-3; mean cost ~8 along a DTW path or between equal lengths: 2.0e-3; ~51 where 23 zero-filled frames
    dominate: 3.1e-4) + 2^-24.  So 2.0e-3 with DTW and 3.1e-4 / 2.0e-3 without; the exact figure is computed per pair below and printed
    (measured errors: at most 2.2e-7)."""
    a, b = MM.e2e_batches()
    mcd, pen, fr = MT.mel_mcd(_t(a, dev), _t(b, dev), list(MM.E2E_LEN_1), list(MM.E2E_LEN_2), use_dtw=use_dtw)
    assert mcd.dtype == torch.float32 and pen.dtype == torch.float32 and fr.dtype == torch.int64 and mcd.is_cuda and pen.is_cuda and fr.is_cuda
    mcd, pen, fr = mcd.cpu().numpy(), pen.cpu().numpy(), fr.cpu().numpy()
    assert np.isfinite(mcd).all()
    for r, (l1, l2) in enumerate(zip(MM.E2E_LEN_1, MM.E2E_LEN_2)):
        m1, m2 = a[r, :l1].astype(np.float64), b[r, :l2].astype(np.float64)
        want_mcd, want_pen, want_fr = MM.mel_mcd(m1, m2, use_dtw=use_dtw)
        tol, _ = MM.e2e_rel_tol(m1, m2, 39, use_dtw)
        err = abs(float(mcd[r]) - want_mcd) / want_mcd
        print("mel_mcd use_dtw=%d pair %d (%d, %d): mcd %.6f, model %.6f, relative error %.3e, tolerance %.3e, frames %d, penalty %.6f"
              % (use_dtw, r, l1, l2, mcd[r], want_mcd, err, tol, fr[r], pen[r]))
        assert fr[r] == want_fr and pen[r] == np.float32(want_pen)
        assert (want_pen > 0) == (l1 != l2)
        assert err <= tol, (err, tol)
        s_mcd, s_pen, s_fr = MT.mel_mcd(_t(a[r, :l1], dev), _t(b[r, :l2], dev), use_dtw=use_dtw)  # the pair alone, [T, M]
        assert s_mcd.shape == () and float(s_mcd) == float(mcd[r]) and float(s_pen) == float(pen[r]) and int(s_fr) == fr[r]


@pytest.mark.parametrize("use_dtw", [True, False])
def test_an_identical_pair_scores_zero(MT, dev, use_dtw):
    a, _ = MM.e2e_batches()
    mel = _t(a[2, :64], dev)
    mcd, pen, fr = MT.mel_mcd(mel, mel.clone(), use_dtw=use_dtw)
    assert float(mcd) == 0.0 and float(pen) == 0.0 and int(fr) == 64


def test_wav_mcd_is_mel_mcd_of_the_log_mels(MT, dev):
    from set_amd.melspec import LogMel
    n = 256 * 20
    t = np.arange(n) / 22050.0
    w1 = _t((0.5 * np.sin(2 * np.pi * 220.0 * t)).astype(np.float32), dev)[None]
    w2 = _t((0.4 * np.sin(2 * np.pi * 330.0 * t)).astype(np.float32)[:256 * 15], dev)[None]
    fe = LogMel(HP, "librosa")
    for use_dtw in (True, False):
        got = MT.wav_mcd(w1, w2, HP, use_dtw=use_dtw)
        want = MT.mel_mcd(fe(w1), fe(w2), use_dtw=use_dtw)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert float(got[0]) > 0 and int(got[2]) >= 21
    got = MT.wav_mcd(w1, w1[:, :256 * 15].contiguous(), HP, [256 * 15], [256 * 15])  # lengths in samples -> frames
    assert float(got[0][0]) == 0.0 and int(got[2][0]) == 16


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(MT, ops, dev):
    from set_amd._lib import SetAmdError
    x, y = torch.zeros(1, 8, 39, device=dev), torch.zeros(1, 9, 39, device=dev)
    mel = torch.zeros(1, 8, 80, device=dev)
    for call in (lambda: MT.dtw(x.cpu(), y), lambda: MT.dtw(x, y.cpu()), lambda: MT.mfcc(mel.cpu()), lambda: MT.mel_mcd(mel.cpu(), mel),
                 lambda: MT.wav_mcd(torch.zeros(4096), torch.zeros(4096), HP)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        MT.dtw(torch.zeros(1, 8, 65, device=dev), torch.zeros(1, 9, 65, device=dev))          # K > 64
    with pytest.raises(SetAmdError, match="set_dtw"):
        ops.dtw(torch.zeros(1, 8, 65, device=dev), torch.zeros(1, 9, 65, device=dev))
    with pytest.raises(SetAmdError, match="set_dtw"):
        ops.dtw(torch.zeros(1, 1, 2, device=dev), torch.zeros(1, 8193, 2, device=dev))        # Ty beyond the boundary buffer
    with pytest.raises(ValueError):
        MT.mfcc(torch.ones(1, 8, 97, device=dev))                                              # M > 96
    with pytest.raises(SetAmdError, match="set_mfcc"):
        ops.mfcc(torch.ones(1, 8, 97, device=dev), torch.ones(39, 97, device=dev))
    with pytest.raises(ValueError):
        MT.mfcc(mel, n_mfcc=65)
    with pytest.raises(ValueError):
        MT.dtw(x, torch.zeros(1, 9, 34, device=dev))                                           # K mismatch
    with pytest.raises(ValueError):
        MT.mel_mcd(mel, torch.zeros(1, 8, 96, device=dev))
    for bad in ([0], [9], [-1]):                                                               # a length of 0 or beyond T
        with pytest.raises(ValueError):
            MT.dtw(x, y, len_x=bad)
        with pytest.raises(ValueError):
            MT.mel_mcd(mel, mel, len_2=bad, use_dtw=True)
    with pytest.raises(ValueError):
        MT.dtw(x, y, len_y=[10])
    with pytest.raises(ValueError):
        MT.dtw(x, y, len_x=[4, 4])
    for kw in (dict(warp=2), dict(w=3), dict(s=1.5)):
        with pytest.raises(NotImplementedError):
            MT.dtw(x, y, **kw)
    with pytest.raises(ValueError):
        MT.dtw(torch.zeros(1, 39, 8, device=dev).transpose(1, 2), y)                           # not contiguous
    with pytest.raises(ValueError):
        MT.mfcc(torch.zeros(1, 80, 8, device=dev).transpose(1, 2))
    with pytest.raises(TypeError):
        MT.dtw(x.double(), y.double())
    # lengths that are already on the device are not brought back to be checked: the kernels read them clamped into [1, T]
    xr, yr = MM.grid_pair(8, 9, 39, "34", 3, seed=1)
    lo = MT.dtw(_t(xr[None], dev), _t(yr[None], dev), len_x=torch.tensor([0], device=dev), len_y=torch.tensor([99], device=dev))
    m = MM.dtw(xr[:1], yr)
    assert float(lo[0][0]) == float(m["dist"]) and int(lo[1][0]) == m["steps"] == 9
    assert math.isfinite(float(lo[0][0]))
