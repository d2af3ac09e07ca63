"""CPU checks of the mel-cepstral distortion path (set_amd.metrics, csrc/mcd.hip's host side): the float64 models of mcd_models.py against
the reference's own DTW, scipy's DCT and the oracle's equal-length MCD; the two conditions the GPU tests lean on (the integer-grid cases are
exact in fp32, the real-valued cases keep a margin at every decision along their optimal path); the DCT table; the entries' refusals on
the built library.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mcd_models as MM


@pytest.fixture(scope="module")
def metrics():
    import set_amd  # noqa: F401
    from set_amd import metrics
    return metrics


def _reference_dtw():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference checkout is not on this machine")
    spec = importlib.util.spec_from_file_location("_ref_metrics_dtw", os.path.join(ref_import.REF_ROOT, "utils", "metrics", "dtw.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.accelerated_dtw


@pytest.mark.parametrize("lx,ly", [(1, 7), (9, 1), (37, 53), (130, 97)])
@pytest.mark.parametrize("kind", ["normal", "grid"])
def test_model_equals_the_reference_dtw(lx, ly, kind):
    """dist, D and path of the model against accelerated_dtw(x, y, 'euclidean'); the carried L[-1, -1] is len(path).  The grid inputs
    are full of exact ties, so the path only agrees if the tie order is _traceback's."""
    accelerated_dtw = _reference_dtw()
    x, y = MM.real_pair(lx, ly, 39, seed=lx) if kind == "normal" else MM.grid_pair(lx, ly, 39, "236", 5, seed=lx)
    x, y = x.astype(np.float64), y.astype(np.float64)
    dist, C, D, path = accelerated_dtw(x, y, "euclidean")
    m = MM.dtw(x, y)
    p, q = np.asarray(list(path[0]), dtype=np.int64), np.asarray(list(path[1]), dtype=np.int64)
    assert np.allclose(m["C"], C, rtol=1e-13, atol=0) and np.allclose(m["D"], D, rtol=1e-12, atol=0)
    assert abs(m["dist"] - dist) <= 1e-12 * dist
    assert np.array_equal(m["path"][:, 0], p) and np.array_equal(m["path"][:, 1], q)
    assert m["steps"] == len(p) == m["L"][-1, -1]


def test_mfcc_model_equals_scipy_dct_and_the_table_its_definition(metrics):
    from scipy.fft import dct
    rng = np.random.default_rng(0)
    for M, K in ((80, 39), (96, 64), (80, 64), (20, 19)):
        x = rng.standard_normal((7, M)) * 3.0 - 4.0
        want = dct(x, type=2, norm=None, axis=-1)[..., 1:K + 1] / 2.0
        assert np.abs(MM.mfcc(x, K) - want).max() <= 1e-13 * np.abs(x).sum(-1).max()
        pos = np.exp(x)
        assert np.abs(MM.mfcc(pos, K, take_log=True) - dct(np.log10(pos), type=2, norm=None, axis=-1)[..., 1:K + 1] / 2.0).max() <= 1e-12 * M
        t32, t64 = metrics.dct_table(K, M), MM.dct_table(K, M)
        assert t32.dtype == np.float32 and t32.shape == (K, M)
        # 1 ulp of fp32; 1e-13 covers the float64 model itself, whose unreduced angle (up to K (2M - 1) pi / (2M) ~ 200 rad) is off by
        # ~200 x 2^-53 -- all that is left to compare where the cosine is 0
        assert (np.abs(t32.astype(np.float64) - t64) <= np.spacing(np.abs(t32)) + 1e-13).all()


def test_mel_mcd_model_equal_lengths_is_the_oracle_and_penalty_by_hand():
    from oracle import oracle as O
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((8, 80)) - 3.0, rng.standard_normal((8, 80)) - 3.0
    mcd, pen, fr = MM.mel_mcd(a[:5], b[:5])
    assert abs(mcd - O.mel_mcd(a[:5], b[:5])) <= 1e-12 * mcd and pen == 0.0 and fr == 5
    for t1, t2 in ((5, 5), (5, 8), (8, 5)):
        mcd, pen, fr = MM.mel_mcd(a[:t1], b[:t2])
        assert fr == max(t1, t2) and pen == 2.0 - (t1 + t2) / max(t1, t2)
        ca, cb = MM.mfcc(a[:t1], 39), MM.mfcc(b[:t2], 39)
        n = min(t1, t2)
        tail = ca[n:] if t1 > t2 else cb[n:]
        by_hand = (np.linalg.norm(ca[:n] - cb[:n], axis=1).sum() + np.linalg.norm(tail, axis=1).sum()) / max(t1, t2)
        assert abs(mcd - by_hand) <= 1e-12 * by_hand
        mcd_d, pen_d, fr_d = MM.mel_mcd(a[:t1], b[:t2], use_dtw=True)
        assert max(t1, t2) <= fr_d <= t1 + t2 - 1 and pen_d == 2.0 - (t1 + t2) / fr_d and 0.0 <= pen_d < 1.0


@pytest.mark.parametrize("case", MM.exact_cases(), ids=lambda c: "%dx%d-K%d-g%s" % c[:4])
def test_integer_grid_cases_are_exact_in_fp32(case):
    """Every D of an exact case is an integer below 2^24, so fp32 holds it and every sum and compare exactly: the fp32 model equals the
    float64 model bit for bit (D, L, path).  The sizable cases hold at least 100 exact ties each, so the tie rule is really exercised."""
    lx, ly, K, grid, off, seed = case
    x, y = MM.grid_pair(lx, ly, K, grid, off, seed)
    m64, m32 = MM.dtw(x, y), MM.dtw(x, y, dtype=np.float32)
    assert np.array_equal(m64["D"], np.rint(m64["D"])) and m64["D"].max() < 2 ** 24
    assert m32["D"].dtype == np.float32 and np.array_equal(m32["D"].astype(np.float64), m64["D"])
    assert np.array_equal(m32["L"], m64["L"]) and np.array_equal(m32["dir"], m64["dir"]) and np.array_equal(m32["path"], m64["path"])
    assert m64["steps"] == len(m64["path"])
    if min(lx, ly) > 32:
        assert MM.count_ties(m64) >= 100, MM.count_ties(m64)


@pytest.mark.parametrize("case", MM.REAL_CASES, ids=lambda c: "%dx%d-K%d" % c[:3])
def test_real_valued_cases_keep_the_margin_along_the_optimal_path(case):
    """The smallest relative predecessor gap along the float64 optimal path is at least 4 x the derived bound on the fp32 kernel's
    relative error in D; where it holds, the fp32 path must be the float64 path."""
    lx, ly, K, seed, kind = case
    x, y = MM.real_pair(lx, ly, K, seed, kind)
    m = MM.dtw(x, y)
    gap, need = MM.path_min_gap(m), 4.0 * MM.dist_rel_bound(lx, ly, K)
    print("%dx%d K=%d: smallest gap on the path %.3e, 4 x bound %.3e" % (lx, ly, K, gap, need))
    assert gap >= need, (gap, need)


def test_end_to_end_pairs_keep_the_margin_with_the_mfcc_bar_included():
    """The pairs test_gpu_mcd.py scores end to end: their path is decided on MFCCs that are themselves within `bar` of the model's, which
    moves a cost by at most 2 sqrt(K) bar and so any D by that relative to the smallest cost.  The smallest gap along the float64
    optimal path is at least 4 x (that + the kernel's own bound); then `frames` is the model's exactly.  Both lengths differ, so penalty > 0."""
    a, b = MM.e2e_batches()
    for r, (l1, l2) in enumerate(zip(MM.E2E_LEN_1, MM.E2E_LEN_2)):
        assert np.isnan(a[r, l1:]).all() and np.isnan(b[r, l2:]).all() and np.isfinite(a[r, :l1]).all() and np.isfinite(b[r, :l2]).all()
        m = MM.dtw(MM.mfcc(a[r, :l1], 39), MM.mfcc(b[r, :l2], 39))
        bar = max(MM.mfcc_bar(a[r, :l1], 80).max(), MM.mfcc_bar(b[r, :l2], 80).max())
        need = 4.0 * (MM.dist_rel_bound(l1, l2, 39) + 2.0 * np.sqrt(39.0) * bar / m["C"].min())
        gap = MM.path_min_gap(m)
        print("pair %d (%d x %d): smallest gap on the path %.3e, 4 x bound %.3e, steps %d" % (r, l1, l2, gap, need, m["steps"]))
        assert gap >= need, (r, gap, need)
        mcd, pen, fr = MM.mel_mcd(a[r, :l1], b[r, :l2], use_dtw=True)
        assert fr == m["steps"] and (pen > 0.0) == (l1 != l2)


def test_entries_refuse_on_the_host(built_lib, metrics):
    from set_amd import _lib
    L = built_lib
    p = 4096  # any non-null address: the checks below all fail before a launch
    assert L.set_mfcc(p, None, p, p, 1, 8, 80, 65, 0, None) == _lib.E_UNSUPPORTED and b"set_mfcc" in L.set_last_error()
    assert L.set_mfcc(p, None, p, p, 1, 8, 97, 39, 0, None) == _lib.E_UNSUPPORTED
    assert L.set_mfcc(None, None, p, p, 1, 8, 80, 39, 0, None) == _lib.E_INVALID
    assert L.set_mfcc(p, None, p, p, 1, 0, 80, 39, 0, None) == _lib.E_INVALID
    assert L.set_dtw(p, p, None, None, p, p, None, 1, 8, 8, 65, None) == _lib.E_UNSUPPORTED and b"set_dtw" in L.set_last_error()
    assert L.set_dtw(p, p, None, None, p, p, None, 1, 8, 8193, 39, None) == _lib.E_UNSUPPORTED
    assert L.set_dtw(p, p, None, None, None, p, None, 1, 8, 8, 39, None) == _lib.E_INVALID
    assert L.set_dtw(p, p, None, None, p, p, None, 0, 8, 8, 39, None) == _lib.E_INVALID
    assert L.set_dtw_path(None, None, None, p, p, 1, 8, 8, None) == _lib.E_INVALID
    assert L.set_zero_fill_dist(p, p, None, None, p, 1, 8, 8, 65, None) == _lib.E_UNSUPPORTED
    assert L.set_mcd_finish(p, None, None, None, p, p, None, 1, 8, 8, None) == _lib.E_INVALID
    a, b = torch.zeros(1, 8, 80), torch.zeros(1, 9, 80)
    for call in (lambda: metrics.mfcc(a), lambda: metrics.dtw(a, b), lambda: metrics.mel_mcd(a, b), lambda: metrics.mel_mcd(a, b, use_dtw=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for kw in (dict(warp=2), dict(w=5), dict(s=1.2)):
        with pytest.raises(NotImplementedError):
            metrics.dtw(a, b, **kw)
