"""CPU checks of the wav-level MCD's float64 model (wavmcd_models.py), of the host tables the kernels take (melspec.htk_mel_basis,
metrics.dct_ortho_table) and of the conditions the GPU cases of test_gpu_wavmcd.py stand on.  Neither librosa nor the reference's
eval/mcd.py runs here: the model is pinned to scipy where scipy has the piece (DCT, window), to the published HTK formula, and to
properties of the filterbank's definition -- not to librosa's array."""
import numpy as np
import pytest
import scipy.fft
import scipy.signal

import wavmcd_models as W


@pytest.fixture(scope="module")
def pkg():
    import set_amd  # noqa: F401
    from set_amd import melspec, metrics
    return melspec, metrics


@pytest.fixture(scope="module")
def cases():
    """name -> (y, float64 dB, bars) of the three clamp cases, computed once."""
    out = {}
    for name in W.CLAMP_CASES:
        y = W.clamp_case(name)
        out[name] = (y,) + W.db_bars(y)
    return out


# ---- what the model is pinned to --------------------------------------------------------------------------------------------------------------
def test_dct_is_scipys_orthonormal_dct(pkg):
    x = np.random.default_rng(0).standard_normal((7, 80))
    want = scipy.fft.dct(x, type=2, norm="ortho", axis=1)[:, :34]
    assert np.abs(x @ W.dct_ortho(34).T - want).max() < 1e-13
    t = pkg[1].dct_ortho_table(34, 80)
    assert t.dtype == np.float32 and t.shape == (34, 80)
    assert np.array_equal(t, W.dct_ortho(34).astype(np.float32))  # float64 rounded once
    assert np.array_equal(pkg[1].dct_ortho_table(1, 80), np.full((1, 80), np.sqrt(1.0 / 80), dtype=np.float32))


def test_window_is_scipys_periodic_hann(pkg):
    want = scipy.signal.get_window("hann", 1024, fftbins=True)
    assert np.abs(W.WIN64 - want).max() < 1e-15
    assert np.abs(pkg[0].hann_padded(1024, 1024) - want).max() < 1e-15


def test_htk_scale():
    assert abs(float(W.hz_to_mel(1000.0)) - 999.98553714) < 1e-8
    f = np.array([55.0, 700.0, 7600.0])
    assert np.abs(W.mel_to_hz(W.hz_to_mel(f)) - f).max() < 1e-9


def test_filterbank_properties(pkg):
    b = W.BASIS64
    assert b.shape == (80, 513) and (b >= 0).all() and (b.sum(1) > 0).all()  # every row non-empty
    cols = np.nonzero((b != 0).any(0))[0]
    assert (cols[0], cols[-1]) == (3, 352)
    e = W.htk_edges()
    assert abs(e[0] - 55.0) < 1e-9 and abs(e[-1] - 7600.0) < 1e-9 and np.abs(np.diff(W.hz_to_mel(e), 2)).max() < 1e-9  # equal in mel
    hz = np.arange(513) * W.SR / W.NFFT
    for m in range(80):
        # a triangle of height 2 / (f_{m+2} - f_m): the continuous area is 1; sampled at the bins, the slopes are those of the definition
        inside = (hz > e[m]) & (hz < e[m + 2])
        assert np.array_equal(inside, b[m] > 0)
        up = inside & (hz <= e[m + 1])
        assert np.abs(b[m][up] - 2.0 / (e[m + 2] - e[m]) * (hz[up] - e[m]) / (e[m + 1] - e[m])).max(initial=0) < 1e-15
        assert b[m].max() <= 2.0 / (e[m + 2] - e[m]) + 1e-18
        k = np.argmax(b[m])  # the peak is at the bin next to the mel-spaced centre
        assert abs(hz[k] - e[m + 1]) <= W.SR / W.NFFT
    got = pkg[0].htk_mel_basis(W.SR, W.NFFT, 80, 55, 7600)
    assert got.dtype == np.float32 and np.array_equal(got, W.BASIS32)
    assert pkg[0].bin_range(got) == (0, 384)  # bins 3 .. 352 widened to whole 32-bin chunks


def test_slaney_filterbank_is_what_it_was(pkg):
    """htk_mel_basis shares its triangles with slaney_mel_basis: the Slaney rows are still those of the definition."""
    b = pkg[0].slaney_mel_basis(22050, 1024, 80, 80, -1)
    e = pkg[0]._mel_to_hz(np.linspace(pkg[0]._hz_to_mel(80.0), pkg[0]._hz_to_mel(11025.0), 82))
    hz = np.linspace(0.0, 11025.0, 513)
    for m in (0, 40, 79):
        want = np.maximum(0.0, np.minimum((hz - e[m]) / (e[m + 1] - e[m]), (e[m + 2] - hz) / (e[m + 2] - e[m + 1]))) * 2.0 / (e[m + 2] - e[m])
        assert np.array_equal(b[m], want.astype(np.float32))


def test_power_to_db_and_distance_by_hand():
    S = np.array([[1.0, 1e-12], [100.0, 1e-3]])
    d = W.DB_C * np.log(np.maximum(W.AMIN, S))
    assert np.abs(d - [[0.0, -100.0], [20.0, -30.0]]).max() < 1e-12
    assert np.abs(W.clamp(d, 80.0) - [[0.0, -60.0], [20.0, -30.0]]).max() < 1e-12
    # [T = 2, K = 2]: the squared differences are summed over the frames, one value per coefficient
    a, b = np.array([[0.0, 0.0], [0.0, 0.0]]), np.array([[3.0, 1.0], [4.0, 1.0]])
    want = (W.DB_C * np.sqrt(2 * 25.0) + W.DB_C * np.sqrt(2 * 2.0)) / 2 / 2
    assert abs(W.cal_mcd(a, b) - want) < 1e-14
    assert W.rms_dist_kernel_order(a, b) == np.float32(want)


def test_frame_counts_and_reflection(pkg):
    for n, t in ((513, 3), (600, 3), (767, 3), (768, 4), (63 * 256, 64), (64 * 256, 65), (129 * 256, 130)):
        assert W.n_frames(n) == t == pkg[1].htk_frames(n) and W.frames_of(np.zeros(n)).shape == (t, 1024)
    assert W.n_frames(512) == 0 == pkg[1].htk_frames(512)
    y = np.arange(600, dtype=np.float64)
    fr = W.frames_of(y)
    assert fr[0, 0] == 512 and fr[0, 511] == 1 and fr[0, 512] == 0 and fr[2, -1] == 2 * 599 - (2 * 256 + 1023 - 512)
    assert all(pkg[0].reflect_index(i, 600, 512) == fr[0, i] for i in range(1024))


def test_packed_images_round_trip(pkg):
    ms = pkg[0]
    lo, hi = ms.bin_range(W.BASIS32)
    tab = ms.dft_table(1024, 1024, lo, hi - lo)
    assert np.array_equal(ms.unpack_dft_table(ms.pack_dft_table(tab), hi - lo), tab)
    assert np.array_equal(tab, W.dft32()[:, lo:hi])
    img = ms.pack_mel_basis(W.BASIS32, lo, hi - lo)  # [chunk][r][lane][4]
    r, lane = np.arange(16)[:, None], np.arange(64)[None, :]
    bins = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    for ch in range(img.shape[0]):
        for e in range(3):
            rows = 32 * e + (lane & 31)
            want = np.where(rows < 80, W.BASIS32[np.minimum(rows, 79), np.minimum(lo + 32 * ch + bins, 512)], 0.0)
            assert np.array_equal(img[ch, :, :, e], want)
    assert not img[..., 3].any()


def test_all_zero_waveform():
    c = W.mfcc(np.zeros(W.N_SIG, dtype=np.float32))
    assert np.abs(W.db(np.zeros(2048, dtype=np.float32)) + 100.0).max() < 1e-12
    assert np.abs(c[:, 0] + 100.0 * np.sqrt(80.0)).max() < 1e-11 and np.abs(c[:, 1:]).max() < 1e-12


# ---- the conditions the GPU cases stand on ------------------------------------------------------------------------------------------------------
def test_clamp_cases_clamp_what_they_should(cases):
    share, _ = W.clamped_share(cases["unclamped"][0])
    assert share == 0.0
    y = cases["zero_gap"][0]
    share, d = W.clamped_share(y)
    assert abs(share - 0.208) < 0.002
    rows = np.nonzero((d < d.max() - W.TOP_DB).any(1))[0]
    fr = W.frames_of(y)
    assert not fr[rows].any() and np.abs(d[rows] + 100.0).max() < 1e-12  # all from frames that are wholly zero
    share, _ = W.clamped_share(cases["noise_floor"][0])
    assert 0.10 <= share <= 0.80 and abs(share - 0.24) < 0.01
    assert abs(W.clamped_share(W.signal(3e-4))[0] - 0.69) < 0.01


def test_bars_hold_the_float32_mirror_and_are_not_slack(cases):
    """A bar below the mirror's error is wrong; one more than 100 x above it tests nothing.  Entry by entry the mirror uses at most the
    whole bar, and on its worst entry at least 1 % of it.  The MFCC bar is the triangle-inequality sum of 80 dB bars, which errors of
    independent sign fill to about 1 / sqrt(80): its worst use is asserted over the three cases together."""
    worst_mfcc = 0.0
    for name, (y, bar, peak_bar, cbar, d64) in cases.items():
        d32 = W.db32(y).astype(np.float64)
        use = np.abs(d32 - d64) / bar
        print("%s: mirror dB error %.2e, worst use of the dB bar %.3f, largest bar %.2e" % (name, np.abs(d32 - d64).max(), use.max(), bar.max()))
        assert 0.01 <= use.max() <= 1.0
        assert abs(d32.max() - d64.max()) <= peak_bar
        x64, x32 = W.clamp(d64), np.maximum(d32, d32.max() - 80.0)
        assert (np.abs(x32 - x64) <= cbar).all()
        mbar = W.mfcc_bars(cbar, x64, W.NMFCC)
        err = np.abs(W.mfcc32(y).astype(np.float64) - W.mfcc(y))
        print("%s: mirror MFCC error %.2e at |c| <= %.0f, worst use of the MFCC bar %.3f" % (name, err.max(), np.abs(W.mfcc(y)).max(),
                                                                                          (err / mbar).max()))
        assert (err <= mbar).all()
        worst_mfcc = max(worst_mfcc, float((err / mbar).max()))
    assert worst_mfcc >= 0.01


def test_score_allowance_holds_the_mirror(cases):
    y = cases["unclamped"][0]
    z = W.degraded(y)
    (_, _, cb1, d1), (_, _, cb2, d2) = W.db_bars(y), W.db_bars(z)
    c1, c2 = W.mfcc(y), W.mfcc(z)
    bar = W.mcd_bar(c1, c2, W.mfcc_bars(cb1, W.clamp(d1), W.NMFCC), W.mfcc_bars(cb2, W.clamp(d2), W.NMFCC))
    want = W.cal_mcd(c1, c2)
    print("mcd %.6f, mirror off by %.2e, allowance %.2e" % (want, abs(W.mcd32(y, z) - want), bar))
    assert abs(W.mcd32(y, z) - want) <= bar < 0.01 * want


def test_host_refusals_need_no_gpu(pkg):
    import torch
    with pytest.raises(RuntimeError):
        pkg[1].htk_mfcc(torch.zeros(2, 4096))
    with pytest.raises(RuntimeError):
        pkg[1].wav_mcd_htk(torch.zeros(4096), torch.zeros(4096))


def test_dtw_pair_keeps_a_margin_and_the_mirror_takes_the_models_path():
    """The fading pair of the GPU DTW test: along the model's path the best predecessor leads the second by more than 4 x the fp32 DTW's
    own bound (mcd_models.dist_rel_bound), nothing is clamped, and the float32 mirror walks the same path."""
    import mcd_models as MM
    y, z = W.ramp_pair()
    assert W.clamped_share(y)[0] == 0.0 and W.clamped_share(z)[0] == 0.0
    want, m = W.mcd_dtw(W.mfcc(y), W.mfcc(z))
    m32 = MM.dtw(W.mfcc32(y), W.mfcc32(z), dtype=np.float32)
    gap, bound = MM.path_min_gap(m), MM.dist_rel_bound(130, 121, W.NMFCC)
    print("dtw pair: mcd %.6f over %d steps, smallest gap on the path %.2e against 4 x %.2e" % (want, m["steps"], gap, bound))
    assert m["steps"] == 130 and gap > 4 * bound and np.array_equal(m32["path"], m["path"])
    assert abs(float(m32["dist"]) / m32["steps"] - want) < 1e-4
