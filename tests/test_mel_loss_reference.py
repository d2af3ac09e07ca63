"""CPU checks of the mel loss's float64 model (mel_loss_models.py) and of the conditions the GPU tests (test_gpu_mel_loss.py) stand on:
the model against torch's own stft + autograd in float64, its gradient against finite differences of its loss, the fold, the clamp and
floor masks, the kernel images' element maps, and -- per fixture -- the bars derived from a float32 mirror and the share of entries
whose sign / floor decision is within four of the mirror's errors."""
import numpy as np
import pytest

import mel_loss_models as LM
from mel_loss_models import FLOOR, HOP, MAG_EPS, N_FFT, PAD


@pytest.fixture(scope="module")
def M():
    import set_amd  # noqa: F401
    from set_amd import melspec
    return melspec


@pytest.mark.parametrize("name", ["mel80", "win600", "narrow20"])
def test_model_matches_torch_stft_and_autograd_in_float64(name):
    """Same float32 inputs and filterbank, unrounded float64 window / twiddles on both sides; the input carries the clamp probe (samples
    beyond +-1 and exactly at +-1.0).  Bound: a DFT sum has 1024 terms, so its rounding error is at most 1024 u sum|terms| with u = 2^-53;
    against the result that is a factor sum|terms| / |result|, ~sqrt(1024) = 32 for noise-like frames and at most ~1e3 for the smallest
    bins of these fixtures: 1024 * 1e3 * 1.1e-16 ~ 1e-10 relative on a magnitude, which ln and 1 / mel pass on one to one.  The loss, a
    mean of O(1) terms, and the gradient relative to its largest element are held to 1e-9."""
    bk = LM.bank(name)
    y_hat, y = LM.pair(2, 5000, seed=3)
    y_hat, beyond, at = LM.clamp_probe(y_hat)
    t64 = LM.dft_table64(bk.win, bk.bin_lo, bk.nbins)
    loss, grad, _ = LM.loss_and_grad(y_hat, y, bk, np.float64, table=t64)
    tl, tg = LM.torch_loss_and_grad(y_hat, y, bk)
    print("%s: model loss %.12f, torch %.12f; max |d grad| / max |grad| = %.3e" % (name, loss, tl, np.abs(grad - tg).max() / np.abs(tg).max()))
    assert abs(loss - tl) <= 1e-9
    assert np.abs(grad - tg).max() <= 1e-9 * np.abs(tg).max()
    assert not grad[0, beyond].any() and not tg[0, beyond].any()          # beyond the clamp: exactly 0
    assert np.all(grad[0, at] != 0) and np.all(tg[0, at] != 0)            # exactly +-1.0: the gradient passes


def test_gradient_matches_central_differences_of_the_models_own_loss():
    """h = 1e-5 along unit directions: truncation ~ h^2 |f'''|, rounding ~ u |loss| / h = 1e-11; held to 1e-5 of the gradient's norm.  No
    sign or floor decision changes within the step (asserted), so the loss is smooth on it."""
    bk = LM.bank("mel80")
    y_hat, y = LM.pair(1, 2000, seed=7)
    x = y_hat.astype(np.float64)
    _, grad, parts = LM.loss_and_grad(x, y, bk)
    rng = np.random.default_rng(0)
    h = 1e-5
    for _ in range(3):
        v = rng.standard_normal(x.shape)
        v /= np.linalg.norm(v)
        lp, _, pp = LM.loss_and_grad(x + h * v, y, bk)
        lm, _, pm = LM.loss_and_grad(x - h * v, y, bk)
        for q in (pp, pm):
            assert np.array_equal(np.sign(q["d"]), np.sign(parts["d"])) and np.array_equal(q["passed"], parts["passed"])
        fd, an = (lp - lm) / (2 * h), float((grad * v).sum())
        print("finite difference %.9e, analytic %.9e" % (fd, an))
        assert abs(fd - an) <= 1e-5 * np.linalg.norm(grad)


@pytest.mark.parametrize("n", [512, 1000, 385, 2048 + 17])
def test_fold_gather_form_equals_the_scatter_by_the_pad_index(n):
    rng = np.random.default_rng(n)
    g_p = rng.integers(-1000, 1000, n + 2 * PAD).astype(np.float64)       # integers: both orders of addition are exact
    want = np.zeros(n)
    np.add.at(want, LM.pad_index(n), g_p)
    assert np.array_equal(LM.fold(g_p, n), want)
    hits = LM.fold(np.ones(n + 2 * PAD), n)
    if n - 1 > PAD:                                                       # (else each mirror reaches the far edge sample)
        assert hits[0] == 1 and hits[n - 1] == 1                          # the edge samples are not repeated
    if n == 512:                                                          # both mirrors land on samples 127 .. 384
        assert np.all(hits[127:385] == 3) and np.all(hits[1:127] == 2) and np.all(hits[385:511] == 2)


def test_tail_beyond_the_last_frame_is_mirror_samples_only():
    """N = 1000: T = 3 frames cover padded samples [0, 1536) of 1768.  The 232 uncovered ones all lie in the right reflect pad (fewer
    than hop <= PAD of them, for every N), so every sample of the row itself is under a frame; what the uncovered ones withhold is their
    mirror's share, and the padded gradient is exactly 0 there."""
    n = 1000
    assert LM.n_frames(n) == 3
    covered = (LM.n_frames(n) - 1) * HOP + N_FFT
    assert covered == 1536 and covered >= PAD + n
    for m in (385, 512, 1000, 4096 + 255):
        assert m + 2 * PAD - ((LM.n_frames(m) - 1) * HOP + N_FFT) < HOP <= PAD
    bk = LM.bank("mel80")
    y_hat, _ = LM.pair(1, n, seed=n % 97)
    g_mel = LM.given_g_mel(1, n, 80)
    g_p = LM.padded_grad(y_hat[0], g_mel[0], bk, np.float64)
    assert not g_p[covered:].any() and np.count_nonzero(g_p[:covered]) > 0.99 * covered
    want = LM.wave_grad(y_hat, g_mel, bk, np.float64)[0]
    assert np.allclose(LM.fold(g_p[:covered], n), want, rtol=0, atol=1e-18 + 1e-12 * np.abs(want).max())


def test_clamp_mask_at_and_beyond_the_ends():
    bk = LM.bank("mel80")
    y_hat, _ = LM.pair(1, 2000, seed=7)
    w, beyond, at = LM.clamp_probe(y_hat)
    assert w[0, beyond[0]] > 1 and -1.0000002 < w[0, beyond[1]] < -1 and w[0, at[0]] == 1 and w[0, at[1]] == -1
    g_mel = LM.given_g_mel(1, 2000, 80)
    g = LM.wave_grad(w, g_mel, bk, np.float64)[0]
    assert not g[beyond].any() and np.all(g[at] != 0)
    # the unmasked value: the same clamped signal with the hot samples set to the ends gives the same gradient elsewhere
    c = np.clip(w, -1.0, 1.0)
    gc = LM.wave_grad(c, g_mel, bk, np.float64)[0]
    keep = np.ones(2000, dtype=bool)
    keep[beyond] = False
    assert np.array_equal(g[keep], gc[keep]) and np.all(gc[beyond] != 0)


@pytest.mark.parametrize("name", LM.BANKS)
def test_floor_mask_on_silence(name):
    """A frame of zeros has mel = sqrt(1e-9) * sum of a filterbank row, which lies under the floor 1e-5 for these filterbanks (asserted):
    such entries pass no gradient, and samples under silent frames only get exactly 0."""
    bk = LM.bank(name)
    silent_mel = np.sqrt(MAG_EPS) * bk.basis.astype(np.float64).sum(axis=1)
    print("%s: largest silent mel %.3e (floor %.1e)" % (name, silent_mel.max(), FLOOR))
    assert silent_mel.max() < 0.9 * FLOOR
    y_hat, y = LM.pair(1, 16 * HOP, seed=2)
    y_hat = np.array(y_hat, copy=True)
    y_hat[0, 3 * HOP:11 * HOP] = 0.0
    _, grad, parts = LM.loss_and_grad(y_hat, y, bk)
    silent = [t for t in range(LM.n_frames(16 * HOP)) if t * HOP - PAD >= 3 * HOP and t * HOP - PAD + N_FFT <= 11 * HOP]
    assert len(silent) >= 4
    assert not parts["passed"][0, silent].any() and not parts["g_mel"][0, silent].any()
    lo, hi = silent[0] * HOP - PAD + N_FFT - HOP, silent[-1] * HOP - PAD + HOP   # samples no other frame reaches
    assert hi > lo and not grad[0, lo:hi].any()


def test_kernel_images_follow_their_documented_element_maps(M):
    bk = LM.bank("narrow20")
    rng = np.random.default_rng(1)
    bt = M.pack_mel_basis_t(bk.basis, bk.bin_lo, bk.nbins)
    nch = (bk.nbins + 31) // 32
    assert bt.shape == (nch, 48, 64) and bt.dtype == np.float32
    for _ in range(2000):
        ch, s, lane = rng.integers(nch), rng.integers(48), rng.integers(64)
        m, f = 2 * s + (lane >> 5), 32 * ch + (lane & 31)
        want = bk.basis[m, bk.bin_lo + f] if m < bk.n_mels and f < bk.nbins else 0.0
        assert bt[ch, s, lane] == want
    it = M.pack_idft_table(bk.table)
    assert it.shape == (nch, 4, 4, 2, 16, 64, 2) and it.size == 2 * nch * 32 * N_FFT
    for _ in range(4000):
        ch, w, q, part, s, lane, e = (rng.integers(k) for k in it.shape)
        f, n = 32 * ch + 2 * s + (lane >> 5), 256 * q + 64 * w + 32 * e + (lane & 31)
        assert it[ch, w, q, part, s, lane, e] == (bk.table[part, f, n] if f < bk.nbins else 0.0)
    assert np.count_nonzero(it) == np.count_nonzero(bk.table) and np.count_nonzero(bt) == np.count_nonzero(bk.basis)


def test_loss_launch_restatement_agrees_with_the_mirror():
    bk = LM.bank("mel80")
    y_hat, y = LM.pair(3, 130 * 256 + 17, seed=(130 * 256 + 17) % 97)
    mh, my = LM.linear_mel(y_hat, bk, np.float32), LM.linear_mel(y, bk, np.float32)
    loss, g, d, _ = LM.loss_and_g_mel(mh, my, np.float32)
    assert mh.size > 4096 * 7                                            # several blocks, a ragged last one
    rl, rg = LM.loss_launch_f32(mh, LM.log_mel(mh, np.float32), LM.log_mel(my, np.float32))
    assert rl.dtype == np.float32 and abs(float(rl) - float(np.abs(d.astype(np.float64)).mean())) <= 2.0 ** -24 * 20 * float(rl)
    assert np.array_equal(rg, (g.astype(np.float64) * g.size).astype(np.float32)) or np.abs(rg - g.astype(np.float64) * g.size).max() <= 2.0 ** -22 * np.abs(rg).max()
    part = np.random.default_rng(0).random((151, 64)).astype(np.float32)
    assert np.allclose(LM.rows_sum_f32(part), part.astype(np.float64).sum(axis=0), rtol=1e-6)


@pytest.mark.parametrize("name,B,n", LM.ALL_CASES)
def test_derived_bars_and_decision_margins(name, B, n):
    d = LM.derived(name, B, n)
    print("%s B=%d N=%d: loss %.6f, bars (4 x float32 mirror): %s, undecided share %.2e" % (
        name, B, n, d["loss"], ", ".join("%s %.3e" % kv for kv in sorted(d["bars"].items())), d["share"]))
    assert d["share"] <= LM.UNDECIDED_CAP
    assert all(np.isfinite(v) and v > 0 for v in d["bars"].values())
    # the bars are roundings, not slack: float32 carries 2^-24; a 1024-term sum of it stays far below these
    assert d["bars"]["mel"] <= 1e-3 * d["parts"]["mel_hat"].max() and d["bars"]["loss"] <= 1e-4 * d["loss"] \
        and abs(float(LM.loss_and_g_mel(LM.linear_mel(d["y_hat"], d["bank"], np.float32), LM.linear_mel(d["y"], d["bank"], np.float32),
                                        np.float32)[0]) - d["loss"]) <= d["bars"]["loss"] / LM.BAR_FACTOR
    assert d["bars"]["g_wav"] <= 1e-3 * np.abs(d["gw_given"]).max() and d["bars"]["grad"] <= 1e-2 * np.abs(d["grad"]).max()


def test_refusals_that_need_no_gpu():
    import torch
    from set_amd.vocoder_losses import MelSpectrogramLoss, mel_l1_loss
    fn = MelSpectrogramLoss(LM.HP)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(torch.zeros(2, 4096), torch.zeros(2, 4096))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_l1_loss(torch.zeros(2, 4096), torch.zeros(2, 4096), LM.HP)
    for over in ({"hop_size": 128}, {"fft_size": 2048, "win_size": 2048}, {"audio_num_mel_bins": 128}):
        with pytest.raises(ValueError):
            MelSpectrogramLoss(dict(LM.HP, **over))
