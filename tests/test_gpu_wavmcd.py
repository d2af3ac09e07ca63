"""GPU checks of the wav-level MCD (csrc/wav_mcd.hip through set_amd.ops and set_amd.metrics) against the models of wavmcd_models.py,
launch by launch and end to end.  The dB mel lies within the bars derived in wavmcd_models.s_bound / db_bars; the peak is bit for bit the
maximum of the GPU's own dB; the clamped DCT, fed the GPU's dB, lies within the FMA chain's bar; the distance on integer-valued
coefficients is bit for bit the float64 value rounded once; end to end the bars are the propagated ones (test_wavmcd_reference.py checks
each against the float32 mirror).  Every kernel output is a view inside a sentinel-filled buffer that is compared whole.

Measured on the MI355X (profiles/wav_mcd_gpu_accuracy.log): see test_report_measured_maxima."""
import functools

import numpy as np
import pytest
import torch

import wavmcd_models as W

pytestmark = pytest.mark.gpu

SENT_F32, GUARD = -12345.0, 64
MEASURED = {}  # name of a bar -> the largest fraction of it seen


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _note(name, frac):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(frac))


def _within(name, got, want, bar):
    """|got - want| <= bar everywhere (bar 0: equal), the worst fraction noted and printed before the assertion."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    print("%s: largest error %.3e, worst fraction of its bar %.3g" % (name, err.max(), frac.max()))
    _note(name.split("[")[0], frac.max())
    assert frac.max() <= 1.0, name


class Sent:
    """A contiguous view of `shape` in the middle of a buffer filled with a sentinel; get(): the view's contents after checking the guards."""

    def __init__(self, shape, dev, dtype=torch.float32, sentinel=SENT_F32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        self.sentinel, self.shape = sentinel, shape

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.sentinel).all() and (b[-GUARD:] == self.sentinel).all(), "written outside the output"
        return b[GUARD:-GUARD].reshape(self.shape)


def _batch(rows):
    """rows of unequal length -> ([B, N] float32 with NaN beyond each row's length -- a read there shows --, lengths)."""
    N = max(len(r) for r in rows)
    out = np.full((len(rows), N), np.nan, dtype=np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int64)


def _db_mel(ops, MT, dev, wav, lens=None):
    table, basis, lo, nbins, n_mels = MT._htk_images(dev)
    B, N = wav.shape
    out = Sent((B, 1 + N // 256, n_mels), dev)
    ops.db_mel(_t(wav, dev), table, basis, None if lens is None else _t(lens, dev), n_mels=n_mels, bin_lo=lo, nbins=nbins, out=out.view)
    return out.get()


@functools.lru_cache(maxsize=None)
def _model(name, n=W.N_SIG):
    """(y, dB bar, peak bar, clamped-dB bar, float64 dB) of a named signal, computed once."""
    if name.startswith("ramp"):
        y = W.ramp_pair(n)[name == "ramp_short"]
    elif name == "zeros":
        y = np.zeros(n, dtype=np.float32)
    else:
        y = W.degraded(W.clamp_case(name[:-4], n)) if name.endswith("_deg") else W.clamp_case(name, n)
    return (y,) + W.db_bars(y)


# ---- set_db_mel ---------------------------------------------------------------------------------------------------------------------------
TILE_N = {3: 600, 64: 63 * 256, 65: 64 * 256, 129: 128 * 256}


@pytest.mark.parametrize("T", sorted(TILE_N))
def test_db_mel_at_the_tile_edges(ops, MT, dev, T):
    """The first tile alone, a full tile, one frame into the second, a third tile; reflection reaches the first and the last frames."""
    y, bar, _, _, d64 = _model("unclamped", TILE_N[T])
    got = _db_mel(ops, MT, dev, y[None])
    assert got.shape == (1, T, 80) and W.n_frames(len(y)) == T
    _within("db_mel[T=%d]" % T, got[0], d64, bar)


def test_db_mel_ragged_batch_with_padding_tiles(ops, MT, dev):
    """Rows of 130, 3 and 65 frames in a batch of three 64-frame tiles: the short row's second and third tiles are collater padding.
    Each row equals the same waveform run alone bit for bit; frames beyond a row's own are +0.0; nothing past a length is read (NaN)."""
    rows = [_model("unclamped", n)[0] for n in (129 * 256 + 17, 600, 64 * 256 + 5)]
    wav, lens = _batch(rows)
    got = _db_mel(ops, MT, dev, wav, lens)
    assert not np.isnan(got).any()
    for b, y in enumerate(rows):
        Tb = W.n_frames(len(y))
        alone = _db_mel(ops, MT, dev, y[None])[0]
        assert np.array_equal(_bits(got[b, :Tb]), _bits(alone)), "row %d differs from its single run" % b
        assert not _bits(got[b, Tb:]).any(), "pad frames of row %d are not +0.0" % b
        _, bar, _, _, d64 = _model("unclamped", len(y))
        _within("db_mel[ragged row %d]" % b, got[b, :Tb], d64, bar)


# ---- set_db_peak --------------------------------------------------------------------------------------------------------------------------
def test_db_peak_is_the_maximum_of_the_gpus_own_db_bit_for_bit(ops, MT, dev):
    """A quiet utterance (every dB negative) beside pad frames of +0.0, a loud one, a row without frames (-inf)."""
    loud = _model("unclamped")[0]
    rows = [loud, (1e-4 * loud[:70 * 256]).astype(np.float32), loud[:600], loud[:400]]
    wav, lens = _batch(rows)
    db = _db_mel(ops, MT, dev, wav, lens)
    frames = np.array([W.n_frames(len(r)) for r in rows], dtype=np.int64)
    assert frames[3] == 0 and db[1, :frames[1]].max() < 0.0 and not db[1, frames[1]:].any()
    peak = Sent((4,), dev)
    ops.db_peak(_t(db, dev), _t(frames, dev), peak=peak.view)
    want = np.array([db[b, :frames[b]].max() if frames[b] else -np.inf for b in range(4)], dtype=np.float32)
    assert np.array_equal(_bits(peak.get()), _bits(want))
    full = Sent((4,), dev)
    ops.db_peak(_t(db, dev), None, peak=full.view)  # no frame counts: the whole array, pad frames included
    assert np.array_equal(_bits(full.get()), _bits(db.reshape(4, -1).max(1)))


# ---- set_db_mfcc --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clamp_batch(ops, MT, dev):
    """The three clamp cases and the all-zero waveform through set_db_mel and set_db_peak: (names, dB on the GPU, dB, peak)."""
    names = ("unclamped", "zero_gap", "noise_floor", "zeros")
    wav = np.stack([_model(n)[0] for n in names])
    db = _db_mel(ops, MT, dev, wav)
    db_dev = _t(db, dev)
    return names, db_dev, db, ops.db_peak(db_dev).cpu().numpy()


@pytest.mark.parametrize("K", (1, 34))
def test_db_mfcc_against_the_model_on_the_gpus_db(ops, MT, dev, clamp_batch, K):
    names, db_dev, db, peak = clamp_batch
    out = Sent(db.shape[:2] + (K,), dev)
    ops.db_mfcc(db_dev, _t(MT.dct_ortho_table(K, 80), dev), _t(peak, dev), None, 80.0, out=out.view)
    got = out.get()
    for b, name in enumerate(names):
        x = np.maximum(db[b], np.float32(peak[b]) - np.float32(80.0)).astype(np.float64)
        share = float((db[b] < np.float32(peak[b]) - np.float32(80.0)).mean())
        print("%s: %.1f %% of the GPU's dB entries clamped" % (name, 100 * share))
        assert (share == 0.0) if name in ("unclamped", "zeros") else (0.10 <= share <= 0.80)
        _within("db_mfcc[%s, K=%d]" % (name, K), got[b], W.mfcc_of_db(db[b], peak[b], K), W.chain_bars(x, K))
    z = got[names.index("zeros")]
    # dB = -100 throughout: c0 = -100 sqrt(80), the rest cancels to within the chain's bar (82 u sum |x t| < 5e-3 for every k)
    assert np.abs(z[:, 0] + 100.0 * np.sqrt(80.0)).max() < 5e-3 and (K == 1 or np.abs(z[:, 1:]).max() < 5e-3)


def test_db_mfcc_pad_rows_are_plus_zero(ops, MT, dev, clamp_batch):
    _, db_dev, db, peak = clamp_batch
    frames = np.array([130, 64, 17, 0], dtype=np.int64)
    out = Sent(db.shape[:2] + (34,), dev)
    ops.db_mfcc(db_dev, _t(MT.dct_ortho_table(34, 80), dev), _t(peak, dev), _t(frames, dev), 80.0, out=out.view)
    got = out.get()
    full = ops.db_mfcc(db_dev, _t(MT.dct_ortho_table(34, 80), dev), _t(peak, dev)).cpu().numpy()
    for b, f in enumerate(frames):
        assert np.array_equal(_bits(got[b, :f]), _bits(full[b, :f])) and not _bits(got[b, f:]).any()


# ---- set_coef_rms_dist --------------------------------------------------------------------------------------------------------------------
def _bool_sent(n, dev):
    buf = torch.full((n + 2 * GUARD,), 7, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(torch.bool)


def test_coef_rms_dist_is_exact_on_integer_coefficients(ops, dev):
    """T in {1, 255, 256, 257} (and an unequal and an empty pair) in one batch: integer coefficients make every sum exact, so the result is
    the float64 value rounded once, bit for bit."""
    Ts, K = (1, 255, 256, 257, 100, 0), 34
    fy = np.array([1, 255, 256, 257, 101, 0], dtype=np.int64)
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, (6, 257, K)).astype(np.float32)
    y = rng.integers(-8, 9, (6, 260, K)).astype(np.float32)
    for b, t in enumerate(Ts):  # nothing at or beyond a row's frames is read
        x[b, t:] = np.nan
        y[b, fy[b]:] = np.nan
    mcd = Sent((6,), dev)
    vbuf, valid = _bool_sent(6, dev)
    ops.coef_rms_dist(_t(x, dev), _t(y, dev), _t(np.array(Ts, dtype=np.int64), dev), _t(fy, dev), mcd=mcd.view, valid=valid)
    got, v = mcd.get(), vbuf.cpu().numpy()
    assert (v[:GUARD] == 7).all() and (v[-GUARD:] == 7).all() and v[GUARD:-GUARD].tolist() == [1, 1, 1, 1, 0, 0]
    want = np.array([W.rms_dist_kernel_order(x[b, :t], y[b, :t]) for b, t in enumerate(Ts[:4])], dtype=np.float32)
    assert np.array_equal(_bits(got[:4]), _bits(want)) and np.isnan(got[4:]).all()
    assert np.allclose(want, [W.cal_mcd(x[b, :t], y[b, :t]) for b, t in enumerate(Ts[:4])], rtol=1e-6)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
PAIRS = ("unclamped", "noise_floor")


@functools.lru_cache(maxsize=None)
def _mfcc_bars(name, n=W.N_SIG):
    """(float64 MFCC [T, 34], its bars) of a named signal."""
    _, _, _, cbar, d64 = _model(name, n)
    x = W.clamp(d64)
    return x @ W.dct_ortho(W.NMFCC).T, W.mfcc_bars(cbar, x, W.NMFCC)


@pytest.fixture(scope="module")
def singles(MT, dev):
    """Every end-to-end pair run alone: name -> (mcd, valid) as numpy scalars; "ramp" is the DTW pair, run in that mode."""
    out = {}
    for name in PAIRS:
        m, v = MT.wav_mcd_htk(_t(_model(name)[0], dev), _t(_model(name + "_deg")[0], dev))
        assert m.shape == () and m.dtype == torch.float32 and v.dtype == torch.bool
        out[name] = (m.cpu().numpy(), bool(v))
    m, v = MT.wav_mcd_htk(_t(_model("ramp")[0], dev), _t(_model("ramp_short")[0], dev), use_dtw=True)
    out["ramp"] = (m.cpu().numpy(), bool(v))
    return out


@pytest.mark.parametrize("name", PAIRS + tuple(p + "_deg" for p in PAIRS))
def test_htk_mfcc_end_to_end(MT, dev, name):
    want, bar = _mfcc_bars(name)
    got = MT.htk_mfcc(_t(_model(name)[0], dev))
    assert got.shape == (130, 34)
    _within("htk_mfcc[%s]" % name, got.cpu().numpy(), want, bar)


@pytest.mark.parametrize("name", PAIRS)
def test_wav_mcd_default_mode(MT, dev, singles, name):
    (c1, b1), (c2, b2) = _mfcc_bars(name), _mfcc_bars(name + "_deg")
    want = W.cal_mcd(c1, c2)
    print("%s: model mcd %.6f" % (name, want))
    assert singles[name][1]
    _within("wav_mcd_htk[%s]" % name, singles[name][0], want, np.float64(W.mcd_bar(c1, c2, b1, b2)))


def test_wav_mcd_dtw_mode(MT, dev, singles):
    """T against T - 9 frames on the fading pair (wavmcd_models.ramp_pair: its path keeps a margin of more than 4 x the fp32 DTW's bound).  The score
    is dist / steps of metrics.dtw on htk_mfcc's output, bit for bit, and the model's within the propagated bar; the kernel's path has the
    model's length."""
    y, z = _model("ramp")[0], _model("ramp_short")[0]
    (c1, b1), (c2, b2) = _mfcc_bars("ramp"), _mfcc_bars("ramp_short")
    assert (len(c1), len(c2)) == (130, 121)
    want, m = W.mcd_dtw(c1, c2)
    dist, steps = MT.dtw(MT.htk_mfcc(_t(y, dev)), MT.htk_mfcc(_t(z, dev)))
    print("model mcd %.6f over %d steps, the kernel's path has %d" % (want, m["steps"], int(steps)))
    assert singles["ramp"][1] and int(steps) == m["steps"]
    assert _bits(singles["ramp"][0]) == _bits(np.float32(np.float64(dist.cpu().numpy()) / int(steps)))
    _within("wav_mcd_htk_dtw", singles["ramp"][0], want, np.float64(W.dtw_bar(b1, b2, m, W.NMFCC)))


def test_ragged_batch_equals_single_runs_and_two_runs_agree(MT, dev, singles):
    """Both pairs plus one of 70 frames in a batch with device lengths; each row is its single run bit for bit; a second run gives the
    same bits; htk_mfcc's pad rows are +0.0."""
    short = 70 * 256 - 3
    refs = [_model(n)[0] for n in PAIRS] + [_model("unclamped")[0][:short]]
    ests = [_model(n + "_deg")[0] for n in PAIRS] + [_model("unclamped_deg")[0][:short]]
    (wr, lr), (we, le) = _batch(refs), _batch(ests)
    args = (_t(wr, dev), _t(we, dev), _t(lr, dev), _t(le, dev))
    m, v = MT.wav_mcd_htk(*args)
    m2, _ = MT.wav_mcd_htk(*args)
    alone, _ = MT.wav_mcd_htk(_t(refs[2], dev), _t(ests[2], dev))
    assert v.cpu().numpy().all()
    want = [singles[PAIRS[0]][0], singles[PAIRS[1]][0], alone.cpu().numpy()]
    assert np.array_equal(_bits(m.cpu().numpy()), _bits(np.array(want))) and np.array_equal(_bits(m.cpu().numpy()), _bits(m2.cpu().numpy()))
    c, frames = MT.htk_mfcc(args[0], args[2])
    assert frames.cpu().numpy().tolist() == [130, 130, 70] and not _bits(c[2, 70:].cpu().numpy()).any()
    assert np.array_equal(_bits(c[2, :70].cpu().numpy()), _bits(MT.htk_mfcc(_t(refs[2], dev)).cpu().numpy()))
    # the DTW pair in a batch beside a shorter one
    (wr, lr), (we, le) = _batch([_model("ramp")[0], refs[2]]), _batch([_model("ramp_short")[0], ests[2][:-5 * 256]])
    md, vd = MT.wav_mcd_htk(_t(wr, dev), _t(we, dev), _t(lr, dev), _t(le, dev), use_dtw=True)
    md2, _ = MT.wav_mcd_htk(_t(wr, dev), _t(we, dev), _t(lr, dev), _t(le, dev), use_dtw=True)
    assert vd.cpu().numpy().all() and np.array_equal(_bits(md.cpu().numpy()), _bits(md2.cpu().numpy()))
    assert _bits(md[0].cpu().numpy()) == _bits(singles["ramp"][0])


def test_invalid_pairs_means_and_host_refusals(MT, dev, singles):
    y, z = _model("unclamped")[0], _model("unclamped_deg")[0]
    wr, we = _t(np.stack([y, y, y]), dev), _t(np.stack([z, z, z]), dev)
    lr = torch.tensor([W.N_SIG, W.N_SIG, 512], dtype=torch.int64, device=dev)
    le = torch.tensor([W.N_SIG, W.N_SIG - 256, 512], dtype=torch.int64, device=dev)
    m, v = MT.wav_mcd_htk(wr, we, lr, le)  # device lengths: unequal frame counts and an unreflectable row are flagged, not raised
    assert v.cpu().numpy().tolist() == [True, False, False] and np.isnan(m.cpu().numpy()[1:]).all()
    assert _bits(m[0].cpu().numpy()) == _bits(singles["unclamped"][0])
    md, vd = MT.wav_mcd_htk(wr, we, lr, le, use_dtw=True)
    assert vd.cpu().numpy().tolist() == [True, True, False] and np.isnan(md.cpu().numpy()[2]) and np.isfinite(md.cpu().numpy()[:2]).all()
    mean = MT.mcd_mean(m, v)
    assert mean.shape == () and mean.is_cuda and _bits(mean.cpu().numpy()) == _bits(singles["unclamped"][0])
    assert np.isnan(MT.mcd_mean(m[1:], v[1:]).cpu().numpy())
    # both means from one call equal the separate calls
    both = MT.eval_wav_pairs(wr[:2], we[:2], lr[:2], lr[:2])
    m2, v2 = MT.wav_mcd_htk(wr[:2], we[:2], lr[:2], lr[:2])
    assert sorted(both) == ["mcd", "stoi"] and all(t.shape == () and t.is_cuda for t in both.values())
    assert _bits(both["mcd"].cpu().numpy()) == _bits(MT.mcd_mean(m2, v2).cpu().numpy())
    assert _bits(both["stoi"].cpu().numpy()) == _bits(MT.stoi_mean(*MT.wav_stoi(wr[:2], we[:2], lr[:2], lr[:2])).cpu().numpy())
    assert 0.0 < float(both["stoi"]) < 1.0
    # host values are checked on the host
    with pytest.raises(ValueError):
        MT.wav_mcd_htk(wr, we, [W.N_SIG] * 3, [W.N_SIG, W.N_SIG - 256, W.N_SIG])
    with pytest.raises(ValueError):
        MT.wav_mcd_htk(wr[0], we[0, :-256].contiguous())
    with pytest.raises(ValueError):
        MT.wav_mcd_htk(wr, we, [W.N_SIG, W.N_SIG, 512], None)
    with pytest.raises(ValueError):
        MT.htk_mfcc(wr[:, :512].contiguous())
    with pytest.raises(ValueError):
        MT.htk_mfcc(wr, n_mfcc=81)
    with pytest.raises(RuntimeError):
        MT.htk_mfcc(wr.cpu())


def test_mel_basis_argument(MT, dev):
    """A caller's own filterbank takes the restated one's place: the same array gives the same bits."""
    y = _t(_model("unclamped")[0], dev)
    assert torch.equal(MT.htk_mfcc(y, mel_basis=W.BASIS32), MT.htk_mfcc(y))


def test_report_measured_maxima():
    """Printed last: the largest fraction of each bar seen by the tests above (DESIGN.md 3.10 quotes them)."""
    for k in sorted(MEASURED):
        print("measured: %s = %.3g" % (k, MEASURED[k]))
    assert all(v <= 1.0 for v in MEASURED.values())
