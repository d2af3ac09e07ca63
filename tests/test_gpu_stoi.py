"""GPU checks of the STOI path (csrc/stoi.hip through set_amd.ops and set_amd.metrics) against the models of stoi_models.py, stage by stage
and end to end.  Selection and compaction are bit for bit (test_stoi_reference.py asserts the margin that makes the selection so); the band
envelopes lie within the bound derived in stoi_models.envelope_bound; the score kernel, fed the model's envelopes, is the float64 score
rounded once; end to end the bar is 16 x the float32 mirror's own distance from float64 (same file).  Every output is a view inside a
sentinel-filled buffer that is compared whole.  Shapes are the smallest at which each edge can go wrong.

Measured on the MI355X (profiles/stoi_accuracy.log): see test_report_measured_maxima."""
import json
import os

import numpy as np
import pytest
import torch

import stoi_models as SM
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SENT_F32, SENT_I32, SENT_I64, GUARD = -12345.0, -777, -778, 64
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


@pytest.fixture(scope="module")
def images(MT, dev):
    return MT._stoi_images(22050, dev)


@pytest.fixture(scope="module")
def singles(MT, dev):
    """Every end-to-end case run alone: id -> (d as a numpy fp32 scalar, valid)."""
    out = {}
    for k in SM.E2E:
        x, y = SM.pair(k)
        d, v = MT.stoi(_t(x, dev), _t(y, dev))
        assert d.shape == () and v.shape == () and d.dtype == torch.float32 and v.dtype == torch.bool
        out[k] = (d.cpu().numpy(), bool(v))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _note(name, frac):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(frac))


class Sent:
    """A contiguous view of `shape` in the middle of a buffer filled with a sentinel; `whole(expected)`: the buffer as it must look when
    the view holds `expected` (a numpy array in which untouched elements are the sentinel)."""

    def __init__(self, shape, dtype, sentinel, dev):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        self.sentinel, self.shape = sentinel, shape

    def expected(self, np_dtype):
        return np.full(self.shape, self.sentinel, dtype=np_dtype)

    def get(self):
        """The view's contents, after checking that the guards on both sides still hold the sentinel."""
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.sentinel).all() and (b[-GUARD:] == self.sentinel).all(), "written outside the output"
        return b[GUARD:-GUARD].reshape(self.shape)


def _batch(rows, fill=np.nan):
    """rows of unequal length -> ([B, N] float32 with `fill` beyond each row's length -- a read there shows --, lengths)."""
    N = max(len(r) for r in rows)
    out = np.full((len(rows), N), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- select -------------------------------------------------------------------------------------------------------------------------------
def _select(ops, dev, images, rows, lengths=True):
    wav, lens = _batch(rows)
    B, N = wav.shape
    F, _, _ = SM.sizes(N)
    kept, K, nrm = Sent((B, F), torch.int32, SENT_I32, dev), Sent((B,), torch.int32, SENT_I32, dev), Sent((B, F), torch.float32, SENT_F32, dev)
    ops.stoi_select(_t(wav, dev), images[0], _t(lens, dev) if lengths else None, nrm=nrm.view, kept=kept.view, K=K.view)
    return kept.get(), K.get(), nrm.get(), F


SELECT_BATCHES = {
    "one_two_frames_ragged": ("len1025", "len1536", "len1537"),
    "silence_and_a_short_row": ("silence_start", "silence_mid", "silence_end", "short"),
    "one_kept_probes_zero_ragged": ("one_kept", "probes", "all_zero", "plain"),
}


@pytest.mark.parametrize("name", list(SELECT_BATCHES))
def test_select_bit_for_bit(ops, dev, images, name):
    cases = dict(SM.select_cases(), short=SM.speech(1000, 38))
    rows = [cases[k] for k in SELECT_BATCHES[name]]
    kept, K, nrm, F = _select(ops, dev, images, rows)
    want_kept, want_K = np.full(kept.shape, SENT_I32, dtype=np.int32), np.zeros(len(rows), dtype=np.int32)
    for b, x in enumerate(rows):
        m, _ = SM.select64(x)
        want_kept[b, :len(m)], want_K[b] = m, len(m)
        f = SM.energy_frames(len(x))
        ref = SM.norms64(x)
        # gamma(1027) / 2 on the norm (test_stoi_reference.py, the selection margin) plus the square root's own rounding
        assert (np.abs(nrm[b, :f] - ref) <= 3.2e-5 * ref).all(), (name, b)
        if f:
            _note("select: norm error / (3.2e-5 nrm)", np.max(np.abs(nrm[b, :f] - ref) / np.maximum(3.2e-5 * ref, 1e-300)) if ref.max() > 0 else 0.0)
        assert (nrm[b, f:] == SENT_F32).all(), (name, b)
        if len(x) <= 1024:
            continue
        single = _select(ops, dev, images, [x], lengths=False)  # the row alone, full length: the same bits
        assert np.array_equal(single[0][0, :len(m)], m) and single[1][0] == len(m) and np.array_equal(_bits(single[2][0, :f]), _bits(nrm[b, :f]))
    assert np.array_equal(K, want_K), (name, K, want_K)
    assert np.array_equal(kept, want_kept), name
    if name == "one_kept_probes_zero_ragged":
        x, probes = SM.threshold_probes()
        assert K[0] == 1 and probes[0] in kept[1, :K[1]] and probes[1] not in kept[1, :K[1]] and K[2] == SM.energy_frames(5000)
        assert not nrm[2, :K[2]].any()
    if name == "silence_and_a_short_row":
        assert K[3] == 0 and (kept[3] == SENT_I32).all()


# ---- compact ------------------------------------------------------------------------------------------------------------------------------
def test_compact_bit_for_bit_with_the_clean_signals_list(ops, dev, images):
    """y's own energies would select other frames (its silence lies elsewhere): it is cut by x's list all the same.  Row 3 has no kept
    frame (K = 0: 512 zeros).  The list and counts come from the model, not from the select kernel."""
    cases = SM.select_cases()
    xs = [cases["silence_start"], cases["silence_mid"], cases["silence_end"], cases["plain"]]
    ys = [xs[1], xs[2], xs[0], xs[0]]
    assert not np.array_equal(SM.select64(ys[0])[0], SM.select64(xs[0])[0])
    B, N = 4, 9000
    F, S, _ = SM.sizes(N)
    lists = [SM.select64(x)[0] for x in xs[:3]] + [np.zeros(0, dtype=np.int32)]
    kept = np.full((B, F), -5, dtype=np.int32)  # entries beyond K are never used
    for b, m in enumerate(lists):
        kept[b, :len(m)] = m
    K = np.array([len(m) for m in lists], dtype=np.int32)
    sil, sil_len = Sent((2 * B, S), torch.float32, SENT_F32, dev), Sent((2 * B,), torch.int64, SENT_I64, dev)
    ops.stoi_compact(_t(np.stack(xs), dev), _t(np.stack(ys), dev), images[0], _t(kept, dev), _t(K, dev), sil=sil.view, sil_len=sil_len.view)
    want = sil.expected(np.float32)
    for b in range(B):
        for sig, s in enumerate((xs[b], ys[b])):
            m = SM.compact(s, lists[b], SM.W32, np.float32)
            assert len(m) == 512 * (K[b] + 1)
            want[sig * B + b, :len(m)] = m
    assert np.array_equal(_bits(sil.get()), _bits(want))  # positions at or beyond L untouched
    assert sil_len.get().tolist() == [512 * (k + 1) for k in K] * 2


# ---- bands --------------------------------------------------------------------------------------------------------------------------------
def _bands(ops, dev, images, rows, lengths=True):
    sil, lens = _batch(rows)
    R, S = sil.shape
    T = -(-(S - 1024) // 256)
    tob = Sent((R, T, 15), torch.float32, SENT_F32, dev)
    ops.stoi_bands(_t(sil, dev), images[1], images[2], _t(lens, dev) if lengths else None, n_bands=15, bin_lo=0, nbins=images[3], tob=tob.view)
    return tob.get()


def _check_bands(out, rows, what):
    for r, s in enumerate(rows):
        ref = SM.bands64(s)
        Tr = ref.shape[0]
        bound = SM.envelope_bound(s, ref)
        err = np.abs(out[r, :Tr].astype(np.float64) - ref)
        _note("bands: envelope error / derived bound", (err / bound).max())
        assert (err <= bound).all(), (what, r, float((err / bound).max()))
        assert not _bits(out[r, Tr:]).any(), (what, r)  # +0.0 beyond the row's frames


def test_bands_within_the_derived_bound_at_the_tile_edges(ops, dev, images):
    inp = SM.band_inputs()
    rows = [inp[k] for k in ("T1", "T63", "T64", "T65")]
    assert [SM.bands64(s).shape[0] for s in rows] == [1, 63, 64, 65]
    out = _bands(ops, dev, images, rows)
    assert out.shape == (4, 65, 15)
    _check_bands(out, rows, "ragged")
    alone = _bands(ops, dev, images, [inp["T64"]], lengths=False)  # a row of the ragged batch equals the same signal run alone
    assert alone.shape == (1, 64, 15) and np.array_equal(_bits(alone[0]), _bits(out[2, :64]))
    big = _bands(ops, dev, images, [inp["T129"]], lengths=False)
    assert big.shape == (1, 129, 15)
    _check_bands(big, [inp["T129"]], "three tiles")
    twice = _bands(ops, dev, images, [2.0 * inp["T129"]], lengths=False)
    assert np.array_equal(_bits(twice), _bits(2.0 * big))  # a factor of 2 goes through every stage exactly


def test_bands_tones_pin_every_band_edge(ops, dev, images):
    """Bin-centred tones at bins 5, 6, 7, 8 (the first edges) and 198, 199 (the last): the model with the edges one bin off is more than
    100 bounds away in some band for each (test_stoi_reference.py), so a kernel inside the bound has its edges right."""
    inp = SM.band_inputs()
    for names in (("tone5", "tone6", "tone7", "tone8"), ("tone198", "tone199")):
        rows = [inp[k] for k in names]
        out = _bands(ops, dev, images, rows, lengths=False)
        _check_bands(out, rows, names)
    e = {k: SM.bands64(inp[k])[0] for k in ("tone5", "tone8", "tone199")}
    assert e["tone5"][0] < 0.6 * e["tone8"][1] and e["tone199"][14] < 0.6 * SM.bands64(inp["tone198"])[0][14]  # what the tones tell apart


# ---- score --------------------------------------------------------------------------------------------------------------------------------
SCORE_TB = ((29, 30, 31, 156), (157, 158, 285, 286))  # below / at / above one segment; J = 127 | 128, 129 | 256, 257: the 128-segment tiles


def _score(ops, dev, pairs):
    """pairs of envelopes [T_b, 15] of unequal T_b -> (d, valid) in sentinel buffers; frames beyond T_b are NaN."""
    B, T = len(pairs), max(p[0].shape[0] for p in pairs)
    tob = np.full((2 * B, T, 15), np.nan, dtype=np.float32)
    for b, (x, y) in enumerate(pairs):
        tob[b, :len(x)], tob[B + b, :len(y)] = x, y
    lens = np.array([1024 + 256 * len(p[0]) for p in pairs], dtype=np.int64)
    d, valid = Sent((B,), torch.float32, SENT_F32, dev), Sent((B,), torch.bool, True, dev)
    ops.stoi_score(_t(tob, dev), _t(lens, dev), d=d.view, valid=valid.view)
    return d.get(), valid.get()


def _check_score(d, valid, pairs, what):
    for b, (x, y) in enumerate(pairs):
        ref = SM.score64(x.astype(np.float64), y.astype(np.float64))
        if ref is None:
            assert np.isnan(d[b]) and not valid[b], (what, b)
            continue
        # the kernel sums in double from the same fp32 envelopes (~1e-14) and rounds once to fp32
        tol = 2.0 ** -24 * abs(ref) + 1e-12
        _note("score: |d - float64| / (fp32 rounding of d)", abs(float(d[b]) - ref) / tol)
        assert valid[b] and abs(float(d[b]) - ref) <= tol, (what, b, float(d[b]), ref)


@pytest.mark.parametrize("tbs", SCORE_TB, ids=lambda t: "Tb" + "_".join(map(str, t)))
def test_score_at_the_segment_and_tile_edges(ops, dev, tbs):
    pairs = [SM.envelopes(tb, 100 + tb) for tb in tbs]
    d, valid = _score(ops, dev, pairs)
    _check_score(d, valid, pairs, tbs)
    for b in (0, 3):  # a row of the ragged batch equals the same pair run alone
        d1, v1 = _score(ops, dev, [pairs[b]])
        assert np.array_equal(_bits(d1), _bits(d[b:b + 1])) and v1[0] == valid[b]


def test_score_identities_and_clipping(ops, dev):
    x, y = SM.envelopes(70, 7)
    xc, yc = SM.envelopes(200, 8, clipy=True)
    _, clipped = SM.correlations(xc.astype(np.float64), yc.astype(np.float64))
    assert 0.1 <= clipped.mean() <= 0.9
    pairs = [(x, np.zeros_like(x)), (x, x), (x, 2.0 * x), (xc, yc)]
    d, valid = _score(ops, dev, pairs)
    _check_score(d, valid, pairs, "identities")
    assert _bits(d[0:1])[0] == 0                             # y = 0: exactly +0.0
    assert np.array_equal(_bits(d[1:2]), _bits(d[2:3]))     # d(x, 2x) is d(x, x) bit for bit
    assert abs(float(d[1]) - 1.0) <= 2.0 ** -23
    d2, _ = _score(ops, dev, pairs)
    assert np.array_equal(_bits(d), _bits(d2))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_model_and_the_recorded_reference(singles):
    bar, _ = SM.e2e_bar()
    with open(os.path.join(GOLDEN, "stoi_reference.json")) as f:
        recorded = {c["id"]: c["d"] for c in json.load(f)["cases"]}
    for k in SM.E2E:
        x, y = SM.pair(k)
        d, valid = singles[k]
        ref = SM.stoi64(x, y)["d"]
        print("%s: d = %.9f model %.12f reference %s" % (k, float(d), ref if ref is not None else float("nan"), recorded[k]))
        if k in SM.INVALID_CASES:
            assert ref is None and recorded[k] is None and not valid and np.isnan(d), k
            continue
        _note("end to end: |d - float64 model| / bar (bar = %.3e)" % bar, abs(float(d) - ref) / bar)
        assert valid and abs(float(d) - ref) <= bar, (k, float(d), ref, bar)
        assert abs(float(d) - recorded[k]) <= bar + 1e-12, (k, float(d), recorded[k])


def test_ragged_batch_rows_equal_single_runs_and_runs_repeat(MT, dev, singles):
    names = ("n40001_snrm5_gap_ends", "n24000_clip", "n8704_too_short", "n22050_snr0")  # an invalid row among valid ones
    xs, ys = zip(*(SM.pair(k) for k in names))
    x, lens = _batch(xs)
    y, _ = _batch(ys)
    d, valid = MT.stoi(_t(x, dev), _t(y, dev), lens.tolist())
    d2, valid2 = MT.stoi(_t(x, dev), _t(y, dev), _t(lens, dev))  # lengths as a device tensor; a second run
    assert d.shape == (4,) and valid.tolist() == [True, True, False, True] and torch.equal(valid, valid2)
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(d2.cpu().numpy()))
    for b, k in enumerate(names):
        assert np.array_equal(_bits(d[b:b + 1].cpu().numpy()), _bits(singles[k][0].reshape(1))), k
    mean = MT.stoi_mean(d, valid)
    assert mean.shape == () and mean.is_cuda
    assert abs(float(mean) - np.mean([float(singles[k][0]) for k in names if singles[k][1]])) <= 1e-6


def test_wav_stoi_cuts_each_pair_to_the_shorter_length(MT, dev, singles):
    k = "n22050_snr0"
    x, y = SM.pair(k)
    longer = np.concatenate([y, SM.speech(3000, 77)])
    d, valid = MT.wav_stoi(_t(x, dev), _t(longer, dev))
    assert bool(valid) and np.array_equal(_bits(d.cpu().numpy().reshape(1)), _bits(singles[k][0].reshape(1)))
    # batched, with lengths: row 0 is cut by len_gen, row 1 by len_ref
    k2 = "n8705_first_valid"
    x2, y2 = SM.pair(k2)
    ref, _ = _batch([x, np.concatenate([x2, SM.speech(5000, 78)])], fill=0.0)
    gen, _ = _batch([longer, y2], fill=0.0)
    d, valid = MT.wav_stoi(_t(ref, dev), _t(gen, dev), [ref.shape[1], len(x2)], [len(x), gen.shape[1]])
    assert valid.tolist() == [True, True]
    for b, name in enumerate((k, k2)):
        assert np.array_equal(_bits(d[b:b + 1].cpu().numpy()), _bits(singles[name][0].reshape(1))), name


def test_refusals_on_the_device(MT, dev):
    x = torch.zeros(2, 9000, device=dev)
    with pytest.raises(NotImplementedError):
        MT.stoi(x, x, extended=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.stoi(x.cpu(), x.cpu())
    with pytest.raises(ValueError):
        MT.stoi(x[:, :1024].contiguous(), x[:, :1024].contiguous())
    with pytest.raises(ValueError):
        MT.stoi(x, x[:, :8000].contiguous())
    with pytest.raises(ValueError):
        MT.stoi(x, x, [9001, 5])
    d, valid = MT.stoi(x[:, :1025].contiguous(), x[:, :1025].contiguous())  # one energy frame: no envelope frame, no launch of the band kernel
    assert valid.tolist() == [False, False] and torch.isnan(d).all()


def test_report_measured_maxima():
    """Printed last: the largest fraction of each bar seen by the tests above (DESIGN.md 3.9 quotes them)."""
    for k in sorted(MEASURED):
        print("measured: %s = %.4f" % (k, MEASURED[k]))
    assert all(v <= 1.0 for v in MEASURED.values())
