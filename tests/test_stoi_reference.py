"""CPU checks of the STOI path (set_amd.metrics.stoi, csrc/stoi.hip's host side): the float64 model of stoi_models.py against the recorded
and, where the checkout is present, the live reference; the band matrix and the kernel images; the count rules; the conditions the GPU
tests rest on (selection margins, clip activity, the end-to-end allowance and what a mistake costs, the envelope bound); the entries'
refusals on the built library.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import stoi_models as SM
from conftest import GOLDEN

LO_LISTED = [6, 8, 10, 12, 16, 20, 25, 31, 39, 50, 63, 79, 99, 125, 158]


@pytest.fixture(scope="module")
def MT():
    import set_amd  # noqa: F401
    from set_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "stoi_reference.json")) as f:
        return {c["id"]: c for c in json.load(f)["cases"]}


@pytest.fixture(scope="module")
def models():
    return {k: SM.stoi64(*SM.pair(k)) for k in SM.E2E}


# ---- the model is the reference -----------------------------------------------------------------------------------------------------------
def test_model_matches_the_recorded_reference(recorded, models):
    assert set(recorded) == set(SM.E2E)
    for k, c in SM.E2E.items():
        assert (recorded[k]["n"], recorded[k]["seed"]) == (c["n"], c["seed"])
        d, ref = models[k]["d"], recorded[k]["d"]
        assert (d is None) == (ref is None), k
        assert d is None or abs(d - ref) <= 1e-12, (k, d, ref)
    assert all(recorded[k]["d"] is None for k in SM.INVALID_CASES) and all(recorded[k]["d"] is not None for k in SM.VALID_CASES)


def test_model_matches_the_live_reference(models):
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference checkout is not on this machine")
    ref = SM.load_reference_stoi(ref_import.REF_ROOT)
    for k in SM.E2E:
        x, y = SM.pair(k)
        d, r = models[k]["d"], ref.stoi(x, y, SM.FS, extended=False)
        assert (d is None) == (r is None), k
        assert d is None or abs(d - r) <= 1e-12, (k, d, r)
    x = SM.speech(5000, 3)
    assert ref.stoi(x[:1023], x[:1023], SM.FS) is None  # below one frame
    with pytest.raises(Exception):                       # exactly one frame's worth: zero frames, the reference raises
        ref.stoi(x[:1024], x[:1024], SM.FS)
    z = np.zeros(12000, dtype=np.float32)
    x = SM.speech(12000, 4)
    assert ref.stoi(x, z, SM.FS) == 0.0 and SM.stoi64(x, z)["d"] == 0.0
    assert abs(ref.stoi(x, x, SM.FS) - 1.0) < 1e-12 and abs(SM.stoi64(x, x)["d"] - 1.0) < 1e-12


def test_third_octave_bands_are_the_listed_contiguous_disjoint_ones(MT):
    obm, edges = MT.third_octave_bands()
    assert obm.shape == (15, 513) and obm.dtype == np.float64 and set(np.unique(obm)) == {0.0, 1.0}
    assert edges[:, 0].tolist() == LO_LISTED and int(edges[-1, 1]) == 199
    assert (edges[1:, 0] == edges[:-1, 1]).all()                     # contiguous
    assert (obm.sum(axis=0) <= 1).all() and obm.sum() == 199 - 6      # disjoint
    assert np.array_equal(obm, SM.band_matrix()) and tuple(edges[:, 0]) + (int(edges[-1, 1]),) == SM.LO
    from oracle import ref_import
    if ref_import.available():
        utils = SM.load_reference_stoi(ref_import.REF_ROOT).utils
        ref_obm, ref_cf = utils.thirdoct(22050, 1024, 15, 150)
        assert np.array_equal(ref_obm, obm)
    with pytest.raises(ValueError):
        MT._stoi_images(10, torch.device("cpu"))  # no band below 5 Hz


# ---- images -------------------------------------------------------------------------------------------------------------------------------
def test_every_packed_image_unpacks_to_its_definition(MT):
    from set_amd import melspec
    win, table, basis, nbins = MT._stoi_images(22050, torch.device("cpu"))
    assert nbins == 199 and table.shape == (7, 256, 64, 4) and basis.shape == (7, 16, 64, 4)  # 7 chunks of 32 from bin 0; one row block
    w64 = np.hanning(1026)[1:-1]
    assert np.array_equal(win.numpy(), w64.astype(np.float32)) and win.numpy()[0] == win.numpy()[-1] > 0  # symmetric, not periodic
    n = np.arange(1024)
    want = np.stack([np.stack([w64 * np.cos(2 * np.pi * ((f * n) % 1024) / 1024) for f in range(199)]),
                     np.stack([-w64 * np.sin(2 * np.pi * ((f * n) % 1024) / 1024) for f in range(199)])]).astype(np.float32)
    got = melspec.unpack_dft_table(table.numpy(), 199)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not table.numpy().reshape(7, 256, 2, 32, 4)[6, :, :, 199 - 192:].any()  # rows of bins 199 .. 223 are zero
    obm = SM.band_matrix()
    img = basis.numpy()
    for ch in range(7):
        for r in range(16):
            for lane in range(64):
                b = 32 * ch + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
                row = lane & 31
                want_e0 = obm[row, b] if row < 15 and b < 199 else 0.0
                assert img[ch, r, lane, 0] == want_e0 and not img[ch, r, lane, 1:].any()


# ---- counts -------------------------------------------------------------------------------------------------------------------------------
def test_count_rules_at_the_edges(built_lib):
    from set_amd import ops
    assert [SM.energy_frames(n) for n in (1023, 1024, 1025, 1536, 1537, 2048, 2049)] == [0, 0, 1, 1, 2, 2, 3]
    for n in (1025, 1536, 1537, 8705, 40001):  # the reference's own loop
        assert SM.energy_frames(n) == len(range(0, n - 1024, 512))
        assert ops.stoi_sizes(n) == SM.sizes(n)
    for K in range(0, 40):
        L = 512 * (K + 1)
        assert SM.envelope_frames(K) == len(range(0, L - 1024, 256)) == (2 * (K - 1) if K >= 2 else 0)
    # validity is first reached at 8705 samples with every frame kept: F = K = 16, T_b = 30
    assert SM.energy_frames(8704) == 15 and SM.envelope_frames(15) == 28
    assert SM.energy_frames(8705) == 16 and SM.envelope_frames(16) == 30
    x = SM.speech(8705, 5)
    assert SM.stoi64(x, x)["K"] == 16 and SM.stoi64(x, x)["d"] is not None and SM.stoi64(x[:8704], x[:8704])["d"] is None
    # 1024 samples: zero frames, invalid here (the reference raises)
    m = SM.stoi64(x[:1024], x[:1024])
    assert m["K"] == 0 and m["T"] == 0 and m["d"] is None


# ---- conditions of the GPU tests -----------------------------------------------------------------------------------------------------------
def test_selection_margin_of_every_gpu_case():
    """Every frame of every waveform the GPU tests select on is at least 0.01 dB from the threshold.  The kernel's norm is off by at most
    gamma(1027) ~ 6.1e-5 on e2 (1024 squares and sums, the two roundings of each square), half of it on the norm; both sides of the
    comparison carry it, and the two products of the comparison 2^-23 more: below 1.5e-4 relative = 0.0013 dB.  0.01 dB is more than
    4 x that, so the float32 selection must be the float64 one."""
    rows = dict(SM.select_cases())
    rows.update({k: SM.pair(k)[0] for k in SM.E2E})
    for k, x in rows.items():
        kept, margin = SM.select64(x)
        assert margin >= 0.01, (k, margin)
        assert np.array_equal(SM.select32(x), kept), k
    x, probes = SM.threshold_probes()
    nrm = SM.norms64(x)
    off = 20 * np.log10((nrm[probes] + SM.EPS64) / (0.01 * (nrm.max() + SM.EPS64)))
    assert abs(off[0] - 0.02) < 1e-4 and abs(off[1] + 0.02) < 1e-4, off
    kept = SM.select64(x)[0].tolist()
    assert probes[0] in kept and probes[1] not in kept
    assert SM.select64(SM.one_kept_frame())[0].tolist() == [4]
    assert SM.select64(np.zeros(5000, dtype=np.float32))[0].tolist() == list(range(8))  # an all-zero row keeps every frame
    for name, lo, hi in (("silence_start", 0, 4), ("silence_mid", 6, 10), ("silence_end", 12, 16)):
        kept = SM.select64(rows[name])[0]
        assert 0 < len(kept) < 16 and not set(range(lo + 1, hi - 1)) & set(kept.tolist()), (name, kept)


def test_clip_activity_of_the_clip_cases(models):
    for k in SM.CLIP_CASES:
        _, clipped = SM.correlations(models[k]["xt"], models[k]["yt"])
        assert 0.10 <= clipped.mean() <= 0.90, (k, clipped.mean())
    x, y = SM.envelopes(70, 3, clipy=True)
    _, clipped = SM.correlations(x.astype(np.float64), y.astype(np.float64))
    assert 0.10 <= clipped.mean() <= 0.90


def test_float32_mirror_is_within_1e_6_of_float64():
    bar, diffs = SM.e2e_bar()
    print("largest |float32 mirror - float64 model| = %.3e, GPU bar = %.3e" % (max(diffs.values()), bar), diffs)
    assert set(diffs) == set(SM.VALID_CASES) and max(diffs.values()) <= 1e-6
    assert bar == 16.0 * max(diffs.values())
    for k in SM.INVALID_CASES:
        assert SM.stoi32(*SM.pair(k)) is None


def test_the_allowance_is_far_below_what_a_mistake_costs(models):
    """Each one-line mistake moves d by more than 100 x the GPU bar on every end-to-end case (or leaves no score at all)."""
    bar, _ = SM.e2e_bar()
    for k in SM.VALID_CASES:
        x, y = SM.pair(k)
        for name, kw in SM.MUTANTS.items():
            d = SM.stoi64(x, y, **kw)["d"]
            assert d is None or abs(d - models[k]["d"]) > 100.0 * bar, (k, name, d, models[k]["d"], bar)
        assert sum(SM.stoi64(x, y, **kw)["d"] is not None for kw in SM.MUTANTS.values()) >= 3


def test_envelope_bound_is_far_below_a_one_bin_band_shift():
    """The bound of stoi_models.envelope_bound (derived there term by term) against the float32 mirror, which must lie inside it, and
    against the model with every band edge one bin up: the typical cost of that mistake is more than 10 bounds on the noise inputs, and
    more than 100 in some band for every tone at a band edge."""
    shifted = tuple(v + 1 for v in SM.LO)
    for k, s in SM.band_inputs().items():
        t = SM.bands64(s)
        bound = SM.envelope_bound(s, t)
        assert (np.abs(SM.bands32(s) - t) <= bound).all(), k
        cost = np.abs(SM.bands64(s, lo=shifted) - t) / bound
        if k.startswith("tone"):
            assert cost.max() > 100.0, (k, cost.max())
        else:
            assert np.median(cost) > 10.0 and (bound <= 0.03 * t).all(), (k, np.median(cost))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_before_any_device_call(built_lib):
    from set_amd import _lib
    L, p = built_lib, 64  # p: a non-null, aligned address that is never dereferenced
    sel = lambda **o: L.set_stoi_select(*[{**dict(x=p, bs=4096, ln=None, win=p, nrm=p, kept=p, K=p, B=1, N=4096, nf=1024, st=None), **o}[k]
                                          for k in ("x", "bs", "ln", "win", "nrm", "kept", "K", "B", "N", "nf", "st")])
    com = lambda **o: L.set_stoi_compact(*[{**dict(x=p, y=p, bs=4096, win=p, kept=p, K=p, sil=p, sbs=3584, sl=p, B=1, N=4096, nf=1024, st=None),
                                            **o}[k] for k in ("x", "y", "bs", "win", "kept", "K", "sil", "sbs", "sl", "B", "N", "nf", "st")])
    ban = lambda **o: L.set_stoi_bands(*[{**dict(sil=p, sbs=3584, ln=None, tab=p, bas=p, tob=p, R=2, N=3584, T=10, nfft=1024, hop=256, nb=15,
                                                 lo=0, nbins=199, st=None), **o}[k]
                                         for k in ("sil", "sbs", "ln", "tab", "bas", "tob", "R", "N", "T", "nfft", "hop", "nb", "lo", "nbins", "st")])
    sco = lambda **o: L.set_stoi_score(*[{**dict(tob=p, ln=None, d=p, v=p, B=1, T=40, nb=15, seg=30, st=None), **o}[k]
                                         for k in ("tob", "ln", "d", "v", "B", "T", "nb", "seg", "st")])
    for call, name, unsupported, invalid in (
            (sel, b"set_stoi_select", [dict(nf=512)], [dict(x=None), dict(K=None), dict(B=0), dict(N=1024), dict(bs=100)]),
            (com, b"set_stoi_compact", [dict(nf=2048)], [dict(y=None), dict(sl=None), dict(N=1024), dict(sbs=3583), dict(B=0)]),
            (ban, b"set_stoi_bands", [dict(nfft=2048), dict(hop=128), dict(nb=33)],
             [dict(sil=None), dict(tob=None), dict(T=9), dict(N=1024, T=0), dict(lo=16), dict(nbins=514), dict(tab=68), dict(R=0)]),
            (sco, b"set_stoi_score", [dict(nb=33), dict(seg=29)], [dict(d=None), dict(v=None), dict(tob=None), dict(B=0), dict(T=-1)])):
        for over in unsupported:
            assert call(**over) == _lib.E_UNSUPPORTED, (name, over)
            assert name in L.set_last_error()
        for over in invalid:
            assert call(**over) == _lib.E_INVALID, (name, over)
            assert name in L.set_last_error()


def test_no_cpu_fallback_and_argument_checks(MT):
    x = torch.zeros(2, 9000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.stoi(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.wav_stoi(x, x)
    with pytest.raises(NotImplementedError):
        MT.stoi(x, x, extended=True)  # refused before the tensors are looked at
    from set_amd import ops
    for fn, args in ((ops.stoi_select, (x, torch.zeros(1024))), (ops.stoi_compact, (x, x, torch.zeros(1024), None, None)),
                     (ops.stoi_bands, (x, torch.zeros(4), torch.zeros(4))), (ops.stoi_score, (torch.zeros(2, 40, 15),))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args) if fn is not ops.stoi_bands else fn(*args, n_bands=15, bin_lo=0, nbins=199)
    assert float(MT.stoi_mean(torch.tensor([0.5, float("nan"), 0.7]), torch.tensor([True, False, True]))) == pytest.approx(0.6)
