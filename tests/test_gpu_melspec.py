"""GPU checks of the log-mel front end (csrc/melspec.hip through set_amd.melspec): every branch of the kernel against the float64 model
of the reference (melspec_models.model_a) at the project's mel parity bar, max |d log-mel| < 1e-4 over all frames t < T_b.

Signals: two sines (220 Hz, and 3300 Hz at 0.3x) plus white noise at 5 % of the amplitude, six leading hops silent, at amplitude 0.5 and
1e-3.  The noise floor is a condition of the bar: with it the reference's own float32 arithmetic stays within ~5e-6 of the float64 model;
without it, float32 itself is at 1.5e-4 to 2.6e-4.  Waveforms of six hops or fewer would be silence only under that rule, so they run twice:
as stated (all frames at the floor) and with one silent hop.  Shapes are the smallest at which each branch can go wrong (TT = 64 frames per
block)."""
import math

import numpy as np
import pytest
import torch

import melspec_models as MM
from melspec_models import HOP, N_FFT, SR

pytestmark = pytest.mark.gpu

TT = 64  # the kernel's frame tile
BAR = 1e-4
FLAVOURS = ("librosa", "hifigan")
HP = {"fft_size": 1024, "win_size": 1024, "hop_size": 256, "audio_num_mel_bins": 80, "audio_sample_rate": SR, "fmin": 55, "fmax": 7600}
FLOOR_LOG = {f: MM.LOG_SCALE[f] * math.log(MM.FLOOR[f]) for f in FLAVOURS}  # log10(1e-6f), ln(1e-5f)
MEASURED = {}


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import set_amd  # noqa: F401
    from set_amd import melspec
    return melspec


_FE = {}


def _fe(M, flavour, mel_basis=None, key=None, **over):
    k = (flavour, key, tuple(sorted(over.items())))
    if k not in _FE:
        _FE[k] = M.LogMel(dict(HP, **over), flavour, mel_basis=mel_basis)
    return _FE[k]


def _check(fe, wav, dev, lead):
    """Run one waveform, compare with Model A at the bar, check the silent frames; returns the kernel's [T, n_mels] array."""
    out = fe(torch.from_numpy(wav).to(dev)).cpu().numpy()
    ref = MM.model_a(wav, fe.flavour, fe._basis, fe.win_length)
    assert out.shape == ref.shape and out.dtype == np.float32
    err = float(np.abs(out.astype(np.float64) - ref).max())
    MEASURED[fe.flavour] = max(MEASURED.get(fe.flavour, 0.0), err)
    print("%s N=%d n_mels=%d win=%d bins [%d, %d): max |d log-mel| = %.3e" % (fe.flavour, len(wav), fe.n_mels, fe.win_length, fe.bin_lo,
                                                                               fe.bin_hi, err))
    assert err < BAR, err
    # frames whose whole window lies in the silent lead (reflections of silence included) sit at the floor value
    silent = [t for t in range(out.shape[0]) if t * HOP + N_FFT - fe.pad <= lead]
    if silent:
        assert np.abs(out[silent].astype(np.float64) - FLOOR_LOG[fe.flavour]).max() <= 1e-6
    return out


def _n_for_frames(flavour, T):
    return (T - 1) * HOP if flavour == "librosa" else T * HOP


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("amp", [0.5, 1e-3])
def test_frame_tile_edges(M, dev, flavour, amp):
    fe = _fe(M, flavour)
    for T in (TT - 1, TT, TT + 1):
        n = _n_for_frames(flavour, T)
        assert fe.frames(n) == T
        assert _check(fe, MM.signal(n, amp, seed=T), dev, 6 * HOP).shape[0] == T
    for n in (768, 256 * 5 + 77):  # every frame mostly padding; not a hop multiple
        _check(fe, MM.signal(n, amp, seed=n), dev, 6 * HOP)          # six silent hops: silence only, every frame at the floor
        _check(fe, MM.signal(n, amp, seed=n, lead=HOP), dev, HOP)    # one silent hop: the padding rule at both ends under signal


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("amp", [0.5, 1e-3])
def test_bin_ranges_small_filterbank_and_short_window(M, dev, flavour, amp):
    wav = MM.signal(256 * 9 + 33, amp, seed=11)
    full = _fe(M, flavour, fmin=0, fmax=-1)                          # bins [0, 512): 16 whole chunks
    assert (full.bin_lo, full.bin_hi) == (0, 512)
    _check(full, wav, dev, 6 * HOP)
    nyq = _fe(M, flavour, mel_basis=MM.with_nyquist_weight(full._basis), key="nyquist", fmin=0, fmax=-1)
    assert (nyq.bin_lo, nyq.bin_hi) == (0, 513)                      # 17 chunks, the last with one live bin
    out = _check(nyq, wav, dev, 6 * HOP)
    assert not np.array_equal(out, full(torch.from_numpy(wav).to(dev)).cpu().numpy())  # bin 512 is really summed
    hi_band = _fe(M, flavour, audio_num_mel_bins=40, fmin=1500, fmax=7600)
    assert hi_band.bin_lo == 64                                      # bin_lo > 0
    _check(hi_band, wav, dev, 6 * HOP)
    assert (_fe(M, flavour).bin_lo, _fe(M, flavour).bin_hi) == (0, 384)
    _check(_fe(M, flavour, audio_num_mel_bins=20), wav, dev, 6 * HOP)    # 20 mel rows: zero rows in the first 32-row block, two empty blocks
    _check(_fe(M, flavour, audio_num_mel_bins=22), wav, dev, 6 * HOP)    # not a multiple of 4: the scalar stores
    _check(_fe(M, flavour, win_size=512), wav, dev, 6 * HOP)             # short window, centred in 1024


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_ragged_batch_rows_equal_single_runs_bit_for_bit(M, dev, flavour):
    fe = _fe(M, flavour)
    n = 256 * 70 + 3  # two tiles; the short rows leave the second tile, and most of the first, to the pad value
    lens = [n, 256 * 7 + 5, 400]
    wav = np.full((3, n), np.nan, dtype=np.float32)  # a read past a row's length shows up as NaN
    for b, ln in enumerate(lens):
        wav[b, :ln] = MM.signal(ln, 0.5, seed=20 + b, lead=HOP)
    mel, mel_len = fe(torch.from_numpy(wav).to(dev), lengths=lens)
    again, _ = fe(torch.from_numpy(wav).to(dev), lengths=torch.tensor(lens, device=dev))
    assert torch.equal(mel, again)  # reproducible, bit for bit
    mel = mel.cpu().numpy()
    assert mel_len.tolist() == [fe.frames(ln) for ln in lens] and mel.shape == (3, fe.frames(n), 80)
    assert np.isfinite(mel).all()
    for b, ln in enumerate(lens):
        Tb = fe.frames(ln)
        single = fe(torch.from_numpy(wav[b, :ln].copy()).to(dev)).cpu().numpy()
        assert single.shape == (Tb, 80)
        assert np.array_equal(mel[b, :Tb].view(np.uint32), single.view(np.uint32)), (flavour, b)
        assert not mel[b, Tb:].any() and not np.signbit(mel[b, Tb:]).any()  # exactly 0.0 beyond the row's frames
        ref = MM.model_a(wav[b, :ln], flavour, fe._basis)
        err = float(np.abs(mel[b, :Tb].astype(np.float64) - ref).max())
        MEASURED[flavour] = max(MEASURED.get(flavour, 0.0), err)
        assert err < BAR, (b, err)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_two_runs_are_bit_identical(M, dev, flavour):
    fe = _fe(M, flavour)
    wav = torch.from_numpy(np.stack([MM.signal(256 * 130, 0.5, seed=s) for s in range(4)])).to(dev)
    assert torch.equal(fe(wav), fe(wav))


def test_input_clamp_in_the_hifigan_flavour_only(M, dev):
    wav = MM.signal(256 * 10, 0.5, seed=5)
    hot, clamped = wav.copy(), wav.copy()
    hot[2000], clamped[2000] = 1.5, 1.0
    for flavour in FLAVOURS:
        fe = _fe(M, flavour)
        a, b = fe(torch.from_numpy(hot).to(dev)), fe(torch.from_numpy(clamped).to(dev))
        assert torch.equal(a, b) == (flavour == "hifigan")
        ref = MM.model_a(hot, flavour, fe._basis)
        assert float(np.abs(a.cpu().numpy().astype(np.float64) - ref).max()) < BAR


def test_refusals(M, dev):
    fe = _fe(M, "hifigan")
    with pytest.raises(ValueError):
        fe(torch.zeros(384, device=dev))                              # reflect pad of 384 needs more than 384 samples
    with pytest.raises(ValueError):
        fe(torch.zeros(2, 2048, device=dev), lengths=[2048, 384])
    assert fe(torch.zeros(385, device=dev)).shape == (1, 80)
    with pytest.raises(ValueError):
        M.LogMel(HP, "librosa", mel_basis=np.zeros((80, 512), dtype=np.float32))
    with pytest.raises(ValueError):
        _fe(M, "librosa")(torch.zeros(2, 2048, device=dev), lengths=[2048, 4096])
    from set_amd._lib import SetAmdError
    for over in ({"fft_size": 2048, "win_size": 2048}, {"hop_size": 128}, {"audio_num_mel_bins": 128}):
        with pytest.raises(SetAmdError, match="set_log_mel"):
            M.LogMel(dict(HP, **over), "librosa")(torch.zeros(8192, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _fe(M, "librosa")(torch.zeros(4096))


def test_wav2spec_returns_the_reference_dict(M, dev):
    for n in (256 * 9, 256 * 9 + 77, 256 * 9 - 1):
        wav = MM.signal(n, 0.5, seed=n)
        d = M.wav2spec(wav, HP)
        T = 1 + n // HOP
        assert set(d) == {"wav", "mel", "mel_basis"}
        assert d["mel"].shape == (T, 80) and d["wav"].shape == (T * HOP,) and d["mel_basis"].shape == (80, 513)
        assert np.array_equal(d["wav"].cpu().numpy()[:n], wav) and not d["wav"].cpu().numpy()[n:].any()
        assert float(np.abs(d["mel"].cpu().numpy().astype(np.float64) - MM.model_a(wav, "librosa", d["mel_basis"])).max()) < BAR
    mine = MM.with_nyquist_weight(M.slaney_mel_basis(SR, N_FFT, 80, 0, -1))
    d = M.wav2spec(torch.from_numpy(wav).to(dev), HP, mel_basis=mine, flavour="hifigan")
    assert d["mel_basis"] is mine and d["mel"].shape == (n // HOP, 80) and d["wav"].shape == (n // HOP * HOP,)
    assert float(np.abs(d["mel"].cpu().numpy().astype(np.float64) - MM.model_a(wav, "hifigan", mine)).max()) < BAR
    d20 = M.wav2spec(wav, HP, audio_num_mel_bins=20)
    assert d20["mel"].shape == (T, 20)
    with pytest.raises(TypeError):
        M.wav2spec(wav, HP, loud_norm=True)


def _item(n_frames_, wav=None, mel=None):
    rng = np.random.default_rng(4)
    it = {"item_name": "x", "text": "t", "ph": "p", "ph_token": [1, 2, 3], "edited_ph_token": [1, 2, 4, 3], "ph2word": [1, 1, 2],
          "edited_ph2word": [1, 1, 2, 2], "mel2ph": rng.integers(1, 4, n_frames_), "mel2word": rng.integers(1, 3, n_frames_),
          "dur": [3, 3, 3], "f0": rng.random(n_frames_).astype(np.float32), "uv": np.zeros(n_frames_, dtype=np.float32),
          "spk_embed": rng.random(256).astype(np.float32), "words_region": [[2, 2]], "edited_words_region": [[2, 2]]}
    if wav is not None:
        it["wav"] = wav
    if mel is not None:
        it["mel"] = mel
    return it


def test_input_to_batch_computes_the_mel_from_the_wav(M, dev):
    from set_amd.infer import SpecDenoiserInfer
    inf = SpecDenoiserInfer(dict(HP), device=dev, model=torch.nn.Module(), vocoder=torch.nn.Module())
    n = 256 * 9 + 77
    wav = MM.signal(n, 0.5, seed=9)
    T = 1 + n // HOP
    batch = inf.input_to_batch(_item(T, wav=wav))
    want = M.LogMel(HP, "librosa")(torch.from_numpy(wav).to(dev)[None])
    assert batch["mel"].shape == (1, T, 80) and torch.equal(batch["mel"], want)
    assert torch.equal(batch["wav"], torch.from_numpy(wav).to(dev)[None])
    with pytest.raises(ValueError):
        inf.input_to_batch(_item(T - 1, wav=wav))  # mel2ph one frame short
    # an item that carries 'mel' takes the path it always took: the batch of the code before this feature, key by key
    mel = np.random.default_rng(1).standard_normal((T - 1, 80)).astype(np.float32)  # (its frame count is not checked, as before)
    it = _item(T, wav=wav, mel=mel)
    got = inf.input_to_batch(it)

    def L(k):
        return torch.as_tensor(np.asarray(it[k]), dtype=torch.int64)[None, :].to(dev)

    def Fl(k):
        return torch.as_tensor(np.asarray(it[k]), dtype=torch.float32)[None, :].to(dev)

    exp = {"item_name": ["x"], "text": ["t"], "ph": ["p"], "ph2word": L("ph2word"), "edited_ph2word": L("edited_ph2word"),
           "mel2ph": L("mel2ph"), "mel2word": L("mel2word"), "dur": L("dur"), "txt_tokens": L("ph_token"),
           "edited_txt_tokens": L("edited_ph_token"), "words_region": it["words_region"], "edited_words_region": it["edited_words_region"],
           "mel": Fl("mel"), "spk_embed": Fl("spk_embed"), "f0": Fl("f0"), "uv": Fl("uv"),
           "txt_lengths": torch.tensor([3], dtype=torch.int64, device=dev), "wav": Fl("wav")}
    assert list(got) == list(exp)
    for k in exp:
        if isinstance(exp[k], torch.Tensor):
            assert got[k].dtype == exp[k].dtype and got[k].device == exp[k].device and torch.equal(got[k], exp[k]), k
        else:
            assert got[k] == exp[k], k


def test_report_measured_maxima():
    """Printed last: the largest |d log-mel| against Model A seen by the tests above, per flavour (DESIGN.md quotes them)."""
    print("measured max |d log-mel|: " + ", ".join("%s %.3e" % kv for kv in sorted(MEASURED.items())))
    assert all(v < BAR for v in MEASURED.values())
