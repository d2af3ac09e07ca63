"""CPU checks of the log-mel front end (set_amd.melspec, csrc/melspec.hip's host side): the float64 model of the kernel's formulation
against the float64 model of the reference, the DFT table and its image, the restated Slaney filterbank, frame counts and pad rules,
and the entry's refusals on the built library.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import melspec_models as MM
from melspec_models import HOP, N_FFT, SR

FLAVOURS = ("librosa", "hifigan")


@pytest.fixture(scope="module")
def M():
    import set_amd  # noqa: F401
    from set_amd import melspec
    return melspec


@pytest.fixture(scope="module")
def shipped(M):
    return M.slaney_mel_basis(SR, N_FFT, 80, 55, 7600)


@pytest.fixture(scope="module")
def fullband(M):
    return M.slaney_mel_basis(SR, N_FFT, 80, 0, -1)


# ---- Model A (the reference, line by line) against Model B (the kernel's matrices), to table rounding ------------------------------------
def _ab_case(M, wav, flavour, basis, win_length):
    lo, hi = M.bin_range(basis)
    table = M.dft_table(N_FFT, win_length, lo, hi - lo)
    a = MM.model_a(wav, flavour, basis, win_length)
    b, mel_b, frames = MM.model_b(wav, flavour, basis, table, lo, win_length, return_parts=True)
    assert a.shape == b.shape == (M.n_frames(len(wav), flavour, N_FFT, HOP), basis.shape[0])
    # The bound, from the table's rounding alone: an entry is its float64 value rounded once, so it is off by at most 2^-24 |entry| <=
    # 2^-24 win[n]; over a frame, |d re|, |d im| <= 2^-24 ||win||_2 ||frame||_2 (Cauchy-Schwarz), so |d mag| <= sqrt(2) times that (the
    # magnitude, with or without its epsilon, is 1-Lipschitz in (re, im)); |d mel[m]| <= rowsum(basis[m]) |d mag|; and the clamped log
    # moves by at most scale |d mel| / (the smaller of the two clamped arguments).  1e-10 covers the float64 arithmetic of both models.
    win_norm = np.linalg.norm(M.hann_padded(N_FFT, win_length))
    d_mag = math.sqrt(2.0) * 2.0 ** -24 * win_norm * np.linalg.norm(frames, axis=1)                  # [T]
    d_mel = d_mag[:, None] * np.asarray(basis, dtype=np.float64).sum(axis=1)[None, :]                # [T, n_mels]
    floor = MM.FLOOR[flavour]
    bound = MM.LOG_SCALE[flavour] * d_mel / np.maximum(floor, np.maximum(mel_b, floor) - d_mel) + 1e-10
    err = np.abs(a - b)
    assert (err <= bound).all(), (flavour, len(wav), win_length, float(err.max()), float(bound.max()))
    return float(err.max()), float(bound.max())


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n", [256 * 24, 256 * 9 + 77, 768])
@pytest.mark.parametrize("amp", [0.5, 1e-3])
def test_kernel_formulation_equals_the_reference_to_table_rounding(M, shipped, flavour, n, amp):
    """A wrong window, bin offset, pad rule, frame count or log base shows here as an error of 1e-2 or more; the allowance is ~1e-6."""
    lead = 6 * HOP if n > 12 * HOP else HOP
    _ab_case(M, MM.signal(n, amp, seed=n, lead=lead), flavour, shipped, N_FFT)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_allowance_is_far_below_what_a_mistake_costs(M, shipped, flavour):
    """The same comparison with the table shifted by one bin, or built for a 1023-sample window, must fail."""
    wav = MM.signal(256 * 12, 0.5, seed=1)
    real = M.dft_table
    for wrong in (lambda n_fft, win, lo, nb: real(n_fft, win, lo + 1, nb), lambda n_fft, win, lo, nb: real(n_fft, win - 1, lo, nb)):
        M.dft_table = wrong
        try:
            with pytest.raises(AssertionError):
                _ab_case(M, wav, flavour, shipped, N_FFT)
        finally:
            M.dft_table = real


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_kernel_formulation_short_window_and_other_filterbanks(M, fullband, flavour):
    wav = MM.signal(256 * 12 + 5, 0.5, seed=3)
    _ab_case(M, wav, flavour, M.slaney_mel_basis(SR, N_FFT, 80, 55, 7600), 512)       # win_length 512, centred in 1024
    _ab_case(M, wav, flavour, fullband, N_FFT)                                         # 512 bins from bin 0
    _ab_case(M, wav, flavour, MM.with_nyquist_weight(fullband), N_FFT)                 # 513 bins: the one-bin last chunk
    _ab_case(M, wav, flavour, M.slaney_mel_basis(SR, N_FFT, 20, 55, 7600), N_FFT)      # 20 mel rows
    hi_band = M.slaney_mel_basis(SR, N_FFT, 40, 1500, 7600)                            # a filterbank that starts above the first chunk
    assert M.bin_range(hi_band)[0] == 64
    _ab_case(M, wav, flavour, hi_band, N_FFT)


def test_input_clamp_only_in_the_hifigan_flavour(M, shipped):
    wav = MM.signal(256 * 10, 0.5, seed=5)
    hot = wav.copy()
    hot[2000] = 1.5
    clamped = hot.copy()
    clamped[2000] = 1.0
    lo, hi = M.bin_range(shipped)
    table = M.dft_table(N_FFT, N_FFT, lo, hi - lo)
    assert np.array_equal(MM.model_b(hot, "hifigan", shipped, table, lo), MM.model_b(clamped, "hifigan", shipped, table, lo))
    assert not np.array_equal(MM.model_b(hot, "librosa", shipped, table, lo), MM.model_b(clamped, "librosa", shipped, table, lo))


# ---- the DFT table and its image -----------------------------------------------------------------------------------------------------------
def _table_definition(win_length, bin_lo, nbins):
    """win[n] cos / -sin(2 pi f n / n_fft) in float64 from scalar code of its own (torch's window, the angle reduced in integers)."""
    win = torch.zeros(N_FFT, dtype=torch.float64)
    left = (N_FFT - win_length) // 2
    win[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    f = torch.arange(bin_lo, bin_lo + nbins, dtype=torch.int64)[:, None]
    n = torch.arange(N_FFT, dtype=torch.int64)[None, :]
    ang = ((f * n) % N_FFT).double() * (2.0 * math.pi / N_FFT)
    return torch.stack([win * torch.cos(ang), -win * torch.sin(ang)]).numpy()


@pytest.mark.parametrize("win_length,bin_lo,nbins", [(1024, 0, 384), (512, 0, 513), (1024, 64, 300)])
def test_table_rows_are_the_definition_rounded_once(M, win_length, bin_lo, nbins):
    t = M.dft_table(N_FFT, win_length, bin_lo, nbins)
    assert t.dtype == np.float32 and t.shape == (2, nbins, N_FFT)
    d = _table_definition(win_length, bin_lo, nbins)
    # one rounding to float32: within half an ulp, 2^-24 |value| (2^-150 in the subnormal range); 1e-15 for the two float64 evaluations
    assert (np.abs(t.astype(np.float64) - d) <= 2.0 ** -24 * np.abs(d) + 2.0 ** -150 + 1e-15).all()
    if bin_lo == 0:  # bin 0 is the window itself, and has no imaginary part
        assert np.array_equal(t[0, 0], M.hann_padded(N_FFT, win_length).astype(np.float32)) and not t[1, 0].any()


def test_short_window_is_centred(M):
    t = M.dft_table(N_FFT, 512, 0, 32)
    assert not t[:, :, :256].any() and not t[:, :, 768:].any()
    assert np.array_equal(t[0, 0, 256:768], torch.hann_window(512, periodic=True, dtype=torch.float64).numpy().astype(np.float32))
    with pytest.raises(ValueError):
        M.hann_padded(N_FFT, 2048)


@pytest.mark.parametrize("nbins", [384, 513, 32])
def test_pack_and_unpack_are_inverse_bit_for_bit(M, built_lib, nbins):
    rng = np.random.default_rng(nbins)
    t = rng.standard_normal((2, nbins, N_FFT)).astype(np.float32)
    img = M.pack_dft_table(t)
    assert img.dtype == np.float32 and img.size == built_lib.set_log_mel_table_size(N_FFT, nbins)
    assert np.array_equal(M.unpack_dft_table(img, nbins).view(np.uint32), t.view(np.uint32))
    # the documented element order (include/set_amd.h), at random places of the image
    nch = (nbins + 31) // 32
    for _ in range(200):
        ch, p, lane, e = rng.integers(nch), rng.integers(N_FFT // 4), rng.integers(64), rng.integers(4)
        row, n = 32 * ch + (lane & 31), 4 * p + 2 * (e >> 1) + (lane >> 5)
        assert img[ch, p, lane, e] == (t[e & 1, row, n] if row < nbins else 0.0)
    real = M.dft_table(N_FFT, 1024, 0, nbins)
    assert np.array_equal(M.unpack_dft_table(M.pack_dft_table(real), nbins).view(np.uint32), real.view(np.uint32))


def test_filterbank_image_lists_bins_in_accumulator_row_order(M, fullband):
    lo, hi = M.bin_range(fullband)
    img = M.pack_mel_basis(fullband, lo, hi - lo)
    assert img.shape == ((hi - lo + 31) // 32, 16, 64, 4) and not img[..., 3].any()
    rng = np.random.default_rng(0)
    for _ in range(400):
        ch, r, lane, e = rng.integers(img.shape[0]), rng.integers(16), rng.integers(64), rng.integers(3)
        m, b = 32 * e + (lane & 31), lo + 32 * ch + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        assert img[ch, r, lane, e] == (fullband[m, b] if m < 80 and b < 513 else 0.0)
    # every (mel row, bin) of the matrix is in the image exactly once: the image's sum is the matrix's sum, bit for bit in float64
    assert img.astype(np.float64).sum() == pytest.approx(float(fullband.astype(np.float64).sum()), rel=1e-12)
    assert np.count_nonzero(img) == np.count_nonzero(fullband)


def test_bin_range_is_the_support_widened_to_chunks(M, shipped, fullband):
    def last_weighted(b):
        return int(np.nonzero(b.any(axis=0))[0][-1])
    # fmin = 0, fmax = sr/2: the last triangle's upper edge IS bin 512 (11025 Hz exactly, on a linspace and on an rfftfreq grid alike), where
    # its weight is exactly 0 -- the last bin with weight is 511, not 512.  A caller's matrix with weight there gets all 513 bins.
    assert last_weighted(shipped) == 352 and last_weighted(fullband) == 511 and not fullband[:, 512].any() and not fullband[:, 0].any()
    assert M.bin_range(shipped) == (0, 384)       # bins 3 .. 352 carry weight: chunks 0 .. 11
    assert M.bin_range(fullband) == (0, 512)      # bins 1 .. 511: 16 whole chunks
    assert M.bin_range(MM.with_nyquist_weight(fullband)) == (0, 513)  # 17 chunks, the last with the one live bin 512
    for b in (shipped, fullband, M.slaney_mel_basis(SR, N_FFT, 40, 1500, 7600), M.slaney_mel_basis(SR, N_FFT, 20, 700, 3000)):
        cols = np.nonzero(b.any(axis=0))[0]
        lo, hi = M.bin_range(b)
        assert lo % 32 == 0 and lo <= cols[0] < lo + 32
        assert hi == min(513, (cols[-1] // 32 + 1) * 32) and hi - 32 <= cols[-1] < hi


# ---- the filterbank ------------------------------------------------------------------------------------------------------------------------
def _slaney_hz(m):
    return 200.0 / 3 * m if m < 15.0 else 1000.0 * math.exp(math.log(6.4) / 27.0 * (m - 15.0))


def _slaney_mel(f):
    return f / (200.0 / 3) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


@pytest.mark.parametrize("n_mels,fmin,fmax", [(80, 55, 7600), (80, 0, SR / 2), (20, 55, 7600), (96, 80, 11025)])
def test_filterbank_is_slaney_triangles_with_unit_area(M, n_mels, fmin, fmax):
    w = M.slaney_mel_basis(SR, N_FFT, n_mels, fmin, fmax)
    assert w.dtype == np.float32 and w.shape == (n_mels, 513) and (w >= 0).all()
    lo, hi = _slaney_mel(fmin), _slaney_mel(fmax)
    edges = [_slaney_hz(lo + (hi - lo) * k / (n_mels + 1)) for k in range(n_mels + 2)]
    df = SR / N_FFT
    for m in range(n_mels):
        f0, f1, f2 = edges[m], edges[m + 1], edges[m + 2]
        # a single triangle of height 2 / (f2 - f0) at f1: every weight is the triangle's value at its bin, zero outside (f0, f2)
        h = 2.0 / (f2 - f0)
        want = np.array([h * max(0.0, min((k * df - f0) / (f1 - f0), (f2 - k * df) / (f2 - f1))) for k in range(513)])
        assert (np.abs(w[m] - want) <= 1e-6 * h).all(), m
        nz = np.nonzero(w[m])[0]
        if nz.size:
            assert nz.tolist() == list(range(nz[0], nz[-1] + 1)) and f0 < nz[0] * df and nz[-1] * df < f2
            peak = int(np.argmax(w[m]))
            assert (np.diff(w[m, nz[0]:peak + 1]) >= 0).all() and (np.diff(w[m, peak:nz[-1] + 1]) <= 0).all()
        # unit area: the Riemann sum of a piecewise-linear function at spacing df misses its integral (1) by at most df^2 / 8 times the
        # slope change at each of its three kinks, (df^2 / 4) (s1 + s2) in all; float32 rounding of the weights adds 2^-24 per term
        if f1 - f0 > 2 * df and f2 - f1 > 2 * df:
            s1, s2 = h / (f1 - f0), h / (f2 - f1)
            assert abs(float(w[m].astype(np.float64).sum()) * df - 1.0) <= df * df / 4 * (s1 + s2) + 1e-6, m


def test_filterbank_minus_one_conventions(M):
    assert np.array_equal(M.slaney_mel_basis(SR, N_FFT, 80, -1, -1), M.slaney_mel_basis(SR, N_FFT, 80, 0, SR / 2))
    assert np.array_equal(M.slaney_mel_basis(SR, N_FFT, 80, 55, -1), M.slaney_mel_basis(SR, N_FFT, 80, 55, 11025.0))
    assert not np.array_equal(M.slaney_mel_basis(SR, N_FFT, 80, 55, -1), M.slaney_mel_basis(SR, N_FFT, 80, 55, 7600))


# ---- frames, 'wav' length, pad rules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n", [256 * 8, 256 * 8 - 1, 256 * 8 + 1, 768, 1023, 400, 385])
def test_frame_counts_and_wav_length(M, flavour, n):
    y = MM.padded(np.zeros(n, dtype=np.float32), flavour)
    want = 1 + (y.shape[0] - N_FFT) // HOP if y.shape[0] >= N_FFT else 0
    if y.shape[0] >= N_FFT:
        assert torch.stft(y, N_FFT, hop_length=HOP, window=torch.ones(N_FFT, dtype=torch.float64), center=False,
                          return_complex=True).shape[1] == want
    assert M.n_frames(n, flavour, N_FFT, HOP) == want
    if flavour == "librosa":
        assert want == 1 + n // HOP
        # librosa_pad_lr (utils/audio/__init__.py:8-17,76-78): right-pad to (n // hop + 1) hop, cut to T hop: exactly T hop samples
        assert min((n // HOP + 1) * HOP, want * HOP) == want * HOP
    else:
        assert want == (1 + (n - HOP) // HOP if n >= HOP else 0)


@pytest.mark.parametrize("n", [385, 400, 1000, 256 * 7 + 5])
def test_reflect_index_rule_at_both_ends(M, n):
    pad = M.flavour_pad("hifigan", N_FFT, HOP)
    assert pad == 384 and M.flavour_pad("librosa", N_FFT, HOP) == 512
    x = np.arange(n, dtype=np.float32) / 4096.0  # exactly representable, all different, inside the clamp
    y = MM.padded(x, "hifigan").numpy()
    got = np.array([x[M.reflect_index(i, n, pad)] for i in range(n + 2 * pad)], dtype=np.float64)
    assert np.array_equal(got, y)
    assert M.reflect_index(0, n, pad) == pad and M.reflect_index(pad - 1, n, pad) == 1
    assert M.reflect_index(pad + n, n, pad) == n - 2 and M.reflect_index(n + 2 * pad - 1, n, pad) == n - 1 - pad
    with pytest.raises(RuntimeError):  # torch refuses pad >= length; so does LogMel (GPU test) and the entry below
        MM.padded(np.zeros(384, dtype=np.float32), "hifigan")


# ---- the entry's refusals, on the built library without a GPU ------------------------------------------------------------------------------
def _args(_lib, **over):
    a = _lib.SetLogMelArgs(wav=16, lengths=None, table=16, basis=16, mel=16, wav_bs=4096, log_scale=1.0, B=1, N=4096, T=17, n_fft=1024,
                           hop=256, n_mels=80, bin_lo=0, nbins=384, pad=512, reflect=0, clamp_input=0, mag_eps=0.0, floor=1e-6)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entry_refuses_before_any_device_call(built_lib):
    from set_amd import _lib
    L = built_lib
    assert L.set_sizeof_log_mel_args() == C.sizeof(_lib.SetLogMelArgs)
    assert L.set_log_mel(None, None) == _lib.E_INVALID
    assert b"set_log_mel" in L.set_last_error()
    for over in (dict(n_fft=2048, T=13), dict(hop=128, T=33), dict(n_mels=128)):
        assert L.set_log_mel(C.byref(_args(_lib, **over)), None) == _lib.E_UNSUPPORTED, over
        assert b"set_log_mel" in L.set_last_error()
    for over in (dict(wav=None), dict(mel=None), dict(B=0), dict(T=16), dict(bin_lo=16), dict(nbins=514), dict(floor=0.0),
                 dict(reflect=1, pad=384, N=384, wav_bs=384, T=1), dict(table=20)):
        assert L.set_log_mel(C.byref(_args(_lib, **over)), None) == _lib.E_INVALID, over
    assert L.set_log_mel_table_size(1024, 352) == 2 * 352 * 1024 and L.set_log_mel_table_size(1024, 513) == 2 * 544 * 1024
    assert L.set_abi_version() == 5


def test_no_cpu_fallback(M, shipped):
    from set_amd import ops
    wav = torch.zeros(1, 4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.log_mel(wav, torch.zeros(4), torch.zeros(4), None, n_fft=1024, hop=256, n_mels=80, bin_lo=0, nbins=384, pad=512,
                    **M.FLAVOURS["librosa"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.LogMel({"fft_size": 1024, "hop_size": 256, "win_size": 1024, "audio_num_mel_bins": 80, "audio_sample_rate": SR, "fmin": 55,
                  "fmax": 7600})(wav)
    with pytest.raises(ValueError):
        M.LogMel({"audio_num_mel_bins": 80}, mel_basis=np.zeros((80, 512), dtype=np.float32))
    with pytest.raises(ValueError):
        M.LogMel({}, flavour="htk")
