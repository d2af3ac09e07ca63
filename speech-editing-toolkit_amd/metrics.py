"""Evaluation metrics on the GPU: mel-cepstral distortion (csrc/mcd.hip), short-time objective intelligibility (csrc/stoi.hip; the
second part of this file) and the wav-level mel-cepstral distortion of the reference's eval script (csrc/wav_mcd.hip; the third part).

Mel-cepstral distortion: mel -> MFCC -> exact DTW or zero fill -> (mcd, penalty, frames) per pair.

After the reference's utils/eval/mcd.py `get_metrics_mels`, term by term:

    mfcc      `get_mfccs_of_mel_spectogram`: librosa.feature.mfcc(S=., n_mfcc=K+1, norm=None, dct_type=2, lifter=0)[1:] / 2.  The factor 2
              of the unnormalised DCT-II and the /2 cancel: c_k = sum_n x_n cos(pi k (2n+1) / (2M)), k = 1..K.
    dtw       utils/metrics/dtw.py `accelerated_dtw(x, y, 'euclidean', warp=1)`: the exact dynamic time warping, ties to the first of
              (diagonal, i-1, j-1) as `_traceback`'s argmin takes them.
    mel_mcd   `get_metrics_mels`.  use_dtw: mcd = dist / steps, frames = steps.  Otherwise the shorter input is zero-filled:
              mcd = sum ||.|| / max(len), frames = max(len).  penalty = 2 - (len_1 + len_2) / frames in both.
    wav_mcd   melspec.LogMel(hparams, "librosa") on both waveforms, then mel_mcd.

One thing is NOT what a run of the reference's file gives:
  * The reference calls `fastdtw` (radius 1), an APPROXIMATION of DTW (and not a dependency here).  This module computes the exact DTW that
    the reference's own utils/metrics/dtw.py defines, so its `dist` is <= fastdtw's, and the two are equal whenever fastdtw finds the optimum.

eval/mcd.py's wav-level variant -- the MCD column eval/get_metrics.py prints -- is the third part of this file (csrc/wav_mcd.hip):
`htk_mfcc`, `wav_mcd_htk`, `mcd_mean`, and `eval_wav_pairs` for the MCD and STOI means of a batch of waveform pairs in one call.

Mels are [B, T, M], the package's layout; the reference's single-pair (k, n) = [M, T] layout is one `transpose` away.  Everything is a
kernel of libset_amd.so: CPU tensors are refused, there is no eager fallback.  The only host work is the DCT table (float64, once per
(K, M) and device) and the check of lengths that arrive as host values.
"""
import numpy as np
import torch

from . import ops

K_MAX, M_MAX = 64, 96
_TABLES = {}  # (K, M, device) -> the DCT table on that device


def dct_table(n_mfcc, n_mels):
    """float32 [K, M]: cos(pi k (2n+1) / (2M)) for k = 1..K, each rounded once from float64; the angle is reduced exactly in integers,
    (k (2n+1)) mod 4M, as melspec.dft_table does."""
    k = np.arange(1, n_mfcc + 1, dtype=np.int64)[:, None]
    n = np.arange(n_mels, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((k * (2 * n + 1)) % (4 * n_mels)).astype(np.float64) / (4 * n_mels)
    return np.cos(ang).astype(np.float32)


def _table(K, M, device):
    key = (K, M, device)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(dct_table(K, M)).to(device)
    return _TABLES[key]


def _lengths(lengths, B, T, device, name, lo=1):
    """int64 [B] on `device`, or None.  Host values (list, array, CPU tensor) are checked against [lo, T] here; a device tensor is passed
    through without a host sync, and the kernels read each value clamped into that range."""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int64 or lengths.shape != (B,):
            raise ValueError("%s must be int64 [%d], got %s %s" % (name, B, lengths.dtype, tuple(lengths.shape)))
        return lengths.contiguous()
    host = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths).astype(np.int64).reshape(-1)
    if host.shape[0] != B or host.min() < lo or host.max() > T:
        raise ValueError("%s must be %d values in [%d, %d], got %s" % (name, B, lo, T, host.tolist()))
    return torch.from_numpy(host).to(device)


def mfcc(mel, lengths=None, n_mfcc=39, take_log=False):
    """mel [B, T, M] (or [T, M]) -> MFCC 1..n_mfcc [B, T, n_mfcc]; x = mel, or log10(mel) with take_log.  Rows t >= lengths[b] are +0.0.
    n_mfcc <= 64, M <= 96."""
    ops._f(mel, "mel")
    single = mel.dim() == 2
    if single:
        mel = mel[None]
    if mel.dim() != 3:
        raise ValueError("mel must be [B, T, M] or [T, M], got %s" % (tuple(mel.shape),))
    B, T, M = mel.shape
    n_mfcc = int(n_mfcc)
    if not 1 <= n_mfcc <= K_MAX or not 1 <= M <= M_MAX:
        raise ValueError("mfcc is built for 1 <= n_mfcc <= %d and n_mels <= %d, got n_mfcc = %d, n_mels = %d" % (K_MAX, M_MAX, n_mfcc, M))
    out = ops.mfcc(mel, _table(n_mfcc, M, mel.device), _lengths(lengths, B, T, mel.device, "lengths", lo=0), take_log)
    return out[0] if single else out


def dtw(x, y, len_x=None, len_y=None, return_path=False, *, warp=1, w=float("inf"), s=1.0):
    """Exact DTW of x [B, Tx, K] and y [B, Ty, K] (or [Tx, K] and [Ty, K]: one pair) under the euclidean cost ->
    (dist [B] fp32, steps [B] int32), with return_path also (path [B, Tx+Ty-1, 2] int32, count [B] int32): row b's path is
    path[b, :count[b]], from (0, 0) to (len_x-1, len_y-1); entries beyond are zero.  `steps` (= count) is the path's length, carried forward
    with D, so no traceback runs unless the path is asked for.  Only warp=1, w=inf, s=1.0 are built.  K <= 64, Ty <= 8192."""
    if warp != 1 or w != float("inf") or s != 1.0:
        raise NotImplementedError("dtw is built for warp=1, w=inf, s=1.0 only, got warp=%r, w=%r, s=%r" % (warp, w, s))
    ops._f(x, "x"), ops._f(y, "y")
    single = x.dim() == 2 and y.dim() == 2
    if single:
        x, y = x[None], y[None]
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("x and y must be [B, Tx, K] and [B, Ty, K] (or [Tx, K] and [Ty, K]), got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if x.shape[2] != y.shape[2]:
        raise ValueError("the number of coefficients per frame has to be the same for both inputs, got %d and %d" % (x.shape[2], y.shape[2]))
    B, Tx, K = x.shape
    Ty = y.shape[1]
    if K > K_MAX:
        raise ValueError("dtw is built for K <= %d, got %d" % (K_MAX, K))
    len_x, len_y = _lengths(len_x, B, Tx, x.device, "len_x"), _lengths(len_y, B, Ty, x.device, "len_y")
    if not return_path:
        dist, steps = ops.dtw(x, y, len_x, len_y)
        return (dist[0], steps[0]) if single else (dist, steps)
    dir_ = torch.empty(B, Tx, Ty, dtype=torch.uint8, device=x.device)
    dist, steps = ops.dtw(x, y, len_x, len_y, dir=dir_)
    path = ops.dtw_path(dir_, steps, len_x, len_y, path=torch.zeros(B, Tx + Ty - 1, 2, dtype=torch.int32, device=x.device))
    return (dist[0], steps[0], path[0], steps[0]) if single else (dist, steps, path, steps)


def mel_mcd(mel_1, mel_2, len_1=None, len_2=None, *, n_mfcc=39, take_log=False, use_dtw=False):
    """`get_metrics_mels` for a batch: mel_1 [B, T1, M], mel_2 [B, T2, M] (or one pair [T1, M], [T2, M]; the reference's (k, n) arrays are
    `.T` of these) with frame counts len_1 / len_2 -> (mcd [B] fp32, penalty [B] fp32, frames [B] int64), all on the device; nothing is
    synchronised or copied to the host.  take_log=False when log10 has already been applied, as for the mels of this package."""
    ops._f(mel_1, "mel_1"), ops._f(mel_2, "mel_2")
    single = mel_1.dim() == 2 and mel_2.dim() == 2
    if single:
        mel_1, mel_2 = mel_1[None], mel_2[None]
    if mel_1.dim() != 3 or mel_2.dim() != 3 or mel_1.shape[0] != mel_2.shape[0]:
        raise ValueError("mel_1 and mel_2 must be [B, T1, M] and [B, T2, M], got %s and %s" % (tuple(mel_1.shape), tuple(mel_2.shape)))
    if mel_1.shape[2] != mel_2.shape[2]:
        raise ValueError("the number of mel bands has to be equal, got %d and %d" % (mel_1.shape[2], mel_2.shape[2]))
    B, T1, _ = mel_1.shape
    T2 = mel_2.shape[1]
    len_1, len_2 = _lengths(len_1, B, T1, mel_1.device, "len_1"), _lengths(len_2, B, T2, mel_1.device, "len_2")
    c1, c2 = mfcc(mel_1, len_1, n_mfcc, take_log), mfcc(mel_2, len_2, n_mfcc, take_log)
    if use_dtw:
        num, steps = ops.dtw(c1, c2, len_1, len_2)
    else:
        num, steps = ops.zero_fill_dist(c1, c2, len_1, len_2), None
    out = ops.mcd_finish(num, steps, len_1, len_2, T1, T2)
    return tuple(o[0] for o in out) if single else out


def wav_mcd(wav_1, wav_2, hparams, len_1=None, len_2=None, **kw):
    """melspec.LogMel(hparams, "librosa") on both waveforms ([B, N] or [N]; len_1 / len_2 in samples), then mel_mcd(**kw)."""
    from .melspec import LogMel
    fe = LogMel(hparams, "librosa")
    mel_1, fr_1 = (fe(wav_1), None) if len_1 is None else fe(wav_1, len_1)
    mel_2, fr_2 = (fe(wav_2), None) if len_2 is None else fe(wav_2, len_2)
    return mel_mcd(mel_1, mel_2, fr_1, fr_2, **kw)


# ---- short-time objective intelligibility (eval/stoi.py `stoi`, non-extended) --------------------------------------------------------------
# Four launches (include/set_amd.h, the STOI block): frame energies and the list of frames within 40 dB of the loudest; the overlap-add of
# the kept frames of both signals; third-octave band envelopes (the log-mel kernel's DFT GEMM with a power epilogue and a 0/1 band matrix);
# the clipped, normalised correlation of every 30-frame segment.  FS = 22050 with no resampling; `extended=True` is not built (its
# EPS * randn terms are not reproducible); utils/eval/stoi.py's NegSTOILoss is another quantity and is not built either.
STOI_SR, STOI_NFFT, STOI_BANDS, STOI_MIN_FREQ = 22050, 1024, 15, 150
_STOI_IMAGES = {}  # sr -> ops.CacheSlot of (window, packed DFT table, packed band matrix, nbins) on the device they were last used on


def third_octave_bands(sr=STOI_SR, n_fft=STOI_NFFT, num_bands=STOI_BANDS, min_freq=STOI_MIN_FREQ):
    """(obm float64 [num_bands, n_fft/2 + 1] of 0/1, edges int [num_bands, 2]): band k has the centre min_freq 2^(k/3) and covers the bins
    [lo_k, hi_k), lo_k / hi_k = the bin whose frequency f_j = j sr / n_fft is nearest (first of equals) to min_freq 2^((2k -/+ 1)/6)
    (eval/utils.py `thirdoct`, restated from the definition in float64)."""
    f = np.linspace(0, sr, n_fft + 1)[:n_fft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    lo_hz, hi_hz = min_freq * np.power(2.0, (2 * k - 1) / 6), min_freq * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((num_bands, f.shape[0]), dtype=np.float64)
    edges = np.zeros((num_bands, 2), dtype=np.int64)
    for i in range(num_bands):
        edges[i] = int(np.argmin(np.square(f - lo_hz[i]))), int(np.argmin(np.square(f - hi_hz[i])))
        obm[i, edges[i, 0]:edges[i, 1]] = 1.0
    return obm, edges


def stoi_window():
    """The symmetric Hann window np.hanning(1026)[1:-1] (matlab's hanning(1024)): float64."""
    return np.hanning(STOI_NFFT + 2)[1:-1]


def _stoi_images(sr, device):
    from . import melspec

    def build(_old):
        obm, edges = third_octave_bands(sr)
        nbins = int(edges[:, 1].max())  # bins [0, nbins): whole 32-bin chunks from bin_lo = 0
        if not obm.any():
            raise ValueError("stoi: no third-octave band lies below sr / 2 = %g Hz" % (sr / 2.0))
        table = melspec.pack_dft_table(melspec.dft_table(STOI_NFFT, STOI_NFFT, 0, nbins, window=stoi_window()))
        basis = melspec.pack_mel_basis(obm.astype(np.float32), 0, nbins)
        win = stoi_window().astype(np.float32)
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (win, table, basis)) + (nbins,)
    return _STOI_IMAGES.setdefault(int(sr), ops.CacheSlot()).get((device,), build)


def stoi(ref, deg, lengths=None, *, sr=STOI_SR, extended=False):
    """eval/stoi.py `stoi(x, y, 22050, extended=False)` for a batch: ref, deg [B, N] (or [N]) fp32 on the GPU, `lengths` samples per pair ->
    (d [B] fp32, valid [B] bool) on the device; nothing is synchronised or copied to the host.  A pair the reference returns None for
    (fewer than 30 envelope frames after the silent frames are removed) has valid = False and d = NaN.  `sr` only selects the band matrix:
    nothing is resampled."""
    if extended:
        raise NotImplementedError("stoi: extended=True is not built (its EPS * randn terms are not reproducible)")
    ops._f(ref, "ref"), ops._f(deg, "deg")
    single = ref.dim() == 1
    if single:
        ref, deg = ref[None], deg[None] if deg.dim() == 1 else deg
    if ref.dim() != 2 or ref.shape != deg.shape or ref.device != deg.device:
        raise ValueError("ref and deg must both be [B, N] (or [N]) on one device, got %s and %s" % (tuple(ref.shape), tuple(deg.shape)))
    B, N = ref.shape
    if N <= STOI_NFFT:
        raise ValueError("stoi needs more than %d samples, got %d" % (STOI_NFFT, N))
    lengths = _lengths(lengths, B, N, ref.device, "lengths", lo=0)
    win, table, basis, nbins = _stoi_images(sr, ref.device)
    kept, K, _ = ops.stoi_select(ref, win, lengths)
    sil, sil_len = ops.stoi_compact(ref, deg, win, kept, K)
    tob = ops.stoi_bands(sil, table, basis, sil_len, n_bands=STOI_BANDS, bin_lo=0, nbins=nbins)
    d, valid = ops.stoi_score(tob, sil_len[:B])
    return (d[0], valid[0]) if single else (d, valid)


def wav_stoi(wav_ref, wav_gen, len_ref=None, len_gen=None):
    """eval/stoi.py `cal_stoi` for a batch of waveform pairs ([B, N1] and [B, N2], or [N1] and [N2]; len_* in samples): each pair is cut
    to the shorter of its two lengths, on the device, then `stoi`.  The reference's / 32768.1 is not applied: STOI is scale-invariant."""
    ops._f(wav_ref, "wav_ref"), ops._f(wav_gen, "wav_gen")
    single = wav_ref.dim() == 1 and wav_gen.dim() == 1
    if single:
        wav_ref, wav_gen = wav_ref[None], wav_gen[None]
    if wav_ref.dim() != 2 or wav_gen.dim() != 2 or wav_ref.shape[0] != wav_gen.shape[0]:
        raise ValueError("wav_ref and wav_gen must be [B, N1] and [B, N2], got %s and %s" % (tuple(wav_ref.shape), tuple(wav_gen.shape)))
    B, N = wav_ref.shape[0], min(wav_ref.shape[1], wav_gen.shape[1])
    len_ref = _lengths(len_ref, B, wav_ref.shape[1], wav_ref.device, "len_ref", lo=0)
    len_gen = _lengths(len_gen, B, wav_gen.shape[1], wav_ref.device, "len_gen", lo=0)
    lengths = None
    if len_ref is not None or len_gen is not None:
        full = torch.full((B,), N, dtype=torch.int64, device=wav_ref.device)
        lengths = torch.minimum(full if len_ref is None else len_ref, full if len_gen is None else len_gen).clamp_(max=N)
    d, valid = stoi(wav_ref[:, :N].contiguous(), wav_gen[:, :N].contiguous(), lengths)
    return (d[0], valid[0]) if single else (d, valid)


def stoi_mean(d, valid):
    """The mean of d over the valid pairs (eval/stoi.py `cal_stoi_with_waves_batch`), a 0-dim tensor on the device; NaN when none is."""
    return torch.where(valid, d, torch.zeros_like(d)).sum() / valid.sum()


# ---- wav-level mel-cepstral distortion (eval/mcd.py `cal_mcd`, the MCD of eval/get_metrics.py) ----------------------------------------------
# librosa.feature.mfcc(y, sr=22050, n_fft=1024, win_length=1024, hop_length=256, n_mels=80, fmin=55, fmax=7600, n_mfcc=34, htk=True) under
# the reference's librosa 0.8.0, restated: reflection padding of 512, periodic Hann, |STFT|^2, the HTK-scale area-normalised filterbank,
# 10 log10(max(1e-10, S)), the clamp at 80 dB under the utterance's own maximum, the orthonormal DCT-II with c0.  Three launches per
# signal (include/set_amd.h, the wav-level block): dB mel, the peak, the clamped DCT; then one for the distance, or set_dtw and
# set_mcd_finish.  Built for these constants: the kernel body is the log-mel's (n_fft 1024, hop 256, n_mels <= 96).
HTK_SR, HTK_NFFT, HTK_HOP, HTK_MELS, HTK_FMIN, HTK_FMAX, HTK_MFCC, HTK_TOP_DB = 22050, 1024, 256, 80, 55, 7600, 34, 80.0
HTK_PAD = HTK_NFFT // 2
_HTK_IMAGES = ops.CacheSlot()  # (packed DFT table, packed filterbank, bin_lo, nbins, n_mels) of the restated filterbank on the device last used
_ORTHO_TABLES = {}  # (K, M, device) -> the orthonormal DCT table on that device


def dct_ortho_table(n_mfcc, n_mels):
    """float32 [K, M]: s_k cos(pi k (2n+1) / (2M)) for k = 0..K-1, s_0 = 1/sqrt(M), s_k = sqrt(2/M) -- rows of scipy.fft.dct(type=2,
    norm='ortho') -- each rounded once from float64; the angle is reduced exactly in integers as `dct_table` does."""
    k = np.arange(n_mfcc, dtype=np.int64)[:, None]
    n = np.arange(n_mels, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((k * (2 * n + 1)) % (4 * n_mels)).astype(np.float64) / (4 * n_mels)
    scale = np.where(k == 0, np.sqrt(1.0 / n_mels), np.sqrt(2.0 / n_mels))
    return (scale * np.cos(ang)).astype(np.float32)


def _htk_images(device, mel_basis=None):
    from . import melspec

    def build(_old):
        b = melspec.htk_mel_basis(HTK_SR, HTK_NFFT, HTK_MELS, HTK_FMIN, HTK_FMAX) if mel_basis is None else mel_basis
        b = (b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)).astype(np.float32)
        if b.ndim != 2 or b.shape[1] != HTK_NFFT // 2 + 1 or not 1 <= b.shape[0] <= M_MAX:
            raise ValueError("mel_basis must be [n_mels <= %d, %d], got %s" % (M_MAX, HTK_NFFT // 2 + 1, tuple(b.shape)))
        lo, hi = melspec.bin_range(b)
        table = melspec.pack_dft_table(melspec.dft_table(HTK_NFFT, HTK_NFFT, lo, hi - lo))
        basis = melspec.pack_mel_basis(b, lo, hi - lo)
        return torch.from_numpy(table).to(device), torch.from_numpy(basis).to(device), lo, hi - lo, b.shape[0]
    return _HTK_IMAGES.get((device,), build) if mel_basis is None else build(None)


def htk_frames(n_samples):
    """Frames of a waveform of n_samples under center=True: 1 + N // 256; 0 when reflection is impossible (N <= 512)."""
    return 1 + int(n_samples) // HTK_HOP if n_samples > HTK_PAD else 0


def _sample_lengths(lengths, B, N, device, name):
    """(samples int64 [B] on the device or None, frames int64 [B] on the device or None, frames as host ints or None).  Host values are
    checked here: a row of <= 512 samples cannot be reflected and is refused.  A device tensor passes without a host sync; the kernels
    read it clamped into [0, N], and such a row has no frames and is invalid."""
    if lengths is None:
        return None, None, [htk_frames(N)] * B
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int64 or lengths.shape != (B,):
            raise ValueError("%s must be int64 [%d], got %s %s" % (name, B, lengths.dtype, tuple(lengths.shape)))
        lengths = lengths.contiguous()
        n = lengths.clamp(0, N)
        return lengths, torch.where(n > HTK_PAD, 1 + n // HTK_HOP, torch.zeros_like(n)), None
    host = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths).astype(np.int64).reshape(-1)
    if host.shape[0] != B or host.min() <= HTK_PAD or host.max() > N:
        raise ValueError("%s must be %d values in (%d, %d] (reflection padding of %d needs more samples than that), got %s"
                         % (name, B, HTK_PAD, N, HTK_PAD, host.tolist()))
    frames = [htk_frames(n) for n in host]
    return torch.from_numpy(host).to(device), torch.tensor(frames, dtype=torch.int64, device=device), frames


def _htk_mfcc(wav, lengths, n_mfcc, top_db, mel_basis, name):
    """wav [B, N] -> (c [B, T, n_mfcc], frames on the device or None, frames on the host or None)."""
    B, N = wav.shape
    if N <= HTK_PAD:
        raise ValueError("%s: reflection padding of %d needs more than %d samples, got %d" % (name, HTK_PAD, HTK_PAD, N))
    n_mfcc = int(n_mfcc)
    samples, frames, host = _sample_lengths(lengths, B, N, wav.device, name)
    table, basis, lo, nbins, n_mels = _htk_images(wav.device, mel_basis)
    if not 1 <= n_mfcc <= min(K_MAX, n_mels):
        raise ValueError("htk_mfcc is built for 1 <= n_mfcc <= min(%d, n_mels = %d), got %d" % (K_MAX, n_mels, n_mfcc))
    key = (n_mfcc, n_mels, wav.device)
    if key not in _ORTHO_TABLES:
        _ORTHO_TABLES[key] = torch.from_numpy(dct_ortho_table(n_mfcc, n_mels)).to(wav.device)
    db = ops.db_mel(wav, table, basis, samples, n_mels=n_mels, bin_lo=lo, nbins=nbins)
    c = ops.db_mfcc(db, _ORTHO_TABLES[key], ops.db_peak(db, frames), frames, top_db)
    return c, frames, host


def htk_mfcc(wav, lengths=None, *, n_mfcc=HTK_MFCC, top_db=HTK_TOP_DB, mel_basis=None):
    """librosa.feature.mfcc(htk=True) at the constants of eval/mcd.py for a batch: wav [B, N] (or [N]) fp32 on the GPU -> c [B, T, n_mfcc]
    (or [T, n_mfcc]), T = 1 + N // 256, c0 included; with `lengths` (samples per row) also the frames per row, int64 on the device.  Rows at
    or beyond a row's frame count are +0.0.  The 80 dB clamp hangs under each row's own maximum over its own frames.  `mel_basis` replaces
    the restated filterbank (float32 [n_mels <= 96, 513], e.g. librosa's own array).  The filterbank is restated from its definition
    (melspec.htk_mel_basis); librosa is not a dependency."""
    ops._f(wav, "wav")
    single = wav.dim() == 1
    if single:
        wav = wav[None]
    if wav.dim() != 2:
        raise ValueError("wav must be [B, N] or [N], got %s" % (tuple(wav.shape),))
    c, frames, _ = _htk_mfcc(wav, lengths, n_mfcc, top_db, mel_basis, "lengths")
    if single:
        c = c[0]
    return c if lengths is None else (c, frames)


def wav_mcd_htk(wav_ref, wav_est, len_ref=None, len_est=None, *, use_dtw=False):
    """eval/mcd.py `cal_mcd` for a batch of waveform pairs: wav_ref [B, N1], wav_est [B, N2] (or one pair [N1], [N2]; len_* in samples) ->
    (mcd [B] fp32, valid [B] bool) on the device; nothing is synchronised or copied to the host.

    use_dtw=False (what `cal_mcd_with_wave_batch` runs), term by term: on the [34, T] arrays diff2sum = sum over axis 1 -- over the
    FRAMES, one value per coefficient -- and mcd = mean_k(10 / ln 10 sqrt(2 diff2sum_k)) / T_ref.  It needs equal frame counts (the
    reference's subtraction would raise): when both lengths are host values an unequal pair raises here; when one lives on the device the
    pair has valid = False and mcd = NaN, as has a pair with a row of <= 512 samples.

    use_dtw=True is NOT what the reference's file runs: that hands the [34, T] arrays to fastdtw as they are, aligning coefficient indices
    with frames as the feature axis, and fails for unequal T.  Built here is the evident intent: the exact DTW over frames ([T, 34]
    sequences, `dtw`) and mcd = dist / steps, the mean distance of the aligned frames, as the branch's last lines compute."""
    ops._f(wav_ref, "wav_ref"), ops._f(wav_est, "wav_est")
    single = wav_ref.dim() == 1 and wav_est.dim() == 1
    if single:
        wav_ref, wav_est = wav_ref[None], wav_est[None]
    if wav_ref.dim() != 2 or wav_est.dim() != 2 or wav_ref.shape[0] != wav_est.shape[0] or wav_ref.device != wav_est.device:
        raise ValueError("wav_ref and wav_est must be [B, N1] and [B, N2] (or [N1] and [N2]) on one device, got %s and %s"
                         % (tuple(wav_ref.shape), tuple(wav_est.shape)))
    c1, f1, h1 = _htk_mfcc(wav_ref, len_ref, HTK_MFCC, HTK_TOP_DB, None, "len_ref")
    c2, f2, h2 = _htk_mfcc(wav_est, len_est, HTK_MFCC, HTK_TOP_DB, None, "len_est")
    if not use_dtw:
        if h1 is not None and h2 is not None and h1 != h2:
            raise ValueError("wav_mcd_htk(use_dtw=False) needs equal frame counts in every pair, got %s and %s" % (h1, h2))
        mcd, valid = ops.coef_rms_dist(c1, c2, f1, f2)
    else:
        dist, steps = ops.dtw(c1, c2, f1, f2)
        mcd = ops.mcd_finish(dist, steps, f1, f2, c1.shape[1], c2.shape[1])[0]
        valid = torch.ones_like(steps, dtype=torch.bool)
        for f in (f1, f2):
            if f is not None:
                valid &= f > 0
        mcd = torch.where(valid, mcd, torch.full_like(mcd, float("nan")))
    return (mcd[0], valid[0]) if single else (mcd, valid)


def mcd_mean(mcd, valid):
    """The mean of mcd over the valid pairs (eval/mcd.py `cal_mcd_with_wave_batch`), a 0-dim tensor on the device; NaN when none is."""
    return torch.where(valid, mcd, torch.zeros_like(mcd)).sum() / valid.sum()


def eval_wav_pairs(wav_ref, wav_est, len_ref=None, len_est=None):
    """The two means eval/get_metrics.py prints that are built here, for a batch of (ground truth, prediction) waveform pairs:
    {"mcd": mcd_mean(wav_mcd_htk), "stoi": stoi_mean(wav_stoi)}, 0-dim tensors on the device.  PESQ is a third-party C library and is not
    built."""
    return {"mcd": mcd_mean(*wav_mcd_htk(wav_ref, wav_est, len_ref, len_est)),
            "stoi": stoi_mean(*wav_stoi(wav_ref, wav_est, len_ref, len_est))}
