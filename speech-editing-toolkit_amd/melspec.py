"""Log-mel front end on the GPU: waveform -> the mel the models consume (csrc/melspec.hip, `set_log_mel`).

Two flavours of one kernel, after the two places the reference computes a mel:

    "librosa"   utils/audio/__init__.py:36-82 `librosa_wav2spec` (what inference/tts/spec_denoiser.py:258 puts into item['mel']):
                zero pad of n_fft/2 each side, |STFT|, log10(max(1e-6, mel))
    "hifigan"   modules/vocoder/hifigan/mel_utils.py:45-80 `mel_spectrogram`: input clamped to [-1, 1], reflect pad of (n_fft - hop)/2,
                sqrt(re^2 + im^2 + 1e-9), ln(max(1e-5, mel))

Everything here is host-side preparation in numpy float64 (filterbank, DFT table, their kernel images), done once per configuration and
held on the device; the arithmetic on the waveform is the kernel's.  librosa is not a dependency: `slaney_mel_basis` restates its default
filterbank from the definition, and every entry takes `mel_basis=` for a caller who holds librosa's own matrix.
"""
import math

import numpy as np
import torch

from . import ops

CHUNK = 32  # bins per kernel chunk: the bin range is the filterbank's support widened outward to whole chunks

FLAVOURS = {
    "librosa": dict(reflect=0, clamp_input=0, mag_eps=0.0, floor=1e-6, log_scale=1.0 / math.log(10.0)),
    "hifigan": dict(reflect=1, clamp_input=1, mag_eps=1e-9, floor=1e-5, log_scale=1.0),
}


def flavour_pad(flavour, n_fft, hop):
    """Samples of padding on each side: n_fft/2 (librosa.stft, center=True) or (n_fft - hop)/2 (mel_utils.py:66)."""
    return n_fft // 2 if flavour == "librosa" else (n_fft - hop) // 2


def n_frames(n_samples, flavour, n_fft, hop):
    """Frames of a waveform of n_samples: 1 + N // hop (librosa) or 1 + (N + 2 pad - n_fft) // hop (hifigan); 0 when it is too short."""
    n = n_samples + 2 * flavour_pad(flavour, n_fft, hop) - n_fft
    return 1 + n // hop if n >= 0 else 0


def reflect_index(i, length, pad):
    """Index into a row of `length` samples of sample i of its reflect-padded form (torch / numpy 'reflect': mirrored about sample 0
    and about sample length - 1, the edge samples not repeated).  Needs length > pad."""
    j = i - pad
    if j < 0:
        return -j
    if j >= length:
        return 2 * (length - 1) - j
    return j


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    logstep = math.log(6.4) / 27.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax):
    """The Slaney-scale (linear below 1 kHz, logarithmic above), area-normalised triangular filterbank: librosa.filters.mel's default
    (htk=False, norm='slaney').  float64 arithmetic, float32 [n_mels, n_fft/2 + 1] result.  fmin = -1 -> 0, fmax = -1 -> sr/2
    (utils/audio/__init__.py:69-70)."""
    fmin = 0.0 if fmin == -1 else float(fmin)
    fmax = sr / 2.0 if fmax == -1 else float(fmax)
    return _triangles(sr, n_fft, _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2)))


def htk_mel_basis(sr, n_fft, n_mels, fmin, fmax):
    """The HTK-scale filterbank, mel = 2595 log10(1 + f / 700): librosa.filters.mel(htk=True), whose default area normalisation
    2 / (f_{m+2} - f_m) still applies.  Triangles between n_mels + 2 points equally spaced in mel from fmin to fmax.  float64 arithmetic,
    float32 [n_mels, n_fft/2 + 1] result."""
    mel = 2595.0 * np.log10(1.0 + np.array([float(fmin), float(fmax)]) / 700.0)
    return _triangles(sr, n_fft, 700.0 * (np.power(10.0, np.linspace(mel[0], mel[1], n_mels + 2) / 2595.0) - 1.0))


def _triangles(sr, n_fft, edges):
    """Area-normalised triangles between consecutive triples of `edges` (Hz, float64 [n_mels + 2]) on the n_fft/2 + 1 bin frequencies."""
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)) + 0.0  # (+ 0.0: no negative zeros)
    w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w.astype(np.float32)


def bin_range(mel_basis):
    """[bin_lo, bin_hi): the columns the filterbank has weight on, widened outward to whole 32-bin chunks (and cut at the last bin)."""
    b = np.asarray(mel_basis)
    cols = np.nonzero(np.any(b != 0, axis=0))[0]
    if cols.size == 0:
        return 0, min(CHUNK, b.shape[1])
    lo, hi = int(cols[0]), int(cols[-1]) + 1
    return lo // CHUNK * CHUNK, min((hi + CHUNK - 1) // CHUNK * CHUNK, b.shape[1])


def hann_padded(n_fft, win_length):
    """The periodic Hann window of win_length (torch.hann_window, librosa 'hann'), centred and zero-padded to n_fft; float64."""
    if not 0 < win_length <= n_fft:
        raise ValueError("win_length must be in (0, n_fft], got %d" % win_length)
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return w


def dft_table(n_fft, win_length, bin_lo, nbins, window=None):
    """float32 [2, nbins, n_fft]: [0][f][n] = win[n] cos(2 pi (bin_lo + f) n / n_fft), [1][f][n] = -win[n] sin(...), each rounded once
    from float64 (the angle is reduced exactly: (f n) mod n_fft in integers).  win = hann_padded(n_fft, win_length), or `window`
    (float64 [n_fft]) when one is given (metrics.stoi: the symmetric Hann)."""
    win = hann_padded(n_fft, win_length) if window is None else np.asarray(window, dtype=np.float64).reshape(n_fft)
    f = np.arange(bin_lo, bin_lo + nbins, dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((f * n) % n_fft).astype(np.float64) / n_fft
    return np.stack([win[None, :] * np.cos(ang), -win[None, :] * np.sin(ang)]).astype(np.float32)


def pack_dft_table(table):
    """The kernel's image of dft_table's result: rows padded with zeros to whole chunks, ordered [chunk][n / 4][lane][4] with element
    e = table[e & 1][32 chunk + (lane & 31)][4 (n / 4) + 2 (e >> 1) + (lane >> 5)] -- the A fragments of two k-steps of the real and
    the imaginary row block as one 16-byte unit per lane (include/set_amd.h, set_log_mel)."""
    table = np.asarray(table, dtype=np.float32)
    _, nbins, n_fft = table.shape
    nch = (nbins + CHUNK - 1) // CHUNK
    full = np.zeros((2, nch * CHUNK, n_fft), dtype=np.float32)
    full[:, :nbins] = table
    v = full.reshape(2, nch, CHUNK, n_fft // 4, 2, 2)          # part, chunk, i, p, s, h      (n = 4 p + 2 s + h)
    return np.ascontiguousarray(v.transpose(1, 3, 5, 2, 4, 0)).reshape(nch, n_fft // 4, 64, 4)  # chunk, p, (h, i), (s, part)


def unpack_dft_table(image, nbins):
    """Inverse of pack_dft_table: float32 [2, nbins, n_fft]."""
    image = np.asarray(image, dtype=np.float32)
    nch, quarter = image.shape[0], image.shape[1]
    v = image.reshape(nch, quarter, 2, CHUNK, 2, 2).transpose(5, 0, 3, 1, 4, 2)  # part, chunk, i, p, s, h
    return np.ascontiguousarray(v).reshape(2, nch * CHUNK, quarter * 4)[:, :nbins]


def pack_mel_basis(mel_basis, bin_lo, nbins):
    """The kernel's image of the filterbank: [chunk][r][lane][4], element e < 3 = mel_basis[32 e + (lane & 31)][bin_lo + 32 chunk +
    (r & 3) + 8 (r >> 2) + 4 (lane >> 5)], zero outside the matrix and for bins beyond bin_lo + nbins; e = 3 is zero (mel rows beyond 96 have no place in it: the entry refuses
    such a filterbank).  The bin order
    of k-step r is the row order of an MFMA accumulator register, so the magnitude tile is GEMM 2's B operand as it stands."""
    b = np.asarray(mel_basis, dtype=np.float32)
    n_mels = min(b.shape[0], 3 * 32)
    nch = (nbins + CHUNK - 1) // CHUNK
    full = np.zeros((3 * 32, nch * CHUNK), dtype=np.float32)
    full[:n_mels, :nbins] = b[:n_mels, bin_lo:bin_lo + nbins]
    r, h = np.arange(16)[:, None], np.arange(2)[None, :]
    rows = (r & 3) + 8 * (r >> 2) + 4 * h                       # [16, 2]
    g = full.reshape(3, 32, nch, CHUNK)[:, :, :, rows]          # e, i, chunk, r, h
    img = np.zeros((nch, 16, 2, 32, 4), dtype=np.float32)
    img[..., :3] = g.transpose(2, 3, 4, 1, 0)
    return img.reshape(nch, 16, 64, 4)


def pack_mel_basis_t(mel_basis, bin_lo, nbins):
    """The image of the transposed filterbank for the mel loss's backward (include/set_amd.h, set_mel_loss_bwd): [chunk][s][lane] =
    mel_basis[2 s + (lane >> 5)][bin_lo + 32 chunk + (lane & 31)], s = 0..47, zero outside the matrix and beyond bin_lo + nbins -- the A
    operand of g_mag = basis^T g_mel, whose result lands in the register layout of re / im."""
    b = np.asarray(mel_basis, dtype=np.float32)
    n_mels = min(b.shape[0], 3 * 32)
    nch = (nbins + CHUNK - 1) // CHUNK
    full = np.zeros((3 * 32, nch * CHUNK), dtype=np.float32)
    full[:n_mels, :nbins] = b[:n_mels, bin_lo:bin_lo + nbins]
    v = full.reshape(48, 2, nch, CHUNK)                          # s, h, chunk, i
    return np.ascontiguousarray(v.transpose(2, 0, 1, 3)).reshape(nch, 48, 64)


def pack_idft_table(table):
    """The image of dft_table's result for the inverse product of the mel loss's backward (set_mel_loss_bwd): [chunk][wave][q][part][s]
    [lane][2], element e = table[part][32 chunk + 2 s + (lane >> 5)][256 q + 64 wave + 32 e + (lane & 31)], rows beyond nbins zero."""
    table = np.asarray(table, dtype=np.float32)
    _, nbins, n_fft = table.shape
    nch = (nbins + CHUNK - 1) // CHUNK
    full = np.zeros((2, nch * CHUNK, n_fft), dtype=np.float32)
    full[:, :nbins] = table
    v = full.reshape(2, nch, 16, 2, n_fft // 256, 4, 2, 32)     # part, chunk, s, h, q, wave, e, i
    return np.ascontiguousarray(v.transpose(1, 5, 4, 0, 2, 3, 7, 6)).reshape(nch, 4, n_fft // 256, 2, 16, 64, 2)


def pack_stft_table(table, win_length):
    """The image of dft_table's result for the STFT loss (include/set_amd.h, set_stft_magnitude): only the win_length non-zero window
    samples, [chunk][s][lane][2] with element e = table[e][32 chunk + (lane & 31)][left + 2 s + (lane >> 5)], left = (n_fft -
    win_length) / 2, rows beyond nbins zero -- the A fragment of k-step s of the real and the imaginary row block as one 8-byte unit."""
    table = np.asarray(table, dtype=np.float32)
    _, nbins, n_fft = table.shape
    left = (n_fft - win_length) // 2
    nch = (nbins + CHUNK - 1) // CHUNK
    full = np.zeros((2, nch * CHUNK, win_length), dtype=np.float32)
    full[:, :nbins] = table[:, :, left:left + win_length]
    v = full.reshape(2, nch, CHUNK, win_length // 2, 2)                                      # part, chunk, i, s, h
    return np.ascontiguousarray(v.transpose(1, 3, 4, 2, 0)).reshape(nch, win_length // 2, 64, 2)  # chunk, s, (h, i), part


def unpack_stft_table(image, nbins, n_fft):
    """Inverse of pack_stft_table: float32 [2, nbins, n_fft], zero outside the window."""
    image = np.asarray(image, dtype=np.float32)
    nch, half = image.shape[0], image.shape[1]
    v = image.reshape(nch, half, 2, CHUNK, 2).transpose(4, 0, 3, 1, 2)                      # part, chunk, i, s, h
    out = np.zeros((2, nbins, n_fft), dtype=np.float32)
    left = (n_fft - 2 * half) // 2
    out[:, :, left:left + 2 * half] = np.ascontiguousarray(v).reshape(2, nch * CHUNK, 2 * half)[:, :nbins]
    return out


def stft_idft_layout(hop, win_length):
    """(Q, row blocks of a hop, NW): the taps a window spans, the 32-sample row blocks of a hop, and the waves the inverse kernel gives
    a 64-hop tile -- one per row block when a hop has 4 or 8, four (a row block and a column block each) when it has 2."""
    q, rbt = -(-win_length // hop), -(-hop // 32)
    if rbt not in (2, 4, 8):
        raise ValueError("a hop of %d samples is %d row blocks of 32; the inverse kernel takes 2, 4 or 8" % (hop, rbt))
    return q, rbt, (rbt if rbt >= 4 else 4)


def pack_stft_idft_table(table, hop, win_length):
    """The image of dft_table's result for the inverse product of the STFT loss's backward (set_stft_loss_bwd): [chunk][wave][kk][lane]
    with q = kk >> 5, part = (kk >> 4) & 1, s = kk & 15 = table[part][32 chunk + 2 s + (lane >> 5)][left + hop q + c], c = 32 rb +
    (lane & 31), rb = wave (4 or 8 row blocks) or wave >> 1 (2 row blocks); zero where c >= hop, hop q + c >= win_length or the row is
    beyond nbins."""
    table = np.asarray(table, dtype=np.float32)
    _, nbins, n_fft = table.shape
    left = (n_fft - win_length) // 2
    Q, rbt, NW = stft_idft_layout(hop, win_length)
    nch = (nbins + CHUNK - 1) // CHUNK
    full = np.zeros((2, nch * CHUNK, Q, rbt * 32), dtype=np.float32)                        # part, bin, q, c
    for q in range(Q):
        n = min(hop, win_length - hop * q)
        full[:, :nbins, q, :n] = table[:, :, left + hop * q:left + hop * q + n]
    ch, wave, kk, lane = np.ix_(np.arange(nch), np.arange(NW), np.arange(32 * Q), np.arange(64))
    rb = wave if rbt >= 4 else wave >> 1
    return np.ascontiguousarray(full[(kk >> 4) & 1, 32 * ch + 2 * (kk & 15) + (lane >> 5), kk >> 5, 32 * rb + (lane & 31)])


class LogMel:
    """wav [B, N] (or [N]) fp32 on the GPU -> log-mel [B, T, n_mels] (or [T, n_mels]); with `lengths` also the frames per row.

    Reads fft_size, win_size, hop_size, audio_num_mel_bins, audio_sample_rate, fmin, fmax from `hparams`.  `mel_basis` replaces the
    restated Slaney filterbank (float32 [n_mels, fft_size/2 + 1], e.g. librosa's own array).  The kernel covers fft_size 1024,
    hop_size 256, win_size <= fft_size, n_mels <= 96; anything else raises."""

    def __init__(self, hparams, flavour="librosa", mel_basis=None):
        if flavour not in FLAVOURS:
            raise ValueError("flavour must be one of %s, got %r" % (sorted(FLAVOURS), flavour))
        self.flavour = flavour
        self.n_fft = int(hparams.get("fft_size", 1024))
        self.win_length = int(hparams.get("win_size", self.n_fft))
        self.hop = int(hparams.get("hop_size", 256))
        self.n_mels = int(hparams.get("audio_num_mel_bins", 80))
        self.sr = int(hparams.get("audio_sample_rate", 22050))
        self.pad = flavour_pad(flavour, self.n_fft, self.hop)
        if mel_basis is None:
            mel_basis = slaney_mel_basis(self.sr, self.n_fft, self.n_mels, hparams.get("fmin", 80), hparams.get("fmax", -1))
        self.mel_basis = mel_basis
        b = mel_basis.detach().cpu().numpy() if isinstance(mel_basis, torch.Tensor) else np.asarray(mel_basis)
        if b.shape != (self.n_mels, self.n_fft // 2 + 1):
            raise ValueError("mel_basis must be [%d, %d], got %s" % (self.n_mels, self.n_fft // 2 + 1, tuple(b.shape)))
        self._basis = b.astype(np.float32)
        self.bin_lo, self.bin_hi = bin_range(self._basis)
        self._images = ops.CacheSlot()  # (packed DFT table, packed filterbank) on the device they were last used on

    @property
    def nbins(self):
        return self.bin_hi - self.bin_lo

    def frames(self, n_samples):
        return n_frames(int(n_samples), self.flavour, self.n_fft, self.hop)

    def _build_images(self, device):
        table = pack_dft_table(dft_table(self.n_fft, self.win_length, self.bin_lo, self.nbins))
        basis = pack_mel_basis(self._basis, self.bin_lo, self.nbins)
        return torch.from_numpy(table).to(device), torch.from_numpy(basis).to(device)

    def __call__(self, wav, lengths=None):
        ops._f(wav, "wav")
        single = wav.dim() == 1
        if single:
            wav = wav[None, :]
        if wav.dim() != 2:
            raise ValueError("wav must be [B, N] or [N], got %s" % (tuple(wav.shape),))
        B, N = wav.shape
        if self.frames(N) < 1:
            raise ValueError("a waveform of %d samples is shorter than one frame" % N)
        if self.flavour == "hifigan" and N <= self.pad:
            raise ValueError("reflect padding of %d needs more than %d samples, got %d" % (self.pad, self.pad, N))
        len_dev = mel_lengths = None
        if lengths is not None:
            host = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
            host = host.astype(np.int64).reshape(-1)
            if host.shape[0] != B or host.min() < 0 or host.max() > N:
                raise ValueError("lengths must be %d values in [0, %d], got %s" % (B, N, host.tolist()))
            if self.flavour == "hifigan" and host.min() <= self.pad:
                raise ValueError("reflect padding of %d needs more than %d samples in every row, got %s" % (self.pad, self.pad, host.tolist()))
            len_dev = torch.from_numpy(host).to(wav.device)
            mel_lengths = torch.tensor([self.frames(n) for n in host], dtype=torch.int64, device=wav.device)
        table, basis = self._images.get((wav.device,), lambda old: self._build_images(wav.device))
        fl = FLAVOURS[self.flavour]
        mel = ops.log_mel(wav, table, basis, len_dev, n_fft=self.n_fft, hop=self.hop, n_mels=self.n_mels, bin_lo=self.bin_lo,
                          nbins=self.nbins, pad=self.pad, **fl)
        if single:
            mel = mel[0]
        return mel if lengths is None else (mel, mel_lengths)


_HP_KEYS = ("fft_size", "win_size", "hop_size", "audio_num_mel_bins", "audio_sample_rate", "fmin", "fmax")
_CACHE = {}  # configuration -> LogMel, for wav2spec calls without a caller's filterbank


def wav2spec(wav, hparams, **overrides):
    """The dict of the reference's librosa_wav2spec for one waveform (numpy array or tensor, [N]): 'wav' right-padded with zeros and cut
    to T * hop_size samples (librosa_pad_lr), 'mel' [T, n_mels], 'mel_basis'.  'wav' and 'mel' are fp32 tensors on the GPU; 'mel_basis'
    is the array that was passed in, else the restated Slaney filterbank (numpy float32).  `overrides`: flavour=, mel_basis=, or any of
    the hparams keys LogMel reads.  'linear', loud_norm and trim_long_sil are not built."""
    flavour = overrides.pop("flavour", "librosa")
    mel_basis = overrides.pop("mel_basis", None)
    unknown = set(overrides) - set(_HP_KEYS)
    if unknown:
        raise TypeError("wav2spec: unknown overrides %s" % sorted(unknown))
    hp = {k: hparams[k] for k in _HP_KEYS if k in hparams}
    hp.update(overrides)
    if mel_basis is None:
        key = (flavour,) + tuple(hp.get(k) for k in _HP_KEYS)
        fe = _CACHE.get(key)
        if fe is None:
            fe = _CACHE[key] = LogMel(hp, flavour)
    else:
        fe = LogMel(hp, flavour, mel_basis=mel_basis)
    if not isinstance(wav, torch.Tensor):
        if not torch.cuda.is_available():
            raise RuntimeError("wav2spec (set_amd) needs an MI355X: there is no CPU fallback for this path")
        wav = torch.as_tensor(np.asarray(wav), dtype=torch.float32).cuda()
    ops._f(wav, "wav")
    if wav.dim() != 1:
        raise ValueError("wav2spec takes one waveform [N], got %s" % (tuple(wav.shape),))
    mel = fe(wav)
    n_out = mel.shape[0] * fe.hop
    out = torch.zeros(n_out, dtype=torch.float32, device=wav.device)
    n = min(n_out, wav.shape[0])
    out[:n] = wav[:n]
    return {"wav": out, "mel": mel, "mel_basis": fe.mel_basis}
