"""float64 models of the log-mel front end, shared by test_melspec_reference.py (CPU) and test_gpu_melspec.py.

Model A follows the reference line by line (utils/audio/__init__.py:64-75 and modules/vocoder/hifigan/mel_utils.py:59-76): torch.stft with
center=False on the explicitly padded signal, magnitude, filterbank product, clamp, log.  Model B is the kernel's formulation: frames
gathered by index from the padded signal, the float32 DFT table and filterbank of set_amd.melspec as matrices, all arithmetic float64.
"""
import math

import numpy as np
import torch

N_FFT, HOP, SR = 1024, 256, 22050
FLOOR = {"librosa": float(np.float32(1e-6)), "hifigan": float(np.float32(1e-5))}
MAG_EPS = {"librosa": 0.0, "hifigan": float(np.float32(1e-9))}
LOG_SCALE = {"librosa": 1.0 / math.log(10.0), "hifigan": 1.0}


def signal(n, amp, seed=0, lead=6 * HOP):
    """Two sines (220 Hz, and 3300 Hz at 0.3x) plus white noise at 5 % of the amplitude; `lead` leading samples silent.  float32 [n]."""
    t = np.arange(n, dtype=np.float64) / SR
    rng = np.random.default_rng(seed)
    x = amp * (np.sin(2 * np.pi * 220.0 * t) + 0.3 * np.sin(2 * np.pi * 3300.0 * t)) + 0.05 * amp * rng.standard_normal(n)
    x[:lead] = 0.0
    return x.astype(np.float32)


def padded(wav, flavour):
    """The padded signal the STFT runs over, float64, by torch's own pad (Model A's and the tests' reference for the pad rule)."""
    y = torch.from_numpy(np.asarray(wav, dtype=np.float32)).double()
    if flavour == "hifigan":
        p = (N_FFT - HOP) // 2
        return torch.nn.functional.pad(y.clamp(-1.0, 1.0)[None, None], (p, p), mode="reflect")[0, 0]
    return torch.nn.functional.pad(y, (N_FFT // 2, N_FFT // 2))


def model_a(wav, flavour, basis, win_length=N_FFT):
    """[T, n_mels] float64 log-mel of one float32 waveform."""
    y = padded(wav, flavour)
    spec = torch.stft(y, N_FFT, hop_length=HOP, win_length=win_length, window=torch.hann_window(win_length, dtype=torch.float64),
                      center=False, normalized=False, onesided=True, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + MAG_EPS[flavour]) if flavour == "hifigan" else spec.abs()
    mel = torch.from_numpy(np.asarray(basis, dtype=np.float32)).double() @ mag
    return (LOG_SCALE[flavour] * torch.log(torch.clamp(mel, min=FLOOR[flavour]))).T.numpy()


def model_b(wav, flavour, basis, table, bin_lo, win_length=N_FFT, return_parts=False):
    """The matrix form: frames[t][n] = y[t hop + n] by the kernel's own index rule (melspec.reflect_index / zero pad), re / im = frames
    times the float32 table, mel = basis[:, bin_lo : bin_lo + nbins] times the magnitude.  float64 arithmetic on the float32 constants."""
    from set_amd import melspec as M
    x = np.asarray(wav, dtype=np.float32).astype(np.float64)
    if flavour == "hifigan":
        x = np.clip(x, -1.0, 1.0)
    n, pad = x.shape[0], M.flavour_pad(flavour, N_FFT, HOP)
    T = M.n_frames(n, flavour, N_FFT, HOP)
    y = np.zeros(n + 2 * pad)
    for i in range(n + 2 * pad):
        if flavour == "hifigan":
            y[i] = x[M.reflect_index(i, n, pad)]
        elif 0 <= i - pad < n:
            y[i] = x[i - pad]
    frames = np.stack([y[t * HOP:t * HOP + N_FFT] for t in range(T)])       # [T, n_fft]
    tab = np.asarray(table, dtype=np.float32).astype(np.float64)
    re, im = frames @ tab[0].T, frames @ tab[1].T                            # [T, nbins]
    mag = np.sqrt(re ** 2 + im ** 2 + MAG_EPS[flavour])
    b = np.asarray(basis, dtype=np.float32).astype(np.float64)[:, bin_lo:bin_lo + tab.shape[1]]
    mel = mag @ b.T
    out = LOG_SCALE[flavour] * np.log(np.maximum(mel, FLOOR[flavour]))
    return (out, mel, frames) if return_parts else out


def with_nyquist_weight(basis):
    """A caller's filterbank with weight on the last bin (the restated Slaney triangles end exactly AT Nyquist, where their weight is
    0): 513 bins, so the kernel's last chunk holds a single live bin."""
    b = np.array(basis, dtype=np.float32, copy=True)
    b[-1, -1] = b[-1, -2]
    return b
