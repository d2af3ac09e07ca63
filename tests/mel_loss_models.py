"""Models of the HiFi-GAN mel loss and of its waveform gradient, shared by test_mel_loss_reference.py (CPU) and test_gpu_mel_loss.py.

The model is the matrix form the kernels use (csrc/mel_loss.hip): frames gathered from the clamped, reflect-padded row by index, re / im =
frames times the DFT table, mag = sqrt(re^2 + im^2 + 1e-9), mel = mag times the filterbank, L = ln(max(mel, 1e-5)), loss = mean |L_hat -
L_y|; and backwards g_mel = sign(d) [mel_hat >= floor] / mel_hat / count, g_mag = g_mel times the filterbank, g_re = g_mag re / mag,
g_frames = g_re times the table, overlap-add, reflect fold (a scatter-add by the forward's own index map), clamp mask.  Every function
takes the dtype it computes in: float64 is the model, float32 the mirror whose distance from the model sets the GPU tests' bars."""
import functools

import numpy as np
import torch

import set_amd  # noqa: F401
from set_amd import vocoder_losses  # noqa: F401  (the feature these models describe: without it both test files fail here)
from melspec_models import HOP, N_FFT, SR

PAD = (N_FFT - HOP) // 2
FLOOR = float(np.float32(1e-5))
MAG_EPS = float(np.float32(1e-9))
HP = {"fft_size": 1024, "win_size": 1024, "hop_size": 256, "audio_num_mel_bins": 80, "audio_sample_rate": SR, "fmin": 55, "fmax": 7600}
BAR_FACTOR = 4.0  # GPU bar = 4 x the float32 mirror's error: the MFMA tiles split and order the sums otherwise than the mirror (mm below)
UNDECIDED_CAP = 1e-3


def n_frames(n):
    return 1 + (n + 2 * PAD - N_FFT) // HOP


def dft_table64(win_length, bin_lo, nbins):
    """melspec.dft_table before its rounding to float32: float64 [2, nbins, n_fft]."""
    from set_amd import melspec as M
    win = M.hann_padded(N_FFT, win_length)
    f = np.arange(bin_lo, bin_lo + nbins, dtype=np.int64)[:, None]
    n = np.arange(N_FFT, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((f * n) % N_FFT).astype(np.float64) / N_FFT
    return np.stack([win[None, :] * np.cos(ang), -win[None, :] * np.sin(ang)])


class Bank:
    """A filterbank configuration as the kernels see it: float32 basis and table, the bin range, by set_amd.melspec's own functions."""

    def __init__(self, name, mel_basis=None, **over):
        from set_amd import melspec as M
        self.name, self.hp = name, dict(HP, **over)
        self.n_mels, self.win = self.hp["audio_num_mel_bins"], self.hp["win_size"]
        self.mel_basis = mel_basis
        self.basis = np.asarray(mel_basis, dtype=np.float32) if mel_basis is not None else \
            M.slaney_mel_basis(SR, N_FFT, self.n_mels, self.hp["fmin"], self.hp["fmax"])
        self.bin_lo, self.bin_hi = M.bin_range(self.basis)
        self.nbins = self.bin_hi - self.bin_lo
        self.table = M.dft_table(N_FFT, self.win, self.bin_lo, self.nbins)


@functools.lru_cache(maxsize=None)
def bank(name):
    from set_amd import melspec as M
    if name == "mel80":
        return Bank(name)
    if name == "mel96":
        return Bank(name, audio_num_mel_bins=96)
    if name == "win600":
        return Bank(name, win_size=600)
    if name == "narrow20":  # 20 rows from 1 kHz up, with weight on the Nyquist bin: bins 47 .. 512, so bin_lo = 32 and 481 bins: a last
        basis = M.slaney_mel_basis(SR, N_FFT, 20, 1000.0, -1)  # chunk with one live bin, and dead bins 32 .. 46 inside the first
        basis[-1, -1] = basis[-1, -2]
        b = Bank(name, mel_basis=basis, audio_num_mel_bins=20)
        assert b.bin_lo == 32 and b.nbins == 481 and not b.basis[:, 32:47].any(), (b.bin_lo, b.nbins)
        return b
    raise KeyError(name)


BANKS = ("mel80", "mel96", "narrow20", "win600")


def speech_like(n, seed):
    """A sum of decaying harmonics of 140 Hz under a slow envelope plus a little noise: energy in every mel band, peak below 1.  float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / SR
    x = np.zeros(n)
    for k in range(1, 75):
        x += k ** -1.1 * np.sin(2 * np.pi * 140.0 * k * t + rng.uniform(0, 2 * np.pi))
    x *= 0.22 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + 1.0))
    x += 0.003 * rng.standard_normal(n)
    assert np.abs(x).max() < 0.95
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair(B, n, seed=0):
    """(y_hat, y) float32 [B, n]: y speech-like, y_hat = y + 0.05 noise; |y_hat| < 1 (the clamp has its own fixtures)."""
    rng = np.random.default_rng(1000 + seed)
    y = np.stack([speech_like(n, 10 * seed + b) for b in range(B)])
    y_hat = (y.astype(np.float64) + 0.05 * 0.22 * rng.standard_normal((B, n))).astype(np.float32)
    assert np.abs(y_hat).max() < 1.0
    y.setflags(write=False), y_hat.setflags(write=False)
    return y_hat, y


def mm(a, b, dtype):
    """a @ b.  In float64 plainly; in float32 the way one MFMA accumulator sums it: ascending k into a single accumulator, each step a
    fused multiply-add (the float32 product is exact in float64; the sum is rounded to float32).  BLAS's float32 product keeps many
    partial sums per element, which makes it more accurate than any single accumulator and so no mirror of one."""
    if dtype is np.float64:
        return a @ b
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for k in range(a.shape[1]):
        acc = (acc + a64[:, k, None] * b64[None, k, :]).astype(np.float32)
    return acc


def pad_index(n):
    """Index into a row of n samples of each of the n + 2 PAD padded samples (melspec.reflect_index)."""
    from set_amd import melspec as M
    return np.array([M.reflect_index(i, n, PAD) for i in range(n + 2 * PAD)], dtype=np.int64)


def spectrum(wav, bk, dtype, table=None):
    """One row: (re, im [T, nbins], frames [T, n_fft]) in `dtype` from the waveform (float32 fixtures; float64 for finite differences) and
    the float32 (or given) table."""
    x = np.clip(np.asarray(wav), -1.0, 1.0).astype(dtype)
    n = x.shape[0]
    p = x[pad_index(n)]
    T = n_frames(n)
    frames = np.stack([p[t * HOP:t * HOP + N_FFT] for t in range(T)])
    tab = np.asarray(bk.table if table is None else table).astype(dtype)
    return mm(frames, tab[0].T, dtype), mm(frames, tab[1].T, dtype), frames


def linear_mel(wav, bk, dtype, table=None):
    """[B, T, n_mels] linear mel of the rows of wav [B, n]."""
    b = bk.basis[:, bk.bin_lo:bk.bin_hi].astype(dtype)
    out = []
    for row in np.asarray(wav):
        re, im, _ = spectrum(row, bk, dtype, table)
        out.append(mm(np.sqrt(re * re + im * im + dtype(MAG_EPS)), b.T, dtype))
    return np.stack(out)


def log_mel(mel, dtype):
    """ln(max(mel, floor)): evaluated in double and rounded once for float32 (the kernels' rule), plainly in float64."""
    return np.log(np.maximum(mel, dtype(FLOOR)).astype(np.float64)).astype(dtype)


def loss_and_g_mel(mel_hat, mel_y, dtype, sign=None, passed=None):
    """(loss, g_mel, d, passed): d = L_hat - L_y; g_mel = sign(d) [mel_hat >= floor] / mel_hat / count.  `sign` / `passed` override the
    model's own decisions where given (arrays with NaN / -1 meaning "the model's own")."""
    mel_hat, mel_y = np.asarray(mel_hat, dtype=dtype), np.asarray(mel_y, dtype=dtype)
    d = log_mel(mel_hat, dtype) - log_mel(mel_y, dtype)
    s = np.sign(d)
    ok = mel_hat >= dtype(FLOOR)
    if sign is not None:
        s = np.where(np.isnan(sign), s, sign).astype(dtype)
    if passed is not None:
        ok = np.where(passed < 0, ok, passed > 0)
    count = d.size
    g = np.where(ok, s * dtype(dtype(1.0) / dtype(count)) / np.where(ok, mel_hat, 1), 0).astype(dtype)
    loss = dtype(np.abs(d).sum(dtype=dtype) / dtype(count))
    return loss, g, d, ok


def fold(g_p, n):
    """The reflect fold in the kernels' gather form: g[j] = g_p[j + P] + g_p[P - j] (1 <= j <= P) + g_p[P + 2 (n - 1) - j]
    (n - 1 - P <= j <= n - 2), g_p read as 0 beyond its end."""
    g_p = np.concatenate([g_p, np.zeros(max(0, n + 2 * PAD - g_p.shape[0]), dtype=g_p.dtype)])
    j = np.arange(n)
    g = g_p[j + PAD].copy()
    lo = (j >= 1) & (j <= PAD)
    g[lo] += g_p[PAD - j[lo]]
    hi = (j >= n - 1 - PAD) & (j <= n - 2)
    g[hi] += g_p[PAD + 2 * (n - 1) - j[hi]]
    return g


def overlap_add(g_re, g_im, tab, n, dtype):
    """The padded row's gradient [n + 2 PAD] from g_re, g_im [T, nbins]: frames = g_re W_re + g_im W_im, overlap-added.  In float32 the
    way the inverse launch sums it: a padded sample 256 u + c has ONE accumulator, which takes its taps in the order 32-bin chunk, tap q
    (frame u - q), part (re, im), bin -- fused multiply-adds, as in mm."""
    T = g_re.shape[0]
    if dtype is np.float64:
        g_frames = g_re @ tab[0] + g_im @ tab[1]
        g_p = np.zeros(n + 2 * PAD, dtype=dtype)
        for t in range(T):
            g_p[t * HOP:t * HOP + N_FFT] += g_frames[t]
        return g_p
    U = T + N_FFT // HOP - 1
    acc = np.zeros((U, HOP), dtype=np.float32)
    g = [np.zeros((U + 3, g_re.shape[1])), np.zeros((U + 3, g_re.shape[1]))]     # frame t at row t + 3: row u + 3 - q is frame u - q
    g[0][3:3 + T], g[1][3:3 + T] = g_re, g_im
    w = np.asarray(tab, dtype=np.float64)
    for c0 in range(0, g_re.shape[1], 32):
        for q in range(N_FFT // HOP):
            for part in range(2):
                for f in range(c0, min(c0 + 32, g_re.shape[1])):
                    acc = (acc + g[part][3 - q:3 - q + U, f, None] * w[part, f, None, HOP * q:HOP * q + HOP]).astype(np.float32)
    g_p = np.zeros(max(n + 2 * PAD, U * HOP), dtype=np.float32)
    g_p[:U * HOP] = acc.reshape(-1)
    return g_p[:n + 2 * PAD]


def wave_grad(wav_hat, g_mel, bk, dtype, table=None):
    """[B, n]: d/d wav_hat of sum g_mel * linear_mel(wav_hat); the fold is a scatter-add by the forward's own index map."""
    b = bk.basis[:, bk.bin_lo:bk.bin_hi].astype(dtype)
    tab = np.asarray(bk.table if table is None else table).astype(dtype)
    out = []
    for row, g in zip(np.asarray(wav_hat), np.asarray(g_mel)):
        n = row.shape[0]
        re, im, _ = spectrum(row, bk, dtype, table)
        q = mm(g.astype(dtype), b, dtype) / np.sqrt(re * re + im * im + dtype(MAG_EPS))
        g_p = overlap_add(q * re, q * im, tab, n, dtype)
        gw = np.zeros(n, dtype=dtype)
        np.add.at(gw, pad_index(n), g_p)
        out.append(np.where((row >= -1.0) & (row <= 1.0), gw, 0).astype(dtype))
    return np.stack(out)


def padded_grad(wav_hat_row, g_mel_row, bk, dtype):
    """The overlap-added gradient of the padded row before the fold (for the fold's own tests)."""
    b = bk.basis[:, bk.bin_lo:bk.bin_hi].astype(dtype)
    tab = bk.table.astype(dtype)
    n = wav_hat_row.shape[0]
    re, im, _ = spectrum(wav_hat_row, bk, dtype)
    q = (np.asarray(g_mel_row).astype(dtype) @ b) / np.sqrt(re * re + im * im + dtype(MAG_EPS))
    g_frames = (q * re) @ tab[0] + (q * im) @ tab[1]
    g_p = np.zeros(n + 2 * PAD, dtype=dtype)
    for t in range(g_frames.shape[0]):
        g_p[t * HOP:t * HOP + N_FFT] += g_frames[t]
    return g_p


def loss_and_grad(y_hat, y, bk, dtype=np.float64, table=None, sign=None, passed=None):
    """The whole model: (loss, g_wav [B, n], parts) with parts = dict(mel_hat, mel_y, d, g_mel, passed)."""
    mel_hat, mel_y = linear_mel(y_hat, bk, dtype, table), linear_mel(y, bk, dtype, table)
    loss, g_mel, d, ok = loss_and_g_mel(mel_hat, mel_y, dtype, sign, passed)
    return loss, wave_grad(y_hat, g_mel, bk, dtype, table), dict(mel_hat=mel_hat, mel_y=mel_y, d=d, g_mel=g_mel, passed=ok)


def torch_loss_and_grad(y_hat, y, bk):
    """The reference's formula (mel_utils.py:59-76, hifigan.py:35-38) in torch float64 on the CPU: loss and autograd's d loss / d y_hat."""
    basis = torch.from_numpy(bk.basis).double()
    win = torch.hann_window(bk.win, dtype=torch.float64)

    def mel(w):
        w = torch.nn.functional.pad(torch.clamp(w, -1.0, 1.0).unsqueeze(1), (PAD, PAD), mode="reflect").squeeze(1)
        spec = torch.stft(w, N_FFT, hop_length=HOP, win_length=bk.win, window=win, center=False, normalized=False, onesided=True,
                          return_complex=True)
        mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + MAG_EPS)
        return torch.log(torch.clamp(torch.matmul(basis, mag), min=FLOOR))

    with torch.enable_grad():  # whatever grad mode an earlier test module left behind
        a = torch.from_numpy(np.array(y_hat, dtype=np.float32)).double().requires_grad_(True)
        loss = torch.nn.functional.l1_loss(mel(a), mel(torch.from_numpy(np.array(y, dtype=np.float32)).double()))
        loss.backward()
    return float(loss.detach()), a.grad.numpy()


# ---- what the GPU tests stand on: bars from the float32 mirror, decision margins in the float64 model --------------------------------

CASES = ((1, 512), (1, 1000), (3, 64 * 256), (1, 65 * 256), (3, 130 * 256 + 17))  # (B, N) of the real-valued fixtures
ALL_CASES = [("mel80", B, n) for B, n in CASES] + [(name, 1, 65 * 256) for name in BANKS[1:]]  # (bank, B, N): what the GPU tests run


@functools.lru_cache(maxsize=None)
def given_g_mel(B, n, n_mels, seed=5):
    """A random mel gradient of the size a loss would give it, float32 [B, T, n_mels]."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((B, n_frames(n), n_mels)) / (B * n_frames(n) * n_mels)).astype(np.float32)
    g.setflags(write=False)
    return g


def clamp_probe(y_hat):
    """A copy of y_hat with samples beyond and exactly at the clamp's ends: returns (wav, beyond indices, at-the-end indices) of row 0."""
    w = np.array(y_hat, copy=True)
    n = w.shape[1]
    beyond, at = [n // 3, n // 2 + 1], [n // 3 + 7, n // 2 + 9]
    w[0, beyond[0]], w[0, beyond[1]] = np.float32(1.5), np.nextafter(np.float32(-1.0), np.float32(-2.0))
    w[0, at[0]], w[0, at[1]] = np.float32(1.0), np.float32(-1.0)
    return w, beyond, at


@functools.lru_cache(maxsize=None)
def derived(bank_name, B, n):
    """For one fixture: the float64 model's parts, the float32 mirror's errors and the GPU bars (4 x those), and the decision margins.
      bars: mel (max |d linear mel|), loss (mean |d of the entries' L_hat - L_y| + 2 u loss), g_mel (over decided entries), g_wav (the
      waveform gradient given given_g_mel(...)), grad (the mirror's g_mel through the mirror's backward)
      undecided [B, T, n_mels] bool: |d| <= 4 x the mirror's error of d there, or |mel_hat - floor| <= 4 x the mirror's error of the
      frame's mel (the mirror's error of a frame's mel is taken as the largest over the frame's rows: it scales with the frame's energy,
      not with the entry; the error of L follows to first order as that over mel, plus one rounding of L)."""
    bk = bank(bank_name)
    y_hat, y = pair(B, n, seed=n % 97)
    loss64, _, p64 = loss_and_grad(y_hat, y, bk, np.float64)
    mel_hat32, mel_y32 = linear_mel(y_hat, bk, np.float32), linear_mel(y, bk, np.float32)
    loss32, g32, d32, _ = loss_and_g_mel(mel_hat32, mel_y32, np.float32)
    e_hat = np.abs(mel_hat32 - p64["mel_hat"]).max(axis=2, keepdims=True)
    e_y = np.abs(mel_y32 - p64["mel_y"]).max(axis=2, keepdims=True)
    u = 2.0 ** -24
    err_d = e_hat / np.maximum(p64["mel_hat"], FLOOR) + e_y / np.maximum(p64["mel_y"], FLOOR) \
        + u * (np.abs(np.log(np.maximum(p64["mel_hat"], FLOOR))) + np.abs(np.log(np.maximum(p64["mel_y"], FLOOR))) + np.abs(p64["d"]))
    undecided = (np.abs(p64["d"]) <= BAR_FACTOR * err_d) | (np.abs(p64["mel_hat"] - FLOOR) <= BAR_FACTOR * e_hat)
    dec = ~undecided
    gm = given_g_mel(B, n, bk.n_mels)
    w_probe, _, _ = clamp_probe(y_hat)
    gw64, gw32 = wave_grad(w_probe, gm, bk, np.float64), wave_grad(w_probe, gm, bk, np.float32)
    bars = {
        "mel": BAR_FACTOR * float(max(e_hat.max(), e_y.max())),
        # the mirror's own |loss32 - loss64| is one draw that may come out at 0; what bounds it is the mean of the entries' errors
        # (| mean|a| - mean|b| | <= mean|a - b|) plus the roundings of the sum and of the result
        "loss": BAR_FACTOR * (float(np.abs(d32 - p64["d"]).mean()) + 2.0 * u * float(loss64)),
        "g_mel": BAR_FACTOR * float(np.abs(g32 - p64["g_mel"])[dec].max()),
        "g_wav": BAR_FACTOR * float(np.abs(gw32 - gw64).max()),
    }
    # the end-to-end gradient: the mirror's own g_mel (its decisions forced to the model's, so that only rounding is measured) through
    # the mirror's backward
    _, g32f, _, _ = loss_and_g_mel(mel_hat32, mel_y32, np.float32, sign=np.sign(p64["d"]), passed=p64["passed"].astype(np.int64))
    gfull64 = wave_grad(y_hat, p64["g_mel"], bk, np.float64)
    bars["grad"] = BAR_FACTOR * float(np.abs(wave_grad(y_hat, g32f, bk, np.float32) - gfull64).max())
    return dict(bank=bk, y_hat=y_hat, y=y, loss=float(loss64), parts=p64, undecided=undecided, share=float(undecided.mean()), bars=bars,
                g_given=gm, w_probe=w_probe, gw_given=gw64, grad=gfull64)


# ---- the loss launch restated in float32, in the kernel's documented order ---------------------------------------------------------------

def rows_sum_f32(part):
    """csrc/rows_sum.h on part [rows, 64] float32: 16 row groups; group rg walks rows rg, rg + 16, ... as four chains (rows rg + 64 k +
    0 / 16 / 32 / 48 while all four exist, the rest onto chain 0), (s0 + s1) + (s2 + s3); then the groups in ascending order."""
    part = np.asarray(part, dtype=np.float32)
    rows = part.shape[0]
    tot = np.zeros(64, dtype=np.float32)
    for rg in range(16):
        s = [np.zeros(64, dtype=np.float32) for _ in range(4)]
        r = rg
        while r + 48 < rows:
            for c in range(4):
                s[c] = s[c] + part[r + 16 * c]
            r += 64
        while r < rows:
            s[0] = s[0] + part[r]
            r += 16
        tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
    return tot


def loss_launch_f32(mel_hat, log_hat, log_y):
    """set_mel_loss_fwd restated: float32 (loss, g_mel = count times the loss's gradient) from the GPU's own linear mel of y_hat and its two log-mels, the sum in the order
    include/set_amd.h documents."""
    mh = np.asarray(mel_hat, dtype=np.float32).reshape(-1)
    d = (np.asarray(log_hat, dtype=np.float32).reshape(-1) - np.asarray(log_y, dtype=np.float32).reshape(-1)).astype(np.float32)
    n = d.size
    ok = (mh >= np.float32(FLOOR)) & (d != 0)
    g = np.where(ok, np.copysign(np.float32(1), d) / np.where(ok, mh, np.float32(1)), np.float32(0)).astype(np.float32)
    blocks = (n + 4095) // 4096
    a = np.zeros(blocks * 4096, dtype=np.float32)
    a[:n] = np.abs(d)
    a = a.reshape(blocks, 16, 4, 64)                      # block, i, wave, column
    s = a[:, 0]
    for i in range(1, 16):
        s = s + a[:, i]
    part = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]      # [blocks, 64]
    col = rows_sum_f32(part)
    tot = np.float32(0)
    for c in range(64):
        tot = np.float32(tot + col[c])
    return np.float32(np.float64(tot) / np.float64(n)), g.reshape(np.asarray(mel_hat).shape)
