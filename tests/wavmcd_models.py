"""float64 models of the wav-level mel-cepstral distortion (csrc/wav_mcd.hip), written from the definitions of librosa 0.8.0's
`feature.mfcc(htk=True)` and of eval/mcd.py `cal_mcd`; shared by test_wavmcd_reference.py (CPU) and test_gpu_wavmcd.py.  Nothing here
imports the package: the filterbank, the window, the DCT and the distance are restated a second time.

    htk_basis     triangles between n_mels + 2 points equally spaced in mel = 2595 log10(1 + f / 700), area-normalised
    power         |rfft(periodic Hann x frame)|^2 of the reflect-padded waveform, hop 256: [T, 513], T = 1 + N // 256
    db            10 log10(max(1e-10, power @ basis.T)): [T, 80]
    clamp         max(dB, max dB - 80), the maximum over the utterance's own frames and all bands
    mfcc          clamp(db) @ dct_ortho(K, 80).T: [T, K], c0 included
    cal_mcd       mean_k(10 / ln 10 sqrt(2 sum_t (a - b)^2)) / T, the sum over the FRAMES as the reference's axis=1 on [K, T] arrays
    mcd_dtw       exact DTW over frames (mcd_models.dtw), dist / steps
    *32           float32 mirrors of the same arithmetic (numpy on the CPU): what the bars are cross-checked against
"""
import numpy as np

import mcd_models as MM

SR, NFFT, HOP, NMELS, FMIN, FMAX, NMFCC, TOP_DB, AMIN = 22050, 1024, 256, 80, 55.0, 7600.0, 34, 80.0, 1e-10
PAD, NBIN = NFFT // 2, NFFT // 2 + 1
DB_C = 10.0 / np.log(10.0)
U32 = 2.0 ** -24


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def htk_edges(n_mels=NMELS, fmin=FMIN, fmax=FMAX):
    """The n_mels + 2 triangle corners in Hz."""
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))


def htk_basis(sr=SR, n_fft=NFFT, n_mels=NMELS, fmin=FMIN, fmax=FMAX):
    """float64 [n_mels, n_fft/2 + 1], one row at a time from the definition of a triangle."""
    e = htk_edges(n_mels, fmin, fmax)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    b = np.zeros((n_mels, f.shape[0]))
    for m in range(n_mels):
        up = (f - e[m]) / (e[m + 1] - e[m])
        down = (e[m + 2] - f) / (e[m + 2] - e[m + 1])
        b[m] = np.maximum(0.0, np.minimum(up, down)) * 2.0 / (e[m + 2] - e[m])
    return b


BASIS64 = htk_basis()
BASIS32 = BASIS64.astype(np.float32)  # what the kernel multiplies with
WIN64 = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)


def n_frames(n):
    return 1 + n // HOP if n > PAD else 0


def frames_of(y, dtype=np.float64):
    """[T, 1024]: frame t of the waveform reflected by 512 at both ends starts at padded sample 256 t."""
    y = np.asarray(y, dtype=dtype)
    p = np.pad(y, PAD, mode="reflect")
    T = n_frames(len(y))
    return p[np.arange(T)[:, None] * HOP + np.arange(NFFT)[None, :]]


def power(y):
    return np.abs(np.fft.rfft(frames_of(y) * WIN64[None, :], axis=1)) ** 2


def db(y, basis=None):
    """float64 [T, 80] from the fp32 samples y; the filterbank is the fp32 one the kernel holds unless another is given."""
    b = BASIS32.astype(np.float64) if basis is None else np.asarray(basis, dtype=np.float64)
    return DB_C * np.log(np.maximum(AMIN, power(y) @ b.T))


def clamp(d, top_db=TOP_DB):
    return np.maximum(d, d.max() - top_db)


def dct_ortho(K, M=NMELS):
    k = np.arange(K, dtype=np.int64)[:, None]
    n = np.arange(M, dtype=np.int64)[None, :]
    t = np.sqrt(2.0 / M) * np.cos(np.pi * ((k * (2 * n + 1)) % (4 * M)) / (2.0 * M))  # the angle reduced in integers
    t[0] = np.sqrt(1.0 / M)
    return t


def mfcc(y, K=NMFCC, top_db=TOP_DB):
    return clamp(db(y), top_db) @ dct_ortho(K).T


def mfcc_of_db(d32, peak32, K, top_db=TOP_DB):
    """The clamp and DCT of set_db_mfcc in float64 on an fp32 dB array [T, M] and its fp32 peak: the floor is the one fp32 subtraction
    the kernel makes, the table the fp32 one (rows of dct_ortho rounded once), the sum exact to float64."""
    lo = np.float32(peak32) - np.float32(top_db)
    x = np.maximum(np.asarray(d32, dtype=np.float32), lo).astype(np.float64)
    return x @ dct_ortho(K, x.shape[1]).astype(np.float32).astype(np.float64).T


def cal_mcd(c_ref, c_est):
    """eval/mcd.py `cal_mcd(use_dtw=False)` on [T, K] arrays (its own are the transposes), term by term."""
    a, b = np.asarray(c_ref, dtype=np.float64), np.asarray(c_est, dtype=np.float64)
    assert a.shape == b.shape
    diff2sum = np.sum((b - a) ** 2, 0)  # over the frames: one value per coefficient
    return float(np.mean(DB_C * np.sqrt(2 * diff2sum), 0) / a.shape[0])


def rms_dist_kernel_order(x, y):
    """cal_mcd in the kernel's own order in float64, rounded once: per k four partial sums over t = q, q + 4, ... added as
    (0 + 1) + (2 + 3), the K terms summed ascending, / K / T.  On integer-valued inputs every sum is exact."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    T, K = x.shape
    d2 = (x - y) ** 2
    p = [np.zeros(K) for _ in range(4)]
    for t in range(T):
        p[t & 3] = p[t & 3] + d2[t]
    s = (p[0] + p[1]) + (p[2] + p[3])
    term = 4.3429448190325175 * np.sqrt(2.0 * s)
    acc = 0.0
    for k in range(K):
        acc += term[k]
    return np.float32(acc / K / T)


def mcd_dtw(c_ref, c_est):
    m = MM.dtw(np.asarray(c_ref, dtype=np.float64), np.asarray(c_est, dtype=np.float64))
    return float(m["dist"]) / m["steps"], m


# ---- float32 mirrors ------------------------------------------------------------------------------------------------------------------------
_DFT32 = []


def dft32():
    """fp32 [2, 513, 1024]: win cos and -win sin, each rounded once from float64 (what melspec.dft_table holds)."""
    if not _DFT32:
        f = np.arange(NBIN, dtype=np.int64)[:, None]
        n = np.arange(NFFT, dtype=np.int64)[None, :]
        ang = 2.0 * np.pi * ((f * n) % NFFT) / NFFT
        _DFT32.append(np.stack([WIN64 * np.cos(ang), -WIN64 * np.sin(ang)]).astype(np.float32))
    return _DFT32[0]


def db32(y):
    """The kernel's arithmetic in numpy float32: both matrix products and the power in fp32, the log in double rounded once."""
    fr = frames_of(y, np.float32)
    W = dft32()
    re, im = fr @ W[0].T, fr @ W[1].T
    S = (re * re + im * im) @ BASIS32.T
    return (DB_C * np.log(np.maximum(S, np.float32(AMIN)).astype(np.float64))).astype(np.float32)


def mfcc32(y, K=NMFCC, top_db=TOP_DB):
    d = db32(y)
    x = np.maximum(d, d.max() - np.float32(top_db))
    return x @ dct_ortho(K).astype(np.float32).T


def mcd32(ref, est):
    return float(cal_mcd(mfcc32(ref), mfcc32(est)))


# ---- signals --------------------------------------------------------------------------------------------------------------------------------
N_SIG = 129 * 256


def signal(sigma, n=N_SIG, seed=7, gap=None):
    """0.5 sin 220 Hz + 0.25 sin 3 kHz + sigma N(0, 1), float32; `gap` = (first, last) hops set to exact zero."""
    t = np.arange(n) / SR
    rng = np.random.default_rng(seed)
    y = 0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.25 * np.sin(2 * np.pi * 3000.0 * t) + sigma * rng.standard_normal(n)
    if gap is not None:
        y[gap[0] * HOP:gap[1] * HOP] = 0.0
    return y.astype(np.float32)


CLAMP_CASES = {"unclamped": dict(sigma=0.025), "zero_gap": dict(sigma=0.025, gap=(40, 70)), "noise_floor": dict(sigma=6e-4)}


def clamp_case(name, n=N_SIG):
    return signal(n=n, **CLAMP_CASES[name])


def clamped_share(y):
    d = db(y)
    return float((d < d.max() - TOP_DB).mean()), d


def degraded(y, seed=11, level=0.05, scale=0.9):
    """The prediction beside the ground truth y: a slightly scaled copy plus noise."""
    rng = np.random.default_rng(seed)
    return (scale * y + level * rng.standard_normal(len(y))).astype(np.float32)


# ---- the bars -------------------------------------------------------------------------------------------------------------------------------
LAMBDA = 8.0  # the margin of the bars: see s_bound


def s_bound(y):
    """[T, 80] bound on |kernel S - float64 S| for S = basis |DFT|^2 when both take the same fp32 samples, and the float64 S itself.

    GEMM 1: a table entry is its float64 value rounded once and the product has n = 1024 terms.  The worst case, (n + 2) u sum |w y|, is
    attained only when every rounding error has the same sign; with it the bar on a noise-floor band would be 0.4 dB, thousands of times
    what any fp32 evaluation shows, and would test nothing.  The bars take the root-sum-square form instead (Higham & Mary 2019): n
    independent errors of at most u grow as sqrt(n), so
        |d re|, |d im| <= LAMBDA sqrt(n + 2) u ||w y||_2 <= LAMBDA sqrt(n + 2) u ||frame||_2 =: delta      (|w cos|, |w sin| <= 1)
    where the 2-norm of the terms stands for the partial sums they make up in whatever order the hardware adds them.  LAMBDA = 8 is the
    margin taken: the float32 mirror uses a seventh of the bar on its worst entry (test_wavmcd_reference.py asserts it stays
    inside, and that the bar is within 100 x of it), which leaves room for the MFMA's different summation order and no more.
    The power: |d (re^2 + im^2)| <= 2 sqrt(2) |X| delta + 2 delta^2 + 2 u P.  GEMM 2 sums at most 513 non-negative terms against a
    filterbank held as rounded fp32 (the model holds the same one): LAMBDA sqrt(width + 2) u S with width the triangle's bins."""
    fr = frames_of(y)
    X = np.fft.rfft(fr * WIN64[None, :], axis=1)
    P = np.abs(X) ** 2
    delta = LAMBDA * np.sqrt(NFFT + 2.0) * U32 * np.linalg.norm(fr, axis=1)[:, None]
    dP = 2.0 * np.sqrt(2.0) * np.abs(X) * delta + 2.0 * delta ** 2 + 2.0 * U32 * P
    B = BASIS32.astype(np.float64)
    S = P @ B.T
    width = (B != 0).sum(1).astype(np.float64)
    return dP @ B.T + LAMBDA * np.sqrt(width + 2.0)[None, :] * U32 * S, S


def db_bars(y, top_db=TOP_DB):
    """(bar on the unclamped dB [T, 80], bar on the peak, bar on the clamped dB [T, 80], the float64 dB).  d(10 log10 S) <= 10 / ln 10
    dS / S (the floor 1e-10 only lowers the slope), plus the one rounding of the fp32 result.  The clamp max(dB, peak - 80) is
    1-Lipschitz in both arguments: a clamped entry carries the peak's bar (and the rounding of the fp32 subtraction), an unclamped one its
    own, and one within reach of the threshold the larger of the two."""
    dS, S = s_bound(y)
    d = DB_C * np.log(np.maximum(AMIN, S))
    bar = DB_C * dS / np.maximum(S, AMIN) + U32 * np.abs(d)
    # the peak may be taken at any entry within the bars of the largest: the largest bar among those
    near = d >= d.max() - 2.0 * bar.max()
    peak_bar = float(bar[near].max())
    lo = d.max() - top_db
    lo_bar = peak_bar + U32 * abs(lo)
    clamped = np.where(d < lo - bar - lo_bar, lo_bar, np.where(d > lo + bar + lo_bar, bar, np.maximum(bar, lo_bar)))
    return bar, peak_bar, clamped, d


def mfcc_bars(clamped_bar, x, K):
    """[T, K] bar on the MFCC given the bars on the clamped dB x [T, M]: sum_n |table[k][n]| bar_n, plus the table's rounding and the FMA
    chain's M roundings, (M + 2) u sum_n |table[k][n] x_n|."""
    t = np.abs(dct_ortho(K, x.shape[1]))
    return clamped_bar @ t.T + (x.shape[1] + 2) * U32 * (np.abs(x) @ t.T)


def chain_bars(x, K):
    """The MFCC bar of set_db_mfcc alone, fed an fp32 clamped dB x it shares with the model: the table's rounding and the FMA chain."""
    return mfcc_bars(np.zeros_like(x), x, K)


def mcd_bar(c_ref, c_est, bar_ref, bar_est):
    """The allowance on cal_mcd by propagation: a coefficient pair off by e = bar_ref + bar_est moves sqrt(sum_t d^2) by at most
    sqrt(sum_t e^2) (a norm is 1-Lipschitz), so the score by mean_k(10 / ln 10 sqrt(2 sum_t e^2)) / T; plus the fp32 result's rounding."""
    e = bar_ref + bar_est
    return float(np.mean(DB_C * np.sqrt(2.0 * (e ** 2).sum(0))) / e.shape[0]) + U32 * cal_mcd(c_ref, c_est)


def dtw_bar(bar_ref, bar_est, m, K):
    """The allowance on dist / steps along the model's path: every cost moves by at most ||e_i||_2 + ||e_j||_2 with e the per-frame MFCC
    bars, so the mean over the path by their mean; plus the fp32 DTW's own error (mcd_models.dist_rel_bound) and the division's."""
    i, j = m["path"][:, 0], m["path"][:, 1]
    move = np.linalg.norm(bar_ref, axis=1)[i] + np.linalg.norm(bar_est, axis=1)[j]
    mcd = float(m["dist"]) / m["steps"]
    return float(move.mean()) + (MM.dist_rel_bound(len(bar_ref), len(bar_est), K) + U32) * mcd


def ramp_pair(n=N_SIG, short=9):
    """The DTW pair: the unclamped signal fading by 20 dB over its length, so that every frame differs from its neighbours (c0 falls by
    0.15 sqrt(80) = 1.4 per frame) and the alignment has one clear optimum, beside a copy with a little more noise that ends `short`
    frames early.  A stationary signal leaves thousands of near-equal paths (the relative gap between the best two predecessors falls to
    2e-9 on the clamp cases), and dist / steps would hang on fp32 ties."""
    fade = 10.0 ** (-1.0 * np.arange(n) / n)
    y = (signal(0.025, n) * fade).astype(np.float32)
    return y, degraded(y, level=0.002, scale=1.0)[:n - short * HOP]
