"""Models of the STOI path (set_amd.metrics.stoi, csrc/stoi.hip) for its tests; no tests here.

    *64     the float64 model of the five stages of include/set_amd.h's STOI block, which is eval/stoi.py `stoi(x, y, 22050)` with
            eval/utils.py restated stage by stage (float64 window, the dB form of the selection, np.fft.rfft);
    *32     a numpy float32 mirror: stages 1-3 in the kernels' own arithmetic (compaction bit for bit), and the whole path in float32;
    signals seeded builders, deterministic from numpy's default_rng alone, and the case tables.
"""
import math

import numpy as np

FS, NF, EH, HOP, NSEG, NB = 22050, 1024, 512, 256, 30, 15
EPS64 = float(np.finfo("float").eps)
EPS32 = np.float32(2.220446e-16)
CLIP = 10.0 ** 0.75                      # 10^(-BETA / 20), BETA = -15
W64 = np.hanning(NF + 2)[1:-1]
W32 = W64.astype(np.float32)
LO = (6, 8, 10, 12, 16, 20, 25, 31, 39, 50, 63, 79, 99, 125, 158, 199)  # band i = bins [LO[i], LO[i + 1])
NBINS = LO[-1]


def band_matrix(lo=LO, nbins=NF // 2 + 1):
    m = np.zeros((len(lo) - 1, nbins))
    for i in range(len(lo) - 1):
        m[i, lo[i]:lo[i + 1]] = 1.0
    return m


# ---- counts -------------------------------------------------------------------------------------------------------------------------------
def energy_frames(n):
    """F: frames of 1024 at hop 512 that start in front of n - 1024 (the reference's range(0, n - 1024, 512))."""
    return -(-(n - NF) // EH) if n > NF else 0


def envelope_frames(K):
    """T_b = 2 (K - 1): frames of 1024 at hop 256 of the 512 (K + 1) compacted samples."""
    return 2 * (K - 1) if K >= 2 else 0


def sizes(N):
    """(F_max, S, T) of a batch of N-sample rows."""
    f = energy_frames(N)
    return f, EH * (f + 1), max(2 * (f - 1), 0)


def frames_of(x, hop, n_frames, dtype):
    if n_frames == 0:
        return np.zeros((0, NF), dtype=dtype)
    idx = hop * np.arange(n_frames)[:, None] + np.arange(NF)[None, :]
    return np.asarray(x, dtype=dtype)[idx]


# ---- float64 model ------------------------------------------------------------------------------------------------------------------------
def norms64(x):
    return np.linalg.norm(W64[None, :] * frames_of(x, EH, energy_frames(len(x)), np.float64), axis=1)


def select64(x):
    """(kept indices ascending, margin in dB of the frame nearest to the threshold): the reference's dB comparison."""
    nrm = norms64(x)
    if nrm.size == 0:
        return np.zeros(0, dtype=np.int32), np.inf
    with np.errstate(divide="ignore"):
        e = 20.0 * np.log10(nrm + EPS64)
    dist = e - (np.max(e) - 40.0)
    return np.nonzero(dist > 0)[0].astype(np.int32), float(np.min(np.abs(dist)))


def compact(s, kept, w, dtype):
    """The overlap-add at hop 512 of the kept windowed frames: 512 (K + 1) samples; an absent term is +0.0.  In float32 this is the kernel's
    arithmetic bit for bit: two separately rounded products and one rounded add."""
    s, w = np.asarray(s, dtype=dtype), np.asarray(w, dtype=dtype)
    K = len(kept)
    out = np.zeros(EH * (K + 1), dtype=dtype)
    if K:
        fr = s[EH * np.asarray(kept)[:, None] + np.arange(NF)[None, :]] * w[None, :]
        head = np.concatenate([fr[:, :EH], np.zeros((1, EH), dtype=dtype)])
        tail = np.concatenate([np.zeros((1, EH), dtype=dtype), fr[:, EH:]])
        out = (head + tail).reshape(-1)
    return out


def bands64(sil, lo=LO, start=0):
    """[T_b, 15]: sqrt of the band sums of |rfft(w frame)|^2, frame m from sample 256 m + start."""
    T = max(-(-(len(sil) - NF - start) // HOP), 0) if len(sil) > NF else 0
    fr = frames_of(np.asarray(sil, dtype=np.float64)[start:], HOP, T, np.float64)
    p = np.abs(np.fft.rfft(W64[None, :] * fr, n=NF, axis=1)) ** 2
    return np.sqrt(p @ band_matrix(lo).T)


def correlations(xt, yt, seg=NSEG, clip=CLIP, dtype=np.float64):
    """rho [J, bands] of envelopes [T, bands], and the mask of elements whose min took the clipped branch."""
    J = xt.shape[0] - seg + 1
    idx = np.arange(J)[:, None] + np.arange(seg)[None, :]
    X, Y = xt.astype(dtype)[idx], yt.astype(dtype)[idx]                     # [J, seg, bands]
    nx, ny = np.sqrt(np.sum(X * X, axis=1, keepdims=True)), np.sqrt(np.sum(Y * Y, axis=1, keepdims=True))
    c = np.divide(nx, ny, out=np.zeros_like(nx), where=ny > 0)
    a, b = Y * c, X * dtype(1.0 + clip)
    Yp = np.minimum(a, b)
    X = X - np.mean(X, axis=1, keepdims=True, dtype=dtype)
    Yp = Yp - np.mean(Yp, axis=1, keepdims=True, dtype=dtype)
    dx, dy = np.sqrt(np.sum(X * X, axis=1, keepdims=True)), np.sqrt(np.sum(Yp * Yp, axis=1, keepdims=True))
    X = np.divide(X, dx, out=np.zeros_like(X), where=dx > 0)
    Yp = np.divide(Yp, dy, out=np.zeros_like(Yp), where=dy > 0)
    return np.sum(X * Yp, axis=1), b < a


def score64(xt, yt, seg=NSEG, clip=CLIP):
    """d, or None below `seg` frames."""
    if xt.shape[0] < seg:
        return None
    rho, _ = correlations(xt, yt, seg, clip)
    return float(np.sum(rho) / rho.size)


def stoi64(x, y, lo=LO, start=0, seg=NSEG, clip=CLIP):
    """The whole path in float64: dict(d, kept, K, T, xt, yt).  The keyword arguments are the one-line mistakes of the mutant test."""
    assert len(x) == len(y)
    kept, _ = select64(x)
    xs, ys = compact(x, kept, W64, np.float64), compact(y, kept, W64, np.float64)
    xt, yt = bands64(xs, lo, start), bands64(ys, lo, start)
    return dict(d=score64(xt, yt, seg, clip), kept=kept, K=len(kept), T=xt.shape[0], xt=xt, yt=yt)


# ---- float32 mirror -----------------------------------------------------------------------------------------------------------------------
def norms32(x):
    """The kernel's order: lane l sums fl(fl(w x)^2) over n = l, l + 64, ... ascending, then the butterfly 32, 16, ..., 1."""
    fr = frames_of(x, EH, energy_frames(len(x)), np.float32)
    p = W32[None, :] * fr
    p = (p * p).reshape(-1, NF // 64, 64)
    acc = np.zeros((p.shape[0], 64), dtype=np.float32)
    for k in range(NF // 64):
        acc = acc + p[:, k]
    off = 32
    while off:
        acc = acc + acc[:, np.arange(64) ^ off]
        off >>= 1
    return np.sqrt(acc[:, 0])


def select32(x):
    nrm = norms32(x)
    if nrm.size == 0:
        return np.zeros(0, dtype=np.int32)
    thr = np.float32(0.01) * (np.max(nrm) + EPS32)
    return np.nonzero(nrm + EPS32 > thr)[0].astype(np.int32)


def dft_table32(nbins=NBINS):
    n = np.arange(NF, dtype=np.int64)[None, :]
    f = np.arange(nbins, dtype=np.int64)[:, None]
    ang = 2.0 * np.pi * ((f * n) % NF).astype(np.float64) / NF
    return (W64[None, :] * np.cos(ang)).astype(np.float32), (-W64[None, :] * np.sin(ang)).astype(np.float32)


_TABLE32 = []


def bands32(sil):
    if not _TABLE32:
        _TABLE32.extend(dft_table32())
    T = -(-(len(sil) - NF) // HOP) if len(sil) > NF else 0
    fr = frames_of(sil, HOP, T, np.float32)
    re, im = fr @ _TABLE32[0].T, fr @ _TABLE32[1].T
    p = re * re + im * im
    return np.sqrt(p @ band_matrix(LO, NBINS).T.astype(np.float32))


def stoi32(x, y):
    """The whole path in numpy float32: d (a Python float) or None."""
    kept = select32(x)
    xt, yt = bands32(compact(x, kept, W32, np.float32)), bands32(compact(y, kept, W32, np.float32))
    if xt.shape[0] < NSEG:
        return None
    rho, _ = correlations(xt, yt, dtype=np.float32)
    assert rho.dtype == np.float32
    return float(np.sum(rho, dtype=np.float32) / np.float32(rho.size))


# ---- signals ------------------------------------------------------------------------------------------------------------------------------
def speech(n, seed, gaps=(), gap_level=1e-4, deep=False):
    """A speech-like float32 signal: noise whose low and high half are modulated at syllabic rates of their own, with near-silent
    stretches `gaps` (pairs of sample indices) at gap_level of the amplitude.  deep: every other 80 ms is 26 dB down -- still above the
    -40 dB silence threshold, and where added noise drives the normalised envelope of y above the clip level."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    low = np.convolve(a, np.ones(8) / 8.0, mode="same")                       # below ~1.2 kHz
    high = b - np.convolve(b, np.ones(4) / 4.0, mode="same")                  # above ~2 kHz
    ph = rng.uniform(0, 2 * np.pi, 2)
    x = 0.3 * (0.52 + 0.48 * np.sin(2 * np.pi * 3.7 * t + ph[0])) * low + 0.05 * (0.52 + 0.48 * np.sin(2 * np.pi * 5.3 * t + ph[1])) * high
    if deep:
        x = x * np.where((np.arange(n) % 3528) < 1764, 1.0, 0.05)
    for g0, g1 in gaps:
        x[g0:g1] *= gap_level
    return x.astype(np.float32)


def degrade(x, snr_db, seed, ramp_db=20.0):
    """x + white noise at snr_db (against the whole of x) whose level rises by ramp_db from the first sample to the last: the score then
    depends on where the segments lie, which is what the mutants of the allowance test move."""
    rng = np.random.default_rng(seed + 7919)
    n = len(x)
    noise = rng.standard_normal(n)
    g = np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)) * 10.0 ** (-snr_db / 20.0)
    g = g * 10.0 ** (ramp_db * (np.arange(n) / n - 0.5) / 20.0)
    return (np.asarray(x, dtype=np.float64) + g * noise).astype(np.float32)


# end-to-end cases: id -> n, seed, snr_db, gaps, deep.  The recorded reference values are in tests/golden/stoi_reference.json.
E2E = {
    "n22050_snr0": dict(n=22050, seed=11, snr_db=0.0, gaps=(), deep=False),
    "n30001_snrm3_gap_mid": dict(n=30001, seed=12, snr_db=-3.0, gaps=((9000, 15500),), deep=False),
    "n40001_snrm5_gap_ends": dict(n=40001, seed=13, snr_db=-5.0, gaps=((0, 4200), (33000, 40001)), deep=False),
    "n24000_clip": dict(n=24000, seed=14, snr_db=0.0, gaps=(), deep=True),
    "n36000_clip_gap": dict(n=36000, seed=15, snr_db=3.0, gaps=((12000, 17000),), deep=True),
    "n8705_first_valid": dict(n=8705, seed=16, snr_db=0.0, gaps=(), deep=False),
    "n8704_too_short": dict(n=8704, seed=17, snr_db=5.0, gaps=(), deep=False),
    "n20000_mostly_silent": dict(n=20000, seed=18, snr_db=5.0, gaps=((6000, 20000),), deep=False),
}
CLIP_CASES = ("n24000_clip", "n36000_clip_gap")
INVALID_CASES = ("n8704_too_short", "n20000_mostly_silent")
VALID_CASES = tuple(k for k in E2E if k not in INVALID_CASES)
MUTANTS = {  # one-line mistakes of the model, as keyword arguments of stoi64
    "band edge off by one bin": dict(lo=tuple(v + 1 for v in LO)),
    "STFT start off by one hop": dict(start=HOP),
    "29-frame segments": dict(seg=NSEG - 1),
    "clip constant 10^(-0.75)": dict(clip=10.0 ** -0.75),
}


def pair(case):
    c = E2E[case]
    x = speech(c["n"], c["seed"], c["gaps"], deep=c["deep"])
    return x, degrade(x, c["snr_db"], c["seed"])


# ---- selection cases ------------------------------------------------------------------------------------------------------------------------
def one_kept_frame(n=6000, f=4):
    """Two samples at the centre of frame f and zeros elsewhere: the neighbours see them under w[1023] and w[0], -100 dB."""
    x = np.zeros(n, dtype=np.float32)
    x[EH * f + EH - 1: EH * f + EH + 1] = 0.5
    return x


def threshold_probes(n=16384, seed=21, offsets_db=(0.02, -0.02)):
    """A loud stretch, then silence (exact zeros) holding one isolated 1024-sample burst per offset whose frame norm is placed
    offsets_db above / below the -40 dB threshold.  Returns (x, the probe frames)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.float64)
    x[:4096] = 0.2 * rng.standard_normal(4096)
    probes = []
    for i, off in enumerate(offsets_db):
        f = 12 + 6 * i
        x[EH * f: EH * f + NF] = 1e-3 * rng.standard_normal(NF)  # far below the loud stretch: never the maximum
        probes.append(f)
    x = x.astype(np.float32)
    for f, off in zip(probes, offsets_db):
        for _ in range(3):  # the float32 rounding of the scaled burst moves the norm by ~1e-8 relative: settle it
            nrm = norms64(x)
            x[EH * f: EH * f + NF] *= np.float32(0.01 * (np.max(nrm) + EPS64) * 10.0 ** (off / 20.0) / nrm[f])
    return x, probes


def select_cases():
    """name -> waveform, the rows of the selection tests (each also a compaction case)."""
    s = speech(9000, 31)
    return {
        "len1025": speech(1025, 32), "len1536": speech(1536, 33), "len1537": speech(1537, 34),
        "silence_start": speech(9000, 35, gaps=((0, 3000),)), "silence_mid": speech(9000, 36, gaps=((3000, 6000),)),
        "silence_end": speech(9000, 37, gaps=((6000, 9000),)), "one_kept": one_kept_frame(), "probes": threshold_probes()[0],
        "all_zero": np.zeros(5000, dtype=np.float32), "plain": s,
    }


def selection_margin_db(x):
    return select64(x)[1]


def bar_from(diffs):
    """The GPU allowance on d: 16 x the largest |float32 mirror - float64 model| (MFMA k-order and wave reductions differ from numpy's
    order, and the device's sqrt / division may be 1 ulp off); a margin over a CPU reference, never over the code under test."""
    return 16.0 * max(diffs)


_BAR = []


def e2e_bar():
    """(bar, the per-case |mirror - model|), computed once."""
    if not _BAR:
        diffs = {}
        for k in VALID_CASES:
            x, y = pair(k)
            diffs[k] = abs(stoi32(x, y) - stoi64(x, y)["d"])
        _BAR.append((bar_from(diffs.values()), diffs))
    return _BAR[0]


def tone(bin_, n=NF + HOP * 4, amp=0.25):
    """A bin-centred tone: all of its windowed energy in bins bin_ - 1 .. bin_ + 1 (the Hann main lobe), ~-31 dB beyond for the symmetric
    window."""
    return (amp * np.cos(2 * np.pi * bin_ * np.arange(n) / NF)).astype(np.float32)


def envelopes(T, seed, nb=NB, clipy=False):
    """Positive random envelopes [T, nb] float32 for the score kernel: x, and y = a noisy copy of it.  clipy: x dips to 3 % in 40 % of its
    elements and y does not follow, so the normalised y exceeds the clip level there."""
    rng = np.random.default_rng(seed)
    x = 0.2 + rng.random((T, nb))
    y = x * (0.5 + rng.random((T, nb)))
    if clipy:
        x = x * np.where(rng.random((T, nb)) < 0.4, 0.03, 1.0)
    return x.astype(np.float32), y.astype(np.float32)


# ---- the reference's own function (a host with the reference checkout only; never on the GPU machine) ----------------------------------------
def load_reference_stoi(ref_root):
    """eval/stoi.py's `stoi` of the reference checkout at ref_root.  The file imports `librosa` for its wav loader only and `utils` meaning
    eval/utils.py: a stand-in module for the first and the file itself for the second are put in front of the import and taken away after."""
    import importlib.util
    import os
    import sys
    import types

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    saved = {k: sys.modules.get(k) for k in ("librosa", "utils")}
    try:
        if saved["librosa"] is None:
            try:
                import librosa  # noqa: F401
            except Exception:
                sys.modules["librosa"] = types.ModuleType("librosa")
        sys.modules["utils"] = load("set_ref_eval_utils", os.path.join(ref_root, "eval", "utils.py"))
        mod = load("set_ref_eval_stoi", os.path.join(ref_root, "eval", "stoi.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


# ---- the envelope bound ---------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24


def envelope_bound(sil, tob):
    """[T, 15] bound on |kernel envelope - bands64(sil)| when both take the same fp32 samples `sil`, term by term:
      * a table entry is its float64 value rounded once (1 u relative), and GEMM 1 forms 1024 products and as many fp32 additions in
        whatever order (gamma_1024, (1024 + 2) u to first order): |d re|, |d im| <= (1024 + 3) u sum_n |table[n] s[n]|
        <= (1024 + 3) u ||w||_2 ||frame||_2 (Cauchy-Schwarz; |cos|, |sin| <= 1) =: delta, for every bin;
      * the envelope of a band of `width` bins is the 2-norm of its 2 width real and imaginary parts, and a norm is 1-Lipschitz:
        sqrt(2 width) delta;
      * re^2 + im^2 in fp32 is 2 u relative, the band sum of `width` non-negative terms in any order width u, so the power is
        (width + 2) u off; the square root halves that and adds its own u: (width / 2 + 2) u, taken as (width / 2 + 3) u for the
        second-order terms."""
    T = tob.shape[0]
    fn = np.linalg.norm(frames_of(sil, HOP, T, np.float64), axis=1)
    delta = (NF + 3) * U32 * np.linalg.norm(W64) * fn
    width = np.diff(np.asarray(LO)).astype(np.float64)
    return np.sqrt(2.0 * width)[None, :] * delta[:, None] + (width / 2.0 + 3.0)[None, :] * U32 * tob


def band_inputs():
    """name -> fp32 samples for the band kernel: lengths whose frame counts are 1, 63, 64, 65, 129 (the 64-frame tile of the kernel, one
    and two tiles), and the bin-centred tones that pin the band edges."""
    out = {"T%d" % t: speech(NF + HOP * t - (HOP - 1 if t % 2 else 0), 40 + t) for t in (1, 63, 64, 65, 129)}
    out.update({"tone%d" % b: tone(b) for b in (5, 6, 7, 8, 198, 199)})
    return out
