"""float64 models of the mel-cepstral distortion kernels (csrc/mcd.hip), written from the definitions; shared by test_mcd_reference.py
(CPU) and test_gpu_mcd.py.

    dct_table   cos(pi k (2n+1) / (2M)), k = 1..K
    mfcc        x @ table.T, x = mel or log10(mel)
    dtw         D[i][j] = C[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]), C the euclidean cost in the difference form, ties to the first of
                the three; the path length L carried with D; the chosen predecessor `dir`; the path traced back through `dir`; and per cell
                the relative gap between the best and the second-best predecessor.  `dtype=np.float32` runs the same arithmetic in fp32.
    zero_fill   sum_t ||x_t - y_t||, the shorter side zero-filled
    mel_mcd     utils/eval/mcd.py `get_metrics_mels`, with the exact DTW in place of fastdtw
"""
import numpy as np

GRIDS = {"34": (3, 4), "122": (1, 2, 2), "236": (2, 3, 6), "5": (5,)}  # integer vectors of integer norm: 5, 3, 7, 5


def dct_table(K, M):
    k = np.arange(1, K + 1, dtype=np.float64)[:, None]
    n = np.arange(M, dtype=np.float64)[None, :]
    return np.cos(np.pi * k * (2.0 * n + 1.0) / (2.0 * M))


def mfcc(mel, K, take_log=False):
    """[..., T, M] -> [..., T, K], float64."""
    x = np.asarray(mel, dtype=np.float64)
    if take_log:
        x = np.log10(x)
    return x @ dct_table(K, x.shape[-1]).T


def cost(x, y, dtype=np.float64):
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    d = x[:, None, :] - y[None, :, :]
    acc = np.zeros(d.shape[:2], dtype=dtype)
    for k in range(d.shape[2]):  # ascending k, as the kernel sums
        acc = acc + d[:, :, k] * d[:, :, k]
    return np.sqrt(acc)


def dtw(x, y, dtype=np.float64):
    """dict(dist, steps, D, L, dir, path [steps, 2], gap).  Anti-diagonal by anti-diagonal; the compares are those of the definition."""
    C = cost(x, y, dtype)
    r, c = C.shape
    inf = dtype(np.inf)
    D = np.full((r + 1, c + 1), inf, dtype=dtype)      # D[i+1][j+1] = D(i, j); row / column 0 are the +inf border
    L = np.zeros((r + 1, c + 1), dtype=np.int64)
    dr = np.zeros((r, c), dtype=np.uint8)
    gap = np.full((r, c), np.inf)
    D[1, 1], L[1, 1] = C[0, 0], 1
    for s in range(1, r + c - 1):
        i = np.arange(max(0, s - c + 1), min(r, s + 1))
        j = s - i
        p = np.stack([D[i, j], D[i, j + 1], D[i + 1, j]])         # diagonal, i-1, j-1
        pl = np.stack([L[i, j], L[i, j + 1], L[i + 1, j]])
        best = np.argmin(p, axis=0)                                # the first of equal minima
        cols = np.arange(len(i))
        D[i + 1, j + 1] = C[i, j] + p[best, cols]
        L[i + 1, j + 1] = 1 + pl[best, cols]
        dr[i, j] = best
        srt = np.sort(p.astype(np.float64), axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = (srt[1] - srt[0]) / srt[1]
        gap[i, j] = np.where(np.isfinite(srt[1]), np.where(srt[1] > 0, g, 0.0), np.inf)
    path = [(r - 1, c - 1)]
    while path[-1] != (0, 0):
        i, j = path[-1]
        d = dr[i, j]
        path.append((i - 1, j - 1) if d == 0 else (i - 1, j) if d == 1 else (i, j - 1))
    path = np.array(path[::-1], dtype=np.int64)
    return dict(dist=D[r, c], steps=int(L[r, c]), D=D[1:, 1:], L=L[1:, 1:], dir=dr, path=path, gap=gap, C=C)


def path_min_gap(m):
    """The smallest relative predecessor gap over the cells of the optimal path."""
    return float(m["gap"][m["path"][:, 0], m["path"][:, 1]].min())


def count_ties(m):
    """Cells whose best predecessor is matched exactly by another one."""
    return int((m["gap"] == 0.0).sum())


def dist_rel_bound(lx, ly, K):
    """The derived bound on the fp32 kernel's relative error in D: one rounding per add along a path (at most lx + ly of them), K + 2 for
    a cost (K accumulations, the last subtraction's and the root's)."""
    return (lx + ly + K + 2) * 2.0 ** -24


def zero_fill(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = max(len(x), len(y))
    xp, yp = np.zeros((n, x.shape[1])), np.zeros((n, y.shape[1]))
    xp[:len(x)], yp[:len(y)] = x, y
    return float(np.sqrt(((xp - yp) ** 2).sum(-1)).sum()), n


def mel_mcd(mel_1, mel_2, n_mfcc=39, take_log=False, use_dtw=False):
    """One pair, mels [T1, M] and [T2, M] -> (mcd, penalty, frames)."""
    c1, c2 = mfcc(mel_1, n_mfcc, take_log), mfcc(mel_2, n_mfcc, take_log)
    if use_dtw:
        m = dtw(c1, c2)
        num, frames = float(m["dist"]), m["steps"]
    else:
        num, frames = zero_fill(c1, c2)
    return num / frames, 2.0 - (len(c1) + len(c2)) / frames, frames


def grid_pair(lx, ly, K, grid, offset, seed):
    """x_i = u_i g, y_j = w_j g: integer u, w in [-8, 8], g = GRIDS[grid] placed at `offset` inside K (zeros elsewhere).  Every cost is
    |u_i - w_j| ||g|| exactly.  float32 [lx, K], [ly, K]."""
    g = np.zeros(K)
    gv = GRIDS[grid]
    assert offset + len(gv) <= K
    g[offset:offset + len(gv)] = gv
    rng = np.random.default_rng(seed)
    u, w = rng.integers(-8, 9, lx), rng.integers(-8, 9, ly)
    return (u[:, None] * g[None, :]).astype(np.float32), (w[:, None] * g[None, :]).astype(np.float32)


def real_pair(lx, ly, K, seed, kind="normal"):
    """Seeded float32 [lx, K], [ly, K].  "normal": two independent standard-normal sequences.  "warped": y is x resampled to ly frames
    plus normal noise of 0.3 -- an edit's mel beside the original's, which is what the metric is for."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((lx, K)).astype(np.float32)
    if kind == "normal":
        return x, rng.standard_normal((ly, K)).astype(np.float32)
    idx = np.rint(np.arange(ly) * (lx - 1) / max(ly - 1, 1)).astype(np.int64)
    return x, (x[idx] + 0.3 * rng.standard_normal((ly, K))).astype(np.float32)


E2E_LEN_1, E2E_LEN_2, E2E_M = (120, 97, 64), (97, 120, 64), 80


def e2e_batches(seed=0):
    """Two log-mel-like batches [3, 120, 80] float32 (values around -3 +- 1, as log10-mels are) with the lengths above: both rows of a pair
    are one base sequence of the shorter length, stretched to the row's own length by repeating frames, plus noise of 0.05 (first) and 0.2
    (second).  The stretched side is what makes the margin hold (test_mcd_reference.py): a frame that has NO partner on the other side
    leaves two near-equal ways round it.  Frames at and beyond a row's length are NaN: a read of one shows."""
    rng = np.random.default_rng(seed)
    T = max(E2E_LEN_1 + E2E_LEN_2)
    a = np.full((3, T, E2E_M), np.nan, dtype=np.float32)
    b = np.full((3, T, E2E_M), np.nan, dtype=np.float32)
    for r, (l1, l2) in enumerate(zip(E2E_LEN_1, E2E_LEN_2)):
        n = min(l1, l2)
        base = rng.standard_normal((n, E2E_M)) - 3.0
        i1 = np.rint(np.arange(l1) * (n - 1) / (l1 - 1)).astype(np.int64)
        i2 = np.rint(np.arange(l2) * (n - 1) / (l2 - 1)).astype(np.int64)
        a[r, :l1] = base[i1] + 0.05 * rng.standard_normal((l1, E2E_M))
        b[r, :l2] = base[i2] + 0.2 * rng.standard_normal((l2, E2E_M))
    return a, b


def e2e_rel_tol(mel_1, mel_2, K, use_dtw):
    """(relative tolerance on mcd, the float64 DTW model or None) for one pair [T1, M], [T2, M]: the bound on the distance kernel's own
    error, plus the MFCC bar propagated -- a coefficient off by at most `bar` moves a K-vector by sqrt(K) bar and a cost by twice that,
    so the mean of the costs by at most 2 sqrt(K) bar, relative to that mean (the mcd itself) -- plus the final division's rounding."""
    l1, l2 = len(mel_1), len(mel_2)
    c1, c2 = mfcc(mel_1, K), mfcc(mel_2, K)
    bar = max(mfcc_bar(mel_1, mel_1.shape[1]).max(), mfcc_bar(mel_2, mel_2.shape[1]).max())
    if use_dtw:
        m = dtw(c1, c2)
        return dist_rel_bound(l1, l2, K) + 2.0 * np.sqrt(K) * bar / (m["dist"] / m["steps"]) + 2.0 ** -24, m
    num, n = zero_fill(c1, c2)
    return zero_fill_rel_bound(n, K) + 2.0 * np.sqrt(K) * bar / (num / n) + 2.0 ** -24, None


def mfcc_bar(x, M):
    """The bar on one MFCC coefficient of frame(s) x [..., M] (float64: the mel, or its log10): (M + 2) 2^-24 sum_n |x_n| -- M roundings of
    the FMA chain, one of the table entry, one of x itself where it is a rounded log; |table| <= 1."""
    return (M + 2) * 2.0 ** -24 * np.abs(np.asarray(x, dtype=np.float64)).sum(-1)


def zero_fill_rel_bound(n, K):
    """Relative error of the zero-fill sum in fp32: K + 2 roundings per cost, ceil(n / 256) adds per thread, 8 levels of the tree."""
    return (K + 2 + (n + 255) // 256 + 8) * 2.0 ** -24


def exact_cases():
    """The integer-grid cases, (lx, ly, K, grid, offset, seed): the kernel's strip edges (256 rows: 1, 2, 255, 256, 257, 513), its column
    block and ring edges (64-column blocks, a 320-column ring: 1, 63, 64, 65, 300, 319, 320, 321), each pair in both orientations, K in
    {1, 34, 39, 64} (K = 1 holds the one-element grid (5,)), the 150 x 131 case and 3 x 700 (the ring wraps twice).  A case with a single row or column has no choice to
    make, so no ties; test_mcd_reference.py asserts at least 100 exact ties on every case with both lengths above 32."""
    pairs = [(1, 1), (2, 1), (1, 300), (2, 63), (255, 64), (256, 65), (257, 300), (513, 1), (513, 300), (256, 319), (257, 320), (255, 321),
             (513, 64), (257, 63), (150, 131), (3, 700)]
    ks = [(39, "34", 17), (34, "122", 31), (64, "236", 61), (1, "5", 0), (39, "236", 0), (64, "34", 40)]
    out = []
    for n, (a, b) in enumerate(pairs):
        for m, (lx, ly) in enumerate(((a, b), (b, a)) if a != b else ((a, b),)):
            K, grid, off = ks[(2 * n + m) % len(ks)]
            out.append((lx, ly, K, grid, off, 100 + 2 * n + m))
    return out


# The real-valued tolerance cases, (lx, ly, K, seed, kind); test_mcd_reference.py asserts the margin condition on each.  Independent normal
# sequences hold it at the two small sizes (gaps 2.0e-4 against 4 x bound 3.1e-5 and 6.3e-5); at 257 x 300 none of 150 seeds does (D
# grows with the path while the cost differences do not: best 9.4e-5 against 1.4e-4), so that case is a warped pair (1.3e-2).
REAL_CASES = [(37, 53, 39, 0, "normal"), (130, 97, 34, 1, "normal"), (257, 300, 39, 6, "warped")]
