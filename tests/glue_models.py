"""Numpy models of the small kernels of csrc/glue.hip and csrc/diffusion_ops.hip, one per op, written from the comments next to each kernel
and its prototype in include/set_amd.h.  Integer ops are exact; elementwise float ops repeat the kernel's fp32 operations in its order (the
library is built with -ffp-contract=off, so each operation rounds once and numpy's float32 arithmetic gives the same bits); ops that call a
transcendental are modelled in float64 and compared within a bound.  test_glue_reference.py checks the models against oracle/oracle.py and
the goldens; test_gpu_glue_branches.py checks the kernels against the models."""
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def transpose(x):
    """[B][R][S] -> [B][S][R]"""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)))


def abs_sum_mask(x):
    """[B][C][T] -> [B][T]: 1 where sum_c |x| > 0 (in float64: a denormal counts)."""
    return (np.abs(x.astype(np.float64)).sum(1) > 0).astype(F32)


def embedding_bct(idx, table, scale=1.0, out=None):
    """out[b][c][t] = fl(scale * table[clamp(idx[b][t])][c]), added to `out` with a second rounding when given."""
    rows = np.clip(idx, 0, table.shape[0] - 1)
    v = np.transpose(F32(scale) * table[rows], (0, 2, 1))
    return np.ascontiguousarray(v if out is None else out + v)


def index_mask(idx):
    return (idx > 0).astype(F32)


def expand_states(enc, mel2ph):
    """enc [B][C][T_txt], mel2ph [B][T] -> [B][C][T]: token mel2ph - 1, and 0 where mel2ph is outside 1 .. T_txt."""
    B, C, Tt = enc.shape
    ok = (mel2ph > 0) & (mel2ph <= Tt)
    g = np.take_along_axis(enc, np.broadcast_to(np.where(ok, mel2ph - 1, 0)[:, None, :], (B, C, mel2ph.shape[1])), axis=2)
    return np.where(ok[:, None, :], g, F32(0.0)).astype(F32)


def masked_dur(mel2ph, tmask, txt):
    """Frames per token among the unmasked ones: (1 - mask) is truncated to an integer first (a mask of 0.5 keeps nothing), frames whose
    masked mel2ph is 0 count for nobody, padding tokens (txt == 0) get 0."""
    B, Tt = txt.shape
    keep = (F32(1.0) - tmask.astype(F32)).astype(np.int64)
    m = mel2ph * keep
    out = np.zeros((B, Tt), dtype=np.int64)
    for b in range(B):
        mb = m[b][(m[b] >= 0) & (m[b] <= Tt)]
        out[b] = np.bincount(mb, minlength=Tt + 1)[1:Tt + 1]
    return out * (txt != 0)


def round_dur(dur, txt):
    """round half to even, then integer; 0 on padding tokens"""
    return np.rint(dur.astype(F32)).astype(np.int64) * (txt != 0)


def dur_total(dur, txt):
    return round_dur(dur, txt).sum(1)


def length_regulate(dur, txt):
    """[B][max total]: each 1-based token index repeated its rounded duration; 0 beyond an utterance's total."""
    d = round_dur(dur, txt)
    out = np.zeros((d.shape[0], int(d.sum(1).max())), dtype=np.int64)
    for b in range(d.shape[0]):
        r = np.repeat(np.arange(1, d.shape[1] + 1), d[b])
        out[b, :len(r)] = r
    return out


_EDGES = {}


def pitch_runs():
    """The committed run table of the reference's bin function (tests/golden/pitch_edges.npz): run start bit patterns and their bins."""
    if not _EDGES:
        g = np.load(os.path.join(GOLDEN, "pitch_edges.npz"), allow_pickle=False)
        _EDGES["bits"], _EDGES["bin"] = g["run_bits"], g["run_bin"].astype(np.int64)
    return _EDGES["bits"], _EDGES["bin"]


def pitch_coarse(f0, uv=None, tmask=None, mel2ph_pad=None, uv_from_logit=False):
    """-> (denormalised f0 in float64, bins).  f0 and uv are multiplied by fl(1 - tmask) in fp32; f = clamp(2^f0, 50, 900), 0 where unvoiced
    (uv > 0 after the mask; the raw logit > 0 with uv_from_logit) or where mel2ph_pad == 0; the bin is the run of the masked fp32 f0 (clamped
    to 10.5) when f != 0 and f0 > 5, else the first run's."""
    f0m = f0.astype(F32)
    uvm = None if uv is None else uv.astype(F32)
    if tmask is not None:
        k = F32(1.0) - tmask.astype(F32)
        f0m = f0m * k
        uvm = None if uv is None else uvm * k
    with np.errstate(over="ignore"):  # 2^1e30 = inf, clamped to 900
        f = np.clip(np.exp2(f0m.astype(np.float64)), 50.0, 900.0)
    zero = np.zeros(f0.shape, dtype=bool)
    if uv is not None:
        zero |= (uv > 0) if uv_from_logit else (uvm > 0)
    if mel2ph_pad is not None:
        zero |= mel2ph_pad == 0
    f = np.where(zero, 0.0, f)
    run_bits, run_bin = pitch_runs()
    u = np.minimum(f0m, F32(10.5)).view(np.uint32)
    k = np.searchsorted(run_bits, u, side="right") - 1
    bins = np.where(~zero & (f0m > 5.0), run_bin[np.clip(k, 0, len(run_bin) - 1)], run_bin[0])
    return f, bins.astype(np.int64)


def q_sample(x_start, eps, ab2, nonpad=None):
    """x [B][M][T]: fl(fl(a_b x) + fl(b_b eps)) (* nonpad[b][t])"""
    v = ab2[:, 0, None, None] * x_start + ab2[:, 1, None, None] * eps
    return (v if nonpad is None else v * nonpad[:, None, :]).astype(F32)


def posterior64(x0, x_t, coef4, eps):
    """float64: c1 x0 + c2 x_t + nz exp(lv / 2) eps, coef4 [B or 1][4] = (c1, c2, lv, nz) per batch row"""
    c = coef4.astype(np.float64).reshape(coef4.shape[0], 4, *([1] * (x0.ndim - 1)))
    return c[:, 0] * x0 + c[:, 1] * x_t + c[:, 3] * np.exp(0.5 * c[:, 2]) * eps


def sum_scale(a, b=None, c=None, s=1.0):
    v = a
    if b is not None:
        v = v + b
    if c is not None:
        v = v + c
    return (v / F32(s)).astype(F32)


def blend_mask(a, b, m, inner):
    mm = np.repeat(m.reshape(-1), inner)[:a.size].reshape(a.shape)
    return (a * (F32(1.0) - mm) + b * mm).astype(F32)


def mul_one_minus_mask(x, m, inner):
    mm = np.repeat(m.reshape(-1), inner)[:x.size].reshape(x.shape)
    return (x * (F32(1.0) - mm)).astype(F32)


def sinusoid_embed(t, dim):
    """-> (emb [dim][n] float64, |angle| [dim][n]).  Row j < half: sin(t f_j), row half + j: cos(t f_j), f_j = exp(fl(j * -e)) with the fp32
    scalar e = float32(ln(1e4) / (half - 1)) and the product rounded to fp32, as the kernel documents; everything else in float64."""
    half = dim // 2
    e = F32(9.210340371976184 / (half - 1))
    freq = np.exp((np.arange(half, dtype=F32) * -e).astype(np.float64))
    ang = t.astype(np.float64)[None, :] * freq[:, None]
    return np.concatenate([np.sin(ang), np.cos(ang)], 0), np.abs(np.concatenate([ang, ang], 0))


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
DENORMAL = np.array([1], dtype=np.uint32).view(F32)[0]  # the smallest fp32 denormal


def abs_sum_columns(C, T, seed):
    """x [2][C][T] of random values with special columns in batch row 1 (as far as T allows):
    0 all zero; 1 only the last channel nonzero; 2 .. 5 one nonzero in quarter 0 .. 3 of the channel range in turn; 6 all -0.0;
    7 one denormal.  Returns (x, names of the special columns present)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, C, T)).astype(F32)
    cq = (C + 3) // 4
    special = []
    for t in range(min(T, 8)):
        col = np.zeros(C, dtype=F32)
        if t == 1:
            col[C - 1] = -2.5
        elif 2 <= t <= 5:
            c = min((t - 2) * cq, C - 1)
            col[c] = 3.0 if t % 2 else -3.0
        elif t == 6:
            col[:] = -0.0
        elif t == 7:
            col[C // 2] = DENORMAL
        x[1, :, t] = col
        special.append(t)
    return x, special


def dur_cases(T_txt, seed):
    """dur [3][T_txt] on {0, 0.5, 1.5, 2.5, 3.49, 3.51}, txt [3][T_txt]: row 0 has leading and trailing zero durations and padding tokens
    with nonzero predicted durations; row 1 sums to 0 (padding everywhere but where the duration rounds to 0); row 2 is plain."""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 0.5, 1.5, 2.5, 3.49, 3.51], dtype=F32)
    dur = vals[rng.integers(0, len(vals), (3, T_txt))]
    txt = rng.integers(1, 50, (3, T_txt)).astype(np.int64)
    if T_txt >= 4:
        dur[0, 0], dur[0, -1] = 0.0, 0.5
        txt[0, T_txt // 2] = 0
        dur[0, T_txt // 2] = 3.51
    txt[1] = np.where(dur[1] > 0.5, 0, txt[1])
    return dur, txt
