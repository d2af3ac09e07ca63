"""Float64 models of the discriminator step (csrc/disc_wgrad.hip, set_amd.discriminators with trainable_): every new entry point from
the formulas of include/set_amd.h, the whole step (both discriminators on (y, y_hat), discriminator_loss, the gradient of every
parameter), the float32 mirrors in the documented order of sums, the Python mirror of the slice plan, the case tables of the GPU tests
and the faults the bars must separate.  The forward, the input-gradient chain and the folds are those of mpd_models / msd_models."""
import collections

import numpy as np

import mpd_models as PM
import msd_models as SM
from mpd_models import BAR_FACTOR, INT_X, SLOPE, UNDECIDED_CAP, bar, gate_of, int_array, undecided  # noqa: F401

CHUNK, COLS, MAX_SLICES, FIRST_MAX_SLICES = 32, 128, 64, 64
MIRROR_CU = 256            # the CU count the recorded mirror plans its slices for (an MI355X)
KMAX = 41


def out_len(H, K, s, pad):
    return (H + 2 * pad - K) // s + 1 if H + 2 * pad >= K else 0


# ---- the slice plan -----------------------------------------------------------------------------------------------------------------------
def plan(R, Cin, Cout, groups, H_in, K, s, pad, n_cu):
    """set_gconv1d_wgrad_plan: min(ceil(4 n_cu / tiles), chunks // 8, MAX_SLICES), at least 1."""
    J = R * out_len(H_in, K, s, pad)
    chunks = -(-J // CHUNK)
    tiles = groups * -(-(Cout // groups) // 32) * -(-(Cin // groups) * K // COLS)
    return max(1, min(-(-4 * n_cu // tiles), chunks // 8, MAX_SLICES))


def slice_ranges(J, slices):
    """[(lo, hi)] of the reduction indices of each slice: ceil(chunks / slices) chunks of CHUNK each, the last ones short or empty."""
    chunks = -(-J // CHUNK)
    cps = -(-chunks // slices)
    return [(min(z * cps * CHUNK, J), min((z + 1) * cps * CHUNK, J)) for z in range(slices)]


def first_plan(J, C, n_cu):
    return max(1, min(-(-4 * n_cu // C), J // 4096, FIRST_MAX_SLICES))


# ---- the weight gradient of a grouped strided conv ---------------------------------------------------------------------------------------
def _padded(x, K, s, pad):
    R, Cin, H = x.shape
    xp = np.zeros((R, Cin, H + 2 * pad + s + K), x.dtype)
    xp[:, :, pad:pad + H] = x
    return xp


def gconv_wgrad(dz, x, K, s, pad, groups=1, fault=None, slices=1):
    """dW[co][ci][k] = sum_r sum_h dz[r][co][h] x[r][g Cin/G + ci][s h + k - pad] in the operands' dtype (float64: the model), and
    db[co] = sum dz.  Faults: 'tap' reads one tap further, 'phase' drops the stride, 'last_slice' skips the last non-empty slice of
    `slices`, 'real_rows' leaves the first half of the rows out."""
    R, Cout, Ho = dz.shape
    Cin = x.shape[1]
    assert Ho == out_len(x.shape[2], K, s, pad) and Cin % groups == 0 and Cout % groups == 0
    cig, cog = Cin // groups, Cout // groups
    if fault == "real_rows":
        dz = dz.copy()
        dz[:R // 2] = 0
    if fault == "last_slice":
        lo = [r for r in slice_ranges(R * Ho, slices) if r[1] > r[0]][-1][0]
        flat = np.ascontiguousarray(dz.transpose(0, 2, 1)).reshape(R * Ho, Cout)
        flat[lo:] = 0
        dz = np.ascontiguousarray(flat.reshape(R, Ho, Cout).transpose(0, 2, 1))
    xp = _padded(x, K, s, pad)
    dW = np.zeros((Cout, cig, K), dz.dtype)
    step = 1 if fault == "phase" else s
    for k in range(K):
        k0 = k + 1 if fault == "tap" else k
        win = xp[:, :, k0:k0 + step * (Ho - 1) + 1:step]
        for g in range(groups):
            dW[g * cog:(g + 1) * cog, :, k] = np.einsum("roh,rih->oi", dz[:, g * cog:(g + 1) * cog], win[:, g * cig:(g + 1) * cig])
    return dW, dz.sum(axis=(0, 2))


def gconv_wgrad_mirror(dz, x, K, s, pad, groups=1, slices=1):
    """The float32 mirror in the header's order: per slice one fp32 chain from 0 over j = r H_out + h ascending with unrounded products
    (each step: the float64 sum of the accumulator and the exact product, rounded to float32), the slices added in ascending order.
    db: the float64 sum rounded once (the kernel adds in double)."""
    dz, x = np.asarray(dz, np.float32), np.asarray(x, np.float32)
    R, Cout, Ho = dz.shape
    Cin = x.shape[1]
    cig, cog = Cin // groups, Cout // groups
    xp = _padded(x, K, s, pad).astype(np.float64)
    d64 = dz.astype(np.float64)
    total = None
    for lo, hi in slice_ranges(R * Ho, slices):
        acc = np.zeros((groups, cog, cig, K), np.float32)
        for j in range(lo, hi):
            r, h = divmod(j, Ho)
            a = d64[r, :, h].reshape(groups, cog, 1, 1)
            w = xp[r, :, s * h:s * h + K].reshape(groups, 1, cig, K)
            acc = (acc.astype(np.float64) + a * w).astype(np.float32)
        total = acc if total is None else total + acc
    return total.reshape(Cout, cig, K), d64.sum(axis=(0, 2)).astype(np.float32)


def exact_budget(R, H_out, cig, K):
    """The largest sum of |terms| of any element of an integer case (dW: R H_out terms of at most INT_X^2; db alike with INT_X): below
    2^24 every partial sum is an integer a float32 holds, so any order of summation is exact."""
    return R * H_out * INT_X * INT_X


# ---- the first layers ----------------------------------------------------------------------------------------------------------------------
def fold_wgrad(dz, y, y_hat, p, K, s, pad, fault=None):
    """dW[c][k] = sum over all 2 B p rows of dz[r][c][h] xpad[(s h + k - pad) p + w], db[c] = sum dz (set_mpd_fold_conv_wgrad)."""
    x = np.concatenate([PM.fold(y, p), PM.fold(y_hat, p)]).astype(dz.dtype)        # [2 B p, 1, H]
    dW, db = gconv_wgrad(dz, x, K, s, pad, 1, fault)
    return dW.reshape(dz.shape[1], K), db


def wave_wgrad(dz, wavs, K, pad, fault=None):
    """dW[c][k] = sum_r sum_h dz[r][c][h] wav[r][h + k - pad] over the rows of `wavs` [R, T] (set_wave_conv_wgrad)."""
    dW, db = gconv_wgrad(dz, wavs[:, None, :].astype(dz.dtype), K, 1, pad, 1, fault)
    return dW.reshape(dz.shape[1], K), db


# ---- the backward of the folds -----------------------------------------------------------------------------------------------------------
def wn_fold_bwd(dW, g, v, fault=None):
    """w = g v / |v| per row -> dg = <dW, v> / n, dv = (g / n) (dW - v <dW, v> / n^2).  Fault 'proj': the v <dW, v> term is missing."""
    n0 = v.shape[0]
    v2, d2 = v.reshape(n0, -1), dW.reshape(n0, -1)
    n = np.sqrt((v2 * v2).sum(1))
    dot = (d2 * v2).sum(1)
    proj = 0 if fault == "proj" else v2 * (dot / n ** 2)[:, None]
    return (dot / n).reshape(g.shape), ((g.reshape(-1) / n)[:, None] * (d2 - proj)).reshape(v.shape)


def sn_fold_bwd(dW, W_orig, u, v, fault=None):
    """W = W_orig / sigma, sigma = u^T mat(W_orig) v, u and v constants -> d W_orig = (dW - <dW, W_orig / sigma> u v^T) / sigma.
    Fault 'sigma_const': sigma treated as a constant (dW / sigma)."""
    n0 = W_orig.shape[0]
    sigma = SM.sn_sigma(W_orig, u, v)
    d2 = dW.reshape(n0, -1)
    tot = 0 if fault == "sigma_const" else (d2 * W_orig.reshape(n0, -1)).sum() / sigma
    return ((d2 - tot * np.outer(u, v)) / sigma).reshape(W_orig.shape)


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32)


# ---- the whole step ------------------------------------------------------------------------------------------------------------------------
def _wgrad_fn(mirror, n_cu=MIRROR_CU):
    if not mirror:
        return lambda dz, x, K, s, pad, G: gconv_wgrad(dz, x, K, s, pad, G)

    def run(dz, x, K, s, pad, G):
        R, Cout, _Ho = dz.shape
        return gconv_wgrad_mirror(dz, x, K, s, pad, G, plan(R, x.shape[1], Cout, G, x.shape[2], K, s, pad, n_cu))
    return run


def _gates_all(maps, slope):
    return [gate_of(m, slope) for m in maps[:-1]]


def mpd_step(fw, state, y, y_hat, u_r=1.0, u_f=1.0, gates=None, fault=None):
    """{key: gradient of u_r r_loss + u_f g_loss} for every parameter of the MPD, from a forward `fw` of PM.mpd_forward (float64: the
    model; float32 with chain: the mirror, whose sums take the kernels' order).  `gates`: per period the five gate arrays over ALL rows
    to use instead of the forward's own.  Fault 'real_rows': the real rows' score gradient is left out."""
    dtype, B, D = fw["dtype"], fw["B"], len(PM.PERIODS)
    mirror = dtype == np.float32
    wgrad = _wgrad_fn(mirror)
    cast = (lambda a: _r32(a)) if mirror else (lambda a: a)
    out = collections.OrderedDict()
    for i, p in enumerate(PM.PERIODS):
        layers, maps = fw["layers"][i], fw["maps"][i]
        Rg = B * p
        gts = _gates_all(maps, fw["slope"]) if gates is None else [g.astype(dtype) for g in gates[i]]
        last = maps[5]
        dz = np.empty_like(last)
        n = dtype(last[:Rg].size)
        dz[:Rg] = dtype(0.0 if fault == "real_rows" else u_r / D) * 2 * (last[:Rg] - 1) / n
        dz[Rg:] = dtype(u_f / D) * 2 * last[Rg:] / n
        grads = [None] * 6
        for j in range(5, 0, -1):
            L = layers[j]
            grads[j] = wgrad(dz, maps[j - 1], L.W.shape[2], L.s, L.pad, 1)
            dz = PM.dgrad_rows(dz, L.W, maps[j - 1].shape[2], L.s, L.pad, gate=gts[j - 1], add=None, chain=fw["chain"])
        L = layers[0]
        dW0, db0 = fold_wgrad(dz.astype(np.float64), y, y_hat, p, L.W.shape[2], L.s, L.pad)
        grads[0] = (cast(dW0).reshape(L.W.shape), cast(db0))
        for j, (dW, db) in enumerate(grads):
            pre = "discriminators.%d.%s." % (i, "convs.%d" % j if j < 5 else "conv_post")
            g, v = state[pre + "weight_g"], state[pre + "weight_v"]
            dg, dv = wn_fold_bwd(dW.astype(np.float64).reshape(v.shape), g.astype(np.float64), v.astype(np.float64))
            out[pre + "bias"], out[pre + "weight_g"], out[pre + "weight_v"] = db, cast(dg), cast(dv)
    return out


def _msd_chain(layers, maps, wavs, dz, gts, wgrad, chain, cast):
    """[(dW, db)] of one chain of a DiscriminatorS over the rows of `maps` / `wavs`."""
    n = len(layers)
    grads = [None] * n
    for j in range(n - 1, 0, -1):
        L = layers[j]
        grads[j] = wgrad(dz, maps[j - 1], L.W.shape[2], L.s, L.pad, L.groups)
        dz = SM.gdgrad_rows(dz, L.W, maps[j - 1].shape[2], L.s, L.pad, L.groups, gate=gts[j - 1], add=None, chain=chain)
    L = layers[0]
    dW0, db0 = wave_wgrad(dz.astype(np.float64), wavs, L.W.shape[2], L.pad)
    grads[0] = (cast(dW0).reshape(L.W.shape), cast(db0))
    return grads


def msd_step(fw, state, y, y_hat, groups, train, u_r=1.0, u_f=1.0, gates=None, fault=None):
    """As mpd_step for the MSD, from a forward of SM.msd_forward.  `gates`: per scale (the seven gate arrays of the real rows, those of
    the generated rows).  The spectrally normed scale in train() ran its halves with different weights and u, v: its chain, weight
    gradients and back-projections run per half and weight_orig's gradient is their sum, the real half's first; otherwise one chain runs
    over all rows.  Faults: 'real_rows', 'sigma_const'."""
    dtype, B, D = fw["dtype"], fw["B"], SM.N_SCALES
    mirror = dtype == np.float32
    wgrad = _wgrad_fn(mirror)
    cast = (lambda a: _r32(a)) if mirror else (lambda a: a)
    out = collections.OrderedDict()
    yy, yh = y.astype(dtype), y_hat.astype(dtype)
    for i in range(D):
        if i:
            yy, yh = SM.pool(yy), SM.pool(yh)
        lr, lg, _after = SM.layers_of(state, i, dtype, groups, train)
        real, gen = fw["real"][i], fw["gen"][i]
        g_r, g_g = ([gate_of(m, fw["slope"]) for m in real[:7]], [gate_of(m, fw["slope"]) for m in gen[:7]]) if gates is None else \
            ([g.astype(dtype) for g in gates[i][0]], [g.astype(dtype) for g in gates[i][1]])
        n = dtype(real[7].size)
        dz_r = dtype(0.0 if fault == "real_rows" else u_r / D) * 2 * (real[7] - 1) / n
        dz_g = dtype(u_f / D) * 2 * gen[7] / n
        halves = i == 0 and train
        if halves:
            runs = [_msd_chain(lr, real, yy, dz_r, g_r, wgrad, fw["chain"], cast), _msd_chain(lg, gen, yh, dz_g, g_g, wgrad, fw["chain"], cast)]
        else:
            both = [np.concatenate([a, b]) for a, b in zip(real, gen)]
            runs = [_msd_chain(lg, both, np.concatenate([yy, yh]), np.concatenate([dz_r, dz_g]), [np.concatenate([a, b]) for a, b in zip(g_r, g_g)],
                               wgrad, fw["chain"], cast)]
        for j in range(8):
            pre = SM._pre(i, j)
            db = runs[0][j][1] if len(runs) == 1 else runs[0][j][1] + runs[1][j][1]
            out[pre + "bias"] = db
            if i == 0:
                W = state[pre + "weight_orig"].astype(np.float64)
                u, v = state[pre + "weight_u"].astype(np.float64), state[pre + "weight_v"].astype(np.float64)
                tot = None
                for run in runs:                     # train: the real half after one power iteration, the generated half after two
                    if train:
                        u, v = SM.sn_iterate(W, u, v)
                    d = cast(sn_fold_bwd(run[j][0].astype(np.float64), W, u, v, fault))
                    tot = d if tot is None else tot + d
                out[pre + "weight_orig"] = tot
            else:
                g, v = state[pre + "weight_g"], state[pre + "weight_v"]
                dg, dv = wn_fold_bwd(runs[0][j][0].astype(np.float64), g.astype(np.float64), v.astype(np.float64))
                out[pre + "weight_g"], out[pre + "weight_v"] = cast(dg), cast(dv)
    return out


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
WGRAD_TRIPLES = ((1, 8, 1), (8, 20, 1), (33, 72, 1), (128, 32, 1), (8, 16, 3), (16, 32, 2), (33, 17, 2), (72, 1, 1))   # (Cin/G, Cout/G, G)
WGRAD_KS = (1, 3, 5, 41)
WGRAD_SLICES = (0, 1, 2, 5)


def wgrad_cases():
    """[(cig, cog, G, K, s, pad, H_in, R, slices, accumulate, db)]: every stride x kernel x pad in {0, (K - 1) / 2}; per combination
    the lengths whose R H_out falls one under, on and one over a reduction chunk (and two chunks), lengths with (H_in + 2 pad - K) % s
    != 0, and rows of 1 - 10 frames of which several share a chunk; the triples, R in {1, 3}, the slice counts and the two flags dealt
    round so that every value of every column meets every stride and every kernel."""
    cases, n = [], 0
    for s in (1, 2, 3, 4):
        for K in WGRAD_KS:
            for pad in sorted({0, (K - 1) // 2}):
                houts = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 11, 1 + n % 10]
                for m, ho in enumerate(houts):
                    R = 3 if ho <= 11 or (n + m) % 2 else 1
                    if ho in (CHUNK - 1, CHUNK, CHUNK + 1) and R == 3:        # R H_out around a chunk: 3 rows of about a third
                        ho = {CHUNK - 1: 10, CHUNK: 11, CHUNK + 1: 11}[ho]
                    H = s * (ho - 1) + K - 2 * pad + (m % s)                  # m % s != 0: the last frames feed no output
                    if H < 1 or out_len(H, K, s, pad) < 1:
                        continue
                    cig, cog, G = WGRAD_TRIPLES[n % len(WGRAD_TRIPLES)]
                    cases.append((cig, cog, G, K, s, pad, H, R, WGRAD_SLICES[(n // 2) % 4], bool(n % 2), bool((n // 3) % 2)))
                    n += 1
    return cases


MPD_PAIRS = ((32, 128, 1, 5, 3), (128, 512, 1, 5, 3), (512, 1024, 1, 5, 3), (1024, 1024, 1, 5, 1), (1024, 1, 1, 3, 1))   # (Cin, Cout, G, K, s)
MSD_PAIRS = tuple((cin, cout, g, 41, s) for cin, cout, g, s in SM.MSD_LAYER_SHAPES)
FIRST_T = (23, 64, 97, 200)

# ---- end-to-end cases ----------------------------------------------------------------------------------------------------------------------
U_PAIRS = ((1.0, 1.0), (0.5, 3.0))                   # upstream of (r_loss, f_loss)
MSD_NARROW, MSD_NARROW_GROUPS = SM.NARROW, SM.NARROW_GROUPS
E2E = collections.OrderedDict([                      # id -> (kind, B, T, train, weight seed, waveform seed)
    ("mpd_1024", ("mpd", 2, 1024, False, 61, 71)),
    ("mpd_333", ("mpd", 2, 333, False, 62, 72)),
    ("msd_1024_eval", ("msd", 2, 1024, False, 63, 73)),
    ("msd_333_eval", ("msd", 2, 333, False, 64, 74)),
    ("msd_1024_train", ("msd", 2, 1024, True, 63, 73)),
    ("msd_333_train", ("msd", 2, 333, True, 64, 74)),
])
_CACHE = {}


def e2e_inputs(case):
    kind, B, T, _train, sw, sy = E2E[case]
    y, y_hat = PM.waves(sy, B, T)
    state = PM.seeded_state(sw, PM.NARROW) if kind == "mpd" else SM.seeded_state(sw, MSD_NARROW, MSD_NARROW_GROUPS)
    return PM.state_numpy(state), y, y_hat


def e2e_forward(case, dtype=np.float64):
    """The forward of a case in `dtype` (float32: the chained mirror), computed once per process."""
    key = (case, np.dtype(dtype).name)
    if key not in _CACHE:
        kind, _B, _T, train, _sw, _sy = E2E[case]
        state, y, y_hat = e2e_inputs(case)
        chain = dtype == np.float32
        _CACHE[key] = PM.mpd_forward(y, y_hat, state, dtype=dtype, chain=chain) if kind == "mpd" else \
            SM.msd_forward(y, y_hat, state, MSD_NARROW_GROUPS, train, dtype=dtype, chain=chain)
    return _CACHE[key]


def e2e_step(fw, case, u_r=1.0, u_f=1.0, gates=None, fault=None):
    kind, _B, _T, train, _sw, _sy = E2E[case]
    state, y, y_hat = e2e_inputs(case)
    if kind == "mpd":
        return mpd_step(fw, state, y, y_hat, u_r, u_f, gates, fault)
    return msd_step(fw, state, y, y_hat, MSD_NARROW_GROUPS, train, u_r, u_f, gates, fault)


def gate_operands(fw, case):
    """(real, generated): the lists of gate operands (every map but the last, per sub-discriminator) of a forward."""
    if E2E[case][0] == "mpd":
        B = fw["B"]
        real = [m[:B * p] for p, maps in zip(PM.PERIODS, fw["maps"]) for m in maps[:5]]
        gen = [m[B * p:] for p, maps in zip(PM.PERIODS, fw["maps"]) for m in maps[:5]]
        return real, gen
    return [m for maps in fw["real"] for m in maps[:7]], [m for maps in fw["gen"] for m in maps[:7]]


def model_gates(fw, case):
    """The model's own gate arrays in the shape mpd_step / msd_step take them."""
    if E2E[case][0] == "mpd":
        return [_gates_all(maps, fw["slope"]) for maps in fw["maps"]]
    return [([gate_of(m, fw["slope"]) for m in r[:7]], [gate_of(m, fw["slope"]) for m in g[:7]]) for r, g in zip(fw["real"], fw["gen"])]


def mirror_errors(case):
    """What the end-to-end GPU test needs of the float32 mirror: per parameter and upstream pair the largest error of the mirror's
    gradient (evaluated with the MODEL's gate decisions) against the model's, the errors of the two losses, and the share of undecided
    gate entries of the real and of the generated rows.  tools/make_disc_step_golden.py records it as tests/golden/disc_step_bars.npz."""
    fw, mi = e2e_forward(case), e2e_forward(case, np.float32)
    gates = model_gates(fw, case)
    out = {}
    of_r, of_f = e2e_step(fw, case, 1.0, 0.0), e2e_step(fw, case, 0.0, 1.0)
    for n, (u_r, u_f) in enumerate(U_PAIRS):
        want, got = e2e_step(fw, case, u_r, u_f), e2e_step(mi, case, u_r, u_f, gates=gates)
        out["grads%d" % n] = np.asarray([np.abs(np.asarray(got[k], np.float64) - want[k]).max() for k in want])
        # the gradient's magnitude before the two losses' shares cancel (conv_post's bias of period 11 at u = (0.5, 3): -0.170 of r_loss + 0.177 of f_loss)
        out["scales%d" % n] = np.asarray([abs(u_r) * np.abs(of_r[k]).max() + abs(u_f) * np.abs(of_f[k]).max() for k in want])
    out["losses"] = np.asarray([abs(float(mi[k]) - float(fw[k])) for k in ("disc_r_loss", "disc_g_loss")])
    (r64, g64), (r32, g32) = gate_operands(fw, case), gate_operands(mi, case)
    share = lambda us: sum(int(u.sum()) for u in us) / float(sum(u.size for u in us))  # noqa: E731
    out["undecided"] = np.asarray([share(undecided(r64, r32)), share(undecided(g64, g32))])
    return out


# ---- the recorded reference run (tools/make_disc_step_golden.py; tests/golden/disc_step_reference.npz) ---------------------------------
GOLDEN_B, GOLDEN_T, GOLDEN_ENTRIES = 2, 333, 16
GOLDEN_RUNS = (("mpd", "mpd", False, 81, 91), ("msd_eval", "msd", False, 82, 92), ("msd_train", "msd", True, 82, 92))   # id, kind, train, seeds


def golden_positions(key, numel):
    """The seeded flat positions of a parameter's recorded entries."""
    return np.random.default_rng(sum(key.encode()) + numel).integers(0, numel, size=GOLDEN_ENTRIES)


def golden_stats(key, grad):
    """What is recorded of a gradient: its sum, its L2 norm and GOLDEN_ENTRIES entries."""
    g = np.asarray(grad, np.float64).reshape(-1)
    return np.concatenate([[g.sum(), np.sqrt((g * g).sum())], g[golden_positions(key, g.size)]])


def golden_inputs(run):
    """(state dict of float32 torch tensors at full size, y, y_hat) of a recorded run."""
    _name, kind, _train, sw, sy = run
    y, y_hat = PM.waves(sy, GOLDEN_B, GOLDEN_T)
    return (PM.seeded_state(sw) if kind == "mpd" else SM.seeded_state(sw)), y, y_hat


def golden_model(run):
    """({key: golden_stats of the model's gradient of r_loss + f_loss}, (r_loss, f_loss)) of a recorded run, from the float64 model with
    the reference's slope (the double 0.1; the kernels hold its float32 rounding)."""
    _name, kind, train, _sw, _sy = run
    state, y, y_hat = golden_inputs(run)
    state = PM.state_numpy(state)
    if kind == "mpd":
        fw = PM.mpd_forward(y, y_hat, state, slope=0.1)
        grads = mpd_step(fw, state, y, y_hat)
    else:
        fw = SM.msd_forward(y, y_hat, state, SM.FULL_GROUPS, train, slope=0.1)
        grads = msd_step(fw, state, y, y_hat, SM.FULL_GROUPS, train)
    return {k: golden_stats(k, g) for k, g in grads.items()}, (float(fw["disc_r_loss"]), float(fw["disc_g_loss"]))


def grad_bars(bars, n):
    """The bar of every parameter's gradient for upstream pair n, in the step models' key order: BAR_FACTOR x the larger of the
    mirror's largest error over the parameter and (the rms, over the net's parameters, of that error relative to the gradient's
    magnitude) x the parameter's magnitude, the magnitude being |u_r| max |d r_loss| + |u_f| max |d f_loss|: what the rounding errors
    scale with, where the two losses' shares nearly cancel in the sum.  The second term is the rule of `undecided` carried over to parameters: every
    gradient of a net comes out of the same chains, so the relative errors are draws of one distribution; a weight tensor's maximum is
    taken over thousands of draws, the one of conv_post's scalar weight_g or bias over a single draw that is as often small as not
    (recorded relative errors run from 5e-9 to 1e-6 in one net), and the kernel's rounding there is another draw of the same scale."""
    err, scale = bars["grads%d" % n], bars["scales%d" % n]
    rms = np.sqrt(((err / scale) ** 2).mean())
    return BAR_FACTOR * np.maximum(err, rms * scale)


def load_bars(case):
    """The recorded mirror errors of a case (tests/golden/disc_step_bars.npz)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_step_bars.npz"))
    return {k[len(case) + 1:]: g[k] for k in g.files if k.startswith(case + ".")}
