"""Float64 model of the multi-scale discriminator as the generator step uses it -- the grouped convs and their input gradient, the first
layer on the waveforms, the 4 / 2 average pool, spectral norm with its power iterations, the three scales and every gradient -- written
from the formulas of include/set_amd.h, its float32 mirror, and the case tables of the MSD tests.

As tests/mpd_models.py: every function works in the dtype of its operands; the model (float64) sums with matmul, the mirror
(`chain=True`, float32) takes its products one at a time in the kernels' documented order (16-channel chunk of the group, tap, channel),
then bias / add, then the activation or gate.  BAR_FACTOR times the mirror's largest error is the bar of the non-exact GPU tests;
`undecided`, the list losses and their model are mpd_models' own.
"""
import collections

import numpy as np

from mpd_models import (BAR_FACTOR, INT_SLOPE, INT_W, INT_X, KC, L1, LAMBDA_ADV, SLOPE, SQ0, SQ1, U_PAIRS, UNDECIDED_CAP, bar, gate_of,  # noqa: F401
                        int_array, multi_loss, multi_loss_grad, out_len, sign_of, state_numpy, undecided, waves)

assert BAR_FACTOR == 4 and UNDECIDED_CAP == 1e-3
KERNELS = (15, 41, 41, 41, 41, 41, 5, 3)
STRIDES = (1, 2, 2, 4, 4, 1, 1, 1)
PADS = (7, 20, 20, 20, 20, 20, 2, 1)
FULL = (128, 128, 256, 512, 1024, 1024, 1024)
FULL_GROUPS = (1, 4, 16, 16, 16, 16, 1)
NARROW = (12, 12, 24, 40, 40, 40, 20)
NARROW_GROUPS = (1, 4, 4, 4, 4, 4, 1)
N_SCALES = 3
EPS = 1e-12
GCONV_KMAX, WAVE_KMAX = 41, 15
GCONV_TILES = (128, 64)         # frames per block by the 32-row blocks of a group: one, more (set_gconv1d_tile)


def tile_of(rows_per_group):
    rbn = -(-rows_per_group // 32)
    return GCONV_TILES[0] if rbn == 1 else GCONV_TILES[1]


def _lrelu(v, slope):
    return np.where(v > 0, v, v * v.dtype.type(slope))


# ---- grouped conv -----------------------------------------------------------------------------------------------------------------------
def gconv_rows(x, W, bias, s, pad, groups=1, slope=None, chain=False, group_shift=0, reverse_taps=False):
    """out[r][co][h] = act(bias[co] + sum_{ci of co's group} sum_k W[co][ci][k] x[r][g Cin/G + ci][s h + k - pad]); x [R, Cin, H],
    W [Cout, Cin / G, K].  `group_shift`, `reverse_taps`: planted faults for the tests (output group g reads input group g + shift;
    the taps run backwards)."""
    R, Cin, H = x.shape
    Cout, cig, K = W.shape
    G = groups
    cog = Cout // G
    assert Cin == cig * G and Cout == cog * G
    Ho = out_len(H, K, s, pad)
    assert Ho >= 1
    xp = np.zeros((R, Cin, H + 2 * pad + s), x.dtype)
    xp[:, :, pad:pad + H] = x
    xg = xp.reshape(R, G, cig, -1)
    if group_shift:
        xg = np.roll(xg, -group_shift, axis=1)
    Wg = W.reshape(G, cog, cig, K)
    if reverse_taps:
        Wg = Wg[..., ::-1]
    acc = np.zeros((R, G, cog, Ho), x.dtype)
    for c0 in range(0, cig, KC) if chain else (0,):
        for k in range(K):
            seg = xg[:, :, :, k:k + s * (Ho - 1) + 1:s]                                     # [R, G, cig, Ho]
            if chain:
                for ci in range(c0, min(c0 + KC, cig)):
                    acc = acc + Wg[None, :, :, ci, k, None] * seg[:, :, None, ci, :]
            else:
                acc = acc + np.matmul(np.ascontiguousarray(Wg[None, :, :, :, k]), np.ascontiguousarray(seg))
    acc = acc.reshape(R, Cout, Ho)
    if bias is not None:
        acc = acc + bias[None, :, None]
    return acc if slope is None else _lrelu(acc, slope)


def gdgrad_rows(dz, W, H_in, s, pad, groups=1, gate=None, add=None, chain=False):
    """dz_in[r][ci][j] = gate (add + sum_{co of ci's group} sum_k W[co][ci][k] dz[r][co][(j + pad - k) / s]) over the k that hit an output
    frame; `gate`: the array of gate VALUES or None.  The chain runs over (16-channel chunk of the group's co, tap, co)."""
    R, Cout, Ho = dz.shape
    _, cig, K = W.shape
    G = groups
    cog = Cout // G
    assert Ho == out_len(H_in, K, s, pad)
    Wg = W.reshape(G, cog, cig, K)
    dg = dz.reshape(R, G, cog, Ho)
    gp = np.zeros((R, G, cig, H_in + 2 * pad + s), dz.dtype)
    for c0 in range(0, cog, KC) if chain else (0,):
        for k in range(K):
            sl = slice(k, k + s * (Ho - 1) + 1, s)
            if chain:
                for co in range(c0, min(c0 + KC, cog)):
                    gp[:, :, :, sl] += Wg[None, :, co, :, k, None] * dg[:, :, None, co, :]
            else:
                gp[:, :, :, sl] += np.matmul(np.ascontiguousarray(Wg[None, :, :, :, k].transpose(0, 1, 3, 2)), np.ascontiguousarray(dg))
    g = gp[:, :, :, pad:pad + H_in].reshape(R, G * cig, H_in)
    if add is not None:
        g = g + add
    return g if gate is None else g * gate


# ---- the first layer on the waveforms ---------------------------------------------------------------------------------------------------
def wave_conv(wavs, W, bias, pad, slope=None, chain=False):
    """wavs [R, T] -> [R, C, T]; W [C, 1, K]; one chain over k ascending."""
    return gconv_rows(wavs[:, None, :], W, bias, 1, pad, 1, slope, chain)


def wave_conv_bwd(dz, W, pad, chain=False):
    """dz [B, C, T] -> g_wav [B, T]: the chain runs over c ascending and, inside it, k ascending."""
    B, Cc, T = dz.shape
    K = W.shape[2]
    if not chain:
        return gdgrad_rows(dz, W, T, 1, pad)[:, 0]
    dp = np.zeros((B, Cc, T + 2 * K), dz.dtype)
    dp[:, :, K:K + T] = dz
    acc = np.zeros((B, T), dz.dtype)
    for c in range(Cc):
        for k in range(K):
            off = K + pad - k
            acc = acc + W[c, 0, k] * dp[:, c, off:off + T]
    return acc


# ---- the pool ---------------------------------------------------------------------------------------------------------------------------
def pool_len(T):
    return (T - 2) // 2 + 1 if T >= 2 else 0


def pool(x, edge_count=False):
    """AvgPool1d(4, 2, padding=1) on [B, T]: 0.25 (((x[2j-1] + x[2j]) + x[2j+1]) + x[2j+2]), zeros outside.  `edge_count`: the planted
    fault of dividing by the in-range count."""
    B, T = x.shape
    To = pool_len(T)
    xp = np.zeros((B, 2 * To + 2), x.dtype)
    n = min(T, 2 * To + 1)
    xp[:, 1:1 + n] = x[:, :n]
    v = [xp[:, u:u + 2 * To:2] for u in range(4)]
    tot = ((v[0] + v[1]) + v[2]) + v[3]
    if edge_count:
        j = np.arange(To)
        cnt = sum(((2 * j - 1 + u >= 0) & (2 * j - 1 + u < T)).astype(x.dtype) for u in range(4))
        return tot / cnt
    return x.dtype.type(0.25) * tot


def pool_bwd(g_out, T, add=None):
    """g_in[i] = add[i] + (0.25 g_out[lo] + 0.25 g_out[hi]), lo = (i + 1) // 2 - 1, hi = lo + 1, a term outside an exact 0."""
    B, To = g_out.shape
    assert To == pool_len(T)
    i = np.arange(T)
    lo = (i + 1) // 2 - 1
    hi = lo + 1
    q = g_out.dtype.type(0.25)
    gl = np.where((lo >= 0) & (lo < To), q * g_out[:, np.clip(lo, 0, To - 1)], 0)
    gh = np.where(hi < To, q * g_out[:, np.clip(hi, 0, To - 1)], 0)
    s = (gl + gh).astype(g_out.dtype)
    return s if add is None else add + s


# ---- weight norm, spectral norm ---------------------------------------------------------------------------------------------------------
def wn_fold(g, v):
    n = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1, dtype=v.dtype))
    return v * (g.reshape(-1) / n).reshape(-1, 1, 1)


def sn_iterate(W, u, v):
    """One power iteration of torch.nn.utils.spectral_norm: v = normalize(mat(W)^T u), u = normalize(mat(W) v), eps = 1e-12."""
    m = W.reshape(W.shape[0], -1)
    v = m.T @ u
    v = v / max(np.sqrt((v * v).sum(dtype=W.dtype)), W.dtype.type(EPS))
    u = m @ v
    u = u / max(np.sqrt((u * u).sum(dtype=W.dtype)), W.dtype.type(EPS))
    return u, v


def sn_sigma(W, u, v):
    return u @ (W.reshape(W.shape[0], -1) @ v)


def sn_fold(W, u, v):
    return W / sn_sigma(W, u, v)


# ---- one discriminator ------------------------------------------------------------------------------------------------------------------
Layer = collections.namedtuple("Layer", "W b s pad groups act")


def _pre(i, j):
    return "discriminators.%d.%s." % (i, "convs.%d" % j if j < 7 else "conv_post")


def layers_of(state, i, dtype, groups, train=False, gen_uses_real_sigma=False):
    """(layers for the real rows, layers for the generated rows, {key: u / v after the forward}) of discriminator i from a state dict
    with the reference's key names.  Discriminator 0 is spectrally normed: in eval both halves use weight_orig / sigma of the stored
    u, v; in train the real rows see the weights after one power iteration and the generated rows those after two.
    `gen_uses_real_sigma`: the planted fault."""
    real, gen, after = [], [], {}
    for j in range(8):
        pre = _pre(i, j)
        g = 1 if j == 7 else groups[j]
        b = state[pre + "bias"].astype(dtype)
        mk = lambda W: Layer(W, b, STRIDES[j], PADS[j], g, j < 7)  # noqa: E731
        if i == 0:
            W = state[pre + "weight_orig"].astype(dtype)
            u, v = state[pre + "weight_u"].astype(dtype), state[pre + "weight_v"].astype(dtype)
            if train:
                u, v = sn_iterate(W, u, v)
                Wr = sn_fold(W, u, v)
                u, v = sn_iterate(W, u, v)
                Wg = Wr if gen_uses_real_sigma else sn_fold(W, u, v)
            else:
                Wr = Wg = sn_fold(W, u, v)
            after[pre + "weight_u"], after[pre + "weight_v"] = u, v
            real.append(mk(Wr))
            gen.append(mk(Wg))
        else:
            W = wn_fold(state[pre + "weight_g"].astype(dtype), state[pre + "weight_v"].astype(dtype))
            real.append(mk(W))
            gen.append(mk(W))
    return real, gen, after


def disc_forward(wav, layers, slope=SLOPE, chain=False, faults=None):
    """The eight maps [B, C, H] of one signal [B, T]."""
    faults = faults or {}
    L = layers[0]
    x = wave_conv(wav, L.W, L.b, L.pad, slope if L.act else None, chain)
    maps = [x]
    for L in layers[1:]:
        kw = {}
        if L.groups > 1:
            kw = dict(group_shift=faults.get("group_shift", 0), reverse_taps=faults.get("reverse_taps", False))
        pad = faults.get("pad", L.pad) if L.W.shape[2] == 41 else L.pad
        if pad != L.pad:                       # a planted pad changes the lengths: keep them by trimming / padding at the end
            Ho = out_len(x.shape[2], L.W.shape[2], L.s, L.pad)
            out = np.zeros((x.shape[0], L.W.shape[0], Ho), x.dtype)
            if out_len(x.shape[2], L.W.shape[2], L.s, pad) >= 1:
                full = gconv_rows(x, L.W, L.b, L.s, pad, L.groups, slope if L.act else None, chain, **kw)
                out[:, :, :min(Ho, full.shape[2])] = full[:, :, :Ho]
            x = out
        else:
            x = gconv_rows(x, L.W, L.b, L.s, L.pad, L.groups, slope if L.act else None, chain, **kw)
        maps.append(x)
    return maps


def disc_backward(gen_maps, layers, g_maps, gates=None, slope=SLOPE, chain=False):
    """d / d wav [B, T] from the gradients arriving at the eight generated maps; `gates`: the seven arrays of gate values."""
    if gates is None:
        gates = [gate_of(f, slope) for f in gen_maps[:7]]
    dz = g_maps[7]
    for i in range(7, 0, -1):
        L = layers[i]
        dz = gdgrad_rows(dz, L.W, gen_maps[i - 1].shape[2], L.s, L.pad, L.groups, gate=gates[i - 1], add=g_maps[i - 1], chain=chain)
    return wave_conv_bwd(dz, layers[0].W, layers[0].pad, chain=chain)


# ---- the generator-side step ------------------------------------------------------------------------------------------------------------
def msd_forward(y, y_hat, state, groups=FULL_GROUPS, train=False, dtype=np.float64, chain=False, slope=SLOPE, faults=None):
    """The forward of the three scales in `dtype`: per scale the generated rows' layers, the real and generated maps, scores, decisions
    (gate values of maps 1..7, signs of g - r of maps 1..8) and their operands, the buffers after the forward, and the four losses."""
    faults = faults or {}
    y, y_hat = y.astype(dtype), y_hat.astype(dtype)
    out = dict(B=y.shape[0], T=y.shape[1], dtype=dtype, chain=chain, slope=slope, layers=[], real=[], gen=[], scores_r=[], scores_g=[], gates=[],
               signs=[], gate_ops=[], sign_ops=[], lengths=[], after={})
    gl, fl, dr, dg = dtype(0), dtype(0), dtype(0), dtype(0)
    for i in range(N_SCALES):
        if i:
            y, y_hat = pool(y, faults.get("edge_count", False)), pool(y_hat, faults.get("edge_count", False))
        lr, lg, after = layers_of(state, i, dtype, groups, train, faults.get("gen_uses_real_sigma", False))
        real, gen = disc_forward(y, lr, slope, chain, faults), disc_forward(y_hat, lg, slope, chain, faults)
        out["after"].update(after)
        out["lengths"].append(y.shape[1])
        out["layers"].append(lg)
        out["real"].append(real)
        out["gen"].append(gen)
        out["scores_r"].append(real[7].reshape(real[7].shape[0], -1))
        out["scores_g"].append(gen[7].reshape(gen[7].shape[0], -1))
        gate0 = faults.get("gate0")
        out["gates"].append([gate_of(f, slope) if gate0 is None else np.where(f == 0, f.dtype.type(gate0), gate_of(f, slope)) for f in gen[:7]])
        out["signs"].append([sign_of(g, r) for g, r in zip(gen, real)])
        out["gate_ops"].append(gen[:7])
        out["sign_ops"].append([g - r for g, r in zip(gen, real)])
        gl = gl + ((1 - gen[7]) ** 2).mean(dtype=dtype)
        dr = dr + ((1 - real[7]) ** 2).mean(dtype=dtype)
        dg = dg + (gen[7] ** 2).mean(dtype=dtype)
        for r, g in zip(real, gen):
            fl = fl + np.abs(r - g).mean(dtype=dtype)
    out.update(gen_loss=gl / N_SCALES, fm_loss=fl * 2, disc_r_loss=dr / N_SCALES, disc_g_loss=dg / N_SCALES)
    return out


def scale_grads(fw, u_adv, u_fm, decisions=None, score_only=False, maps_only=False):
    """Per scale d (u_adv gen + u_fm fm) / d (that scale's generated waveform)."""
    dtype = fw["dtype"]
    out = []
    for i in range(N_SCALES):
        gates, signs = (fw["gates"][i], fw["signs"][i]) if decisions is None else decisions[i]
        gates = [g.astype(dtype) for g in gates]
        g8 = fw["gen"][i][7]
        g_maps = [dtype(0.0 if score_only else u_fm * 2.0) * s.astype(dtype) / dtype(s.size) for s in signs]
        if not maps_only:
            g_maps[7] = g_maps[7] + dtype(u_adv / N_SCALES) * 2 * (g8 - 1) / dtype(g8.size)
        out.append(disc_backward(fw["gen"][i], fw["layers"][i], g_maps, gates, fw["slope"], fw["chain"]))
    return out


def msd_grad(fw, u_adv, u_fm, decisions=None, **kw):
    """d (u_adv gen + u_fm fm) / d y_hat [B, T]: g0 + pool^T(g1 + pool^T(g2))."""
    g0, g1, g2 = scale_grads(fw, u_adv, u_fm, decisions, **kw)
    inner = pool_bwd(g2, fw["lengths"][1], add=g1)
    return pool_bwd(inner, fw["lengths"][0], add=g0)


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def seeded_state(seed, channels=FULL, groups=FULL_GROUPS):
    """A state dict with the reference's key names in the module's own key order, drawn from torch's generator: He-scaled Gaussian
    weights; discriminator 0: weight_orig, a random unit u, v = normalize(mat(W)^T u) (torch's own relation after an iteration's first
    half); the others: weight_g = ||v|| (1 + 0.1 N), weight_v.  bias = 0.05 N."""
    import torch
    g = torch.Generator().manual_seed(seed)
    chans = [1] + list(channels)
    state = collections.OrderedDict()
    for i in range(N_SCALES):
        for j in range(8):
            cin, cout, grp = (chans[j], chans[j + 1], groups[j]) if j < 7 else (chans[7], 1, 1)
            K = KERNELS[j]
            pre = _pre(i, j)
            w = torch.randn(cout, cin // grp, K, generator=g) * (2.0 / (cin // grp * K)) ** 0.5
            bias = 0.05 * torch.randn(cout, generator=g)
            state[pre + "bias"] = bias
            if i == 0:
                u = torch.randn(cout, generator=g)
                u = u / u.norm().clamp_min(EPS)
                v = w.reshape(cout, -1).t().mv(u)
                state[pre + "weight_orig"] = w
                state[pre + "weight_u"] = u
                state[pre + "weight_v"] = v / v.norm().clamp_min(EPS)
            else:
                state[pre + "weight_g"] = w.reshape(cout, -1).norm(dim=1).reshape(cout, 1, 1) * (1 + 0.1 * torch.randn(cout, 1, 1, generator=g))
                state[pre + "weight_v"] = w
    return state


# ---- case tables of the kernel tests ----------------------------------------------------------------------------------------------------
GROUP_PAIRS = ((32, 32), (8, 16), (16, 32), (32, 64), (64, 64), (1, 1), (3, 5), (17, 33), (72, 80))   # (Cin / g, Cout / g); the last: more
#                                                                    than two 32-row blocks per group, i.e. more than one block of rows
GROUPS = (1, 3, 4, 16)
KS = (1, 5, 15, 40, 41)
STRIDES_ALL = (1, 2, 3, 4)
RS = (1, 3)


def pads_of(K):
    return sorted({p for p in (0, 20, K - 1) if p < K})


def gconv_cases():
    """[(cig, cog, groups, K, s, pad, H_in, R, bias, act, f_in, add)]: the values of the issue's table dealt round so that every value of
    every column occurs, every (pair, stride) and every (K, stride) occurs, and H_out takes 1, tile - 1, tile, tile + 1, 2 tile + 3 for
    the forward tile of the pair's Cout / g, and H_in the same around the dgrad tile (stride times the tile of Cin / g)."""
    cases, n = [], 0
    for pi, (cig, cog) in enumerate(GROUP_PAIRS):
        for s in STRIDES_ALL:
            for ki, K in enumerate(KS):
                if (pi + s + ki) % 2 and not (K == 41 and pi < 5):      # half of the grid, and every MSD pair at 41 taps at every stride
                    continue
                pads = pads_of(K)
                pad = pads[n % len(pads)]
                G = GROUPS[n % len(GROUPS)] if max(cig, cog) < 64 else GROUPS[n % 2]       # keep the wide pairs small
                tf, td = tile_of(cog), s * tile_of(cig)
                houts = (1, tf - 1, tf, tf + 1, 2 * tf + 3)
                ho = houts[n % 5]
                lengths = [s * (ho - 1) + K - 2 * pad]
                if n % 3 == 0:
                    lengths.append((td - 1, td, td + 1)[n // 3 % 3])
                for H in lengths:
                    if H >= 1 and H + 2 * pad >= K:
                        flags = tuple(bool((n >> b) & 1) for b in range(4))
                        cases.append((cig, cog, G, K, s, pad, H, RS[n % 2]) + flags)
                n += 1
    return cases


def exact_budget(cig, cog, K):
    """Largest magnitude an integer case can reach before the slope, in units of the slope's 0.5: must stay below 2^24."""
    return 2 * max(INT_X * INT_W * cig * K + INT_X, INT_X * INT_W * cog * K + INT_X)


MSD_LAYER_SHAPES = tuple((FULL[j - 1], FULL[j], FULL_GROUPS[j], STRIDES[j]) for j in range(1, 6))     # (Cin, Cout, groups, stride), K = 41
WAVE_T = (1, 14, 15, 63, 64, 65, 200)
POOL_T = (2, 3, 4, 5, 63, 64, 65, 333)

# ---- end-to-end cases -------------------------------------------------------------------------------------------------------------------
E2E = collections.OrderedDict([        # id -> (channels, groups, B, T, train, weight seed, waveform seed)
    ("narrow_333_eval", (NARROW, NARROW_GROUPS, 2, 333, False, 41, 51)),
    ("narrow_333_train", (NARROW, NARROW_GROUPS, 2, 333, True, 41, 51)),
    ("full_256_eval", (FULL, FULL_GROUPS, 1, 256, False, 42, 52)),
    ("full_256_train", (FULL, FULL_GROUPS, 1, 256, True, 42, 52)),
    ("full_1024_eval", (FULL, FULL_GROUPS, 2, 1024, False, 43, 53)),
    ("full_1024_train", (FULL, FULL_GROUPS, 2, 1024, True, 43, 53)),
])
_CACHE = {}


def e2e_inputs(case):
    channels, groups, B, T, _train, sw, sy = E2E[case]
    y, y_hat = waves(sy, B, T)
    return seeded_state(sw, channels, groups), y, y_hat


def e2e_model(case):
    """The float64 forward of a case, computed once per process."""
    if case not in _CACHE:
        state, y, y_hat = e2e_inputs(case)
        _CACHE[case] = msd_forward(y, y_hat, state_numpy(state), E2E[case][1], E2E[case][4])
    return _CACHE[case]


def mirror_errors(case):
    """The float32 mirror's errors against the model for every quantity the end-to-end GPU test compares, and the share of undecided
    gate and sign entries per scale.  tools/make_msd_golden.py records it as tests/golden/msd_bars.npz."""
    state, y, y_hat = e2e_inputs(case)
    fw = e2e_model(case)
    mi = msd_forward(y, y_hat, state_numpy(state), E2E[case][1], E2E[case][4], dtype=np.float32, chain=True)
    d = lambda a, b: np.abs(np.asarray(b, np.float64) - np.asarray(a, np.float64))  # noqa: E731
    out = dict(
        maps=np.asarray([[max(d(a, b).max(), d(c, e).max()) for a, b, c, e in zip(fw["gen"][i], mi["gen"][i], fw["real"][i], mi["real"][i])]
                         for i in range(N_SCALES)]),
        sign_ops=np.asarray([[d(a, b).max() for a, b in zip(fw["sign_ops"][i], mi["sign_ops"][i])] for i in range(N_SCALES)]),
        losses=np.asarray([d(fw[k], mi[k]).max() for k in ("gen_loss", "fm_loss", "disc_r_loss", "disc_g_loss")]),
        grads=np.asarray([d(msd_grad(fw, ua, uf), msd_grad(mi, ua, uf, decisions=list(zip(fw["gates"], fw["signs"])))).max() for ua, uf in U_PAIRS]),
    )
    und_g = [undecided(fw["gate_ops"][i], mi["gate_ops"][i]) for i in range(N_SCALES)]
    und_s = [undecided(fw["sign_ops"][i], mi["sign_ops"][i]) for i in range(N_SCALES)]
    share = lambda us: sum(int(u.sum()) for u in us) / float(sum(u.size for u in us))  # noqa: E731
    out["undecided"] = np.asarray([[share(und_g[i]), share(und_s[i])] for i in range(N_SCALES)])
    return out


def load_bars(case):
    """The recorded mirror errors of a case (tests/golden/msd_bars.npz)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msd_bars.npz"))
    return {k[len(case) + 1:]: g[k] for k in g.files if k.startswith(case + ".")}
