"""Float64 model of the multi-period discriminator as the generator step uses it -- the fold, the six layers, the three losses and
every gradient -- written from the formulas of include/set_amd.h, its float32 mirror, and the case tables of the MPD tests.

Every function works in the dtype of its operands.  The model (float64) evaluates sums with matmul; the mirror (`chain=True`, float32) is
the plain float32 restatement of the kernels' documented order: one accumulator per output that takes its products one at a time
(16-channel chunk, tap, channel), each product rounded, then bias / add, then the activation or gate.  Its error against the model is the
yardstick of the non-exact GPU tests: BAR_FACTOR times the mirror's largest error for the quantity (tests/msstft_models.py:30).  The
kernels fuse each product into its add (one rounding less), so they sit at or below the mirror.

Decisions.  gate(f) = f > 0 ? 1 : slope and sign(g - r) are discontinuous: where the operand lies within BAR_FACTOR of its mirror
errors of 0 an fp32 evaluation may decide either way.  Such an entry is `undecided`; the stage tests leave it out of the comparison
(one gate or sign entry is one output entry there), the end-to-end test evaluates the model's backward with the decisions the GPU's own
maps give and asserts that they differ from the model's at undecided entries only.  UNDECIDED_CAP bounds their share per case.
"""
import collections

import numpy as np

BAR_FACTOR = 4.0
UNDECIDED_CAP = 1e-3
SLOPE = float(np.float32(0.1))        # LRELU_SLOPE as the kernels hold it
PERIODS = (2, 3, 5, 7, 11)
FULL = (32, 128, 512, 1024, 1024)
NARROW = (8, 20, 48, 72, 72)
KC = 16                               # input-channel chunk of the GEMM kernels
LOSS_CHUNK, LOSS_WORDS = 2048, 18
L1, SQ1, SQ0 = 0, 1, 2


def out_len(H, K, s, pad):
    return (H + 2 * pad - K) // s + 1


# ---- fold -------------------------------------------------------------------------------------------------------------------------------
def fold_index(T, p):
    """Source sample of every padded position n < Tp: n for n < T, 2 (T - 1) - n behind it (right reflect pad)."""
    Tp = -(-T // p) * p
    n = np.arange(Tp)
    return np.where(n < T, n, 2 * (T - 1) - n)


def fold(y, p):
    """[B, T] -> rows [B p, 1, H]: row b p + w holds xpad[b][i p + w]."""
    B, T = y.shape
    xp = y[:, fold_index(T, p)]
    return xp.reshape(B, -1, p).transpose(0, 2, 1).reshape(B * p, 1, -1)


def rows_to_map(rows, B, p):
    """[B p, C, H] -> the reference's [B, C, H, p]."""
    _R, C, H = rows.shape
    return rows.reshape(B, p, C, H).transpose(0, 2, 3, 1)


def map_to_rows(m):
    B, C, H, p = m.shape
    return np.ascontiguousarray(m.transpose(0, 3, 1, 2)).reshape(B * p, C, H)


# ---- layers -----------------------------------------------------------------------------------------------------------------------------
def _lrelu(v, slope):
    return np.where(v > 0, v, v * v.dtype.type(slope))


def conv_rows(x, W, bias, s, pad, slope=None, chain=False):
    """out[r][co][h] = act(bias[co] + sum_ci sum_k W[co][ci][k] x[r][ci][s h + k - pad]); x [R, Cin, H], W [Cout, Cin, K]."""
    R, Cin, H = x.shape
    Cout, _, K = W.shape
    Ho = out_len(H, K, s, pad)
    assert Ho >= 1
    xp = np.zeros((R, Cin, H + 2 * pad + s), x.dtype)
    xp[:, :, pad:pad + H] = x
    segs = [xp[:, :, k:k + s * (Ho - 1) + 1:s] for k in range(K)]
    acc = np.zeros((R, Cout, Ho), x.dtype)
    if chain:
        for c0 in range(0, Cin, KC):
            for k in range(K):
                for ci in range(c0, min(c0 + KC, Cin)):
                    acc = acc + W[None, :, ci, k, None] * segs[k][:, None, ci, :]
    else:  # one GEMM per tap over all rows
        for k in range(K):
            seg = np.ascontiguousarray(segs[k].transpose(1, 0, 2)).reshape(Cin, R * Ho)
            acc = acc + (np.ascontiguousarray(W[:, :, k]) @ seg).reshape(Cout, R, Ho).transpose(1, 0, 2)
    if bias is not None:
        acc = acc + bias[None, :, None]
    return acc if slope is None else _lrelu(acc, slope)


def gate_of(f, slope):
    return np.where(f > 0, f.dtype.type(1), f.dtype.type(slope))


def dgrad_rows(dz, W, H_in, s, pad, gate=None, add=None, chain=False):
    """dz_in[r][ci][j] = gate[r][ci][j] (add[r][ci][j] + sum_co sum_k W[co][ci][k] dz[r][co][(j + pad - k) / s]) over the k that hit an
    output frame; `gate` is the array of gate VALUES (gate_of(f_in, slope)) or None."""
    R, Cout, Ho = dz.shape
    _, Cin, K = W.shape
    assert Ho == out_len(H_in, K, s, pad)
    gp = np.zeros((R, Cin, H_in + 2 * pad + s), dz.dtype)
    if chain:
        for c0 in range(0, Cout, KC):
            for k in range(K):
                for co in range(c0, min(c0 + KC, Cout)):
                    gp[:, :, k:k + s * (Ho - 1) + 1:s] += W[co, :, k][None, :, None] * dz[:, None, co, :]
    else:
        dzc = np.ascontiguousarray(dz.transpose(1, 0, 2)).reshape(Cout, R * Ho)
        for k in range(K):
            gp[:, :, k:k + s * (Ho - 1) + 1:s] += (np.ascontiguousarray(W[:, :, k].T) @ dzc).reshape(Cin, R, Ho).transpose(1, 0, 2)
    g = gp[:, :, pad:pad + H_in]
    if add is not None:
        g = g + add
    return g if gate is None else g * gate


def fold_bwd(dz1, W1, B, T, p, s, pad, chain=False):
    """dz1 [B p, C, H_out] (generated rows, at the first layer's pre-activation) -> g_wav [B, T]."""
    H_in = -(-T // p)
    gx = dgrad_rows(dz1, W1.reshape(W1.shape[0], 1, -1), H_in, s, pad, chain=chain)      # [B p, 1, H_in]
    gpad = gx.reshape(B, p, H_in).transpose(0, 2, 1).reshape(B, H_in * p)
    idx = fold_index(T, p)
    g = gpad[:, :T].copy()
    tail = idx[T:]
    g[:, tail] = g[:, tail] + gpad[:, T:]                                                  # the mirror's contribution, second
    return g


def wn_fold(g, v):
    """weight norm: w = g v / ||v|| per output channel, in v's dtype (float32: the sum of squares in float32)."""
    n = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1, dtype=v.dtype))
    return (v * (g.reshape(-1) / n).reshape(-1, 1, 1, 1)).reshape(v.shape[0], v.shape[1], v.shape[2])


# ---- one sub-discriminator -------------------------------------------------------------------------------------------------------------
Layer = collections.namedtuple("Layer", "W b s pad act")


def layers_of(state, i, dtype):
    """The six layers of sub-discriminator i from a state dict with the reference's key names (numpy float32 values)."""
    out = []
    for j in range(6):
        pre = "discriminators.%d.%s." % (i, "convs.%d" % j if j < 5 else "conv_post")
        v = state[pre + "weight_v"].astype(dtype)
        W = wn_fold(state[pre + "weight_g"].astype(dtype), v)
        out.append(Layer(W, state[pre + "bias"].astype(dtype), 3 if j < 4 else 1, 2 if j < 5 else 1, j < 5))
    return out


def disc_forward(y, y_hat, layers, p, slope=SLOPE, chain=False):
    """The six maps as rows [2 B p, C, H], the real signal's rows first."""
    x = np.concatenate([fold(y, p), fold(y_hat, p)])
    maps = []
    for L in layers:
        x = conv_rows(x, L.W, L.b, L.s, L.pad, slope if L.act else None, chain)
        maps.append(x)
    return maps


def disc_backward(maps, layers, B, T, p, g_maps, gates=None, slope=SLOPE, chain=False):
    """d/d y_hat [B, T] from the gradients arriving at the six generated maps (rows [B p, C, H] each, or None); `gates`: the five arrays
    of gate values of maps 1..5 (default: from the maps)."""
    Rg = B * p
    gen = [m[Rg:] for m in maps]
    if gates is None:
        gates = [gate_of(f, slope) for f in gen[:5]]
    dz = g_maps[5]
    for i in range(5, 0, -1):
        L = layers[i]
        dz = dgrad_rows(dz, L.W, gen[i - 1].shape[2], L.s, L.pad, gate=gates[i - 1], add=g_maps[i - 1], chain=chain)
    L = layers[0]
    return fold_bwd(dz, L.W, B, T, p, L.s, L.pad, chain=chain)


# ---- the generator-side step -----------------------------------------------------------------------------------------------------------
def sign_of(g, r):
    return np.sign(g - r)


def mpd_forward(y, y_hat, state, dtype=np.float64, chain=False, slope=SLOPE):
    """The forward of the five sub-discriminators in `dtype`: per period the layers, the maps (rows), the scores, the decisions
    (gate values of maps 1..5, signs of g - r of maps 1..6) and their operands; the losses gen = (1 / D) sum mean (1 - dg)^2,
    fm = 2 sum mean |r - g|, and the discriminator's pair (sum mean (1 - dr)^2, sum mean dg^2) / D."""
    y, y_hat = y.astype(dtype), y_hat.astype(dtype)
    B, T = y.shape
    D = len(PERIODS)
    out = dict(B=B, T=T, dtype=dtype, chain=chain, slope=slope, layers=[], maps=[], scores_r=[], scores_g=[], gates=[], signs=[], gate_ops=[],
               sign_ops=[])
    gl, fl, dr, dg = dtype(0), dtype(0), dtype(0), dtype(0)
    for i, p in enumerate(PERIODS):
        layers = layers_of(state, i, dtype)
        maps = disc_forward(y, y_hat, layers, p, slope, chain)
        Rg = B * p
        real, gen = [m[:Rg] for m in maps], [m[Rg:] for m in maps]
        out["layers"].append(layers)
        out["maps"].append(maps)
        out["scores_r"].append(rows_to_map(real[5], B, p).reshape(B, -1))
        out["scores_g"].append(rows_to_map(gen[5], B, p).reshape(B, -1))
        out["gates"].append([gate_of(f, slope) for f in gen[:5]])
        out["signs"].append([sign_of(g, r) for g, r in zip(gen, real)])
        out["gate_ops"].append(gen[:5])
        out["sign_ops"].append([g - r for g, r in zip(gen, real)])
        gl = gl + ((1 - gen[5]) ** 2).mean(dtype=dtype)
        dr = dr + ((1 - real[5]) ** 2).mean(dtype=dtype)
        dg = dg + (gen[5] ** 2).mean(dtype=dtype)
        for r, g in zip(real, gen):
            fl = fl + np.abs(r - g).mean(dtype=dtype)
    out.update(gen_loss=gl / D, fm_loss=fl * 2, disc_r_loss=dr / D, disc_g_loss=dg / D)
    return out


def mpd_grad(fw, u_adv, u_fm, decisions=None):
    """d (u_adv gen + u_fm fm) / d y_hat [B, T] of a forward `fw`, the periods' gradients added in list order.  `decisions`: per period
    (gate values [5], signs [6]) to use instead of the forward's own."""
    dtype, B, T, D = fw["dtype"], fw["B"], fw["T"], len(PERIODS)
    grad = None
    for i, p in enumerate(PERIODS):
        gates, signs = (fw["gates"][i], fw["signs"][i]) if decisions is None else decisions[i]
        gates = [g.astype(dtype) for g in gates]
        gen6 = fw["maps"][i][5][B * p:]
        g_maps = [dtype(u_fm * 2.0) * s.astype(dtype) / dtype(s.size) for s in signs]
        g_maps[5] = g_maps[5] + dtype(u_adv / D) * 2 * (gen6 - 1) / dtype(gen6.size)
        gw = disc_backward(fw["maps"][i], fw["layers"][i], B, T, p, g_maps, gates, fw["slope"], fw["chain"])
        grad = gw if grad is None else grad + gw
    return grad


def undecided(ops_model, ops_mirror):
    """Per operand array: |operand| <= BAR_FACTOR * (the mirror's error).  The error of an entry is the larger of the mirror's own error
    there and the mirror's rms error over the array: the kernel's rounding at an entry is another draw from the distribution the mirror's
    errors come from, and the rms is that distribution's scale where the mirror's own draw happens to be small."""
    out = []
    for a, b in zip(ops_model, ops_mirror):
        err = np.abs(b.astype(np.float64) - a)
        err = np.maximum(err, np.sqrt((err ** 2).mean()))
        out.append(np.abs(a) <= BAR_FACTOR * err)
    return out


def bar(model, mirror):
    return BAR_FACTOR * float(np.abs(np.asarray(mirror, np.float64) - np.asarray(model, np.float64)).max())


# ---- weights and waveforms --------------------------------------------------------------------------------------------------------------
def seeded_state(seed, channels=FULL, kernel_size=5):
    """A state dict with the reference's key names, drawn from torch's generator (the same draw wherever torch runs): He-scaled Gaussian
    weight_v, weight_g = ||v|| (1 + 0.1 N), bias = 0.05 N.  Returns {key: float32 torch tensor} in the module's own key order."""
    import torch
    g = torch.Generator().manual_seed(seed)
    chans = [1] + list(channels)
    state = collections.OrderedDict()
    for i in range(len(PERIODS)):
        for j in range(6):
            cin, cout, K = (chans[j], chans[j + 1], kernel_size) if j < 5 else (chans[5], 1, 3)
            pre = "discriminators.%d.%s." % (i, "convs.%d" % j if j < 5 else "conv_post")
            v = torch.randn(cout, cin, K, 1, generator=g) * (2.0 / (cin * K)) ** 0.5
            wg = v.reshape(cout, -1).norm(dim=1).reshape(cout, 1, 1, 1) * (1 + 0.1 * torch.randn(cout, 1, 1, 1, generator=g))
            state[pre + "bias"] = 0.05 * torch.randn(cout, generator=g)
            state[pre + "weight_g"] = wg
            state[pre + "weight_v"] = v
    return state


def state_numpy(state):
    return {k: v.detach().cpu().numpy() for k, v in state.items()}


def waves(seed, B, T):
    """y ~ 0.3 N(0, 1), y_hat = y + 0.05 N(0, 1), float32 [B, T]."""
    rng = np.random.default_rng(seed)
    y = (0.3 * rng.standard_normal((B, T))).astype(np.float32)
    y_hat = (y + 0.05 * rng.standard_normal((B, T))).astype(np.float32)
    return y, y_hat


# ---- the list losses in the documented order --------------------------------------------------------------------------------------------
def _halve(v):
    v = v.copy()
    st = 128
    while st > 0:
        v[..., :st] = v[..., :st] + v[..., st:2 * st]
        st //= 2
    return v[..., 0]


def loss_item_sum(terms):
    """The sum of one item's terms (float64, in element order) in the order of set_multi_loss_fwd."""
    n = terms.size
    chunks = -(-n // LOSS_CHUNK)
    t = np.zeros(chunks * LOSS_CHUNK)
    t[:n] = terms.reshape(-1)
    t = t.reshape(chunks, 8, 256)
    s = np.zeros((chunks, 256))
    for u in range(8):
        s = s + t[:, u, :]
    part = _halve(s)                                         # [chunks]
    rows = -(-chunks // 256)
    pp = np.zeros(rows * 256)
    pp[:chunks] = part
    pp = pp.reshape(rows, 256)
    th = np.zeros(256)
    for r in range(rows):
        th = th + pp[r]
    return float(_halve(th))


def loss_terms(a, b, mode):
    a = a.astype(np.float64)
    if mode == L1:
        return np.abs(a - b.astype(np.float64))
    return (1.0 - a) ** 2 if mode == SQ1 else a * a


def multi_loss(items, scale, n_slots):
    """items: [(a, b or None, mode, slot)] with a, b float32 arrays in element order -> float32 [n_slots]."""
    tot = [0.0] * n_slots
    for a, b, mode, slot in items:
        tot[slot] = tot[slot] + loss_item_sum(loss_terms(a, b, mode)) / float(a.size)
    return np.asarray([np.float32(t * float(np.float32(scale))) for t in tot], np.float32)


def multi_loss_grad(a, b, mode, u, scale):
    """grad_a in float32 as set_multi_loss_bwd evaluates it."""
    coef = np.float32(float(np.float32(u)) * float(np.float32(scale)) / float(a.size))
    if mode == L1:
        d = np.sign((a - b).astype(np.float32)).astype(np.float32)
    elif mode == SQ1:
        d = np.float32(2) * (a - np.float32(1))
    else:
        d = np.float32(2) * a
    return (coef * d).astype(np.float32)


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
FWD_TILES = (32, 64)                                         # frames of H_out per block (set_sconv1d_fwd)
DGRAD_TILES = {1: (32, 64), 2: (64,), 3: (96,), 4: (128,)}   # frames of H_in per block (set_sconv1d_dgrad), by stride
CHANNEL_PAIRS = ((1, 8), (8, 20), (20, 48), (33, 72), (128, 32))
INT_X, INT_W, INT_SLOPE = 4, 2, 0.5                          # integer cases: |x|, |dz|, |add|, |bias| <= 4, |w| <= 2, slope 0.5


def sconv_lengths(s, K, pad):
    """H_in of the integer cases of one (stride, kernel): 1..5, the lengths whose H_out is one below, on and one above each forward tile
    width, and the lengths one below, on and one above each dgrad tile width."""
    L = {1, 2, 3, 4, 5}
    for w in FWD_TILES:
        for ho in (w - 1, w, w + 1):
            L.add(s * (ho - 1) + K - 2 * pad)
    for w in DGRAD_TILES[s]:
        L.update((w - 1, w, w + 1))
    return sorted(h for h in L if h >= 1 and h + 2 * pad >= K)


def sconv_cases():
    """[(s, K, pad, Cin, Cout, H_in, R)]: every stride x kernel, every length of sconv_lengths, the channel pairs and R in {1, 3} dealt
    round so that every (stride, pair) and every (kernel, pair) occurs."""
    cases, n = [], 0
    for s in (1, 2, 3, 4):
        for K in (1, 3, 5):
            pad = (K - 1) // 2
            for H in sconv_lengths(s, K, pad):
                cin, cout = CHANNEL_PAIRS[n % len(CHANNEL_PAIRS)]
                cases.append((s, K, pad, cin, cout, H, 1 if (n // len(CHANNEL_PAIRS)) % 2 else 3))
                n += 1
    return cases


def exact_budget(cin, cout, K):
    """Largest magnitude an integer case can reach before the slope, in units of the slope's 0.5: must stay below 2^24."""
    fwd = INT_X * INT_W * cin * K + INT_X
    bwd = INT_X * INT_W * cout * K + INT_X
    return 2 * max(fwd, bwd)


def int_array(rng, shape, lim):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)


# ---- end-to-end cases -------------------------------------------------------------------------------------------------------------------
LAMBDA_ADV = 4.0
U_PAIRS = ((1.0, 1.0), (LAMBDA_ADV, 2.5))                    # (upstream of generator_loss, upstream of feature_loss)
E2E = collections.OrderedDict([                              # id -> (channels, B, T, weight seed, waveform seed)
    ("full_97", (FULL, 2, 97, 21, 31)),
    ("full_200", (FULL, 2, 200, 22, 32)),
    ("full_1024", (FULL, 2, 1024, 23, 33)),
    ("narrow_200", (NARROW, 2, 200, 24, 34)),
])
GPU_E2E = ("full_97", "full_1024", "narrow_200")
_CACHE = {}


def e2e_inputs(case):
    channels, B, T, sw, sy = E2E[case]
    state = seeded_state(sw, channels)
    y, y_hat = waves(sy, B, T)
    return state, y, y_hat


def e2e_model(case):
    """The float64 forward of a case, computed once per process."""
    if case not in _CACHE:
        state, y, y_hat = e2e_inputs(case)
        _CACHE[case] = mpd_forward(y, y_hat, state_numpy(state))
    return _CACHE[case]


def mirror_errors(case):
    """The float32 mirror's errors against the model for every quantity the end-to-end GPU test compares (largest absolute error; for the
    decision operands also the rms), and the share of undecided gate and sign entries per period.  Slow (the mirror takes its products
    one at a time): tools/make_mpd_golden.py records it as tests/golden/mpd_bars.npz, test_mpd_reference.py holds the recording to it."""
    state, y, y_hat = e2e_inputs(case)
    fw = e2e_model(case)
    mi = mpd_forward(y, y_hat, state_numpy(state), dtype=np.float32, chain=True)
    d = lambda a, b: np.abs(np.asarray(b, np.float64) - np.asarray(a, np.float64))  # noqa: E731
    out = dict(
        maps=np.asarray([[d(a, b).max() for a, b in zip(fw["maps"][i], mi["maps"][i])] for i in range(len(PERIODS))]),
        sign_ops=np.asarray([[d(a, b).max() for a, b in zip(fw["sign_ops"][i], mi["sign_ops"][i])] for i in range(len(PERIODS))]),
        losses=np.asarray([d(fw[k], mi[k]).max() for k in ("gen_loss", "fm_loss", "disc_r_loss", "disc_g_loss")]),
        grads=np.asarray([d(mpd_grad(fw, ua, uf), mpd_grad(mi, ua, uf, decisions=list(zip(fw["gates"], fw["signs"])))).max()
                          for ua, uf in U_PAIRS]),
    )
    und_g = [undecided(fw["gate_ops"][i], mi["gate_ops"][i]) for i in range(len(PERIODS))]
    und_s = [undecided(fw["sign_ops"][i], mi["sign_ops"][i]) for i in range(len(PERIODS))]
    share = lambda us: sum(int(u.sum()) for u in us) / float(sum(u.size for u in us))  # noqa: E731
    out["undecided"] = np.asarray([[share(und_g[i]), share(und_s[i])] for i in range(len(PERIODS))])
    return out


def load_bars(case):
    """The recorded mirror errors of a case (tests/golden/mpd_bars.npz)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpd_bars.npz"))
    return {k[len(case) + 1:]: g[k] for k in g.files if k.startswith(case + ".")}
