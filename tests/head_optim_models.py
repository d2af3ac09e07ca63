"""Numpy models, case tables and bars for the branch sweep of the training kernels that had none: the stutter head with its two losses
(csrc/stutter.hip), the step projections and AdamW (csrc/train.hip), and the small entries set_l1_elem, set_frame_weight, set_scale_bcast,
set_row_sum, set_weight_norm_fold, set_gate and set_res_skip.  Nothing here touches the GPU: test_head_optim_reference.py ties the models
to float64 torch and shows that the bars separate planted faults; test_gpu_head_optim_branches.py compares the kernels with the models.

Two modes, as in the other sweeps.
  exact    operands are small integers (times a power of two), so every fp32 product and partial sum is exact in ANY order and the kernel
           must equal the float64 model bit for bit; single correctly rounded operations (l1_elem, scale_bcast, frame_weight, the skip output
           of res_skip) are modelled by rounding to fp32 after each operation and must match on any operands.
  bounded  plain sums of Gaussian operands: gamma(k + 2) sum |t_i| per element, k the number of terms (valid for any order).  Where a
           transcendental or a division chain enters no gamma bound is derivable: every model below takes `dtype`, and run with float32 it is a
           MIRROR of the kernel (the kernel's operations in the kernel's association; the library is built with -ffp-contract=off, so numpy's
           float32 arithmetic rounds where the kernel rounds).  bar = max(4 x the mirror's largest error against the float64 model for that
           output and case, 2 u |value|): the 4 covers another equally good association, device expf / logf / tanhf a few ulp from
           numpy's, and the host's powf."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
BAR_FACTOR = 4.0
G = 64  # floats around every output and scratch view


def gamma(k):
    return k * U / (1.0 - k * U)


def sum_bar(k, abs_sum):
    """|fl(sum of k terms) - sum| in any order, one more rounding for a scale / an accumulate, one for the conversion of the model"""
    return gamma(k + 2) * abs_sum


def mirror_bar(model, mirror):
    model = np.asarray(model, dtype=F64)
    d = np.abs(np.asarray(mirror, dtype=F64) - model)
    d = d[np.isfinite(d)]
    err = float(d.max()) if d.size else 0.0
    return np.maximum(BAR_FACTOR * err, 2.0 * U * np.abs(model))


_LANE = np.arange(64)


def wave_sum(a):
    """common.h's butterfly over the last axis (64 lanes): v += shfl_xor(v, 32), 16, ... 1"""
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., _LANE ^ o]
    return a[..., 0]


def _pad_axis(a, axis, mult):
    n = a.shape[axis]
    pad = -n % mult
    if not pad:
        return a
    w = [(0, 0)] * a.ndim
    w[axis] = (0, pad)
    return np.pad(a, w)


# =====================================================================================================================================
# stutter head
# =====================================================================================================================================
ALPHA = (5e-3, 1.0, 0.0)
SMOOTH = 1e-6
STUTTER_FAULTS = ("ce_over_all", "focal_valid_only", "no_smooth", "alpha_wrong", "drop_channel", "drop_frame")


def stutter_scratch_floats(B, C, T):
    return max(B * -(-T // 64) * 3, B * -(-T // 256) * (3 * C + 3))


def stutter_head(h, w, bias, labels, g_ce=None, g_fo=None, dw0=None, db0=None, dtype=F64, fault=None):
    """h [B][C][T], w [3][C], bias [3], labels [B][T] (clamped to 0 .. 2; 2 = pad) -> dict of
    logits [B][T][3]; ce (mean of -log p_y over labels != 2: NaN when there is none), focal (mean over ALL B T rows), n_valid;
    dh [B][C][T], part [B ceil(T / 256)][3 C + 3] (the backward kernel's partial rows), dw = dw0 + sum of rows, db likewise.
    g_ce / g_fo None is the kernel's NULL: that loss does not contribute.  log p_y = z_y - logsumexp(z) stays finite where p_y underflows.
    A batch of pad rows alone: every gradient is 0 (torch's cross entropy skips ignored rows before it divides by their count)."""
    D = dtype
    B, C, T = h.shape
    hh, ww = h.astype(F64), w.astype(F64)
    if fault == "drop_channel":
        hh = hh.copy()
        hh[:, C - 1] = 0.0
    z = (np.einsum("bct,jc->btj", hh, ww) + bias.astype(F64)).astype(D)  # exact operands: the order does not matter
    out = dict(logits=z)
    if labels is None:
        return out
    y = np.clip(labels, 0, 2)
    S = D(0.0 if fault == "no_smooth" else SMOOTH)
    one, three = D(1.0), D(3.0)
    m = z.max(-1)
    e = np.exp(z - m[..., None])
    s = (e[..., 0] + e[..., 1]) + e[..., 2]
    p = e / s[..., None]
    zy = np.take_along_axis(z, y[..., None], -1)[..., 0]
    # (z_y - max) - log(sum): a common offset cancels exactly.  "lse_first" is the association the kernel had before this sweep, z_y - (max +
    # log(sum)), which rounds at ulp(max): the same value in float64, 1e-4 of the focal gradient away in float32 at an offset of 1e4
    lp = zy - (m + np.log(s)) if fault == "lse_first" else (zy - m) - np.log(s)
    q = np.take_along_axis(p, y[..., None], -1)[..., 0]
    alpha = np.array(ALPHA, dtype=D)[(y + 1) % 3 if fault == "alpha_wrong" else y]
    valid = y != 2
    seen = np.ones((B, T), dtype=bool)
    if fault == "drop_frame":
        seen[:, T - 1] = False
    om = one - (q + S)
    om2 = om * om
    ce_row = np.where(valid & seen, -lp, D(0.0))
    nv_row = (valid & seen).astype(D)
    fo_row = np.where(seen, (-alpha * (om2 * om)) * (lp + S), D(0.0))
    if fault == "focal_valid_only":
        fo_row = fo_row * nv_row

    def total(rows):  # [B][T] -> scalar: one partial per (utterance, 64-frame tile), then lane l takes partials l, l + 64, ...
        part = wave_sum(_pad_axis(rows, 1, 64).reshape(B, -1, 64)).reshape(-1)
        trips = _pad_axis(part, 0, 64).reshape(-1, 64)
        acc = np.zeros(64, dtype=D)
        for r in trips:
            acc = acc + r
        return wave_sum(acc)

    with np.errstate(invalid="ignore", divide="ignore"):
        ce_sum, nv, fo_sum = total(ce_row), total(nv_row), total(fo_row)
        n_all = D(B * T)
        ce_den = n_all if fault == "ce_over_all" else nv
        fo_den = nv if fault == "focal_valid_only" else n_all
        out.update(ce=ce_sum / ce_den, focal=fo_sum / fo_den, n_valid=nv)
        gce, gfo = D(0.0 if g_ce is None else g_ce), D(0.0 if g_fo is None else g_fo)
        kce = gce / ce_den
        inv_all = one / fo_den
    ls = lp + S
    ay = alpha * ((om2 * om) - (((three * q) * om2) * ls))
    if fault == "focal_valid_only":
        ay = ay * valid
    k = (-np.where(valid, kce, D(0.0))) - ((gfo * ay) * inv_all)
    onehot = (np.arange(3)[None, None, :] == y[..., None]).astype(D)
    dz = (onehot - p) * k[..., None]                                                         # [B][T][3]
    wd = w.astype(D)
    dh = (dz[..., 0, None] * wd[0] + dz[..., 1, None] * wd[1]) + dz[..., 2, None] * wd[2]      # [B][T][C]
    out["dh"] = np.ascontiguousarray(np.transpose(dh, (0, 2, 1)))
    hd = np.transpose(hh, (0, 2, 1)).astype(D)                                                # [B][T][C]
    terms = np.concatenate([dz[..., j, None] * hd for j in range(3)] + [dz], -1)            # [B][T][3 C + 3]
    terms = terms * seen[..., None]
    n = 3 * C + 3
    tw = _pad_axis(terms, 1, 256).reshape(B, -1, 4, 64, n)                                    # chunk, wave, lane
    r = wave_sum(np.moveaxis(tw, 3, -1))                                                      # [B][chunks][4][n]
    part = (((r[:, :, 0] + r[:, :, 1]) + r[:, :, 2]) + r[:, :, 3]).reshape(-1, n)
    out["part"] = part
    s = np.zeros(n, dtype=D)
    for row in part:
        s = s + row
    out["dw"] = (np.zeros((3, C), D) if dw0 is None else dw0.astype(D)) + s[:3 * C].reshape(3, C)
    out["db"] = (np.zeros(3, D) if db0 is None else db0.astype(D)) + s[3 * C:]
    return out


def reduce_rows(part, dw0, db0):
    """set_stutter_head_bwd_reduce in fp32: s = the rows added in row order, then dw += s"""
    s = np.zeros(part.shape[1], dtype=F32)
    for row in part.astype(F32):
        s = s + row
    C3 = dw0.size
    return dw0.astype(F32) + s[:C3].reshape(dw0.shape), db0.astype(F32) + s[C3:]


STUTTER_OUTPUTS = ("ce", "focal", "dh", "part", "dw", "db")


def _sc(name, B, C, T, labels="ragged", logits="plain", g_ce=0.37, g_fo=1.9):
    return dict(name=name, B=B, C=C, T=T, labels=labels, logits=logits, g_ce=g_ce, g_fo=g_fo)


_LP = (2, 17, 255)  # the shape of the label- and logit-pattern cases
STUTTER_CASES = [
    # forward: wave wv takes channels wv, wv + 4, ... (`c < C`), lane = frame of a 64-frame tile (`t < T`); backward: 16-channel groups
    # (`c < C`), 256-frame chunks, bias partials from blockIdx.x == 0; final kernel: `r += 64` over B ceil(T / 64) partial rows
    _sc("b1_c1_t1_three_idle_waves_one_frame", 1, 1, 1, labels="all_valid"),
    _sc("c3_t63_wave3_idle_below_tile_edge", 2, 3, 63),
    _sc("c4_t64_even_share_at_tile_edge", 2, 4, 64),
    _sc("c5_t65_uneven_share_one_frame_second_tile", 3, 5, 65),
    _sc("c17_t255_group_guard_below_chunk_edge", *_LP),
    _sc("c16_t256_full_group_at_chunk_edge", 2, 16, 256),
    _sc("c33_t257_three_groups_one_frame_second_chunk", 2, 33, 257),
    _sc("b9_t449_72_partial_rows_final_second_trip", 9, 4, 449),
    _sc("c192_t300_model_width", 2, 192, 300),
    _sc("c1_t200_forward_rows_set_the_scratch_size", 2, 1, 200),  # 2 * 4 * 3 forward floats > 2 * 1 * 6 backward floats
    _sc("labels_one_utterance_all_pad", *_LP, labels="one_pad"),
    _sc("labels_whole_batch_pad_n_valid_0", *_LP, labels="all_pad"),
    _sc("labels_minus1_and_7_clamped", *_LP, labels="out_of_range"),
    _sc("logits_spread_above_110_p_y_underflows", *_LP, logits="underflow"),
    _sc("logits_all_three_equal", *_LP, logits="equal"),
    _sc("logits_common_offset_1e4", *_LP, logits="offset"),
    _sc("g_ce_null", *_LP, g_ce=None),
    _sc("g_focal_null", *_LP, g_fo=None),
]
assert len({c["name"] for c in STUTTER_CASES}) == len(STUTTER_CASES)


# (logits, label): p_y underflows in the first five (a pad row among them, which the focal term still reads); the last is an ordinary row
UNDERFLOW_ROWS = (((0, -120, 5), 1), ((110, 0, -3), 1), ((-2, 3, 128), 0), ((0, 111, -1), 0), ((120, 3, 0), 2), ((0, -120, 5), 2),
                  ((0, -120, 5), 0))


def stutter_w_shift(C):
    """w = integers * 2^-k with k ~ log2(sqrt(C)): the logits stay exact and of order 1, so the softmax is not saturated"""
    return max(0, int(round(0.5 * np.log2(C))))


def stutter_operands(c):
    """-> h, w, bias (fp32, integers times a power of two), labels (int64), dw0, db0 (integer prefills of the gradient targets)"""
    B, C, T = c["B"], c["C"], c["T"]
    rng = np.random.default_rng(1000 * C + T + 7 * B)
    h = rng.integers(-2, 3, (B, C, T)).astype(F32)
    w = (rng.integers(-2, 3, (3, C)) * 2.0 ** -stutter_w_shift(C)).astype(F32)
    bias = rng.integers(-1, 2, 3).astype(F32)
    lab = (rng.random((B, T)) < 0.3).astype(np.int64)
    kind = c["labels"]
    if kind != "all_valid":
        for b in range(B):  # ragged pad tails (the first utterance is full length)
            lab[b, T - (b * T) // (B + 1):] = 2
    if kind == "one_pad":
        lab[B - 1] = 2
    elif kind == "all_pad":
        lab[:] = 2
    elif kind == "out_of_range":
        lab[0, 1::5], lab[0, 2::5] = -1, 7
    if c["logits"] != "plain":  # channels 0 .. 2 carry the logits of the first frames: w[:, :3] = I, the other channels read zeros there
        w[:, :3] = np.eye(3, dtype=F32)
        nt = 12
        h[:, :, :nt] = 0.0
        if c["logits"] == "underflow":  # z_max - z_y from 110 to 133: expf gives 0 (e^-103.97 is the smallest denormal)
            for t, (zz, yy) in enumerate(UNDERFLOW_ROWS):
                h[:, :3, t] = np.array(zz, dtype=F32) - bias
                lab[:, t] = yy
        elif c["logits"] == "equal":
            for t in range(nt):
                h[:, :3, t] = float(t - 5) - bias
            lab[:, :nt] = np.arange(nt) % 3
        else:
            bias += F32(10000.0)  # ulp(1e4) = 2^-10: the logits stay exact
            lab[:, :nt] = np.arange(nt) % 3
    dw0 = rng.integers(-3, 4, (3, C)).astype(F32)
    db0 = rng.integers(-3, 4, 3).astype(F32)
    return h, w, bias, lab, dw0, db0


def stutter_bars(model, mirror):
    return {k: mirror_bar(model[k], mirror[k]) for k in STUTTER_OUTPUTS}


# =====================================================================================================================================
# step projections: h [C][N], W_l [C][C] and b_l [C] at one stride in a flat parameter buffer, out / g [N][L C]
# =====================================================================================================================================
SP_GAP = 12  # floats between one layer's bias and the next layer's weight (a multiple of 4: the forward reads weight rows as 16-byte quads)
E_UNSUPPORTED = -2
STEP_PROJ_CASES = [  # (L, C, N): N at both edges of the NT = 32 and NT = 64 instances; C = 256 with NT = 64 asks for exactly 64 KiB of LDS
    ("n1_nt32_lower_edge", 1, 64, 1), ("n31_nt32", 2, 64, 31), ("n32_nt32_upper_edge", 2, 64, 32),
    ("n33_nt64_lower_edge_c128", 2, 128, 33), ("n64_nt64_upper_edge_c192", 3, 192, 64),
    ("c256_n33_lds_64k", 2, 256, 33), ("c256_n64_lds_64k", 2, 256, 64),
]
STEP_PROJ_REFUSED = [  # (name, L, C, N, entries that refuse)
    ("c96_not_multiple_of_64", 1, 96, 8, ("fwd", "dh", "dw")),
    ("n65_above_64", 1, 64, 65, ("fwd", "dh", "dw")),
    ("c320_n33_lds_80k_forward_only", 1, 320, 33, ("fwd",)),
]


def step_proj_stride(C):
    return C * C + C + SP_GAP


def step_proj_operands(L, C, N, mode, seed=0):
    """-> h [C][N], flat parameters [L stride] (gaps hold 0.5, which nothing may read into a result), g [N][L C], flat prefill of the gradient
    targets.  exact: integers in [-2, 2]; bounded: Gaussian."""
    rng = np.random.default_rng(seed + 31 * C + N + 1000 * L)
    draw = (lambda *s: rng.integers(-2, 3, s).astype(F32)) if mode == "exact" else (lambda *s: rng.standard_normal(s).astype(F32))
    ls = step_proj_stride(C)
    flat, pre = np.full(L * ls, 0.5, dtype=F32), np.full(L * ls, -9.0, dtype=F32)
    for l in range(L):
        flat[l * ls:l * ls + C * C + C] = draw(C * C + C)
        pre[l * ls:l * ls + C * C + C] = draw(C * C + C)
    return draw(C, N), flat, draw(N, L * C), pre


def step_proj_params(flat, L, C):
    ls = step_proj_stride(C)
    W = np.stack([flat[l * ls:l * ls + C * C].reshape(C, C) for l in range(L)])
    b = np.stack([flat[l * ls + C * C:l * ls + C * C + C] for l in range(L)])
    return W, b


def step_proj(h, flat, g, pre, L, C, N):
    """float64 -> dict of (value, sum of |terms|, number of terms) for out [N][L C], dh [C][N] and the flat gradient buffer (prefill + gradient;
    its gaps unchanged)."""
    W, b = step_proj_params(flat.astype(F64), L, C)
    h64, g64 = h.astype(F64), g.astype(F64).reshape(N, L, C)
    out = np.einsum("loi,in->nlo", W, h64) + b[None]
    out_a = np.einsum("loi,in->nlo", np.abs(W), np.abs(h64)) + np.abs(b)[None]
    dh = np.einsum("loi,nlo->in", W, g64)
    dh_a = np.einsum("loi,nlo->in", np.abs(W), np.abs(g64))
    dW = np.einsum("nlo,in->loi", g64, h64)
    dW_a = np.einsum("nlo,in->loi", np.abs(g64), np.abs(h64))
    db, db_a = g64.sum(0), np.abs(g64).sum(0)
    ls = step_proj_stride(C)
    grad, grad_a = pre.astype(F64).copy(), np.abs(pre.astype(F64))
    for l in range(L):
        grad[l * ls:l * ls + C * C] += dW[l].reshape(-1)
        grad_a[l * ls:l * ls + C * C] += dW_a[l].reshape(-1)
        grad[l * ls + C * C:l * ls + C * C + C] += db[l]
        grad_a[l * ls + C * C:l * ls + C * C + C] += db_a[l]
    return dict(out=(out.reshape(N, L * C), out_a.reshape(N, L * C), C + 1), dh=(dh, dh_a, L * C), grad=(grad, grad_a, N + 1))


# =====================================================================================================================================
# AdamW with the gradient clip of clip_grad_norm_
# =====================================================================================================================================
ADAMW_FAULTS = ("eps_in_sqrt", "bias_step_minus_1", "decay_after", "clip_without_scale")


def f32f(x):
    """a Python float that is exactly the fp32 the C ABI passes"""
    return float(F32(x))


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, sumsq=None, max_norm=0.0, grad_scale=1.0, dtype=F64, fault=None):
    """One step -> (p, m, v).  torch.optim.AdamW (amsgrad off) on the gradient g * grad_scale, first multiplied by
    min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6)) when sumsq is given and max_norm > 0 (clip_grad_norm_ of the scaled gradient)."""
    D = dtype
    lr, beta1, beta2, eps, wd, max_norm, gs = (D(x) for x in (lr, beta1, beta2, eps, wd, max_norm, grad_scale))
    one = D(1.0)
    st = step - 1 if fault == "bias_step_minus_1" else step
    with np.errstate(under="ignore"):
        bc1, bc2 = one - np.power(beta1, D(st)), one - np.power(beta2, D(st))
    clip = one
    if sumsq is not None and max_norm > 0:
        c = max_norm / (np.sqrt(D(sumsq)) * (one if fault == "clip_without_scale" else gs) + D(1e-6))
        clip = c if c < one else one
    p, g, m, v = (a.astype(D) for a in (p, g, m, v))
    gi = g * gs * clip
    pi = p if fault == "decay_after" else p * (one - lr * wd)
    mi = beta1 * m + (one - beta1) * gi
    vi = beta2 * v + (one - beta2) * gi * gi
    with np.errstate(divide="ignore", invalid="ignore"):
        denom = np.sqrt(vi / bc2 + eps) if fault == "eps_in_sqrt" else np.sqrt(vi) / np.sqrt(bc2) + eps
        pi = pi - (lr / bc1) * (mi / denom)
    if fault == "decay_after":
        pi = pi * (one - lr * wd)
    return pi, mi, vi


HYPER = dict(lr=f32f(2e-4), beta1=f32f(0.9), beta2=f32f(0.999), eps=f32f(1e-8), wd=0.0)


def _ac(name, n, step=1, p0="zero", clip=None, steps=1, g="log", **hyper):
    """clip: None (sumsq NULL, max_norm 1), or (max_norm as a multiple of the norm of the SCALED gradient, grad_scale); p0: zero | unit;
    g: log (magnitudes log-uniform over 1e-8 .. 1: where eps matters and where it does not) | zeros (half of them +-0) | 1e4 | 1e-12 (every
    |g| that size: a case of its own each, or the one large element would set the bar of every other element's m and v)"""
    return dict(name=name, n=n, step=step, p0=p0, clip=clip, steps=steps, g=g, hyper=dict(HYPER, **{k: f32f(x) for k, x in hyper.items()}))


ADAMW_CASES = (
    [_ac("n%d_p0_wd0_step1_%s" % (n, "off_256" if n % 256 else "on_256"), n) for n in (1, 255, 256, 257, 1000)]
    + [_ac("p0_wd0_step%d" % s, 257, step=s) for s in (2, 1000, 10 ** 6)]
    + [_ac("wd_unit_p_step%d" % s, 257, step=s, p0="unit", wd=0.01) for s in (1, 2, 1000, 10 ** 6)]
    + [_ac("g_exact_zeros", 257, step=2, g="zeros"), _ac("g_1e4", 257, step=2, g="1e4"), _ac("g_1e-12_squares_stay_normal", 257, step=2, g="1e-12"),
       _ac("sumsq_null_no_clip", 1000, step=2, p0="unit", wd=0.01),
       _ac("max_norm_0_no_clip", 1000, step=2, clip=(0.0, 1.0)),
       _ac("norm_0.999_of_max_norm_no_clip", 1000, step=2, clip=(1.0 / 0.999, 1.0)),
       _ac("norm_1.001_of_max_norm_clips", 1000, step=2, clip=(1.0 / 1.001, 1.0)),
       # the threshold lies between the scaled and the unscaled norm: a clip computed without grad_scale takes the other branch
       _ac("grad_scale_0.25_unscaled_norm_above_scaled_below", 1000, step=2, clip=(2.0, 0.25)),
       _ac("grad_scale_4_scaled_norm_above_unscaled_below", 1000, step=2, clip=(0.5, 4.0)),
       # lr wd = 0.05: the one place where the order of decay and update is more than a rounding error of p
       _ac("large_lr_wd_decay_before_update", 257, step=2, p0="unit", lr=0.1, wd=0.5),
       _ac("five_steps_carried_m_v", 1000, p0="unit", steps=5, wd=0.01, clip=(0.7, 1.0))])
assert len({c["name"] for c in ADAMW_CASES}) == len(ADAMW_CASES)


def adamw_operands(c, k=0):
    """-> p, g, m, v (fp32), sumsq (fp32 scalar or None), max_norm, grad_scale for step c['step'] + k.  m, v are a plausible carried state
    past step 1 (zero at step 1, as a fresh optimizer has)."""
    n = c["n"]
    rng = np.random.default_rng(n + 7 * c["step"] + 13 * k + len(c["name"]))
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 0, n)).astype(F32)
    if c["g"] == "zeros":
        g[::2] = 0.0
        g[::4] = -0.0
    elif c["g"] != "log":
        g = (np.sign(g) * float(c["g"])).astype(F32)
    p = np.zeros(n, F32) if c["p0"] == "zero" else rng.standard_normal(n).astype(F32)
    if c["step"] == 1:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    else:
        m = (0.3 * g + 0.1 * np.abs(g) * rng.standard_normal(n)).astype(F32)
        v = (g.astype(F64) ** 2 * rng.uniform(0.2, 2.0, n)).astype(F32)
    sumsq, max_norm, gs = None, 1.0, 1.0
    if c["clip"] is not None:
        mult, gs = c["clip"]
        sumsq = F32((g.astype(F64) ** 2).sum())
        max_norm = f32f(mult * np.sqrt(F64(sumsq)) * gs)
    return p, g, m, v, sumsq, max_norm, gs


def adamw_run(c, dtype=F64, fault=None):
    """all c['steps'] steps (p, m, v carried; a fresh gradient each step) -> (p, m, v)"""
    p, g, m, v, sumsq, max_norm, gs = adamw_operands(c)
    for k in range(c["steps"]):
        if k:
            _, g, _, _, sumsq, max_norm, gs = adamw_operands(c, k)
        p, m, v = adamw(p, g, m, v, step=c["step"] + k, sumsq=sumsq, max_norm=max_norm, grad_scale=gs, dtype=dtype, fault=fault, **c["hyper"])
    return p, m, v


# =====================================================================================================================================
# small entries
# =====================================================================================================================================
def l1_elem(pred, target):
    """-> |d|, sign(d) with d = fl(pred - target); sign(0) = +0.0"""
    d = pred.astype(F32) - target.astype(F32)
    return np.abs(d), (np.sign(d) + F32(0.0)).astype(F32)


def frame_weight(target):
    """[frames][M] -> 1 where sum_m |target| != 0 (float64: a sum of absolute values cannot cancel, so fp32 decides the same way)"""
    return (np.abs(target.astype(F64)).sum(1) != 0).astype(F32)


def scale_bcast(a, w, inner, scale_dev, scale):
    """fl(fl(fl(a scale) w[i / inner]) scale_dev), the optional factors in this order"""
    v = a.astype(F32) * F32(scale)
    if w is not None:
        v = v * np.repeat(w.astype(F32), inner)[:a.size]
    if scale_dev is not None:
        v = v * F32(scale_dev)
    return v.astype(F32)


def row_sum(x, scale):
    """[rows][T] float64 -> (sum_t x * scale, sum_t |x| * |scale|)"""
    x = x.astype(F64)
    return x.sum(1) * scale, np.abs(x).sum(1) * abs(scale)


def weight_norm_fold(g, v, dtype=F64):
    """v [n0][inner], g [n0] -> v g / |v|.  float32: the kernel's order (thread j takes j, j + 256, ... with one fused multiply-add per element,
    then the halving tree over 256 threads; scale = g / sqrt(sum), w = v scale)."""
    if dtype == F64:
        v64 = v.astype(F64)
        return v64 * (g.astype(F64) / np.sqrt((v64 * v64).sum(1)))[:, None]
    out = np.empty(v.shape, F32)
    for i in range(v.shape[0]):
        cols = _pad_axis(v[i].astype(F32), 0, 256).reshape(-1, 256)
        s = np.zeros(256, F32)
        for r in cols:  # fmaf: the product is exact in float64, one rounding of the sum
            s = (r.astype(F64) * r.astype(F64) + s.astype(F64)).astype(F32)
        st = 128
        while st:
            s = s[:st] + s[st:2 * st]
            st //= 2
        out[i] = v[i].astype(F32) * (g[i].astype(F32) / np.sqrt(s[0]))
    return out


def gate(y, dtype=F64):
    """y [B][2 C][T] -> sigmoid(y[:, :C]) tanh(y[:, C:]), sigmoid(x) = 1 / (1 + exp(-x))"""
    C = y.shape[1] // 2
    a, b = y[:, :C].astype(dtype), y[:, C:].astype(dtype)
    return (dtype(1.0) / (dtype(1.0) + np.exp(-a))) * np.tanh(b)


SQRT2_F32 = F32(1.41421356237309504880)


def res_skip(x_in, o, skip, first, dtype=F64):
    """-> x_out = (x_in + o[:, :C]) / fl32(sqrt 2) in `dtype`, skip_out = o[:, C:] (first) or fl(skip + o[:, C:]) in fp32: one rounding"""
    C = x_in.shape[1]
    x_out = (x_in.astype(dtype) + o[:, :C].astype(dtype)) / dtype(SQRT2_F32)
    s = o[:, C:].astype(F32)
    return x_out, (s.copy() if first else skip.astype(F32) + s)
