"""float64 model of the DiffNet inference layer stack (set_diffnet_stack: csrc/diffnet.hip, csrc/diffnet_x3.hip, picked by plan_stack in
csrc/diffusion_loop.hip; and the per-layer kernel set_diffnet_layer), written from diffnet.py:60-81, 123-127 and the header comments of the
three sources, not from the kernel bodies; the case table of the GPU sweep tests/test_gpu_stack_branches.py (every row names the form it
must reach and the C conditions it meets); and the CPU checks of both.  The model extends test_loop_reference.layers (the loop sweep's
(x_L, skip sum)) with a per-layer trace and magnitude sums and is held to it, and to the oracle's residual_block, below.

  stack      per layer: y = dilated_conv(x + d) + b_dil + condproj, z = sigmoid(y[:256]) tanh(y[256:]), o = W_out z + b_out,
             x_l = fl64((x + o[:256]) fl32(2^-1/2)), skip += o[256:]; with S1 = sum |W_dil| |x + d| + |b_dil| + |condproj| and
             S2 = sum |W_out| |z| + |b_out|, the magnitudes every summation bar is proportional to.
  bars       bounded mode, composed per numerics class (NUMERICS) from conv_bound / conv_x2_bound and the terms derived beside
             gemm1_bar / gemm2_bar; the gate term of gate_bar (1/4 bar_g + bar_f and the transcendental slack of
             tests/test_diffnet_bf16_reference.py, both with the factors they lose where the gate saturates), |W_out| @ bar_z, propagation
             of bar_x through |W_dil| into the next layer.
  plan       Python mirror of plan_stack, of `concat` (set_launch_diffnet_stack_f32) and of the task-queue geometry (stack_grid, the words
             a launch clears, the final task counter and tile flags), pinned against ops.stack_variant / ops.stack_x3_winograd.

Exact mode (make_exact).  condproj = +40 on the sigmoid rows (gate = 1), zero dilated weights there; GEMM 1 decides the filter half.
  layer 0    x integer in [-3, 3], d an odd multiple of 1/2 (so x + d is never 0), filter rows of W_dil multiples of 32, their b_dil and
             condproj multiples of 16: every filter pre-activation is a multiple of 16 -- 0 or at least 16 in magnitude -- and
             z is exactly -1, 0 or +1.  Two weight families: `sel` (one non-zero (channel, tap) per filter row, position 7 r + shift mod
             768: the 256 rows of one case meet every tap and 256 distinct (channel, tap) slots, the shift moves with the case and the
             layer) and `dense` (every weight in {-32, 0, 32}: all 768 k-steps count; L = 1 only).
  layer >= 1 x_l = (x + o) 2^-1/2 is on no grid, so only the SIGN of x_l + d may matter: `sel` weights of magnitude 2^12, filter condproj
             +-64, residual rows of W_out 8 x a signed permutation without bias, d an odd multiple of 1/2 at layers 0 and 1 and of 1/4 behind them
             (x_l + d stays on a small lattice that keeps 0.04 away from 0: test_exact_budget_by_hand walks it).  The model asserts
             |x_l + d| >= MARGIN on every element and |y_f| >= 32 on every filter pre-activation (the padding included: there y_f is
             the condproj, +-64), and that |y_f| less its bounded-mode bar stays at 16 or beyond: z is +-1 whatever the form's rounding.
  W_out, b_out on the two-piece grid of test_conv_x2_reference.grid (integer + 2^-12): non-zero low pieces, pack exponents k1 != k2 != 0.
  Then skip is exact for every L, x_out for L = 1 is fl32((x + o) fl32(2^-1/2)), one rounding; x_out for L > 1 has its bounded bar.
test_exact_cases_meet_their_budget asserts every budget (integer sums below 2^24 granules, piece products within BUDGET_BITS with exact
splits, exact Winograd planes), never assumes it."""
import functools
import math
import zlib

import pytest
import torch

import test_loop_reference as R
from test_conv_reference import U, conv_bound, conv_ref, gamma, ints
from test_conv_x2_reference import BUDGET_BITS, conv_x2_bound, conv_x2_ref, grid, split2

torch.set_grad_enabled(False)
DC = 256
RSQRT2 = R.RSQRT2
N_CU = 256          # what the library's shape queries assume without a device
WINO_MAX_DIL = 8    # STACK_WINO_MAX_DIL (csrc/diffnet_host.h)
W0, W1 = 32.0, 2.0 ** 12   # magnitude of an exact-mode dilated weight at layer 0 / at the layers behind it
CP1 = 64.0                 # |condproj| of the filter rows behind layer 0
MARGIN = (CP1 + 32.0) / W1 + 2.0 ** -10   # least |x_l + d| for |y_f| >= 32 with 2^-10 to spare for the error of x_l (asserted: bar_x < 2^-10)


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def dilations(L, dcl):
    return [1 << (l % dcl) for l in range(L)]


def stack(x0, cp, d, Wd, bd, Wo, bo, dils, z32=False, forced=None):
    """The layers in float64 (z32: z rounded to fp32, the gate's output format -- exact mode, where the float64 tanh(16) sigmoid(40) is
    2.5e-14 short of the 1 every fp32 gate returns; the device's values are pinned by the first test of the GPU sweep).  x0 [B][256][T], cp [B][L 512][T], d [L][B][256] (the step offset of layer l, utterance b, channel c),
    Wd [L][512][256][3], Wo [L][512][256][1], dils: dilation per layer.  forced {l: x}: layer l takes this fp32 tensor -- what a kernel wrote
    as x_(l-1) -- for its input in place of the model's own (teacher forcing: the error of the layers below then stays out of the layer's
    bar, see bars).  One dict per layer: xin, y, z, o, x (= x_l, the layer's output),
    skip (the running sum), S1, S2, dil."""
    x, skip, out = x0.double(), None, []
    for l, dil in enumerate(dils):
        if forced and l in forced:
            x = forced[l].double()
        r1 = conv_ref(x, Wd[l], bias=bd[l], in_chan_add=d[l], dil=dil, pad=dil)
        cpl = cp[:, l * 512:(l + 1) * 512].double()
        y = r1["y"] + cpl
        z = torch.sigmoid(y[:, :DC]) * torch.tanh(y[:, DC:])
        if z32:
            z = z.float().double()
        r2 = conv_ref(z, Wo[l], bias=bo[l])
        o = r2["y"]
        xn = (x + o[:, :DC]) * RSQRT2
        skip = o[:, DC:] if skip is None else skip + o[:, DC:]
        out.append(dict(dil=dil, xin=x, xd=x + d[l].double()[:, :, None], y=y, S1=r1["S"] + cpl.abs(), z=z, o=o, S2=r2["S"], x=xn, skip=skip, cp=cpl))
        x = xn
    return out


NUMERICS = ("f32", "wino", "f16x2", "f16x2v", "bf16x3")


def _absconv(v, taps, dil):
    """sum over the channels of taps[0] |v[t - dil]| + taps[1] |v[t]| + taps[2] |v[t + dil]|, taps [512][256] each (zero padding)."""
    return conv_ref(v.abs(), torch.stack(taps, -1), dil=dil, pad=dil)["y"]


def wino_sums(t, Wd):
    """Magnitude sums of the F(2,3) form (header of wino_init / wino_main, csrc/diffnet.hip; the same pairing in csrc/diffnet_x3.hip):
        y0 = U0 (d0 - d2) + U1 (d1 + d2) + U2 (d2 - d1),  y1 = U1 (d1 + d2) - U2 (d2 - d1) - U3 (d1 - d3)
    with U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2 and d0 .. d3 the values of x + d at the frames t0 - dil, t0,
    t0 + dil, t0 + 2 dil of a pair (t0, t0 + dil).  Whether a frame is the even or the odd output of its pair depends on the tile origin,
    so every frame takes the larger of the two sums (SW), of sum |U| over the planes it meets (SU) and of sum |V| (SV):
        even at t: d0 = v[t - dil], d1 = v[t], d2 = v[t + dil]:  |U0| (|d0| + |d2|) + (|U1| + |U2|) (|d1| + |d2|)
        odd  at t: d1 = v[t - dil], d2 = v[t], d3 = v[t + dil]:  (|U1| + |U2|) (|d1| + |d2|) + |U3| (|d1| + |d3|)."""
    g = Wd.double()
    U0, U1, U2, U3 = g[:, :, 0].abs(), (0.5 * g.sum(-1)).abs(), (0.5 * (g[:, :, 0] - g[:, :, 1] + g[:, :, 2])).abs(), g[:, :, 2].abs()
    v, dil = t["xd"], t["dil"]
    even = _absconv(v, [U0, U1 + U2, U0 + U1 + U2], dil)
    odd = _absconv(v, [U1 + U2 + U3, U1 + U2, U3], dil)
    one = torch.ones(1, DC, dtype=torch.float64)
    SV = torch.maximum(_absconv(v, [one, 2 * one, 3 * one], dil), _absconv(v, [3 * one, 2 * one, one], dil))
    SU = torch.maximum(U0 + U1 + U2, U1 + U2 + U3).sum(1)
    return torch.maximum(even, odd), SU, SV


def gemm1_bar(t, Wd, bd, num, k1=None):
    """Bar of the pre-activations y of one layer whose input is exact, per numerics class.  u = 2^-24.
      f32     conv_bound with K = 768 on S1 (the accumulators start at b_dil + condproj: both are in S1).
      wino    fp32 Winograd: the filter planes are formed in float64 and rounded once (u |U|), x + d rounds once, every input-transform
              value rounds once (u (|da| + |db|)), 256 products per plane accumulate in fp32 in any order, the planes are combined with
              two more adds and b_dil + condproj is one add: gamma(256 + 8) SW', SW' = wino_sums' SW + |b_dil| + |condproj|; + 4 u |y|.
      f16x2   conv_x2_bound (K = 3, Cin = 256) on fl32(x + d), + gamma(2) (|condproj| + |y|) for the accumulator start.
      f16x2v  the two-piece form of the Winograd planes (header of diffnet_stack_x3v_kernel: "same piece products and fp32 accumulation",
              U scaled by s / 2, s = 2^k1): as conv_x2_bound, term by term, with SW' in place of sum |W| |P| --
              2 u SW' (one rounding of each transformed operand), (1 + 2^-10) (2^-21 SW' + 2^-25 (SU + SV 2 / s)) (two-piece splits and
              their subnormal floor), 2^-22 (1 + 2^-10) SW' (the product of the two low pieces, each at most 2^-11 of its operand, which
              the kernel leaves out), gamma(3 * 256 + 8) (1 + 2^-10) SW' (fp32 accumulation of the piece products and the combination
              of the planes; the accumulators start at (e +- o) / 2 of b_dil + condproj at BOTH frames of the pair, which SW' takes as
              2 max over the neighbouring frames); + 4 u |y|.
      bf16x3  header of csrc/diffnet_x3.hip: "error <= ~2^-23 |ab| per product" (three of the nine piece products are dropped, the
              pieces carry 24 bits): 2^-23 S1; the six piece products per term accumulate in fp32, their magnitudes sum to at most
              (1 + 2^-7) |ab|: gamma(6 * 768 + 4) (1 + 2^-7) S1; + 4 u |y|."""
    y, S1 = t["y"], t["S1"]
    if num == "f32":
        return conv_bound(dict(S=S1, y=y), 768)
    if num == "bf16x3":
        return 2.0 ** -23 * S1 + gamma(6 * 768 + 4) * (1 + 2.0 ** -7) * S1 + 4 * U * y.abs()
    if num == "f16x2":
        xd = t["xd"]
        r = conv_ref(xd, Wd, bias=bd, dil=t["dil"], pad=t["dil"])
        m = conv_x2_ref(xd, Wd, k1, bias=bd, dil=t["dil"], pad=t["dil"])
        ones = conv_ref(xd, torch.ones(1, DC, 3), dil=t["dil"], pad=t["dil"])["S"]
        return conv_x2_bound(r, m, ones, Wd.abs().sum((1, 2)), k1, Cin=DC, K=3) + gamma(2) * (t["cp"].abs() + y.abs())
    SW, SU, SV = wino_sums(t, Wd)
    start = bd.double().abs()[None, :, None] + t["cp"].abs()
    if num == "wino":
        return gamma(DC + 8) * (SW + start) + 4 * U * y.abs()
    assert num == "f16x2v" and t["dil"] == 1
    pad = torch.nn.functional.pad(start, (1, 1))
    SWp = SW + 2 * torch.maximum(torch.maximum(pad[..., :-2], pad[..., 1:-1]), pad[..., 2:])
    e = 2 * U * SWp + (1 + 2.0 ** -10) * (2.0 ** -21 * SWp + 2.0 ** -25 * (SU[None, :, None] + SV * 2.0 ** (1 - k1))) + \
        2.0 ** -22 * (1 + 2.0 ** -10) * SWp + gamma(3 * DC + 8) * (1 + 2.0 ** -10) * SWp
    return e + 4 * U * y.abs()


def gemm2_bar(t, Wo, bo, num, k2=None):
    """Bar of o = W_out z + b_out for the exact z: gamma(256 + 4) S2 (conv_bound) on the fp32 pipe; conv_x2_bound (K = 1) for both two-piece
    fp16 forms (GEMM 2 of the Winograd form is the direct one); the bf16x3 terms of gemm1_bar with 256 products."""
    r = dict(S=t["S2"], y=t["o"])
    if num in ("f32", "wino"):
        return conv_bound(r, DC)
    if num == "bf16x3":
        return 2.0 ** -23 * t["S2"] + gamma(6 * DC + 4) * (1 + 2.0 ** -7) * t["S2"] + 4 * U * t["o"].abs()
    rr = conv_ref(t["z"], Wo, bias=bo)
    m = conv_x2_ref(t["z"], Wo, k2, bias=bo)
    ones = conv_ref(t["z"], torch.ones(1, DC, 1))["S"]
    return conv_x2_bound(rr, m, ones, Wo.abs().sum((1, 2)), k2, Cin=DC, K=1)


def gate_bar(yg, yf, bg, bf):
    """Bar of z = sigmoid(y_g) tanh(y_f) for pre-activations within bg / bf of the model's.  With a_g = max(|y_g| - bg, 0), a_f likewise,
    the least magnitudes on the two intervals, and m = sigmoid(-a_g) >= min(s, 1 - s), c = 1 - tanh(a_f) >= 1 - |tanh| on them:
      values  sigmoid' = s (1 - s) <= m (1 - m) (<= 1/4) and tanh' = 1 - tanh^2 <= 1 - tanh(a_f)^2 (<= 1), both falling in |y|; |tanh|, s <= 1:
              |s' t' - s t| <= m (1 - m) bg + (1 - tanh(a_f)^2) bf                                   (<= 1/4 bg + bf)
      device  functions (v_exp_f32 and v_rcp_f32: 2 u relative each; expf(a) = exp2(fl(a log2 e)): |a| u more), following the derivation in
              tests/test_diffnet_bf16_reference.py but keeping the factors it bounds by 1:
              sigmoid(a) = rcp(1 + E), E = expf(-a).  a < 0: relative error (|a| + 5) u of s.  a > 0: E <= 2 (1 - s) is off by (|a| + 2) u E,
              the add and rcp round: <= 2 (1 - s) (|a| + 2) u + 3 u.                  Both: ds <= 2 m (|a| + 5) u + 3 u
              tanh(a) = 1 - 2 t, t = rcp(1 + expf(2 a)).  a > 0: 2 t = 1 - tanh, off by (2 |a| + 5) u relative, the subtraction rounds.
              a < 0: E <= 1 - |tanh|, 2 dt <= 2 E (2 |a| + 2) u + 6 u, + u.             Both: dth <= c (4 |a| + 10) u + 7 u
              z = s th rounds once:  dz <= ds + dth + u = (2 m (|y_g| + 5) + c (4 |y_f| + 10) + 11) u
              (unsaturated, m = 1/2 and c = 1: (|y_g| + 4 |y_f| + 26) u against the (|y_g| + 4 |y_f| + 17) u derived there; saturated: 11 u)."""
    ag, af = (yg.abs() - bg).clamp(min=0), (yf.abs() - bf).clamp(min=0)
    m, c = torch.sigmoid(-ag), 1 - torch.tanh(af)
    return m * (1 - m) * bg + (1 - torch.tanh(af) ** 2) * bf + U * (2 * m * (yg.abs() + bg + 5) + c * (4 * (yf.abs() + bf) + 10) + 11)


def bars(tr, o, num, exact0=False, forced=()):
    """Per layer: bar of y, z, o, x (= x_l) and of the running skip sum, for the numerics class `num`.  exact0: layer 0 runs on exact-mode
    operands, whose budget (test_exact_cases_meet_their_budget) makes y, z, o and the skip sum exact in any order: only x_l rounds.
    forced: the layers whose input was teacher-forced (stack(forced=...)): their input carries no error.  Without it the worst-case
    propagation through |W_dil| and |W_out| grows by two orders of magnitude per layer, and from the third layer on the bar is as large
    as the signal: bounded mode is sharp for L <= 2 and for the training forward (every x_l visible), a sanity bound beyond.
      bar_y    = gemm1_bar + |W_dil| (*) bar_x          (the error of the layer's input through the same taps)
      bar_z    = gate_bar(y_g, y_f, bar_g, bar_f)
      bar_o    = gemm2_bar + |W_out| @ bar_z
      bar_x    = (bar_x + bar_o[:256]) 2^-1/2 + 4 u |x_l|     (the add, the product with the fp32 constant, float64 against it)
      bar_skip = bar_skip + bar_o[256:] + u |skip|            (one add per layer behind the first)"""
    bx, bs, out = torch.zeros_like(tr[0]["xin"]), None, []
    for l, t in enumerate(tr):
        Wd, Wo = o["Wd"][l], o["Wo"][l]
        k1, k2 = (R.x2_exponent(Wd), R.x2_exponent(Wo)) if num in ("f16x2", "f16x2v") else (None, None)
        if l in forced:
            bx = torch.zeros_like(bx)
        if exact0 and l == 0:
            zero = torch.zeros_like(t["y"])
            bx, bs = 4 * U * t["x"].abs(), zero[:, DC:]
            out.append(dict(y=zero, z=zero[:, :DC], o=zero, x=bx, skip=bs))
            continue
        by = gemm1_bar(t, Wd, o["bd"][l], num, k1) + conv_ref(bx, Wd.abs(), dil=t["dil"], pad=t["dil"])["y"]
        bg, bf, yg, yf = by[:, :DC], by[:, DC:], t["y"][:, :DC], t["y"][:, DC:]
        bz = gate_bar(yg, yf, bg, bf)
        bo = gemm2_bar(t, Wo, o["bo"][l], num, k2) + torch.einsum("oc,bct->bot", Wo[:, :, 0].double().abs(), bz)
        bx = (bx + bo[:, :DC]) * RSQRT2 + 4 * U * t["x"].abs()
        bs = bo[:, DC:] if bs is None else bs + bo[:, DC:] + U * t["skip"].abs()
        out.append(dict(y=by, z=bz, o=bo, x=bx, skip=bs))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the plan: mirrors of plan_stack, of `concat` and of the queue geometry
# ------------------------------------------------------------------------------------------------------------------------
def plan(B, T, dcl, env, *, have_wino=True, have_split=True, x3_mode=2, aligned8=True, plain=True, n_cu=N_CU):
    """plan_stack (csrc/diffusion_loop.hip) line by line; env: the SET_AMD_* switches as a dict of strings."""
    ei = lambda n, dflt=None: int(env[n]) if n in env else dflt
    if not plain:  # stack_plan: the training outputs leave only the fp32 queue kernels
        have_split, x3_mode = False, 0
    wino_env, wino_set = ei("SET_AMD_WINO", 0), "SET_AMD_WINO" in env
    f32_pinned = ei("SET_AMD_SPLIT_F32", 0) != 0
    have_x3 = x3_mode in (2, 3)
    tiles64, split_blocks = B * ((T + 63) // 64), 4 * B * ((T + 31) // 32)
    split_fits = have_split and dcl <= 4 and split_blocks <= (1 if have_x3 and not f32_pinned else 2) * n_cu
    split_pays = split_blocks <= (1 if have_x3 else 2) * n_cu
    p = dict(family=None, split_x2=False, x3_wino=False, x3_ncb=0)
    se = ei("SET_AMD_SPLIT", 1)
    if split_fits and (se == 2 or (se == 1 and not wino_set and split_pays)):
        p.update(family=3, split_x2=x3_mode == 2 and not f32_pinned)
        return p
    xe = ei("SET_AMD_X3", 1)
    if have_x3 and dcl <= 4 and (xe == 2 or (xe == 1 and not wino_set and tiles64 >= 8)):
        narrow = 5 * tiles64 < 3 * n_cu
        if "SET_AMD_X3_TILE" in env:
            narrow = ei("SET_AMD_X3_TILE") == 32
        p.update(family=4 if x3_mode == 3 else 5, x3_ncb=1 if narrow else 2)
        xw = ei("SET_AMD_X3_WINO", 1)
        if x3_mode == 2 and dcl == 1 and T % 2 == 0 and not narrow and xw > 0 and aligned8:
            tiles96 = (B * ((T + 31) // 32) + 2) // 3
            p.update(x3_wino=True, x3_ncb=xw if xw in (2, 3) else (3 if tiles96 >= n_cu else 2))
        return p
    ncb = 1 if tiles64 < 3 * n_cu else 2
    if "SET_AMD_STACK_NCB" in env:
        ncb = 2 if ei("SET_AMD_STACK_NCB") == 2 else 1
    wino_ok = have_wino and (1 << (dcl - 1)) <= WINO_MAX_DIL
    wino = wino_ok and 25 * tiles64 >= 17 * n_cu
    if wino_set:
        wino = wino_ok and (wino_env == 2 or (wino and wino_env != 0))
    p.update(family=2 if wino else (1 if ncb == 1 else 0))
    return p


def concat_terms(c):
    """The terms of `concat` (set_launch_diffnet_stack_f32) that are FALSE for the row; empty = the concatenated frame axis is on."""
    off = []
    if c["dcl"] != 1:
        off.append("dcl")
    if c["T"] % 2:
        off.append("odd_T")
    if c["T"] < 64:
        off.append("short_T")
    if c["d_bs"] != 0:
        off.append("d_bs")
    if c["train"]:
        off.append("train")
    assert cp_bs(c) * 4 < 2 ** 31
    return off


def stack_grid(workers, ntiles, ntasks, cap_4_5, floor):
    """stack_grid (csrc/stack_queue.h) without its environment override."""
    grid = workers
    if cap_4_5 and grid > ntiles * 4 // 5:
        grid = ntiles * 4 // 5
    if grid < floor:
        grid = floor if floor < ntiles else ntiles
    return max(1, min(grid, ntasks))


def tiling(c, p, n_cu=N_CU):
    """What a launch of the row under plan p leaves in sync_ws: `words` cleared (stack_sync_words; everything behind keeps what it held),
    the final task `counter` (every worker claims once more than it runs: tasks + workers; the row-split kernels have no queue), the
    value of each of the `ntiles` tile flags (layers done; the x3v form counts 8 waves per layer)."""
    B, T, L = c["B"], c["T"], c["L"]
    nb32, fam = (T + 31) // 32, p["family"]
    if fam == 3:
        nt = B * nb32
        return dict(kind="row_split", ntiles=nt, words=4 + 2 * nt, counter=0, flag=None, concat=False)
    if fam in (4, 5):
        nt = -(-B * nb32 // p["x3_ncb"])
        grid = stack_grid(n_cu, nt, nt * L, (not p["x3_wino"]) or p["x3_ncb"] == 2, 0)
        return dict(kind="x3v" if p["x3_wino"] else "x3", ntiles=nt, words=4 + nt, counter=nt * L + grid, flag=(8 if p["x3_wino"] else 1) * L, concat=False)
    wino, ntt = fam == 2, 32 if fam == 1 else 64
    nt, cc = B * -(-T // ntt), wino and not concat_terms(c)
    if cc:
        nt = -(-B * T // 64)
    grid = stack_grid((1 if wino else 2) * n_cu, nt, nt * L, True, n_cu)
    return dict(kind="wino" if wino else "direct", ntiles=nt, words=4 + nt + (12 if wino else 0), counter=nt * L + grid, flag=L, concat=cc)


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
_F32 = {"SET_AMD_X3": "0", "SET_AMD_SPLIT": "0"}
_X3 = {"SET_AMD_X3": "2", "SET_AMD_SPLIT": "0", "SET_AMD_X3_WINO": "0"}
_X3V = {"SET_AMD_X3": "2", "SET_AMD_SPLIT": "0", "SET_AMD_X3_TILE": "64"}
# form -> environment, split-operand images held, expected family (ops.stack_variant), ops.stack_x3_winograd, tile width, numerics class
FORMS = {
    "layer": dict(env={}, x3_mode=0, family=None, x3w=0, W=64, num="f32"),
    "direct32": dict(env=dict(_F32, SET_AMD_WINO="0", SET_AMD_STACK_NCB="1"), x3_mode=2, family=1, x3w=0, W=32, num="f32"),
    "direct64": dict(env=dict(_F32, SET_AMD_WINO="0", SET_AMD_STACK_NCB="2"), x3_mode=2, family=0, x3w=0, W=64, num="f32"),
    "wino": dict(env=dict(_F32, SET_AMD_WINO="2"), x3_mode=2, family=2, x3w=0, W=64, num="wino"),
    "split_f32": dict(env={"SET_AMD_SPLIT": "2", "SET_AMD_SPLIT_F32": "1"}, x3_mode=2, family=3, x3w=0, W=32, num="f32"),
    "split_f32_noimg": dict(env={"SET_AMD_SPLIT": "2"}, x3_mode=0, family=3, x3w=0, W=32, num="f32"),
    "split_x2": dict(env={"SET_AMD_SPLIT": "2"}, x3_mode=2, family=3, x3w=0, W=32, num="f16x2"),
    "x3_bf16_32": dict(env=dict(_X3, SET_AMD_X3_TILE="32"), x3_mode=3, family=4, x3w=0, W=32, num="bf16x3"),
    "x3_bf16_64": dict(env=dict(_X3, SET_AMD_X3_TILE="64"), x3_mode=3, family=4, x3w=0, W=64, num="bf16x3"),
    "x3_f16_32": dict(env=dict(_X3, SET_AMD_X3_TILE="32"), x3_mode=2, family=5, x3w=0, W=32, num="f16x2"),
    "x3_f16_64": dict(env=dict(_X3, SET_AMD_X3_TILE="64"), x3_mode=2, family=5, x3w=0, W=64, num="f16x2"),
    "x3v_64": dict(env=dict(_X3V, SET_AMD_X3_WINO="2"), x3_mode=2, family=5, x3w=2, W=64, num="f16x2v"),
    "x3v_96": dict(env=dict(_X3V, SET_AMD_X3_WINO="3"), x3_mode=2, family=5, x3w=3, W=96, num="f16x2v"),
    # the x3v environment on a shape / an operand the predicate refuses: the direct two-piece form on 64-frame tiles must run
    "x3v_out": dict(env=dict(_X3V, SET_AMD_X3_WINO="2"), x3_mode=2, family=5, x3w=0, W=64, num="f16x2"),
}
SWITCHES = ("SET_AMD_X3", "SET_AMD_SPLIT", "SET_AMD_SPLIT_F32", "SET_AMD_WINO", "SET_AMD_STACK_NCB", "SET_AMD_X3_TILE", "SET_AMD_X3_WINO",
            "SET_AMD_STACK_GRID", "SET_AMD_FAULT_TILE", "SET_AMD_SPLIT_OPERAND")


def _row(form, B, T, L, dcl, why, **kw):
    """d_bs / ncol / col: the step table is [L 256][ncol] (d_cs = ncol), the row's column `col` (+ b when d_bs = 1: a column per utterance);
    cp_pad: floats between the utterances of condproj (cp_bs = L 512 T + cp_pad); cp_off: floats the condproj view is moved off its 256-byte
    alignment; train: x_all / save_y / save_z given; dense: also run the dense exact family (L = 1); bounded: run bounded mode."""
    c = dict(form=form, B=B, T=T, L=L, dcl=dcl, why=why, d_bs=0, ncol=1, col=0, cp_pad=0, cp_off=0, train=False, dense=L == 1, bounded=False, tag="")
    c.update(kw)
    assert c["ncol"] > c["col"] + (B - 1) * c["d_bs"]
    c["name"] = "%s_B%d_T%d_L%d_d%d%s" % (form, B, T, L, dcl, c["tag"])
    return c


def cp_bs(c):
    return c["L"] * 512 * c["T"] + c["cp_pad"]


def _t_rows(form, Ts, spec):
    """One row per T of `Ts`, the batch, depth, dilation cycle and strides cycling through `spec`."""
    rows = []
    for i, T in enumerate(Ts):
        B, L, dcl, kw = spec[i % len(spec)]
        rows.append(_row(form, B, T, L, dcl, "T = %d against the %d-frame tile of %s" % (T, FORMS[form]["W"], form), **kw))
    return rows


_S32 = [(1, 1, 1, dict(bounded=True)), (2, 2, 2, dict(ncol=3, col=1, bounded=True)), (3, 3, 3, dict(d_bs=1, ncol=5, col=1, cp_pad=40)), (2, 4, 4, {})]
CASES = (
    # ---- the per-layer kernel (first = 1 at layer 0, first = 0 behind it), dilation up to 8 through dilation_cycle_length = 4
    _t_rows("layer", (1, 63, 64, 65, 150), [(1, 1, 1, dict(bounded=True)), (2, 2, 2, dict(ncol=3, col=2, bounded=True)), (3, 3, 1, dict(d_bs=1, ncol=4)), (2, 4, 4, {})]) +
    [_row("layer", 2, T, 4, 4, "T = %d below dilation 8: both outer taps of layer 3 in the padding" % T) for T in (1, 3, 5)] +
    # ---- direct fp32 kernel
    _t_rows("direct32", (1, 31, 32, 33, 77), _S32) +
    [_row("direct32", 2, 5, 4, 4, "T = 5 below dilation 8"),
     _row("direct32", 3, 77, 4, 4, "dilation 8 taps cross 32-frame tiles, three utterances", bounded=True, cp_pad=8)] +
    _t_rows("direct64", (1, 63, 64, 65, 150), _S32) +
    # ---- fp32 Winograd kernel: UNIT_DIL true (dcl 1) and false (dcl 2 - 4), the concatenated frame axis on and off by each term
    _t_rows("wino", (1, 63, 65, 150), [(1, 1, 2, dict(bounded=True)), (2, 2, 3, dict(bounded=True)), (3, 3, 1, dict(tag="_odd")), (2, 4, 4, {})]) +
    [_row("wino", 3, 66, 3, 1, "concat on: utterance boundaries at frames 2 and 4 of tiles 1 and 2", bounded=True, ncol=3, col=2),
     _row("wino", 2, 64, 2, 1, "concat on: the boundary falls between two tiles"),
     _row("wino", 1, 150, 1, 1, "concat on with one utterance: ragged last tile (22 frames), T % 4 = 2"),
     _row("wino", 2, 62, 2, 1, "concat off by T < 64 alone (even T, dcl 1)"),
     _row("wino", 3, 66, 2, 1, "concat off by d_bs != 0 alone", d_bs=1, ncol=4, tag="_dbs", bounded=True),
     _row("wino", 3, 66, 2, 1, "concat off by the training outputs alone; x_all / save_y / save_z against x_l / y / z", train=True, tag="_train", bounded=True),
     _row("wino", 2, 150, 3, 3, "training forward with dilations 1, 2, 4, ragged tail", train=True, tag="_train", bounded=True),
     _row("wino", 2, 5, 4, 4, "T = 5 below dilation 8 (UNIT_DIL false, the largest dilation STACK_WINO_MAX_DIL admits)"),
     _row("wino", 1, 3, 4, 4, "T = 3 below dilation 8"),
     _row("wino", 1, 64, 1, 1, "T = W, concat on, one tile")] +
    # ---- row-split kernels: fp32 pipe (pinned, and for want of split-operand images) and two-piece fp16 (L = 1: no warmer blocks)
    _t_rows("split_f32", (1, 31, 32, 33, 77), _S32) +
    [_row("split_f32_noimg", 2, 77, 2, 2, "row-split fp32 because no split-operand image is held", bounded=True),
     _row("split_f32_noimg", 1, 33, 1, 1, "the same, L = 1")] +
    _t_rows("split_x2", (1, 31, 32, 33, 77), _S32) +
    [_row("split_x2", 3, 66, 1, 1, "L = 1 on three utterances: no warmer blocks", bounded=True),
     _row("split_x2", 2, 5, 4, 4, "T = 5 below dilation 8")] +
    # ---- split-operand kernels, direct form, both tile widths
    _t_rows("x3_bf16_32", (1, 31, 32, 33, 77), _S32) +
    _t_rows("x3_f16_32", (1, 31, 32, 33, 77), _S32) +
    _t_rows("x3_bf16_64", (1, 63, 64, 65, 150), _S32) +
    _t_rows("x3_f16_64", (1, 63, 64, 65, 150), _S32) +
    [_row(f, 3, 66, 2, 1, "three column blocks per utterance: 64-frame tiles straddle the utterance boundaries", bounded=True) for f in ("x3_bf16_64", "x3_f16_64")] +
    [_row(f, 2, 5, 4, 4, "T = 5 below dilation 8") for f in ("x3_bf16_32", "x3_f16_64")] +
    # ---- split-operand Winograd form (dilation 1, even T): 64- and 96-frame tiles
    _t_rows("x3v_64", (2, 62, 64, 66, 150), [(1, 1, 1, dict(bounded=True)), (2, 2, 1, dict(ncol=3, col=1, bounded=True)), (3, 3, 1, dict(d_bs=1, ncol=5, col=1, cp_pad=40)), (2, 4, 1, {})]) +
    _t_rows("x3v_96", (2, 94, 96, 98, 198), [(1, 1, 1, dict(bounded=True)), (2, 2, 1, dict(ncol=3, col=1, bounded=True)), (3, 3, 1, dict(d_bs=1, ncol=5, col=1, cp_pad=40)), (2, 4, 1, {})]) +
    [_row("x3v_64", 3, 66, 2, 1, "an utterance boundary inside a 64-frame tile of three-block utterances", bounded=True, tag="_utt"),
     _row("x3v_96", 3, 34, 3, 1, "utterances of two column blocks: both 96-frame tiles hold an utterance boundary", bounded=True, tag="_utt"),
     _row("x3v_96", 2, 130, 2, 1, "five blocks per utterance: every 96-frame tile starts at another block of its utterance")] +
    # ---- the x3v predicate refusing: the direct two-piece form runs
    [_row("x3v_out", 2, 65, 2, 1, "fall-out by odd T"),
     _row("x3v_out", 2, 66, 2, 2, "fall-out by dilation_cycle_length > 1"),
     _row("x3v_out", 2, 66, 2, 1, "fall-out by condproj 4 bytes off (aligned8 false)", cp_off=1, tag="_off4", bounded=True)]
)
BY_NAME = {c["name"]: c for c in CASES}


def aligned8(c):
    return c["cp_off"] % 2 == 0 and cp_bs(c) % 2 == 0 and (512 * c["T"]) % 2 == 0


def row_plan(c, n_cu=N_CU):
    f = FORMS[c["form"]]
    return plan(c["B"], c["T"], c["dcl"], f["env"], x3_mode=f["x3_mode"], aligned8=aligned8(c), plain=not c["train"], n_cu=n_cu)


def numerics(c):
    return FORMS[c["form"]]["num"]


def _seed(name, tag):
    return zlib.crc32(("%s/%s" % (name, tag)).encode()) & 0x7FFFFFFF


def step_table(g, c, exact):
    """[L 256][ncol]: the row's columns hold the offsets, every other column is at least 1000 away, so a wrong column moves every
    pre-activation by far more than any bar (exact mode: flips z)."""
    L, ncol = c["L"], c["ncol"]
    if exact:  # odd multiples of 1/2 in [-1.5, 1.5]; behind layer 1 odd multiples of 1/4 in [-1.25, 1.25]
        tab = (torch.randint(0, 4, (L * DC, ncol), generator=g).float() - 1.5)
        if L > 2:
            tab[2 * DC:] = torch.randint(0, 6, ((L - 2) * DC, ncol), generator=g).float() * 0.5 - 1.25
    else:
        tab = torch.randn(L * DC, ncol, generator=g)
    used = {c["col"] + b * c["d_bs"] for b in range(c["B"])}
    for j in range(ncol):
        if j not in used:
            tab[:, j] += 1000.0 * (j + 1)
    return tab


def offsets(c, tab):
    """d [L][B][256] as the kernels address the table: tab[l 256 + ch][col + b d_bs]."""
    return torch.stack([torch.stack([tab[l * DC:(l + 1) * DC, c["col"] + b * c["d_bs"]] for b in range(c["B"])]) for l in range(c["L"])])


def sel_positions(c, l, fam):
    """(channel, tap) of the one non-zero weight of filter row r: slot 7 r + shift mod 768 (7 is prime to 768: 256 distinct slots, every tap)."""
    shift = _seed(c["name"], "shift%d%s" % (l, fam)) % 768
    p = (7 * torch.arange(DC) + shift) % 768
    return p % DC, p // DC


@functools.lru_cache(maxsize=8)
def _exact(name, fam):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(name, "exact" + fam))
    B, T, L = c["B"], c["T"], c["L"]
    assert fam == "sel" or L == 1
    o = dict(c, mode="exact", fam=fam, dils=dilations(L, c["dcl"]))
    o["x0"] = ints(g, (B, DC, T), -3, 3)
    o["tab"] = step_table(g, c, True)
    o["d"] = offsets(c, o["tab"])
    Wd, bd, cp = torch.zeros(L, 512, DC, 3), torch.zeros(L, 512), torch.zeros(B, L, 512, T)
    cp[:, :, :DC] = 40.0
    Wo, bo = grid(g, (L, 512, DC, 1), 1), grid(g, (L, 512), 3)
    for l in range(L):
        mag = W0 if l == 0 else W1
        sign = (torch.randint(0, 2, (DC,), generator=g) * 2 - 1).float()
        if fam == "dense":
            Wd[l, DC:] = W0 * ints(g, (DC, DC, 3), -1, 1)
        else:
            ch, tap = sel_positions(c, l, fam)
            Wd[l, DC + torch.arange(DC), ch, tap] = mag * sign
        if l == 0:
            bd[l, DC:] = 16.0 * ints(g, (DC,), -1, 1)
            cp[:, l, DC:] = 16.0 * ints(g, (B, DC, T), -1, 1)
        else:
            cp[:, l, DC:] = CP1 * (torch.randint(0, 2, (B, DC, T), generator=g) * 2 - 1).float()
        if L > 1:  # the residual rows: 8 x a signed permutation, no bias, so x_l stays on a small lattice
            perm = torch.randperm(DC, generator=g)
            Wo[l, :DC] = 0
            Wo[l, torch.arange(DC), perm, 0] = 8.0 * (torch.randint(0, 2, (DC,), generator=g) * 2 - 1).float()
            bo[l, :DC] = 0
    o.update(Wd=Wd, bd=bd, Wo=Wo, bo=bo, cp=cp.reshape(B, L * 512, T).contiguous())
    o["tr"] = stack(o["x0"], o["cp"], o["d"], Wd, bd, Wo, bo, o["dils"], z32=True)
    return o


def make_exact(c, fam="sel"):
    return _exact(c["name"], fam)


SCALES = (1.0, 8.0)


@functools.lru_cache(maxsize=8)
def _gauss(name, scale):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(name, "gauss%g" % scale))
    B, T, L = c["B"], c["T"], c["L"]
    rn = lambda *s: torch.randn(*s, generator=g)
    o = dict(c, mode="bounded", scale=scale, dils=dilations(L, c["dcl"]))
    o["Wd"], o["bd"] = rn(L, 512, DC, 3) / 27.7, rn(L, 512) * 0.1
    o["Wo"], o["bo"] = rn(L, 512, DC, 1) / 16 * scale, rn(L, 512) * 0.1
    o["cp"] = rn(B, L * 512, T) * 0.5
    o["x0"] = rn(B, DC, T) * math.sqrt(scale)
    o["tab"] = step_table(g, c, False)
    o["d"] = offsets(c, o["tab"])
    o["tr"] = stack(o["x0"], o["cp"], o["d"], o["Wd"], o["bd"], o["Wo"], o["bo"], o["dils"])
    return o


def make_gauss(c, scale):
    """The _random_stack recipe of tests/test_gpu_parity.py; scale 8: the output convolution, and with it x_l and the skip sum, 8 x larger."""
    return _gauss(c["name"], scale)


# ------------------------------------------------------------------------------------------------------------------------
# CPU checks
# ------------------------------------------------------------------------------------------------------------------------
def test_model_equals_the_loop_model_and_the_oracle_layers_in_float64():
    """stack() against test_loop_reference.layers (the model the loop sweep stands on) and, layer by layer, against oracle.residual_block
    on float64 weights, dilation cycle 3 over 4 layers, a step offset per utterance.  The only difference is the fp32 constant
    fl32(2^-1/2) the kernels multiply by (relative 2.4e-8 per layer) where both references divide by sqrt 2."""
    from oracle import oracle as O
    g = torch.Generator().manual_seed(3)
    B, T, L, dcl, H = 2, 37, 4, 3, 24
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Wd, bd, Wo, bo = rn(L, 512, DC, 3) / 27.7, rn(L, 512) * 0.1, rn(L, 512, DC, 1) / 16, rn(L, 512) * 0.1
    Wc, bc, Wp, bp = rn(L, 512, H, 1) / 5, rn(L, 512) * 0.1, rn(L, DC, DC) / 16, rn(L, DC) * 0.1
    x0, cond, emb = rn(B, DC, T), rn(B, H, T), rn(B, DC)
    cp = torch.cat([torch.nn.functional.conv1d(cond, Wc[l], bc[l]) for l in range(L)], 1)
    d = torch.stack([torch.nn.functional.linear(emb, Wp[l], bp[l]) for l in range(L)])
    tr = stack(x0, cp, d, Wd, bd, Wo, bo, dilations(L, dcl))
    x, skip = x0, 0
    for l in range(L):
        W = {"diffusion_projection.weight": Wp[l], "diffusion_projection.bias": bp[l], "conditioner_projection.weight": Wc[l],
             "conditioner_projection.bias": bc[l], "dilated_conv.weight": Wd[l], "dilated_conv.bias": bd[l],
             "output_projection.weight": Wo[l], "output_projection.bias": bo[l]}
        x, s = O.residual_block(W, "", x, cond, emb, 1 << (l % dcl))
        skip = skip + s
        tol = 1e-7 * (l + 1)
        assert float((tr[l]["x"] - x).abs().max()) <= tol * float(x.abs().max()), l
        assert float((tr[l]["skip"] - skip).abs().max()) <= tol * max(1.0, float(skip.abs().max())), l
        assert float((tr[l]["o"][:, DC:] - s).abs().max()) <= tol * max(1.0, float(s.abs().max())), l
    # one step offset for the whole batch: the loop model's signature
    tr1 = stack(x0, cp, d[:, :1].expand(L, B, DC), Wd, bd, Wo, bo, dilations(L, dcl))
    xl, sk = R.layers(x0, cp, d[:, 0].reshape(-1), Wd, bd, Wo, bo, dcl)
    assert float((tr1[-1]["x"] - xl).abs().max()) <= 1e-7 * L * float(xl.abs().max())
    assert float((tr1[-1]["skip"] - sk).abs().max()) <= 1e-7 * L * float(sk.abs().max())
    # the magnitude sums dominate what they bound and the gate is what the header says
    for t in tr:
        assert bool((t["S1"] >= t["y"].abs() - 1e-9).all()) and bool((t["S2"] >= t["o"].abs() - 1e-9).all())
        assert bool((t["z"].abs() <= 1).all())


def test_wino_sums_dominate_both_outputs_of_a_pair():
    """SW of wino_sums is at least |U0 V0| + |U1 V1| + |U2 V2| summed over the channels for a frame taken as the even output and at least the
    odd form for the same frame taken as the odd output, for dilations 1 and 4; and the F(2,3) identity itself holds for these operands."""
    g = torch.Generator().manual_seed(9)
    Wd, v = torch.randn(512, DC, 3, generator=g).double(), torch.randn(1, DC, 40, generator=g).double()
    for dil in (1, 4):
        SW, SU, SV = wino_sums(dict(xd=v, dil=dil), Wd)
        U0, U1, U2, U3 = Wd[:, :, 0], 0.5 * Wd.sum(-1), 0.5 * (Wd[:, :, 0] - Wd[:, :, 1] + Wd[:, :, 2]), Wd[:, :, 2]
        t0 = 12
        d0, d1, d2, d3 = (v[0, :, t0 + k * dil] for k in (-1, 0, 1, 2))
        m0, m1, m2, m3 = U0 * (d0 - d2), U1 * (d1 + d2), U2 * (d2 - d1), U3 * (d1 - d3)
        y = torch.nn.functional.conv1d(v, Wd, padding=dil, dilation=dil)[0]
        assert float(((m0 + m1 + m2).sum(1) - y[:, t0]).abs().max()) < 1e-9 and float(((m1 - m2 - m3).sum(1) - y[:, t0 + dil]).abs().max()) < 1e-9
        assert bool((SW[0, :, t0] >= (m0.abs() + m1.abs() + m2.abs()).sum(1) - 1e-9).all())
        assert bool((SW[0, :, t0 + dil] >= (m1.abs() + m2.abs() + m3.abs()).sum(1) - 1e-9).all())
        assert bool((SV[0, 0, t0] >= ((d0 - d2).abs() + (d1 + d2).abs() + (d2 - d1).abs()).sum() - 1e-9))
        assert bool((SU >= (U0.abs() + U1.abs() + U2.abs()).sum(1) - 1e-9).all())


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case_reaches_the_form_it_names(built_lib, monkeypatch, c):
    """The library's own shape queries under the row's environment (no device: 256 CUs, aligned operands, no training outputs) against the
    mirror and against the family / x3v tile width the row's form names; the mirror with the row's own alignment and outputs gives the form
    that must run on the GPU."""
    from set_amd import ops
    f = FORMS[c["form"]]
    if f["family"] is None:
        return
    for n in SWITCHES:
        monkeypatch.delenv(n, raising=False)
    for n, v in f["env"].items():
        monkeypatch.setenv(n, v)
    q = plan(c["B"], c["T"], c["dcl"], f["env"], x3_mode=f["x3_mode"])
    assert ops.stack_variant(c["B"], c["T"], c["dcl"], x3_mode=f["x3_mode"]) == q["family"], c["name"]
    assert ops.stack_x3_winograd(c["B"], c["T"], c["dcl"], x3_mode=f["x3_mode"]) == (q["x3_ncb"] if q["x3_wino"] else 0), c["name"]
    p = row_plan(c)
    assert p["family"] == f["family"] and (p["x3_ncb"] if p["x3_wino"] else 0) == f["x3w"], (c["name"], p)
    if not c["train"] and aligned8(c):
        assert p == q
    if f["family"] == 3:
        assert p["split_x2"] == (f["num"] == "f16x2")
    if f["family"] in (4, 5):
        assert 32 * p["x3_ncb"] == f["W"]
    # the words the launch clears fit the workspace callers allocate, and the class the bars are composed for is a known one
    assert ops.sync_ws_size(c["B"], c["T"]) >= tiling(c, p)["words"] and f["num"] in NUMERICS


def _t_class(T, W):
    return {1: "1", 2: "2", W - 2: "W-2", W - 1: "W-1", W: "W", W + 1: "W+1", W + 2: "W+2"}.get(T, "2W+tail" if T > 2 * W and T % W else "other")


def conditions(c):
    """The branch conditions a row meets, computed from the mirrors (never written by hand)."""
    f, p, tags = FORMS[c["form"]], row_plan(c) if FORMS[c["form"]]["family"] is not None else None, set()
    form, W, T, dcl, L = c["form"], f["W"], c["T"], c["dcl"], c["L"]
    tags |= {("T", form, _t_class(T, W)), ("L_parity", form, L % 2), ("dcl", dcl)}
    if T % 4:
        tags.add(("T%4", form))
    if max(dilations(L, dcl)) == 8 and T < 8:
        tags.add(("T<dil", form))
    if max(dilations(L, dcl)) == 8 and W == 32 and T > 32:
        tags.add(("tap_crosses_tiles", form))
    if c["ncol"] > 1:
        tags.add("d_cs")
    if c["d_bs"]:
        tags.add("d_bs")
    if c["cp_pad"]:
        tags.add("cp_view")
    if form == "layer":
        tags |= {("first", 1)} | ({("first", 0)} if L > 1 else set())
        return tags
    t = tiling(c, p)
    tags |= {("family", p["family"]), ("kind", t["kind"])}
    if p["family"] == 3:
        tags |= {("split_x2", p["split_x2"]), ("split_f32_by", "pin" if "SET_AMD_SPLIT_F32" in f["env"] else "no_image") if not p["split_x2"] else ("warmers", L > 1 and 4 * t["ntiles"] + 8 <= N_CU)}
    if p["family"] in (4, 5):
        tags.add(("x3", p["family"], p["x3_wino"], p["x3_ncb"]))
        nbu = (T + 31) // 32
        if c["B"] > 1 and nbu % p["x3_ncb"]:
            tags.add(("utterance_boundary_in_tile", form))
        if f["env"].get("SET_AMD_X3_WINO", "0") != "0" and not p["x3_wino"]:
            tags |= {("x3v_out", why) for why, hit in (("odd_T", T % 2), ("dcl", dcl > 1), ("aligned8", not aligned8(c))) if hit}
    if p["family"] == 2:
        tags |= {("wino_unit_dil", dcl == 1), ("wino_max_dil", 1 << (dcl - 1))}
        off = concat_terms(c)
        tags.add(("concat", not off))
        if len(off) == 1 or off == ["dcl"]:
            tags.add(("concat_off", off[0]))
        if not off and c["B"] > 1 and T % 64:
            tags.add(("utterance_boundary_in_tile", form))
        if c["train"]:
            tags.add("train")
    return tags


STACK_FORMS = [f for f in FORMS if f != "layer"]
REQUIRED = (
    {("family", v) for v in range(6)} | {("kind", k) for k in ("direct", "wino", "row_split", "x3", "x3v")} |
    {("split_x2", False), ("split_x2", True), ("split_f32_by", "pin"), ("split_f32_by", "no_image"), ("warmers", False), ("warmers", True)} |
    {("x3", fam, False, ncb) for fam in (4, 5) for ncb in (1, 2)} | {("x3", 5, True, 2), ("x3", 5, True, 3)} |
    {("x3v_out", w) for w in ("odd_T", "dcl", "aligned8")} |
    {("wino_unit_dil", True), ("wino_unit_dil", False), ("wino_max_dil", 8), ("concat", True), ("concat", False), "train"} |
    {("concat_off", w) for w in ("dcl", "odd_T", "short_T", "d_bs", "train")} |
    {("first", 0), ("first", 1), "d_cs", "d_bs", "cp_view"} | {("dcl", k) for k in (1, 2, 3, 4)} |
    {("T", f, k) for f in FORMS if f not in ("x3v_64", "x3v_96", "x3v_out", "split_f32_noimg") for k in ("1", "W-1", "W", "W+1", "2W+tail")} |
    {("T", f, k) for f in ("x3v_64", "x3v_96") for k in ("2", "W-2", "W", "W+2", "2W+tail")} |
    {("T%4", f) for f in FORMS if f != "split_f32_noimg"} |
    {("L_parity", f, k) for f in FORMS if f not in ("x3v_out", "split_f32_noimg") for k in (0, 1)} |
    {("T<dil", f) for f in ("layer", "direct32", "wino", "split_x2", "x3_bf16_32", "x3_f16_64")} |
    {("tap_crosses_tiles", f) for f in ("direct32", "split_f32", "split_x2", "x3_bf16_32", "x3_f16_32")} |
    {("utterance_boundary_in_tile", f) for f in ("wino", "x3_bf16_64", "x3_f16_64", "x3v_64", "x3v_96")}
)
# conditions of the three predicates that no row can make false, and why
UNREACHED = {
    "wino_ok by STACK_WINO_MAX_DIL": "stack_validate admits dilation_cycle_length <= 4, so 1 << (dcl - 1) <= 8 always holds",
    "dcl <= 4 of split_fits / of the x3 branch": "the same validation",
    "concat off by cp_bs * 4 >= 2^31": "needs a condproj view of more than 2 GiB per utterance (the 2 GiB limits are not swept, as in the loop sweep)",
    "x3v off by `narrow`": "SET_AMD_X3_TILE=32 with SET_AMD_X3_WINO set is the direct 32-frame form, which x3_f16_32 already names",
}


def test_inventory_is_complete():
    """Every form, every family and kernel kind, every term of plan_stack, of `concat` and of the x3v predicate that a caller can reach,
    every T class against every form's tile width, both parities of L per form, dilation cycles 1 - 4, the step-table strides and the
    condproj view have a row; names are unique; shapes stay small."""
    assert len(BY_NAME) == len(CASES) and all(c["why"] for c in CASES)
    have = set().union(*(conditions(c) for c in CASES))
    assert not (REQUIRED - have), sorted(map(str, REQUIRED - have))
    assert {c["form"] for c in CASES} == set(FORMS)
    assert all(c["B"] <= 3 and c["L"] <= 4 and c["T"] <= 200 for c in CASES)
    assert {c["B"] for c in CASES} == {1, 2, 3}
    for f in FORMS:
        assert any(c["bounded"] for c in CASES if c["form"] == f), f
        assert any(c["dense"] for c in CASES if c["form"] == f) or f == "x3v_out", f
    # a plan falling back to another form leaves another tiling word: the (counter, words, flag) triples of the forms differ on a shared shape
    c = dict(BY_NAME["x3v_64_B3_T66_L2_d1_utt"])
    seen = {}
    for f in ("direct32", "direct64", "wino", "split_x2", "x3_f16_32", "x3_f16_64", "x3v_64", "x3v_96"):
        cc = dict(c, form=f)
        t = tiling(cc, row_plan(cc))
        seen[f] = (t["counter"], t["words"], t["flag"])
    assert len(set(seen.values())) == len(seen), seen


def test_mirrors_by_hand():
    """The geometry mirrors on hand-computed rows."""
    c = BY_NAME["wino_B3_T66_L3_d1"]
    t = tiling(c, row_plan(c))  # 198 concatenated frames: 4 tiles, 12 tasks, min(256, 4 * 4 // 5 = 3) -> floor 256 > 4 tiles -> 4 workers
    assert (t["concat"], t["ntiles"], t["counter"], t["words"], t["flag"]) == (True, 4, 16, 20, 3)
    c = BY_NAME["wino_B3_T66_L2_d1_dbs"]
    t = tiling(c, row_plan(c))  # per utterance: 3 x 2 tiles
    assert (t["concat"], t["ntiles"], t["counter"], t["words"]) == (False, 6, 18, 22)
    c = BY_NAME["x3v_96_B3_T34_L3_d1_utt"]
    t = tiling(c, row_plan(c))  # 6 column blocks: 2 tiles of 96 frames, 6 tasks, no 4/5 cap: one worker per task
    assert (t["ntiles"], t["counter"], t["words"], t["flag"]) == (2, 12, 6, 24)
    c = BY_NAME["x3v_64_B3_T66_L2_d1_utt"]
    t = tiling(c, row_plan(c))  # 9 blocks: 5 tiles, 10 tasks, 5 * 4 // 5 = 4 workers
    assert (t["ntiles"], t["counter"], t["words"], t["flag"]) == (5, 14, 9, 16)
    c = BY_NAME["split_x2_B3_T66_L1_d1"]
    t = tiling(c, row_plan(c))
    assert (t["ntiles"], t["counter"], t["words"]) == (9, 0, 22)
    assert stack_grid(512, 416, 8320, True, 256) == 332 and stack_grid(256, 3, 9, True, 0) == 2 and stack_grid(256, 1, 4, True, 0) == 1


def _fp32(v):
    return bool((v.double().float().double() == v.double()).all())


def _multiple(v, q):
    return bool(((v.double() / q).round() * q == v.double()).all())


EXACT_RUNS = [(c, fam) for c in CASES for fam in (("sel", "dense") if c["dense"] else ("sel",))]


@pytest.mark.parametrize("c,fam", EXACT_RUNS, ids=["%s-%s" % (c["name"], fam) for c, fam in EXACT_RUNS])
def test_exact_cases_meet_their_budget(c, fam):
    """Layer 0: every filter pre-activation is a multiple of 16 and an fp32 number, S1 stays below 2^24 granules of 16 (any fp32 order is
    exact); two-piece forms: piece products within BUDGET_BITS, exact splits, nothing in the dropped product; bf16x3: every operand has at
    most 24 significant bits, so its three pieces carry it whole and the dropped products are zero; Winograd forms: the four weight
    planes and the four input planes are fp32 numbers on a grid whose products stay below 2^24 granules.  z of every layer is -1, 0 or
    +1 (0 only at layer 0), o is a multiple of 2^-12 below 2^24 granules, the skip sum too.  Layers behind the first: the margins of the
    module docstring on |x_l + d| and |y_f|, |y_f| less the bounded bar of the row's numerics at least 16, the bar of x_l below 2^-10.
    L = 1: x + o is an fp32 number, so x_out is one rounding."""
    o = make_exact(c, fam)
    tr, num, L = o["tr"], numerics(c), c["L"]
    t0 = tr[0]
    yf = t0["y"][:, DC:]
    assert _multiple(yf, 16.0) and _fp32(yf) and bool((t0["y"][:, :DC] == 40.0).all())
    assert float(t0["S1"].max()) < 2.0 ** 24 * 16.0 and _multiple(t0["xd"], 0.5) and float(t0["xd"].abs().min()) >= 0.5
    if num in ("f16x2", "f16x2v"):
        m = conv_x2_ref(t0["xd"], o["Wd"][0], R.x2_exponent(o["Wd"][0]), bias=o["bd"][0], dil=t0["dil"], pad=t0["dil"])
        assert m["bits"] < BUDGET_BITS and m["split_exact"] and not bool(m["dropped"].any()), (c["name"], m["bits"])
        assert torch.equal(m["y"] + t0["cp"], t0["y"])
    if num == "bf16x3":  # 24 significant bits at the most: granule / magnitude
        assert float(t0["xd"].abs().max()) / 0.5 < 2 ** 24 and float(o["Wd"][0].abs().max()) / W0 < 2 ** 24
    if num in ("wino", "f16x2v"):
        g = o["Wd"][0].double()
        planes = (g[:, :, 0], 0.5 * g.sum(-1), 0.5 * (g[:, :, 0] - g[:, :, 1] + g[:, :, 2]), g[:, :, 2])
        assert all(_multiple(u, 16.0) and _fp32(u) for u in planes)   # U on the grid of 16
        SW, SU, SV = wino_sums(t0, o["Wd"][0])                           # V on the grid of 1/2: products multiples of 8
        assert float(SW.max()) + 2 * float((o["bd"][0].abs().max() + t0["cp"].abs().max())) < 2.0 ** 24 * 8.0
        if num == "f16x2v":  # the planes, scaled by s / 2, and the transformed inputs are two-piece numbers with a zero low piece
            s = 2.0 ** (R.x2_exponent(o["Wd"][0]) - 1)
            assert all(bool((split2(u * s)[1] == 0).all()) and bool((split2(u * s)[0] == u * s).all()) for u in planes)
            assert 2 * float(t0["xd"].abs().max()) < 2048 and SV.shape[1] == 1  # |V| < 2^11 on the grid of 1/2: an fp16 number
    # GEMM 2 of every layer, the gate, the skip sum
    q = 2.0 ** -12
    for l, t in enumerate(tr):
        zs = set(t["z"].unique().tolist())
        assert zs <= ({-1.0, 0.0, 1.0} if l == 0 else {-1.0, 1.0}), (c["name"], l, sorted(zs)[:5])
        assert _multiple(t["o"], q) and float(t["S2"].max()) < 2.0 ** 24 * q and _multiple(t["skip"], q) and _fp32(t["skip"])
        if num in ("f16x2", "f16x2v"):
            m = conv_x2_ref(t["z"], o["Wo"][l], R.x2_exponent(o["Wo"][l]), bias=o["bo"][l])
            assert m["bits"] < BUDGET_BITS and m["split_exact"] and not bool(m["dropped"].any()) and m["lo_w"] > 0.1
            assert torch.equal(m["y"], t["o"])
    k1, k2 = R.x2_exponent(o["Wd"][0]), R.x2_exponent(o["Wo"][0])  # the pack exponents of the two-piece images: -2 and 3 (L = 1) / 0 (the 8s of L > 1)
    assert k1 != 0 and k1 != k2 and (L > 1 or k2 != 0) and (L == 1 or R.x2_exponent(o["Wd"][1]) not in (0, k1))
    if L == 1:
        assert _fp32(t0["xin"] + t0["o"][:, :DC])
        assert float(t0["z"].abs().mean()) > 0.5 and t0["skip"].unique().numel() > 100
        return
    b = bars(tr, o, num, exact0=True)
    for l in range(1, L):
        t = tr[l]
        assert float(b[l - 1]["x"].max()) < 2.0 ** -10, (c["name"], l, float(b[l - 1]["x"].max()))
        assert float(t["xd"].abs().min()) >= MARGIN, (c["name"], l, float(t["xd"].abs().min()))
        assert float(t["y"][:, DC:].abs().min()) >= 32.0, (c["name"], l, float(t["y"][:, DC:].abs().min()))
        room = (t["y"][:, DC:].abs() - b[l]["y"][:, DC:]).min()  # every pre-activation the form can compute stays at 16 or beyond
        assert float(room) >= 16.0, (c["name"], l, float(room))
        assert bool((t["y"][:, :DC] == 40.0).all())


def test_exact_budget_by_hand():
    """The worst case of the construction, by hand: layer 0 dense 768 x 32 x 4.5 + 16 + 16 + 40 granules of 16; GEMM 2 256 x (1 + 2^-12) + 3 + 2^-12
    in granules of 2^-12; the lattice of x_1 + d behind integer x in [-3, 3], o in [-2, 2] and |d| <= 1.5 stays MARGIN away from 0."""
    assert (768 * 32 * 4.5 + 72) / 16 < 2 ** 24 and (256 * (1 + 2.0 ** -12) + 4) * 2 ** 12 < 2 ** 24
    xs, half, quarter = set(range(-3, 4)), (-1.5, -0.5, 0.5, 1.5), (-1.25, -0.75, -0.25, 0.25, 0.75, 1.25)
    for l in range(4):  # x_l + d over every reachable x_l: x in [-3, 3], o in {-8, 0, 8}
        assert min(abs(x + d) for x in xs for d in (half if l < 2 else quarter)) > (0.04 if l else 0.49) > MARGIN
        xs = {round((x + o) * RSQRT2, 9) for x in xs for o in (-8, 0, 8)}
    assert W1 * MARGIN - CP1 >= 32.0 and W0 * 0.5 == 16.0
