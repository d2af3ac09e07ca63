"""Models and case tables of the bf16 reverse-loop sweep (no tests live here): the two opt-in step bodies of set_diffusion_loop
(csrc/diffusion_loop.hip: STEP_BF16_GROUPS and STEP_BF16_LAYERS, taken when SetDiffLoopArgs.img16_all is set) with the host code that
composes them -- plan_steps, step_bf16_groups, step_bf16_layers.  tests/test_bf16_loop_reference.py holds the CPU checks of what is
defined here, tests/test_gpu_bf16_loop_branches.py the GPU sweep.

  loop_c(o)               the plain float64 model: the loop of tests/test_loop_reference.py with the conditioner projection of layer l,
                          cp_l = Wc_l cond + b_cond_l, computed here (the bf16 kernels compute it inside the layer GEMM).  THE reference.
  loop_c(o, mirror=True)  the bf16-operand mirror: the same loop with x + d, cond, Wd, Wc, Wo and z rounded to bf16 (RNE) where the header
                          comment of csrc/diffnet_bf16.hip / the comment above SetDiffnetLayerBf16Args say the kernel rounds them; the
                          residual adds the UNROUNDED x; everything else stays float64.  Written from those comments and diffnet.py:60-81.
  book(o) / plant(...)    the loop's bookkeeping as plain tables (which dstep column, coef4 row and noise slice a step takes, which
                          utterance's cond, which layer's image and biases, which dilation, where `first` is set) and the fault planters
                          that edit them: what a wrong value in the host code would compute.
  make_gauss_c / make_exact_c   operands: make_gauss / make_exact of test_loop_reference.py in the conditioned form.
  plan_mirror(c)          Python mirror of plan_steps + set_diffnet_layers_bf16_plan + the group split of set_diffusion_loop.
  ROWS                    the case table: every row names the branch it reaches and the C condition it meets."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import test_diffnet_bf16_reference as D
import test_loop_reference as R
from test_bf16_reference import rne_bf16

DC, FH = 256, 192


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def cond_proj(o):
    """cp [B][L * 512][T] = Wc_l cond + b_cond_l, float64."""
    return torch.cat([torch.einsum("rh,bht->brt", o["Wc"][l].double(), o["cond"].double()) + o["bc"][l].double()[None, :, None]
                      for l in range(o["L"])], 1)


def book(o):
    """The bookkeeping of the loop, one table per value the host code computes (spec_denoiser.py:181, diffnet.py:123-127)."""
    L, steps, B = o["L"], o["steps"], o["B"]
    sid = [steps - 1 - k for k in range(steps)]
    return dict(dsid=list(sid), csid=list(sid), noise=list(range(steps)), cond_b=list(range(B)), img=list(range(L)), bias=list(range(L)),
                dil=[1 << (l % o["dcl"]) for l in range(L)], first=[l == 0 for l in range(L)])


def group_starts(B, M, T, n_groups):
    """First utterance of every group (set_diffusion_loop: G clamped to [1, 8] and to B; one group unless M T % 4 == 0)."""
    G = min(max(1, min(8, n_groups)), B)
    if (M * T) % 4 != 0:
        G = 1
    return [B * g // G for g in range(G)] + [B]


FAULTS = ("dstep_reversed", "noise_reversed", "coef4_reversed", "cond_of_utterance_0", "tail_biases_of_l0", "tail_image_of_l0",
          "dilation_cycle_shifted", "first_on_a_later_layer")


def plant(o, fault, fuse, n_groups):
    """The bookkeeping with one fault planted.  fuse / n_groups: the plan the fault lives in (tail group = the layers from the last
    multiple of fuse on; groups as set_diffusion_loop splits them)."""
    bk = book(o)
    L, steps, B = o["L"], o["steps"], o["B"]
    l0 = (L - 1) // fuse * fuse
    if fault == "dstep_reversed":
        bk["dsid"] = list(range(steps))
    elif fault == "noise_reversed":
        bk["noise"] = list(reversed(range(steps)))
    elif fault == "coef4_reversed":
        bk["csid"] = list(range(steps))
    elif fault == "cond_of_utterance_0":
        st = group_starts(B, o["M"], o["T"], n_groups)
        assert len(st) > 2
        bk["cond_b"] = [b - max(s for s in st[:-1] if s <= b) for b in range(B)]
    elif fault == "tail_biases_of_l0":
        assert 0 < l0 < L - 1
        bk["bias"] = [min(l, l0) for l in range(L)]
    elif fault == "tail_image_of_l0":
        assert 0 < l0 < L - 1
        bk["img"] = [min(l, l0) for l in range(L)]
    elif fault == "dilation_cycle_shifted":
        assert o["dcl"] > 1
        bk["dil"] = [1 << ((l + 1) % o["dcl"]) for l in range(L)]
    elif fault == "first_on_a_later_layer":
        assert 0 < l0
        bk["first"] = [l == 0 or l == l0 for l in range(L)]
    else:
        raise KeyError(fault)
    return bk


def layers_c(xin, o, dcol, bk, W, r):
    """The L layers (diffnet.py:60-81) on the tables bk: (x_0 .. x_L, skip sum).  W: the (rounded) weights and cond, r: the rounding
    of x + d and z (identity for the plain model)."""
    x, skip, xs = xin.double(), None, [xin.double()]
    cond = W["cond"][bk["cond_b"]]
    for l in range(o["L"]):
        i, j, d = bk["img"][l], bk["bias"][l], bk["dil"][l]
        dv = dcol[l * DC:(l + 1) * DC].double()[None, :, None]
        y = F.conv1d(r(x + dv), W["Wd"][i], None, padding=d, dilation=d) + torch.einsum("rh,bht->brt", W["Wc"][i], cond) + \
            (o["bd"][j].double() + o["bc"][j].double())[None, :, None]
        z = r(torch.sigmoid(y[:, :DC]) * torch.tanh(y[:, DC:]))
        out = torch.einsum("rc,bct->brt", W["Wo"][i], z) + o["bo"][j].double()[None, :, None]
        x = (x + out[:, :DC]) / 2 ** 0.5
        skip = out[:, DC:] if (bk["first"][l] or skip is None) else skip + out[:, DC:]
        xs.append(x)
    return xs, skip


def weights_of(o, mirror):
    r = rne_bf16 if mirror else (lambda t: t.double())
    L = o["L"]
    return dict(cond=r(o["cond"]), Wd=[r(o["Wd"][l]) for l in range(L)], Wc=[r(o["Wc"][l]) for l in range(L)],
                Wo=[r(o["Wo"][l][:, :, 0]) for l in range(L)]), r


def loop_c(o, mirror=False, bk=None, noise=None):
    """The reverse loop: (x after the last step, per-step trace of xin, xs, skip, x0, x)."""
    bk = book(o) if bk is None else bk
    noise = o["noise"] if noise is None else noise
    W, r = weights_of(o, mirror)
    x, trace = o["x_T"].double(), []
    for k in range(o["steps"]):
        xin = R.in_proj(x, o["W_in"], o["b_in"])["y"]
        xs, skip = layers_c(xin, o, o["dstep"][:, bk["dsid"][k]], bk, W, r)
        x0 = R.head(skip, o["L"], o["W_skip"], o["b_skip"], o["W_out"], o["b_out"])["x0"]
        x = R.posterior(x0, x, o["coef4"][bk["csid"][k]], noise[bk["noise"][k]].reshape(x.shape))["y"]
        trace.append(dict(xin=xin, xs=xs, skip=skip, x0=x0, x=x))
    return x, trace


def e2e_bar(o, want=None, mir=None):
    """The end-to-end bar of the GPU sweep: 4 x the cost of bf16 operands measured on the mirror against the reference (the factor the
    mel-loss, STFT-loss and discriminator tests give a mirror) + the fp32 parity bar of the loop sweep.  want / mir: the tensor of the
    reference and of the mirror (default: the final x); the skip sum of the last step is held to the same form of bar."""
    want = loop_c(o)[0] if want is None else want
    mir = loop_c(o, mirror=True)[0] if mir is None else mir
    return 4.0 * float((mir - want).abs().max()) + 1e-4 * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------
def make_gauss_c(c, steps=None, L=None, dcl=None, tag="bf16loop"):
    """make_gauss (scale 1, step_tables unchanged) plus cond, Wc and b_cond.  Every bias of layer l is scaled by 1 + l, as step_tables
    scales dstep per step: a layer that takes another layer's biases moves the result by far more than any bar."""
    steps, L, dcl = (c["steps"] if steps is None else steps), (c["L"] if L is None else L), (c["dcl"] if dcl is None else dcl)
    o = R.make_gauss(c, 1, steps=steps, L=L, dcl=dcl, tag=tag)
    g = torch.Generator().manual_seed(R._seed(c["name"], tag + "/cond"))
    B, T = c["B"], c["T"]
    o["cond"] = torch.randn(B, FH, T, generator=g)
    o["Wc"] = torch.randn(L, 512, FH, generator=g) * (0.5 / math.sqrt(FH))
    o["bc"] = torch.randn(L, 512, generator=g) * 0.1
    per_layer = (1.0 + torch.arange(L).float())[:, None]
    o["bc"], o["bd"], o["bo"] = o["bc"] * per_layer, o["bd"] * per_layer, o["bo"] * per_layer
    o["cp"] = cond_proj(o)
    return o


def make_exact_c(c, steps=1, L=4, tag="bf16exact"):
    """make_exact in the conditioned form: Wd = 0, cond = +-1, Wc zero except that filter row 256 + c carries 40 in column c % 192 (the
    device of exact_layer_weights), the gate rows saturated through b_cond[:256] = 40, integer Wo, bo on the 1 / den grid, L 1 or 4.
    y_g = 40 and y_f = +-40 exactly, z = +-1 = cond[c % 192], so the skip sum is sum_l (Wo_l z + bo_l): `skip_want`."""
    assert L in (1, 4)
    o = R.make_exact(c, steps=steps, L=L, tag=tag)
    o["dcl"] = c.get("dcl", 1)  # (Wd = 0: the dilation changes no value, but it is part of the plan)
    g = torch.Generator().manual_seed(R._seed(c["name"], tag + "/cond"))
    B, T = c["B"], c["T"]
    o["cond"] = (torch.randint(0, 2, (B, FH, T), generator=g) * 2 - 1).float()
    o["Wc"] = torch.zeros(L, 512, FH)
    o["Wc"][:, DC + torch.arange(DC), torch.arange(DC) % FH] = 40.0
    o["bc"] = torch.zeros(L, 512)
    o["bc"][:, :DC] = 40.0
    o["cp"] = cond_proj(o)
    z = o["cond"][:, torch.arange(DC) % FH].double()
    o["skip_want"] = sum(torch.einsum("oc,bct->bot", o["Wo"][l, DC:, :, 0].double(), z) + o["bo"][l, DC:].double()[None, :, None] for l in range(L))
    return o


def exact_budget(o):
    """What exact mode stands on, asserted: GEMM 1 of every layer is exact with a saturated gate (y_g >= 20, |y_f| >= 12, the margins of
    test_diffnet_bf16_reference.py); every operand the kernel rounds is a bf16 number; GEMM 2 and the skip accumulation stay below 2^24
    granules; then the boundary budget of test_loop_reference.test_exact_inputs_meet_their_budget on this skip sum, step by step."""
    L, steps = o["L"], o["steps"]
    for t in (o["cond"], o["Wc"], o["Wo"], o["Wd"]):
        assert torch.equal(rne_bf16(t), t.double())
    assert not bool(o["Wd"].any()) and not bool(o["bd"].any())
    cp = o["cp"]
    assert torch.equal(cp.float().double(), cp)
    for l in range(L):
        y = cp[:, l * 512:(l + 1) * 512]
        assert float(y[:, :DC].min()) >= D.Y_G_MIN and float(y[:, DC:].abs().min()) >= D.Y_F_MIN
    den = 128 // math.isqrt(L)
    S2 = sum(o["Wo"][l, DC:, :, 0].abs().sum(1).double() + o["bo"][l, DC:].double().abs() for l in range(L))
    assert float(S2.max()) * den < 2.0 ** 24 and R._on_grid(o["skip_want"] / math.sqrt(L))
    kh, kin = R.x2_exponents(o)
    skip = o["skip_want"]
    hd = R.head(skip.float(), L, o["W_skip"], o["b_skip"], o["W_out"], o["b_out"], kh)
    for v, S in ((hd["h"], hd["S_h"]), (hd["x0"], hd["S_out"])):
        assert R._on_grid(v) and float(S.max()) < 2.0 ** 24 * R.Q
    x = o["x_T"].double()
    for k in range(steps):
        sid = steps - 1 - k
        c1, c2 = float(o["coef4"][sid][0]), float(o["coef4"][sid][1])
        p = R.posterior(hd["x0"], x, o["coef4"][sid], o["noise"][k])
        a, b = c1 * hd["x0"], c2 * x
        assert R._fp32(a) and R._fp32(b) and R._fp32(a + b) and R._fp32(p["y"]) and p["sigma"] == 1.0 and R._on_grid(p["y"])
        assert float((a.abs() + b.abs() + o["noise"][k].double().abs()).max()) < 2.0 ** 24 * R.Q
        gemms = [hd["rh"], hd["ro"]]
        if k + 1 < steps:
            xi = R.in_proj(p["y"].float(), o["W_in"], o["b_in"], kin)
            assert R._on_grid(xi["y"]) and float(xi["S"].max()) < 2.0 ** 24 * R.Q and float(xi["y"].abs().max()) < 32768.0
            gemms.append(xi)
        for r in gemms:
            m = r["x2"]
            assert m["bits"] < R.BUDGET_BITS and m["split_exact"] and not bool(m["dropped"].any()) and torch.equal(m["y"], r["y"]) and m["amax"] < 32768.0
        x = p["y"]
    assert float(skip.std()) > 4.0 and skip.unique().numel() > 100
    return True


# ------------------------------------------------------------------------------------------------------------------------
# the plan: plan_steps (csrc/diffusion_loop.hip) for the bf16 form, line by line
# ------------------------------------------------------------------------------------------------------------------------
WHYS = ("no_ws", "dcl>2", "plan", "plan_one_layer", "env_below_1", "env", "env_above_16", "scratch_short")
BOUNDARIES = ("x2", "fused_f32", "unfused")


def _env_int(env, name):
    return int(env[name]) if name in env else None


def ws_floats_of(c):
    """bf16_ws_floats of a row: None (bf16_ws = NULL), "exact" = set_diffnet_layers_bf16_scratch_floats(B, T, 0, fuse, dcl) for the fuse
    the plan reaches before it looks at the size, "short" = one float less."""
    if c["ws"] is None or c["dcl"] > 2:
        return 0 if c["ws"] is None else 64
    fuse = _fuse_before_size(c, c["B"])[0]
    n = D.layers_scratch_floats(c["B"], c["T"], 0, max(fuse, 2), c["dcl"])
    return n - 1 if c["ws"] == "short" else n


def _fuse_before_size(c, Bg, n_cu=256):
    fuse, why = D.layers_plan(Bg, c["T"], c["L"], c["dcl"], c["env"].get("SET_AMD_BF16_FUSE_TILE"), n_cu), "plan"
    v = _env_int(c["env"], "SET_AMD_BF16_FUSE")
    if v is not None:
        fuse, why = (1, "env_below_1") if v < 1 else (16, "env_above_16") if v > 16 else (v, "env")
    return fuse, why


def plan_mirror(c, n_cu=256):
    """dict: groups (first utterance, size, fuse, body, why, launches = [(l0, nl, tile)]), boundary, G."""
    B, M, T, L, dcl, env = c["B"], c["M"], c["T"], c["L"], c["dcl"], c["env"]
    st = group_starts(B, M, T, c["n_groups"])
    fused = _env_int(env, "SET_AMD_FUSED_BOUNDARY") != 0 and R.fusable(M, T)
    x2 = fused and c["x2_images"] and M <= 96
    if _env_int(env, "SET_AMD_BOUNDARY_X2") is not None:
        x2 = x2 and _env_int(env, "SET_AMD_BOUNDARY_X2") != 0
    groups = []
    for b0, b1 in zip(st[:-1], st[1:]):
        Bg, fuse = b1 - b0, 1
        if c["ws"] is None:
            why = "no_ws"
        elif dcl > 2:
            why = "dcl>2"
        else:
            fuse, why = _fuse_before_size(c, Bg, n_cu)
            if fuse > 1 and ws_floats_of(c) < D.layers_scratch_floats(B, T, 0, fuse, dcl):
                fuse, why = 1, "scratch_short"
            elif fuse == 1 and why == "plan":
                why = "plan_one_layer"
        assert why in WHYS
        launches = []
        for l0 in range(0, L, fuse):
            nl = min(fuse, L - l0)
            tile = D.layers_launch(dict(B=Bg, T=T, l0=l0, nl=nl, dcl=dcl, env=env.get("SET_AMD_BF16_FUSE_TILE")), n_cu)["tile"] if fuse > 1 else 128
            launches.append((l0, nl, tile))
        groups.append(dict(b0=b0, Bg=Bg, fuse=fuse, body="GROUPS" if fuse > 1 else "LAYERS", why=why, launches=launches))
    return dict(groups=groups, G=len(groups), boundary="x2" if x2 else "fused_f32" if fused else "unfused")


def scratch_written(c, plan, n_cu=256):
    """Which floats of bf16_ws the launches of one step write (boolean array of ws_floats_of(c)): the union over groups and launches of
    layers_scratch_written (tests/test_diffnet_bf16_reference.py), each group at its own slice b0 * floats per utterance."""
    m = np.zeros(ws_floats_of(c), dtype=bool)
    for g in plan["groups"]:
        if g["fuse"] == 1:
            continue
        per_utt = D.layers_scratch_floats(1, c["T"], 0, g["fuse"], c["dcl"])
        for l0, nl, _ in g["launches"]:
            cc = dict(B=g["Bg"], T=c["T"], l0=l0, nl=nl, dcl=c["dcl"], env=c["env"].get("SET_AMD_BF16_FUSE_TILE"))
            r = D.layers_launch(cc, n_cu)
            assert r["rc"] == 0 and r["need"] <= g["Bg"] * per_utt
            m[g["b0"] * per_utt:g["b0"] * per_utt + r["need"]] |= D.layers_scratch_written(cc, r)
    return m


def final_x_layers(L, fuse):
    """Which x_l the ping-pong of for_layers leaves in (ws_x0, ws_x1) after ONE step: launch i writes ws_x1 (i even) or ws_x0 (i odd);
    ws_x0 holds x_0 (the in-projection) before the first."""
    held = {"ws_x0": 0, "ws_x1": None}
    for i, l0 in enumerate(range(0, L, fuse)):
        held["ws_x1" if i % 2 == 0 else "ws_x0"] = min(l0 + fuse, L)
    return held


# ------------------------------------------------------------------------------------------------------------------------
# the case table.  body / fuse / n (launches per step) / boundary: what the row must reach (pinned against plan_mirror on the CPU)
# ------------------------------------------------------------------------------------------------------------------------
def _r(name, body, fuse, n, boundary, why, reason, B, M, T, L, dcl, steps=2, ws="exact", n_groups=1, x2_images=True, **env):
    return dict(name=name, body=body, fuse=fuse, n=n, boundary=boundary, why=why, reason=reason, B=B, M=M, T=T, L=L, dcl=dcl, steps=steps, ws=ws,
                n_groups=n_groups, x2_images=x2_images, env={k: str(v) for k, v in env.items()})


FUSE, TILE = "SET_AMD_BF16_FUSE", "SET_AMD_BF16_FUSE_TILE"
ROWS = [
    # ---- STEP_BF16_LAYERS
    _r("no_ws", "LAYERS", 1, 3, "x2", "no_ws", "a.bf16_ws == NULL: fuse stays 1; L odd: x_L in ws_x1", 2, 80, 68, 3, 1, steps=3, ws=None),
    _r("dcl3_T3", "LAYERS", 1, 3, "unfused", "dcl>2", "dcl 3 with a workspace: dilation 4 above T = 3; T % 4 = 3: unfused boundary", 2, 80, 3, 3, 3),
    _r("dcl3_T132", "LAYERS", 1, 7, "x2", "dcl>2", "dcl 3: dilations 1 2 4 1 2 4 1 over two 128-frame tiles", 1, 80, 132, 7, 3, steps=3),
    _r("dcl4_T5", "LAYERS", 1, 4, "unfused", "dcl>2", "dcl 4: dilation 8 above T = 5; T % 4 = 1", 1, 17, 5, 4, 4),
    _r("dcl4_T260", "LAYERS", 1, 5, "x2", "dcl>2", "dcl 4: dilation 8 over three tiles, the cycle wraps at l = 4", 1, 80, 260, 5, 4),
    _r("fuse0", "LAYERS", 1, 4, "x2", "env_below_1", "SET_AMD_BF16_FUSE=0 clamps to 1", 2, 80, 68, 4, 2, **{FUSE: 0}),
    _r("scratch_short", "LAYERS", 1, 4, "x2", "scratch_short", "bf16_ws_floats one float short: silently one layer per launch", 2, 80, 200, 4, 1,
       ws="short", **{FUSE: 2, TILE: 128}),
    _r("L1", "LAYERS", 1, 1, "x2", "plan_one_layer", "L = 1: the plan itself answers 1", 2, 80, 68, 1, 1),
    # ---- STEP_BF16_GROUPS by the default plan: min(L, 5) on 64-frame tiles
    _r("plan_L3", "GROUPS", 3, 1, "x2", "plan", "L 3 < 5: one launch of nl = 3; x_L in ws_x1, ws_x0 keeps x_0", 2, 80, 100, 3, 2, steps=3),
    _r("plan_L7_dcl1", "GROUPS", 5, 2, "x2", "plan", "L 7: 5 + 2, tail group at l0 = 5", 2, 80, 100, 7, 1, steps=3),
    _r("plan_L7_dcl2", "GROUPS", 5, 2, "x2", "plan", "L 7, dcl 2: the tail group starts on the odd dilation (l0 = 5: 2, 1)", 2, 80, 100, 7, 2),
    # ---- the SET_AMD_BF16_FUSE clamp: both parities of the ping-pong
    _r("fuse2_L4", "GROUPS", 2, 2, "x2", "env", "fuse 2, L 4: an even launch count, x_L in ws_x0", 2, 80, 68, 4, 2, **{FUSE: 2}),
    _r("fuse2_L6", "GROUPS", 2, 3, "x2", "env", "fuse 2, L 6: an odd launch count, x_L in ws_x1", 1, 17, 100, 6, 1, **{FUSE: 2}),
    _r("fuse3_L4", "GROUPS", 3, 2, "x2", "env", "fuse 3, L 4: 3 + 1, a tail group of ONE layer; the ping-pong ends as with one layer per launch, so the scratch of the 128-frame tile is the witness",
       2, 80, 68, 4, 2, steps=3, **{FUSE: 3, TILE: 128}),
    _r("fuse99_L4", "GROUPS", 16, 1, "x2", "env_above_16", "SET_AMD_BF16_FUSE=99 clamps to 16: one launch of nl = L", 2, 80, 68, 4, 1, **{FUSE: 99}),
    # ---- both tile widths, a ragged last tile and T a multiple of the stored width (fuse 2, dcl 1: halo 1, 62 / 126 stored frames)
    _r("t64_ragged", "GROUPS", 2, 2, "x2", "env", "64-frame tiles, T 100 = 62 + 38 (balanced: 50 + 50)", 2, 80, 100, 4, 1, **{FUSE: 2, TILE: 64}),
    _r("t64_full", "GROUPS", 2, 2, "x2", "env", "64-frame tiles, T 124 = 2 x 62", 1, 80, 124, 4, 1, **{FUSE: 2, TILE: 64}),
    _r("t128_ragged", "GROUPS", 2, 2, "x2", "env", "128-frame tiles, T 200 = 126 + 74; scratch exactly as long as asked", 2, 80, 200, 4, 1, **{FUSE: 2, TILE: 128}),
    _r("t128_full", "GROUPS", 2, 2, "x2", "env", "128-frame tiles, T 252 = 2 x 126", 1, 80, 252, 4, 1, **{FUSE: 2, TILE: 128}),
    # ---- utterance groups on forced 128-frame tiles: every group its own scratch slice
    _r("groups1", "GROUPS", 2, 2, "x2", "env", "n_groups 1 at B 3: one launch grid of three utterances, the base of the rows below", 3, 80, 132, 4, 1,
       n_groups=1, **{FUSE: 2, TILE: 128}),
    _r("groups2", "GROUPS", 2, 2, "x2", "env", "n_groups 2 at B 3: groups of 1 + 2", 3, 80, 132, 4, 1, n_groups=2, **{FUSE: 2, TILE: 128}),
    _r("groups3", "GROUPS", 2, 2, "x2", "env", "n_groups 3: 1 + 1 + 1", 3, 80, 132, 4, 1, n_groups=3, **{FUSE: 2, TILE: 128}),
    _r("groups8", "GROUPS", 2, 2, "x2", "env", "n_groups 8 clamped to B = 3", 3, 80, 132, 4, 1, n_groups=8, **{FUSE: 2, TILE: 128}),
    _r("groups_odd", "GROUPS", 2, 2, "unfused", "env", "M T % 4 = 2: one group whatever is asked; T % 4 = 2: unfused", 3, 17, 66, 4, 1, n_groups=3,
       **{FUSE: 2, TILE: 128}),
    # ---- the three boundary forms
    _r("boundary_f32", "GROUPS", 2, 2, "fused_f32", "env", "SET_AMD_BOUNDARY_X2=0: the fused fp32 boundary", 2, 80, 68, 4, 1,
       **{FUSE: 2, "SET_AMD_BOUNDARY_X2": 0}),
    _r("boundary_no_x2_images", "GROUPS", 2, 2, "fused_f32", "env", "no x2 images given: the fused fp32 boundary", 2, 17, 68, 4, 1, x2_images=False, **{FUSE: 2}),
    _r("boundary_unfused_env", "GROUPS", 2, 2, "unfused", "env", "SET_AMD_FUSED_BOUNDARY=0", 2, 80, 68, 4, 1, **{FUSE: 2, "SET_AMD_FUSED_BOUNDARY": 0}),
    _r("boundary_M97", "GROUPS", 3, 1, "unfused", "plan", "M 97 > 96: unfused over three steps", 2, 97, 68, 3, 1, steps=3),
]
# end to end against float64 (section e): steps 2 and 3, L 3 and 7
E2E = [c for c in ROWS if c["name"] in ("no_ws", "dcl3_T132", "plan_L3", "plan_L7_dcl1", "plan_L7_dcl2", "fuse3_L4", "groups2", "boundary_M97", "dcl4_T260")]
# exact mode (L 1 or 4)
EXACT = [c for c in ROWS if c["L"] in (1, 4) and R.fusable(c["M"], c["T"]) and c["n_groups"] == 1]


def row(name):
    return next(c for c in ROWS if c["name"] == name)
