"""float64 / integer model of the bf16 DiffNet layer kernels (csrc/diffnet_bf16.hip) and the CPU checks of that model.
tests/test_gpu_diffnet_bf16_branches.py compares the pack kernel, the per-layer forward (both instantiations), the layer-group
kernels, the backward and the three ordered reductions with it, one raw ABI call per case.

The rounding contract modelled (head comment of the file; include/set_amd.h above SetDiffnetLayerBf16Args): rounded to bf16, round
to nearest even, exactly once: x + d after the fp32 add, cond, every weight, z, d_o = [dx_out * fp32(1 / sqrt 2) ; dskip] after the
fp32 multiply, dy, and y16 as saved.  Everything else is an fp32 accumulation: y starts at fp32(b_dil + b_cond), GEMM 2's residual
rows at fp32(b_out + x), x_out = fp32(acc * RSQRT2), skip = fp32(acc + skip).  rne_bf16 and the quad layout q4 are those of
tests/test_bf16_reference.py, gamma that of tests/test_conv_reference.py.

The module holds what the GPU sweep stands on, each condition asserted here and never assumed:
  image model     the packed layer image from the index comment above pack_layer_bf16_kernel, cross-checked by folding the fragments
                  back into Wcond, Wdil, Wout and their transposes with reshapes alone (no index arithmetic shared with the model)
  launch mirrors  layers_halo, layers_pick_tile (with the environment override), layers_balanced_nv, the scratch size, the plan, the
                  backward tile count, grid and LDS bytes of the three launches; every case of the tables names the branch it reaches
  exact mode      integer-grid operands with rounding probes: every partial sum of every GEMM, in any order, is an fp32 number (the
                  budgets are asserted per case), the gate is saturated (y_g >= 20, |y_f| >= 12 asserted over every element, the sign
                  of y_f varies per channel and frame) so that z is exactly +-1, and the backward gets a class-coded y16 whose gate
                  derivative is 0, +-1/4 or 1/2 exactly.  The kernels must then equal the model BIT FOR BIT.
  bounded mode    operands of Gaussian magnitude at the two scales of SCALES, stage by stage: the sets of bf16 numbers y16, z16 and dy16
                  may take (summation bound, derived gate slack), at most 5 % of the elements with a choice, and the models of what is
                  computed from those tensors, fed with the kernel's own copy (comment above make_forward_bounded)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_bf16_reference import SCALES, bf16_value, granule, q4, rne_bf16, rne_bf16_bits, rounding_kinds  # noqa: F401
from test_conv_reference import gamma  # noqa: F401

FC, FH, FNT = 256, 192, 128           # residual channels, conditioner channels, frames per tile (fixed by the kernels)
XR, CR, DR = FC * 2 + 16, FH * 2 + 16, 2 * FC * 2 + 16  # LDS row bytes of the [frame][256], [frame][192], [frame][512] tiles
KS_C, KS_T = FH // 16, FC // 16
KS1, KS2 = KS_C + 3 * KS_T, FC // 16
RSQRT2 = np.float32(0.70710678118654752440)
LDS_MAX = 160 * 1024
E_INVALID, E_UNSUPPORTED = -1, -2
N_W1B, N_W2B, N_WT2, N_WT1, N_WTC = 8 * KS1 * 2 * 512, 8 * KS2 * 2 * 512, 8 * 32 * 512, 8 * 96 * 512, 6 * 32 * 512
N_IMG = N_W1B + N_W2B + N_WT2 + N_WT1 + N_WTC


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# the packed image, from the index comment above pack_layer_bf16_kernel:
#   lane l of a fragment holds row (l & 31), k = 8 (l >> 5) + e
#   w1b[w][ks][rb][l][e]  row = (rb ? 256 : 0) + 32 w + (l & 31); ks < 12: Wcond[row][16 ks + k], else tap = (ks - 12) / 16,
#                         Wdil[row][16 ((ks - 12) % 16) + k][tap]
#   w2b[w][ks][rb][l][e]  Wout[row][16 ks + k]
#   wt2[w][ks][l][e]      row = 32 w + (l & 31): Wout[16 ks + k][row]
#   wt1[w][ks][l][e]      tap = ks / 32: Wdil[16 (ks % 32) + k][row][tap]
#   wtc[g][ks][l][e]      g < 6, row = 32 g + (l & 31): Wcond[16 ks + k][row]
# ------------------------------------------------------------------------------------------------------------------------
def layer_image(Wdil, Wcond, Wout):
    """uint16 [N_IMG]: the five parts one after the other, every weight rounded once."""
    bd = rne_bf16_bits(Wdil).reshape(512, FC, 3)
    bc = rne_bf16_bits(Wcond).reshape(512, FH)
    bo = rne_bf16_bits(Wout).reshape(512, FC)
    parts = []
    for n_ks, wout_part in ((KS1, False), (KS2, True)):
        w, ks, rb, l, e = np.meshgrid(np.arange(8), np.arange(n_ks), np.arange(2), np.arange(64), np.arange(8), indexing="ij")
        row, k = np.where(rb == 1, 256, 0) + 32 * w + (l & 31), 8 * (l >> 5) + e
        if wout_part:
            parts.append(bo[row, 16 * ks + k])
        else:
            is_c = ks < KS_C
            kt = np.where(is_c, 0, ks - KS_C)
            parts.append(np.where(is_c, bc[row, np.where(is_c, 16 * ks + k, 0)], bd[row, 16 * (kt % 16) + k, kt // 16]))
    w, ks, l, e = np.meshgrid(np.arange(8), np.arange(32), np.arange(64), np.arange(8), indexing="ij")
    parts.append(bo[16 * ks + 8 * (l >> 5) + e, 32 * w + (l & 31)])
    w, ks, l, e = np.meshgrid(np.arange(8), np.arange(96), np.arange(64), np.arange(8), indexing="ij")
    parts.append(bd[16 * (ks % 32) + 8 * (l >> 5) + e, 32 * w + (l & 31), ks // 32])
    g, ks, l, e = np.meshgrid(np.arange(6), np.arange(32), np.arange(64), np.arange(8), indexing="ij")
    parts.append(bc[16 * ks + 8 * (l >> 5) + e, 32 * g + (l & 31)])
    img = np.concatenate([p.reshape(-1) for p in parts]).astype(np.uint16)
    assert img.size == N_IMG
    return img


def fold_image(img):
    """The five parts folded back into matrices by reshapes and axis moves only: a 32 x 16 fragment is [k half][row][e] in memory.
    Returns (W1 [512][192 + 3 * 256], W2 [512][256], Wout^T [256][512], Wdil^T [256][3][512], Wcond^T [192][512]) as uint16."""
    o = np.cumsum([0, N_W1B, N_W2B, N_WT2, N_WT1, N_WTC])
    p = [img[o[i]:o[i + 1]] for i in range(5)]
    w1 = p[0].reshape(8, KS1, 2, 2, 32, 8).transpose(2, 0, 4, 1, 3, 5).reshape(512, 16 * KS1)  # [w][ks][rb][kh][i][e] -> [rb][w][i][ks][kh][e]
    w2 = p[1].reshape(8, KS2, 2, 2, 32, 8).transpose(2, 0, 4, 1, 3, 5).reshape(512, 16 * KS2)
    t2 = p[2].reshape(8, 32, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(256, 512)              # [w][ks][kh][i][e] -> [w][i][ks][kh][e]
    t1 = p[3].reshape(8, 3, 32, 2, 32, 8).transpose(0, 4, 1, 2, 3, 5).reshape(256, 3, 512)     # [w][tap][ks][kh][i][e] -> [w][i][tap][ks][kh][e]
    tc = p[4].reshape(6, 32, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(192, 512)
    return w1, w2, t2, t1, tc


def pack_weights(seed):
    """Weights of the pack cases: rounding probes (10 significant bits: down, up, ties of both parities), bf16 numbers that need no
    rounding, the largest normal bf16 number and one that rounds up to it, the smallest normal number, and a negative zero."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for shape in ((512, FC, 3), (512, FH), (512, FC)):
        n = int(np.prod(shape))
        k = torch.randint(0, 128, (n,), generator=g)
        f = torch.randint(0, 4, (n,), generator=g)
        s = torch.randint(-9, 3, (n,), generator=g)
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        v = (sign * (128.0 + k + f / 4.0) * 2.0 ** s.double()).float()
        v[0], v[1], v[2], v[3], v[4] = -0.0, 0.0, float(np.float32(2.0 ** 127 * (2 - 2.0 ** -7))), 2.0 ** -126, -(2.0 ** 127) * (2 - 2.0 ** -7 - 2.0 ** -10)
        v[5] = 1.0 + 2.0 ** -8          # tie, even kept bit: stays
        v[6] = 1.0 + 3 * 2.0 ** -8      # tie, odd kept bit: goes up
        out.append(v.reshape(shape))
    return out


def test_image_model_folds_back_into_the_weights_and_their_transposes():
    Wd, Wc, Wo = pack_weights(1)
    img = layer_image(Wd, Wc, Wo)
    bd, bc, bo = rne_bf16_bits(Wd).reshape(512, FC, 3), rne_bf16_bits(Wc).reshape(512, FH), rne_bf16_bits(Wo).reshape(512, FC)
    w1, w2, t2, t1, tc = fold_image(img)
    assert np.array_equal(w1, np.concatenate([bc, bd[:, :, 0], bd[:, :, 1], bd[:, :, 2]], axis=1))
    assert np.array_equal(w2, bo) and np.array_equal(t2, bo.T)
    assert np.array_equal(t1, bd.transpose(1, 2, 0)) and np.array_equal(tc, bc.T)
    kinds = np.concatenate([rounding_kinds(w).reshape(-1) for w in (Wd, Wc, Wo)])
    assert all((kinds == k).mean() > 0.1 for k in range(5))  # no rounding, down, up, tie even, tie odd
    assert int(bd.reshape(-1)[0]) == 0x8000 and int(bd.reshape(-1)[2]) == 0x7F7F and int(bd.reshape(-1)[3]) == 0x0080
    assert int(bd.reshape(-1)[4]) == 0xFF7F
    # multiplied back: the folded GEMM 1 operand times [cond ; x(t - d) ; x(t) ; x(t + d)] is the layer's pre-gate sum
    g = torch.Generator().manual_seed(2)
    Wdi, Wci = torch.randint(-2, 3, (512, FC, 3), generator=g).float(), torch.randint(-2, 3, (512, FH), generator=g).float()
    w1i = bf16_value(fold_image(layer_image(Wdi, Wci, Wo))[0])
    x, c = torch.randint(-3, 4, (1, FC, 9), generator=g).double(), torch.randint(-3, 4, (1, FH, 9), generator=g).double()
    y = F.conv1d(x, Wdi.double(), padding=2, dilation=2) + torch.einsum("rh,bht->brt", Wci.double(), c)
    col = torch.cat([c[0, :, 4], x[0, :, 2], x[0, :, 4], x[0, :, 6]])
    assert torch.equal(w1i @ col, y[0, :, 4])


def q4_unpack(flat, B, Cc, T):
    """Inverse of q4 (tests/test_bf16_reference.py): [B][C][T] from the channel-quad interleaved storage [B][C / 4][T][4]."""
    return np.asarray(flat, dtype=np.uint16).reshape(B, Cc // 4, T, 4).transpose(0, 1, 3, 2).reshape(B, Cc, T)


def test_q4_unpack_inverts_q4():
    bits = np.arange(2 * 8 * 5, dtype=np.uint16).reshape(2, 8, 5)
    assert np.array_equal(q4_unpack(q4(bits), 2, 8, 5), bits)


def test_image_size():
    assert N_IMG == 8 * 512 * (2 * KS1 + 2 * KS2 + 32 + 96) + 6 * 32 * 512 == 1245184


# ------------------------------------------------------------------------------------------------------------------------
# launch mirrors (the host code at the end of csrc/diffnet_bf16.hip, line by line)
# ------------------------------------------------------------------------------------------------------------------------
def layers_halo(l0, nl, dcl):
    return sum(1 << ((l0 + m) % dcl) for m in range(1, nl))


def layers_tile_env(env):
    try:
        t = int(env) if env is not None else 0
    except ValueError:
        t = 0
    return t if t in (64, 128) else 0


def layers_pick_tile(B, T, hh, env=None, n_cu=256):
    """(tile, why): why in env64 | env128 | rule64 | rule128 | forced128 (a halo that leaves fewer than 32 of 64 frames)."""
    tile = layers_tile_env(env)
    why = "env%d" % tile
    if not tile:
        tile, why = 64, "rule64"
        if 128 - 2 * hh >= 32:
            nv = 128 - 2 * hh
            if B * ((T + nv - 1) // nv) * 4 >= n_cu * 3:
                tile, why = 128, "rule128"
    if tile - 2 * hh < 32 and tile != 128:
        tile, why = 128, "forced128"
    return tile, why


def layers_balanced_nv(T, tile, hh):
    nv = tile - 2 * hh
    nt = (T + nv - 1) // nv
    return (T + nt - 1) // nt


def layers_scratch_floats(B, T, l0, nl, dcl):
    if B < 1 or T < 1 or nl < 1 or dcl < 1 or l0 < 0:
        return 0
    hs = [layers_halo(s0, nl, dcl) for s0 in range(dcl)]
    hs = [h for h in hs if 128 - 2 * h >= 32]  # first layers whose group the launch admits
    if not hs:
        return 64
    nv = layers_balanced_nv(T, 128, max(hs))
    return B * ((T + nv - 1) // nv) * FC * 128


def layers_plan(B, T, L, dcl, env=None, n_cu=256):
    if B < 1 or T < 1 or L < 1 or dcl < 1 or dcl > 2:
        return 1
    n10 = min(L, 10)
    h10 = layers_halo(0, n10, dcl)
    if 128 - 2 * h10 >= 32 and layers_pick_tile(B, T, h10, env, n_cu)[0] == 128:
        return n10
    return min(L, 5)


def bwd_tiles(T, dil):
    return (T + (FNT - 2 * dil) - 1) // (FNT - 2 * dil)


def layers_scratch_written(c, r):
    """Which floats of the scratch a 128-frame launch writes (csrc/diffnet_bf16.hip, comment above `rps`): block (b, tile) owns
    256 x 128 floats at (b tiles + tile) 256 128, wave w of it 4096 at w 4096, in accumulator order [cb][g4][lane][4]; between the layers of
    a group a wave parks there the skip rows of the column blocks cb >= 1 of the frames the block STORES (frame tile * nv - H + 32 cb +
    (lane & 31) inside [tile nv, min((tile + 1) nv, T))).  A group of one layer parks nothing.  Boolean array of r["need"] floats."""
    m = np.zeros(r["need"], dtype=bool)
    if r["tile"] != 128 or c["nl"] < 2:
        return m
    nt, B = r["grid"]
    m = m.reshape(B, nt, 8, 4, 4, 64, 4)  # [b][tile][w][cb][g4][lane][e]
    for i in range(nt):
        tv0, tv1 = i * r["nv"], min((i + 1) * r["nv"], c["T"])
        for cb in range(1, 4):
            t = i * r["nv"] - r["hh"] + 32 * cb + (np.arange(64) & 31)
            m[:, i, :, cb, :, (t >= tv0) & (t < tv1), :] = True
    return m.reshape(-1)


def fwd_launch(c):
    """set_diffnet_layer_fwd_bf16: return code, grid, LDS bytes and the branch name (form, tiles per utterance, whether the last tile is
    ragged, whether the whole utterance is shorter than the dilation, first)."""
    B, T, dil = c["B"], c["T"], c["dil"]
    if c.get("one_of_y_z") or B <= 0 or T <= 0 or dil < 1 or dil > 8 or 2 * FC * T * 4 >= 1 << 31:
        return dict(rc=E_INVALID, branch=("refused",))
    ldsz = (FNT + 2 * dil) * XR + FNT * CR + 5 * FC * 4
    assert ldsz <= LDS_MAX
    nt = (T + FNT - 1) // FNT
    return dict(rc=0, grid=(nt, B), ldsz=ldsz, branch=("one" if nt == 1 else "many", "ragged" if T % FNT else "full",
                                                      "T<dil" if T < dil else "T>=dil", "first" if c["first"] else "add"))


def bwd_launch(c):
    B, T, dil = c["B"], c["T"], c["dil"]
    if c.get("missing") or B <= 0 or T <= 0 or dil < 1 or dil > 8 or 2 * FC * T * 4 >= 1 << 31 or FNT - 2 * dil < 32:
        return dict(rc=E_INVALID, branch=("refused",))
    ntc = FNT - 2 * dil
    nt = bwd_tiles(T, dil)
    return dict(rc=0, grid=(nt, B), ldsz=(FNT + 2 * dil) * DR, tiles=nt,
                branch=("one" if nt == 1 else "many", "ragged" if T % ntc else "full", "T<dil" if T < dil else "T>=dil",
                        "dxo" if c["dxo"] else "nodxo", "first" if c["dcond_first"] else "add"))


def layers_launch(c, n_cu=256):
    """set_diffnet_layers_fwd_bf16: return code, tile, why, halo, stored frames per tile, grid, LDS bytes, scratch floats the launch asks for."""
    B, T, l0, nl, dcl = c["B"], c["T"], c["l0"], c["nl"], c["dcl"]
    if c.get("alias") or B <= 0 or T <= 0 or nl < 1 or nl > 16 or l0 < 0 or dcl < 1 or dcl > 4 or 2 * FC * T * 4 >= 1 << 31:
        return dict(rc=E_INVALID, branch=("refused", "invalid"))
    hh = layers_halo(l0, nl, dcl)
    tile, why = layers_pick_tile(B, T, hh, c.get("env"), n_cu)
    if tile - 2 * hh < 32:
        return dict(rc=E_UNSUPPORTED, branch=("refused", "nv<32"))
    nv = layers_balanced_nv(T, tile, hh)
    nt = (T + nv - 1) // nv
    need = B * nt * FC * 128 if tile == 128 else 0
    if tile == 128 and c.get("scratch_short"):
        return dict(rc=E_INVALID, branch=("refused", "scratch"))
    dmax = max(1 << ((l0 + m) % dcl) for m in range(nl))
    if tile == 64:
        ldsz = (64 + 2 * dmax) * XR + 64 * CR + 64 * XR + nl * (FC + 1024) * 4
    else:
        ldsz = (128 + 2 * dmax) * XR + 128 * CR + nl * FC * 4 + 2 * 1024 * 4
    if ldsz > LDS_MAX:
        return dict(rc=E_UNSUPPORTED, branch=("refused", "lds"))
    return dict(rc=0, tile=tile, why=why, hh=hh, nv=nv, nv_plain=tile - 2 * hh, grid=(nt, B), ldsz=ldsz, need=need, dmax=dmax,
                branch=(tile, why))


# ------------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------------
def _f(name, branch, B, T, dil, first, d_cs=1, d_pad=0):
    return dict(name=name, branch=branch, B=B, T=T, dil=dil, first=first, d_cs=d_cs, d_bs=FC * d_cs + d_pad)


FWD = [
    # one ragged tile; utterances shorter than the dilation: every tap but the centre one reads zeros
    _f("T1_dil1", ("one", "ragged", "T>=dil", "first"), 1, 1, 1, 1),
    _f("T2_dil2", ("one", "ragged", "T>=dil", "add"), 1, 2, 2, 0),
    _f("T3_dil4_shorter_than_dil", ("one", "ragged", "T<dil", "first"), 3, 3, 4, 1),
    _f("T5_dil8_shorter_than_dil", ("one", "ragged", "T<dil", "add"), 1, 5, 8, 0, d_cs=2, d_pad=3),
    _f("T127_dil1", ("one", "ragged", "T>=dil", "add"), 1, 127, 1, 0),
    # exactly one tile: the right halo rows are all beyond T
    _f("T128_dil2", ("one", "full", "T>=dil", "first"), 1, 128, 2, 1),
    _f("T128_dil8", ("one", "full", "T>=dil", "add"), 1, 128, 8, 0),
    # one frame / three frames in the second tile: its left halo is real data, its right halo zeros
    _f("T129_dil4_B3", ("many", "ragged", "T>=dil", "add"), 3, 129, 4, 0, d_cs=3, d_pad=5),
    _f("T131_dil8", ("many", "ragged", "T>=dil", "first"), 1, 131, 8, 1),
    _f("T256_dil8", ("many", "full", "T>=dil", "add"), 1, 256, 8, 0),
    _f("T256_dil1", ("many", "full", "T>=dil", "first"), 1, 256, 1, 1),
    _f("T257_dil1_B3", ("many", "ragged", "T>=dil", "first"), 3, 257, 1, 1, d_cs=2, d_pad=7),
    _f("T257_dil2", ("many", "ragged", "T>=dil", "add"), 1, 257, 2, 0),
]
FWD_REFUSED = [
    ("only_y16", dict(one_of_y_z="y")), ("only_z16", dict(one_of_y_z="z")), ("dil0", dict(dil=0)), ("dil9", dict(dil=9)),
    ("B0", dict(B=0)), ("T0", dict(T=0)), ("T_too_large", dict(T=(1 << 31) // (2 * FC * 4))),
]


def _b(name, branch, B, T, dil, dxo, dcond_first):
    return dict(name=name, branch=branch, B=B, T=T, dil=dil, dxo=dxo, dcond_first=dcond_first)


BWD = [
    # T relative to the 128 - 2 dil central frames of a tile
    _b("dil1_T126", ("one", "full", "T>=dil", "dxo", "first"), 1, 126, 1, True, 1),
    _b("dil1_T127", ("many", "ragged", "T>=dil", "nodxo", "add"), 1, 127, 1, False, 0),
    _b("dil1_T125_B3", ("one", "ragged", "T>=dil", "dxo", "add"), 3, 125, 1, True, 0),
    _b("dil1_T253", ("many", "ragged", "T>=dil", "dxo", "first"), 1, 253, 1, True, 1),
    _b("dil2_T124", ("one", "full", "T>=dil", "nodxo", "first"), 1, 124, 2, False, 1),
    _b("dil2_T125", ("many", "ragged", "T>=dil", "dxo", "add"), 1, 125, 2, True, 0),
    _b("dil2_T123", ("one", "ragged", "T>=dil", "dxo", "first"), 1, 123, 2, True, 1),
    _b("dil2_T249_B3", ("many", "ragged", "T>=dil", "dxo", "add"), 3, 249, 2, True, 0),
    _b("dil2_T248", ("many", "full", "T>=dil", "nodxo", "add"), 1, 248, 2, False, 0),
    _b("dil8_T112", ("one", "full", "T>=dil", "dxo", "add"), 1, 112, 8, True, 0),
    _b("dil8_T113", ("many", "ragged", "T>=dil", "dxo", "first"), 1, 113, 8, True, 1),
    _b("dil8_T111", ("one", "ragged", "T>=dil", "nodxo", "first"), 1, 111, 8, False, 1),
    _b("dil8_T225_B3", ("many", "ragged", "T>=dil", "nodxo", "first"), 3, 225, 8, False, 1),
    _b("dil2_T1", ("one", "ragged", "T<dil", "dxo", "add"), 1, 1, 2, True, 0),
    _b("dil8_T5_shorter_than_dil", ("one", "ragged", "T<dil", "dxo", "first"), 1, 5, 8, True, 1),
]
BWD_REFUSED = [("no_dskip", dict(missing="dskip")), ("no_part_dd", dict(missing="part_dd")), ("no_y16", dict(missing="y16")),
               ("dil9", dict(dil=9)), ("dil0", dict(dil=0))]
# the 128 - 2 dil >= 32 requirement of set_diffnet_layer_bwd_bf16 cannot fail behind dil <= 8 (112 central frames): it has no case


def _l(name, branch, B, T, l0, nl, dcl, env, first, **kw):
    c = dict(name=name, branch=branch, B=B, T=T, l0=l0, nl=nl, dcl=dcl, env=env, first=first, d_cs=1, d_pad=0, d_lpad=0)
    c.update(kw)
    return c


LAYERS = [
    # ---- 64-frame tiles by the switch ----
    _l("t64_nl1_T_eq_nv", (64, "env64"), 1, 64, 0, 1, 1, "64", 1),                 # no halo: nv 64
    _l("t64_nl1_T1", (64, "env64"), 1, 1, 3, 1, 4, "64", 0),                       # l0 3 of a cycle of 4: dilation 8, T < dil
    _l("t64_nl2_nv_plus1", (64, "env64"), 1, 61, 0, 2, 2, "64", 0),                # halo 2: nv 60
    _l("t64_nl2_nv_minus1", (64, "env64"), 1, 61, 1, 2, 2, "64", 1),               # l0 1: halo 1, nv 62
    _l("t64_nl5_balanced", (64, "env64"), 1, 120, 0, 5, 1, "64", 1),               # halo 4: nv 56 -> 3 tiles of 40
    _l("t64_nl5_l0_3_dcl4", (64, "env64"), 3, 70, 3, 5, 4, "64", 0, d_cs=2, d_pad=3, d_lpad=11),  # dilations 8 | 1 2 4 8: halo 15, nv 34
    _l("t64_nl10_dcl2", (64, "env64"), 1, 37, 0, 10, 2, "64", 1),                  # halo 14: nv 36, T = nv + 1
    _l("t64_nl10_dcl2_T_below_nv", (64, "env64"), 1, 20, 1, 10, 2, "64", 0),
    # full tiles: T a multiple of the stored width, so that balancing changes nothing and the last stored frames of the first tile
    # depend on its right halo rows, which hold real data (a stager that is one frame off there is seen in these alone)
    _l("t64_nl2_two_full_tiles", (64, "env64"), 1, 120, 0, 2, 2, "64", 0),
    _l("t64_nl10_two_full_tiles", (64, "env64"), 1, 72, 0, 10, 2, "64", 1),
    # ---- 128-frame tiles by the switch ----
    _l("t128_nl2_two_full_tiles", (128, "env128"), 1, 248, 0, 2, 2, "128", 1),
    _l("t128_nl10_two_full_tiles", (128, "env128"), 1, 200, 0, 10, 2, "128", 0),
    _l("t128_nl1_T128", (128, "env128"), 1, 128, 0, 1, 1, "128", 0),
    _l("t128_nl2_T_eq_nv", (128, "env128"), 1, 124, 0, 2, 2, "128", 1),            # halo 2: nv 124
    _l("t128_nl2_nv_plus1", (128, "env128"), 1, 125, 0, 2, 2, "128", 0),
    _l("t128_nl2_nv_minus1", (128, "env128"), 1, 125, 1, 2, 2, "128", 1),          # l0 1: halo 1, nv 126
    _l("t128_nl5_B3_distinct_scratch", (128, "env128"), 3, 250, 1, 5, 2, "128", 0, d_cs=3, d_pad=1, d_lpad=5),
    _l("t128_nl10_balanced", (128, "env128"), 1, 230, 0, 10, 2, "128", 1),         # halo 14: nv 100 -> 3 tiles of 77
    _l("t128_nl16_dcl2_T_below_nv", (128, "env128"), 1, 60, 0, 16, 2, "128", 0),   # halo 23: nv 82
    _l("t128_nl5_l0_1_dcl4_T1", (128, "env128"), 1, 1, 1, 5, 4, "128", 1),
    # ---- the default rule: these sizes never fill 3/4 of the chip -> 64, unless the halo leaves fewer than 32 of 64 frames ----
    _l("rule_nl2", (64, "rule64"), 3, 100, 0, 2, 1, None, 1),
    _l("rule_forced128_nl16", (128, "forced128"), 1, 100, 1, 16, 2, None, 0),      # halo 22: 64 - 44 < 32 -> 128, nv 84
    _l("env64_forced128_nl14_dcl4", (128, "forced128"), 1, 60, 0, 14, 4, "64", 1),  # halo 47: nv 34; other first layers of this cycle are refused
]
LAYERS_REFUSED = [
    ("nv_below_32", dict(nl=16, dcl=4, env=None), E_UNSUPPORTED, "nv<32"),
    ("lds_64_nl16", dict(nl=16, dcl=1, env="64"), E_UNSUPPORTED, "lds"),
    ("scratch_one_float_short", dict(nl=2, dcl=1, env="128", scratch_short=True), E_INVALID, "scratch"),
    ("x_in_is_x_out", dict(nl=2, dcl=1, env="64", alias=True), E_INVALID, "invalid"),
    ("nl0", dict(nl=0, dcl=1, env="64"), E_INVALID, "invalid"),
    ("nl17", dict(nl=17, dcl=1, env="64"), E_INVALID, "invalid"),
]
# rule128 needs B ceil(T / nv) >= 192 tiles: out of reach of B <= 3, T <= 400; tests/test_gpu_bf16.py reaches it at the benchmark shape
LAYERS_UNREACHED = {(128, "rule128")}


@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_forward_case_reaches_the_branch_it_names(c):
    r = fwd_launch(c)
    assert r["rc"] == 0 and r["branch"] == c["branch"]
    assert r["grid"] == (-(-c["T"] // 128), c["B"]) and r["ldsz"] == (128 + 2 * c["dil"]) * 528 + 128 * 400 + 5120 < LDS_MAX


@pytest.mark.parametrize("c", BWD, ids=[c["name"] for c in BWD])
def test_backward_case_reaches_the_branch_it_names(c):
    r = bwd_launch(c)
    assert r["rc"] == 0 and r["branch"] == c["branch"] and r["ldsz"] <= LDS_MAX


@pytest.mark.parametrize("c", LAYERS, ids=[c["name"] for c in LAYERS])
def test_layer_group_case_reaches_the_branch_it_names(c):
    r = layers_launch(c)
    assert r["rc"] == 0 and r["branch"] == c["branch"], r
    assert layers_scratch_floats(c["B"], c["T"], c["l0"], c["nl"], c["dcl"]) >= r["need"]


def test_refused_forms_are_refused_by_the_mirrors():
    base = dict(B=1, T=40, dil=1, first=0)
    for name, kw in FWD_REFUSED:
        assert fwd_launch(dict(base, **kw))["rc"] == E_INVALID, name
    base = dict(B=1, T=40, dil=1, dxo=True, dcond_first=0)
    for name, kw in BWD_REFUSED:
        assert bwd_launch(dict(base, **kw))["rc"] == E_INVALID, name
    base = dict(B=1, T=40, l0=0, first=1)
    for name, kw, rc, why in LAYERS_REFUSED:
        r = layers_launch(dict(base, **kw))
        assert r["rc"] == rc and r["branch"] == ("refused", why), name


def test_inventories_are_complete():
    for table in (FWD, BWD, LAYERS):
        assert len({c["name"] for c in table}) == len(table)
    # per-layer forward: the issue's T and dil lists, both `first`, both B, a strided dstep, T < dil
    assert {1, 2, 3, 127, 128, 129, 131, 256, 257} <= {c["T"] for c in FWD} and {1, 2, 4, 8} == {c["dil"] for c in FWD}
    fb = {c["branch"] for c in FWD}
    assert {(n, r) for n in ("one", "many") for r in ("ragged", "full")} == {b[:2] for b in fb}
    assert {"T<dil", "T>=dil"} == {b[2] for b in fb} and {"first", "add"} == {b[3] for b in fb}
    assert {c["first"] for c in FWD if c["B"] == 3} == {0, 1}
    assert any(c["d_cs"] != 1 and c["d_bs"] > FC * c["d_cs"] for c in FWD)
    # backward: dil 1, 2, 8 each at the central width, one more, one less, twice + 1; T = 1, T < dil; every (dx_out, dcond_first) pair
    for d in (1, 2, 8):
        ntc = 128 - 2 * d
        assert {ntc, ntc + 1, ntc - 1, 2 * ntc + 1} <= {c["T"] for c in BWD if c["dil"] == d}, d
    bb = {c["branch"] for c in BWD}
    assert {(n, r) for n in ("one", "many") for r in ("ragged", "full")} == {b[:2] for b in bb}
    assert {(x, f) for x in ("dxo", "nodxo") for f in ("first", "add")} == {b[3:] for b in bb} and "T<dil" in {b[2] for b in bb}
    assert any(c["T"] == 1 for c in BWD) and {c["B"] for c in BWD} == {1, 3}
    # layer groups
    reach = {c["branch"] for c in LAYERS}
    every = {(t, w) for t, w in ((64, "env64"), (64, "rule64"), (128, "env128"), (128, "rule128"), (128, "forced128"))}
    assert every - reach == LAYERS_UNREACHED
    assert {1, 2, 5, 10, 16} <= {c["nl"] for c in LAYERS} and {0, 1, 3} <= {c["l0"] for c in LAYERS} and {1, 2, 4} <= {c["dcl"] for c in LAYERS}
    for tile in (64, 128):
        rs = [(c, layers_launch(c)) for c in LAYERS if c["branch"][0] == tile]
        # T against the tile - 2 H frames a tile stores before balancing (one tile: the balanced width is T itself)
        rel = {("one" if c["T"] == 1 else "eq" if c["T"] == r["nv_plain"] else "plus1" if c["T"] == r["nv_plain"] + 1 else
                "minus1" if c["T"] == r["nv_plain"] - 1 else "below" if c["T"] < r["nv_plain"] else "other") for c, r in rs}
        assert {"eq", "plus1", "minus1", "one", "below"} <= rel, (tile, rel)
        assert any(r["nv"] != r["nv_plain"] and r["grid"][0] > 1 for c, r in rs), tile      # balancing changes nv
        for nl in (2, 10):  # more than one tile of the full stored width, first layer of dilation 1
            assert any(c["nl"] == nl and r["nv"] == r["nv_plain"] and r["grid"][0] > 1 and c["l0"] % c["dcl"] == 0 for c, r in rs), (tile, nl)
        assert {c["first"] for c, _ in rs} == {0, 1}
        assert any(r["dmax"] > (1 << (c["l0"] % c["dcl"])) for c, r in rs), tile            # the stager's filler rows are addressed
    assert any(c["B"] == 3 and c["branch"][0] == 128 and layers_launch(c)["grid"][0] > 1 for c in LAYERS)
    assert any(c["d_lpad"] and c["l0"] > 0 for c in LAYERS)
    assert {w for _, _, _, w in LAYERS_REFUSED} == {"nv<32", "lds", "scratch", "invalid"}


def test_mirrors_by_hand():
    assert layers_halo(0, 10, 2) == 14 and layers_halo(1, 16, 2) == 22 and layers_halo(0, 14, 4) == 47 and layers_halo(1, 14, 4) == 49
    assert layers_pick_tile(32, 800, 14) == (128, "rule128") and layers_pick_tile(1, 800, 14) == (64, "rule64")
    assert layers_pick_tile(32, 800, 14, "64") == (64, "env64") and layers_pick_tile(1, 8, 22, "64") == (128, "forced128")
    assert layers_pick_tile(1, 8, 0, "96") == (64, "rule64")
    assert layers_balanced_nv(800, 128, 14) == 100 and layers_balanced_nv(230, 128, 14) == 77 and layers_balanced_nv(120, 64, 4) == 40
    assert layers_plan(32, 800, 20, 2) == 10 and layers_plan(1, 100, 20, 2) == 5 and layers_plan(1, 100, 3, 1) == 3 and layers_plan(1, 1, 1, 3) == 1
    assert layers_scratch_floats(32, 800, 0, 10, 2) == 32 * 8 * 256 * 128
    assert bwd_tiles(126, 1) == 1 and bwd_tiles(127, 1) == 2 and bwd_tiles(113, 8) == 2


def test_host_mirrors_equal_the_library_without_a_gpu(built_lib):
    """The size functions are host code: image size, backward tile count and the scratch size against the library (the plan depends on
    the CU count of the device and is compared in the GPU file)."""
    L = built_lib
    assert L.set_diffnet_layer_bf16_image_size() == N_IMG
    for T in (1, 5, 111, 112, 113, 126, 127, 253, 400):
        for dil in (1, 2, 4, 8):
            assert L.set_diffnet_layer_bwd_bf16_tiles(T, dil) == bwd_tiles(T, dil)
    for B, T in ((1, 1), (2, 60), (3, 400), (32, 800)):
        for dcl in (1, 2, 3, 4):
            for nl in range(1, 18):
                for l0 in (0, 1, 3):
                    assert L.set_diffnet_layers_bf16_scratch_floats(B, T, l0, nl, dcl) == layers_scratch_floats(B, T, l0, nl, dcl), (B, T, l0, nl, dcl)
    # a group of 14 layers in a cycle of 4: admitted from l0 = 0 (halo 47), refused from l0 = 1, 2 (49, 53): the size serves the admitted ones
    assert L.set_diffnet_layers_bf16_scratch_floats(1, 60, 0, 14, 4) == 2 * FC * 128 == layers_launch(dict(B=1, T=60, l0=0, nl=14, dcl=4, env="64"))["need"]


def test_scratch_size_covers_every_admitted_first_layer():
    """The size set_diffnet_layers_bf16_scratch_floats returns must serve the launch for the l0 it was asked for and for every other
    first layer of the cycle that the launch admits (one buffer serves every group of a network)."""
    for dcl in (1, 2, 3, 4):
        for nl in range(1, 17):
            for T in (1, 60, 400):
                n = layers_scratch_floats(2, T, 0, nl, dcl)
                for l0 in range(dcl):
                    for env in ("64", "128", None):
                        r = layers_launch(dict(B=2, T=T, l0=l0, nl=nl, dcl=dcl, env=env))
                        if r["rc"] == 0:
                            assert n >= r["need"], (dcl, nl, T, l0, env, n, r["need"])


# ------------------------------------------------------------------------------------------------------------------------
# exact mode, forward
# ------------------------------------------------------------------------------------------------------------------------
M_COND, B_GATE = 512.0, 512.0   # the dominant conditioner weight of a filter row, the bias of a gate row
Y_G_MIN, Y_F_MIN = 20.0, 12.0


def _seed(name, salt=0):
    return sum(ord(ch) for ch in name) * 7 + salt


def _probes(g, shape, s):
    """+-(128 + k + f / 4) 2^s: 10 significant bits, 8 are kept; f = 2 is a tie whose kept bit is the parity of k."""
    n = int(np.prod(shape))
    k, f = torch.randint(0, 128, (n,), generator=g), torch.randint(0, 4, (n,), generator=g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (sign * (128.0 + k + f / 4.0) * 2.0 ** s).float().reshape(shape)


def exact_layer_weights(seed):
    """Wdil: integers in [-2, 2].  Wcond: integers in [-1, 1]; filter row 256 + c carries M_COND in column c % 192.  Wout: rounding
    probes in [1, 2) 2^0.  Biases: integers; gate rows + B_GATE."""
    g = torch.Generator().manual_seed(seed)
    Wd = torch.randint(-2, 3, (512, FC, 3), generator=g).float()
    Wc = torch.randint(-1, 2, (512, FH), generator=g).float()
    Wc[FC + torch.arange(FC), torch.arange(FC) % FH] = M_COND
    Wo = _probes(g, (512, FC), -7)
    bd, bc, bo = (torch.randint(-3, 4, (512,), generator=g).float() for _ in range(3))
    bd[:FC] += B_GATE
    return dict(Wd=Wd, Wc=Wc, Wo=Wo, bd=bd, bc=bc, bo=bo)


def make_forward_exact(c):
    """Operands of an exact forward case and the model's outputs.  x = +-(128 + k) 2^-7, the step offset carries the fraction f / 4 2^-7
    (the fp32 sum is exact and has 10 significant bits: rounded down, up, ties of both parities), cond = +-1, skip integers."""
    g = torch.Generator().manual_seed(_seed(c["name"]))
    B, T, dil = c["B"], c["T"], c["dil"]
    o = dict(c)
    o.update(exact_layer_weights(_seed(c["name"], 1)))
    k = torch.randint(1, 128, (B, FC, T), generator=g)
    sign = torch.where(torch.rand(B, FC, T, generator=g) < 0.5, -1.0, 1.0)
    o["x"] = (sign * (128.0 + k) * 2.0 ** -7).float()
    o["d"] = (torch.randint(0, 4, (B, FC), generator=g) / 4.0 * 2.0 ** -7).float()
    o["cond"] = torch.where(torch.rand(B, FH, T, generator=g) < 0.5, -1.0, 1.0).float()
    o["skip0"] = torch.randint(-4, 5, (B, FC, T), generator=g).float()
    xd32 = _np32(o["x"]) + _np32(o["d"])[:, :, None]
    assert xd32.dtype == np.float32 and np.array_equal(xd32.astype(np.float64), o["x"].double().numpy() + o["d"].double().numpy()[:, :, None])
    o["xd32"] = xd32
    xr, cr = rne_bf16(xd32), rne_bf16(o["cond"])
    Wd, Wc, Wo = rne_bf16(o["Wd"]), rne_bf16(o["Wc"]), rne_bf16(o["Wo"])
    b1 = torch.from_numpy((_np32(o["bd"]) + _np32(o["bc"])).astype(np.float64))
    y = F.conv1d(xr, Wd, padding=dil, dilation=dil) + torch.einsum("rh,bht->brt", Wc, cr) + b1[None, :, None]
    S1 = F.conv1d(xr.abs(), Wd.abs(), padding=dil, dilation=dil) + torch.einsum("rh,bht->brt", Wc.abs(), cr.abs()) + b1.abs()[None, :, None]
    q1 = min(granule(xr) * granule(Wd), granule(cr) * granule(Wc), granule(b1))
    o["budget1"] = float(S1.max()) / q1
    assert o["budget1"] < 2 ** 24, (c["name"], o["budget1"])
    yg, yf = y[:, :FC], y[:, FC:]
    o["margin_g"], o["margin_f"] = float(yg.min()), float(yf.abs().min())
    assert o["margin_g"] >= Y_G_MIN and o["margin_f"] >= Y_F_MIN, (c["name"], o["margin_g"], o["margin_f"])
    y32 = y.float()
    assert torch.equal(y32.double(), y)
    o["y"], o["y16"] = y, rne_bf16_bits(y32)
    z = torch.sign(yf)
    o["z16"] = rne_bf16_bits(z.float())
    # GEMM 2: residual rows start at fp32(b_out + x), skip rows at b_out
    start = np.concatenate([(_np32(o["bo"])[None, :FC, None] + _np32(o["x"])), np.broadcast_to(_np32(o["bo"])[None, FC:, None], (B, FC, T))], axis=1)
    assert start.dtype == np.float32
    start = torch.from_numpy(start.astype(np.float64))
    acc = start + torch.einsum("rc,bct->brt", Wo, z)
    S2 = start.abs() + torch.einsum("rc,bct->brt", Wo.abs(), z.abs()) + F.pad(o["skip0"].double().abs(), (0, 0, FC, 0))
    q2 = min(granule(Wo), granule(start), granule(o["skip0"]))
    o["budget2"] = float(S2.max()) / q2
    assert o["budget2"] < 2 ** 24, (c["name"], o["budget2"])
    acc32 = _np32(acc.float())
    assert np.array_equal(acc32.astype(np.float64), acc.numpy())
    o["x_out"] = torch.from_numpy(acc32[:, :FC] * RSQRT2)  # one fp32 multiply
    assert o["x_out"].dtype == torch.float32
    o["skip"] = torch.from_numpy(acc32[:, FC:] if c["first"] else acc32[:, FC:] + _np32(o["skip0"]))
    return o


@pytest.mark.parametrize("c", FWD, ids=[c["name"] for c in FWD])
def test_forward_exact_case_fits_fp32_and_saturates_the_gate(c):
    """Budgets and margins are asserted inside make_forward_exact; here: the probes hit every rounding rule, the sign of z varies per
    channel and per frame, and some y need rounding when they are saved."""
    o = make_forward_exact(c)
    kx = rounding_kinds(o["xd32"]).reshape(-1)
    assert (kx == 3).any() and (kx == 4).any() and (kx == 1).any() and (kx == 2).any() and (kx == 0).any()
    kw = rounding_kinds(o["Wo"]).reshape(-1)
    assert all((kw == k).mean() > 0.05 for k in range(5))
    z = bf16_value(o["z16"])
    assert set(z.reshape(-1).tolist()) == {-1.0, 1.0}
    if c["T"] >= 32:
        assert bool((z.min(dim=2).values < z.max(dim=2).values).all())  # per channel: both signs over the frames
    assert bool((z.min(dim=1).values < z.max(dim=1).values).all())      # per frame: both signs over the channels
    ky = rounding_kinds(o["y"].float()).reshape(-1)
    assert ((ky == 1) | (ky == 2)).mean() > 0.3


def test_saved_y_of_the_exact_cases_includes_ties_of_both_parities():
    kinds = np.concatenate([rounding_kinds(make_forward_exact(c)["y"].float()).reshape(-1) for c in FWD if c["T"] >= 256])
    assert (kinds == 3).sum() >= 1 and (kinds == 4).sum() >= 1, [(kinds == k).sum() for k in range(5)]


def test_exact_forward_budget_by_hand():
    """GEMM 1: 768 products of |w| <= 2, |x + d| <= 2, 192 of |w| <= 1, |cond| = 1 but one of M_COND, the biases: in granules of 2^-7."""
    assert (768 * 4 + 191 + M_COND + B_GATE + 6) * 128 < 2 ** 24
    assert (256 * 2 + 3 + 2 + 4) * 128 < 2 ** 24


# ------------------------------------------------------------------------------------------------------------------------
# exact mode, backward.  y16 is an input: class-coded per (channel, frame)
#     (y_g, y_f) = (0, 0): s = 1/2, th = 0  -> dy_g = 0, dy_f = dz / 2        (0, +-40): s = 1/2, th = +-1 -> dy_g = +-dz / 4, dy_f = 0
#     (40, +-40): s = 1, th = +-1 -> dy_g = dy_f = 0
# (the gate-precondition test of the GPU file shows the device returns these s and th).  d_o is sparse (1 / 32 of its elements) and all
# of its non-zero elements lie in one binade, so that dz, dy and the sums over them keep a common granule.
# ------------------------------------------------------------------------------------------------------------------------
CLASSES = [(0.0, 0.0), (0.0, 40.0), (0.0, -40.0), (40.0, 40.0), (40.0, -40.0)]
CLASS_P = torch.tensor([0.06, 0.03, 0.03, 0.44, 0.44])


def make_backward_exact(c):
    g = torch.Generator().manual_seed(_seed(c["name"], 2))
    B, T, dil = c["B"], c["T"], c["dil"]
    o = dict(c)
    o["Wd"] = torch.randint(-1, 2, (512, FC, 3), generator=g).float()
    o["Wc"] = torch.randint(-2, 3, (512, FH), generator=g).float()
    o["Wo"] = torch.randint(-2, 3, (512, FC), generator=g).float()
    keep = lambda: (torch.rand(B, FC, T, generator=g) < 1.0 / 32).float()
    # dx_out = +-(192 + k) 2^-7, k < 160: in [1.5, 2.75), times 1 / sqrt 2 in [1.06, 1.95): one binade, and the product needs rounding
    sign = lambda: torch.where(torch.rand(B, FC, T, generator=g) < 0.5, -1.0, 1.0)
    o["dxo"] = (sign() * (192.0 + torch.randint(0, 160, (B, FC, T), generator=g)) * 2.0 ** -7 * keep()).float() if c["dxo"] else None
    o["dskip"] = (_probes(g, (B, FC, T), -7) * keep()).float()
    cls = torch.multinomial(CLASS_P, B * FC * T, replacement=True, generator=g).reshape(B, FC, T)
    table = torch.tensor(CLASSES)
    yv = torch.cat([table[cls, 0], table[cls, 1]], dim=1)  # [B][512][T]
    o["y16"] = rne_bf16_bits(yv)
    assert torch.equal(bf16_value(o["y16"]), yv.double())
    o["dcond0"] = torch.randint(-4, 5, (B, FH, T), generator=g).float()
    top = torch.zeros(B, FC, T, dtype=torch.float32) if o["dxo"] is None else torch.from_numpy(_np32(o["dxo"]) * RSQRT2)
    assert top.dtype == torch.float32
    do32 = torch.cat([top, o["dskip"]], dim=1)
    o["do32"], o["do16"] = do32, rne_bf16_bits(do32)
    do = bf16_value(o["do16"])
    nz = do[do != 0].abs()
    assert nz.numel() == 0 or (float(nz.min()) >= 1.0 and float(nz.max()) <= 2.0)
    Wd, Wc, Wo = o["Wd"].double(), o["Wc"].double(), o["Wo"].double()
    dz = torch.einsum("kc,bkt->bct", Wo, do) + 0.0  # (+ 0.0: an accumulator that starts at +0 never ends at -0)
    o["budget_dz"] = float(torch.einsum("kc,bkt->bct", Wo.abs(), do.abs()).max()) / 2.0 ** -7
    s = torch.where(yv[:, :FC] == 0, 0.5, 1.0).double()
    th = torch.sign(yv[:, FC:]).double()
    dy32 = torch.cat([dz * th * s * (1 - s), dz * s * (1 - th * th)], dim=1).float()
    assert torch.equal(dy32.double(), torch.cat([dz * th * s * (1 - s), dz * s * (1 - th * th)], dim=1))
    o["dz"], o["dy32"], o["dy16"] = dz, dy32, rne_bf16_bits(dy32)
    dy = bf16_value(o["dy16"])
    q = min(granule(dy), 1.0)
    dxd = F.conv_transpose1d(dy, Wd, padding=dil, dilation=dil) + 0.0
    Sx = F.conv_transpose1d(dy.abs(), Wd.abs(), padding=dil, dilation=dil)
    dcn = torch.einsum("kh,bkt->bht", Wc, dy) + 0.0
    Sc = torch.einsum("kh,bkt->bht", Wc.abs(), dy.abs()) + (0 if c["dcond_first"] else o["dcond0"].double().abs())
    nt, ntc = bwd_tiles(T, dil), FNT - 2 * dil
    pdbo, pdby, pdd = torch.zeros(B, nt, 512, dtype=torch.float64), torch.zeros(B, nt, 512, dtype=torch.float64), torch.zeros(B, nt, FC, dtype=torch.float64)
    Sp = 0.0
    for i in range(nt):
        sl = slice(i * ntc, min((i + 1) * ntc, T))
        pdbo[:, i], pdby[:, i], pdd[:, i] = do[:, :, sl].sum(2) + 0.0, dy[:, :, sl].sum(2) + 0.0, dxd[:, :, sl].sum(2) + 0.0
        Sp = max(Sp, float(do[:, :, sl].abs().sum(2).max()), float(dy[:, :, sl].abs().sum(2).max()), float(Sx[:, :, sl].sum(2).max()))
    o["budget"] = max(o["budget_dz"], float(Sx.max()) / q, float(Sc.max()) / q, Sp / min(q, 2.0 ** -7))
    assert o["budget"] < 2 ** 24 and q >= 2.0 ** -20, (c["name"], o["budget"], q)
    o["dxd"], o["part_dbo"], o["part_dby"], o["part_dd"] = dxd, pdbo, pdby, pdd
    o["dcond"] = dcn if c["dcond_first"] else dcn + o["dcond0"].double()
    assert torch.equal(o["dcond"].float().double(), o["dcond"]) and torch.equal(dxd.float().double(), dxd)
    if o["dxo"] is None:
        o["dx_sep"] = o["dx_fma"] = dxd.float()
    else:
        # both evaluations of dxd + dx_out * RSQRT2: the product has at most 9 + 24 significant bits and dxd is a multiple of q below
        # 2^24 q: the float64 product is exact, and so is the float64 sum when its error term is zero (checked), so float64 -> fp32 is
        # the ONE rounding of the fused form
        prod = o["dxo"].double() * float(RSQRT2)
        ssum = dxd + prod
        assert torch.equal((ssum - dxd) - prod, torch.zeros_like(prod)) and torch.equal((ssum - prod) - dxd, torch.zeros_like(prod))
        o["dx_fma"] = ssum.float()
        o["dx_sep"] = torch.from_numpy(_np32(dxd.float()) + _np32(o["dxo"]) * RSQRT2)
        assert o["dx_sep"].dtype == torch.float32
    return o


@pytest.mark.parametrize("c", BWD, ids=[c["name"] for c in BWD])
def test_backward_exact_case_fits_fp32_and_mixes_the_classes(c):
    """The budget is asserted inside make_backward_exact.  Both halves of dy are non-zero in every tile, 32-frame column block of the
    tile and 32-channel wave row block (where the tile has that many central frames), and d_o needs rounding."""
    o = make_backward_exact(c)
    dy = bf16_value(o["dy16"])
    T, dil = c["T"], c["dil"]
    ntc = FNT - 2 * dil
    for i in range(bwd_tiles(T, dil)):
        for cb in range(4):
            lo, hi = max(i * ntc - dil + 32 * cb, i * ntc, 0), min(i * ntc - dil + 32 * cb + 32, (i + 1) * ntc, T)
            if hi - lo < 8:
                continue
            blk = dy[:, :, lo:hi].reshape(c["B"], 2, 8, 32, hi - lo)
            assert bool((blk != 0).any(dim=4).any(dim=3).all()), (c["name"], i, cb)
    if T >= 100:
        assert (rounding_kinds(o["do32"]).reshape(-1) > 0).sum() > 100 and (rounding_kinds(o["dy32"]).reshape(-1) > 0).sum() > 100
        if o["dxo"] is not None:
            assert not torch.equal(o["dx_sep"], o["dx_fma"])  # the two evaluations can be told apart


# ------------------------------------------------------------------------------------------------------------------------
# reductions: integer partials, any association is exact
# ------------------------------------------------------------------------------------------------------------------------
ROWS_RG = 16
RED_ROWS = (1, ROWS_RG - 1, ROWS_RG, ROWS_RG + 1, 37, 4 * ROWS_RG + 3)  # the last one enters the four-chain loop of rows_sum_chains
RED_COLS = (1, 63, 64, 65, 200)


def int_partials(seed, shape, hi=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).float()


def test_reduction_cases_stay_exact_and_reach_both_loops():
    assert max(RED_ROWS) * 3 * 64 * 8 < 2 ** 24            # rows x B x |partial| x |scale| and the accumulate target
    assert any(r > 3 * ROWS_RG for r in RED_ROWS) and any(r <= 3 * ROWS_RG for r in RED_ROWS)
    assert {1, ROWS_RG - 1, ROWS_RG, ROWS_RG + 1, 37} <= set(RED_ROWS) and set(RED_COLS) == {1, 63, 64, 65, 200}


# ------------------------------------------------------------------------------------------------------------------------
# bounded mode: operands of Gaussian magnitude at the two scales of SCALES, an unsaturated gate, checked stage by stage so that a flip
# of a bf16 rounding never travels into a bar: y16 / z16 / dy16 must lie in the set of bf16 numbers RNE can return on the model's
# interval, and everything computed FROM such a tensor is modelled on the kernel's own copy of it.
#
# Every sum whose result is rounded to bf16 (y, dz) is built from terms of ONE sign per output row (the row's weights and bias carry
# the row's sign, x, d, cond, dx_out and dskip are magnitudes |N(0, 1)|): sum |terms| = |sum|, so the summation bound gamma(n) |y| is a
# few 1e-5 of the value, against a bf16 spacing of 2^-8 .. 2^-7 of it.  With signed Gaussian terms sum |terms| is ~ sqrt(n) |y| and the
# admissible set of MOST elements would hold two bf16 numbers; here it does for a few percent (asserted: at most 5 % per tensor).
#
# gate slack, in units of u = 2^-24, from the accuracy of the device functions (v_exp_f32 and v_rcp_f32: 1 ulp = 2 u relative):
#   expf(a) = exp2(fp32(a log2e)): the rounded argument is off by |a| log2e u, that is |a| u relative in the result; + 2 u of v_exp_f32
#   sigmoid(a) = rcp(1 + expf(-a)): the add rounds (u), e / (1 + e) <= 1, v_rcp_f32 2 u:            relative error <= (|a| + 5) u
#   tanh(a) = 1 - 2 t, t = rcp(1 + expf(2 a)): t is off by (2 |a| + 5) u t, 2 t <= 2; the subtraction rounds:  absolute error
#                                                                                                    <= (4 |a| + 11) u
#   z = s th: |dz| <= |th| ds + s dth + u |z| <= (|y_g| + 5) u + (4 |y_f| + 11) u + u  = (|y_g| + 4 |y_f| + 17) u              (s, |th| <= 1)
#   G = th s (1 - s)  (dy_g = dz G): d(1 - s) <= ds + u; three products round:
#       |dG| <= s (1 - s) dth + |th| (1 - s) ds + |th| s (ds + u) + 3 u |G| <= ((4 |y_f| + 11) / 4 + (|y_g| + 5) + 1 + 1) u <= (|y_g| + |y_f| + 10) u
#   F = s (1 - th^2)  (dy_f = dz F): d(th^2) <= 2 dth + u, d(1 - th^2) <= 2 dth + 2 u:
#       |dF| <= (1 - th^2) ds + s (2 dth + 2 u) + 2 u |F| <= ((|y_g| + 5) + (8 |y_f| + 24) + 2) u <= (|y_g| + 8 |y_f| + 33) u
# ------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
SHARE_MAX = 0.05


def admissible(lo, hi):
    """(lowest, highest) bf16 value RNE can return for an fp32 number of [lo, hi] (float64 tensors): the interval is first widened to
    fp32 numbers outside it, RNE is monotone."""
    lo32 = np.nextafter(lo.numpy().astype(np.float32), np.float32(-np.inf))
    hi32 = np.nextafter(hi.numpy().astype(np.float32), np.float32(np.inf))
    return rne_bf16(lo32), rne_bf16(hi32)


def in_set(bits, lo_v, hi_v):
    v = bf16_value(bits)
    return (v >= lo_v) & (v <= hi_v)


def _corners(a_lo, a_hi, b_lo, b_hi):
    """min and max of a b over the box."""
    p = torch.stack([a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi])
    return p.min(0).values, p.max(0).values


def _mag(g, shape, scale=1.0):
    return torch.randn(shape, generator=g).abs() * scale


def _signs(g, n):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def make_forward_bounded(c, scale):
    xs, ws = SCALES[scale]
    g = torch.Generator().manual_seed(_seed(c["name"], 100 + scale))
    B, T, dil = c["B"], c["T"], c["dil"]
    o = dict(c)
    sr = _signs(g, 512)
    o["Wd"] = (sr[:, None, None] * _mag(g, (512, FC, 3), ws / 1500.0)).float()
    o["Wc"] = (sr[:, None] * _mag(g, (512, FH), ws / 400.0)).float()
    o["Wo"] = (torch.randn(512, FC, generator=g) * 0.05 * ws).float()
    o["bd"], o["bc"] = (sr * _mag(g, (512,), 0.5 * xs * ws)).float(), (sr * _mag(g, (512,), 0.5 * xs * ws)).float()
    o["bo"] = (torch.randn(512, generator=g) * 0.1 * xs * ws).float()
    o["x"], o["d"], o["cond"] = _mag(g, (B, FC, T), xs).float(), _mag(g, (B, FC), 0.3 * xs).float(), _mag(g, (B, FH, T), xs).float()
    o["skip0"] = (torch.randn(B, FC, T, generator=g) * xs * ws).float()
    xd32 = _np32(o["x"]) + _np32(o["d"])[:, :, None]
    assert xd32.dtype == np.float32
    xr, cr = rne_bf16(xd32), rne_bf16(o["cond"])
    Wd, Wc = rne_bf16(o["Wd"]), rne_bf16(o["Wc"])
    b1 = torch.from_numpy((_np32(o["bd"]) + _np32(o["bc"])).astype(np.float64))
    y = F.conv1d(xr, Wd, padding=dil, dilation=dil) + torch.einsum("rh,bht->brt", Wc, cr) + b1[None, :, None]
    S1 = F.conv1d(xr.abs(), Wd.abs(), padding=dil, dilation=dil) + torch.einsum("rh,bht->brt", Wc.abs(), cr.abs()) + b1.abs()[None, :, None]
    assert bool(((S1 - y.abs()).abs() <= 1e-9 * S1).all())  # one sign per row
    by = gamma(16 * KS1 + 2) * S1
    o["y"], o["by"] = y, by
    o["y_lo"], o["y_hi"] = admissible(y - by, y + by)
    yg, yf, bg, bf = y[:, :FC], y[:, FC:], by[:, :FC], by[:, FC:]
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    z_lo, z_hi = _corners(sig(yg - bg), sig(yg + bg), torch.tanh(yf - bf), torch.tanh(yf + bf))
    slack = U * (yg.abs() + bg + 4 * (yf.abs() + bf) + 17)
    o["z_lo"], o["z_hi"] = admissible(z_lo - slack, z_hi + slack)
    o["share_y"] = float((o["y_lo"] != o["y_hi"]).double().mean())
    o["share_z"] = float((o["z_lo"] != o["z_hi"]).double().mean())
    o["unsaturated"] = float(((sig(yg) * torch.tanh(yf)).abs() < 0.97).double().mean())
    return o


def forward_gemm2(o, z16_bits):
    """x_out and skip of the model's GEMM 2 fed with the kernel's own z16 ([B][256][T] bits), and their bars: the products are exact,
    what is left is the fp32 summation (256 products, the start value), one rounding of the RSQRT2 product / of the skip add."""
    B, T = o["B"], o["T"]
    z, Wo = bf16_value(z16_bits), rne_bf16(o["Wo"])
    start = np.concatenate([(_np32(o["bo"])[None, :FC, None] + _np32(o["x"])), np.broadcast_to(_np32(o["bo"])[None, FC:, None], (B, FC, T))], axis=1)
    assert start.dtype == np.float32
    start = torch.from_numpy(start.astype(np.float64))
    acc = start + torch.einsum("rc,bct->brt", Wo, z)
    S2 = start.abs() + torch.einsum("rc,bct->brt", Wo.abs(), z.abs())
    bar = gamma(FC + 2) * S2
    x_out = acc[:, :FC] * float(RSQRT2)
    bar_x = bar[:, :FC] * float(RSQRT2) + 2 * U * x_out.abs()
    if o["first"]:
        return x_out, bar_x, acc[:, FC:], bar[:, FC:]
    skip = acc[:, FC:] + o["skip0"].double()
    return x_out, bar_x, skip, bar[:, FC:] + 2 * U * (skip.abs() + acc[:, FC:].abs())


BOUNDED_FWD = [(c, k) for c in FWD for k in range(len(SCALES))]


@pytest.mark.parametrize("c,k", BOUNDED_FWD, ids=["%s-%d" % (c["name"], k) for c, k in BOUNDED_FWD])
def test_forward_bounded_case_leaves_few_elements_a_choice(c, k):
    o = make_forward_bounded(c, k)
    assert o["share_y"] <= SHARE_MAX and o["share_z"] <= SHARE_MAX, (c["name"], k, o["share_y"], o["share_z"])
    assert o["unsaturated"] >= 0.5, (c["name"], k, o["unsaturated"])
    assert bool((o["y_lo"] <= o["y_hi"]).all()) and bool((o["z_lo"] <= o["z_hi"]).all())
    assert bool(in_set(rne_bf16_bits(o["y"].float()), o["y_lo"], o["y_hi"]).all())


def make_backward_bounded(c, scale):
    xs, ws = SCALES[scale]
    g = torch.Generator().manual_seed(_seed(c["name"], 200 + scale))
    B, T, dil = c["B"], c["T"], c["dil"]
    o = dict(c)
    sc = _signs(g, FC)
    o["Wo"] = (sc[None, :] * _mag(g, (512, FC), 0.05 * ws)).float()
    o["Wd"], o["Wc"] = (torch.randn(512, FC, 3, generator=g) * 0.03 * ws).float(), (torch.randn(512, FH, generator=g) * 0.05 * ws).float()
    o["dxo"] = _mag(g, (B, FC, T), xs).float() if c["dxo"] else None
    o["dskip"] = _mag(g, (B, FC, T), xs).float()
    yv = (torch.randn(B, 512, T, generator=g) * 0.8).float()  # (|y_f| of 3 and more: 1 - th^2 cancels and most dy_f could round either way)
    o["y16"] = rne_bf16_bits(yv)
    yv = bf16_value(o["y16"])
    o["dcond0"] = (torch.randn(B, FH, T, generator=g) * xs * ws).float()
    top = torch.zeros(B, FC, T, dtype=torch.float32) if o["dxo"] is None else torch.from_numpy(_np32(o["dxo"]) * RSQRT2)
    assert top.dtype == torch.float32
    o["do16"] = rne_bf16_bits(torch.cat([top, o["dskip"]], dim=1))
    do, Wo = bf16_value(o["do16"]), rne_bf16(o["Wo"])
    dz = torch.einsum("kc,bkt->bct", Wo, do)
    Sz = torch.einsum("kc,bkt->bct", Wo.abs(), do.abs())
    assert bool(((Sz - dz.abs()).abs() <= 1e-9 * Sz).all())  # one sign per z channel
    bz = gamma(512 + 2) * Sz
    yg, yf = yv[:, :FC], yv[:, FC:]
    s, th = 1.0 / (1.0 + torch.exp(-yg)), torch.tanh(yf)
    G, Fv = th * s * (1 - s), s * (1 - th * th)
    dG, dF = U * (yg.abs() + yf.abs() + 10), U * (yg.abs() + 8 * yf.abs() + 33)
    g_lo, g_hi = _corners(dz - bz, dz + bz, G - dG, G + dG)
    f_lo, f_hi = _corners(dz - bz, dz + bz, Fv - dF, Fv + dF)
    lo, hi = torch.cat([g_lo, f_lo], dim=1), torch.cat([g_hi, f_hi], dim=1)
    o["dy_model"] = torch.cat([dz * G, dz * Fv], dim=1)
    o["dy_lo"], o["dy_hi"] = admissible(lo, hi)
    o["share_dy"] = float((o["dy_lo"] != o["dy_hi"]).double().mean())
    return o


def backward_from_dy(o, dy16_bits):
    """What the backward computes FROM dy, modelled on the kernel's own dy16 ([B][512][T] bits): dx, dcond, part_dby, part_dd, and
    part_dbo from the model's d_o16.  Returns name -> (want, bar): the bars are fp32 summation bounds (the products are exact)."""
    B, T, dil = o["B"], o["T"], o["dil"]
    dy, do = bf16_value(dy16_bits), bf16_value(o["do16"])
    Wd, Wc = rne_bf16(o["Wd"]), rne_bf16(o["Wc"])
    dxd = F.conv_transpose1d(dy, Wd, padding=dil, dilation=dil)
    bxd = gamma(3 * 512 + 2) * F.conv_transpose1d(dy.abs(), Wd.abs(), padding=dil, dilation=dil)
    dcn = torch.einsum("kh,bkt->bht", Wc, dy)
    Sc = torch.einsum("kh,bkt->bht", Wc.abs(), dy.abs())
    old = torch.zeros_like(dcn) if o["dcond_first"] else o["dcond0"].double()
    out = {"dcond": (dcn + old, gamma(512 + 3) * (Sc + old.abs()))}
    if o["dxo"] is None:
        out["dx"] = (dxd, bxd)
    else:
        p = o["dxo"].double() * float(RSQRT2)
        out["dx"] = (dxd + p, bxd + 2 * U * (dxd.abs() + bxd + p.abs()))
    nt, ntc = bwd_tiles(T, dil), FNT - 2 * dil
    parts = {k: (torch.zeros(B, nt, n, dtype=torch.float64), torch.zeros(B, nt, n, dtype=torch.float64)) for k, n in
             (("part_dbo", 512), ("part_dby", 512), ("part_dd", FC))}
    for i in range(nt):
        sl = slice(i * ntc, min((i + 1) * ntc, T))
        for k, v, extra in (("part_dbo", do, None), ("part_dby", dy, None), ("part_dd", dxd, bxd)):
            parts[k][0][:, i] = v[:, :, sl].sum(2)
            parts[k][1][:, i] = gamma(FNT + 2) * v[:, :, sl].abs().sum(2) + (0 if extra is None else (1 + gamma(FNT + 2)) * extra[:, :, sl].sum(2))
    out.update(parts)
    return out


BOUNDED_BWD = [(c, k) for c in BWD for k in range(len(SCALES))]


@pytest.mark.parametrize("c,k", BOUNDED_BWD, ids=["%s-%d" % (c["name"], k) for c, k in BOUNDED_BWD])
def test_backward_bounded_case_leaves_few_elements_a_choice(c, k):
    o = make_backward_bounded(c, k)
    assert o["share_dy"] <= SHARE_MAX, (c["name"], k, o["share_dy"])
    assert bool((o["dy_lo"] <= o["dy_hi"]).all())
    assert bool(in_set(rne_bf16_bits(o["dy_model"].float()), o["dy_lo"], o["dy_hi"]).all())
    w = backward_from_dy(o, rne_bf16_bits(o["dy_model"].float()))
    assert all(bool((bar >= 0).all()) and bool(torch.isfinite(want).all()) for want, bar in w.values())
