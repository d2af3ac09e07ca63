"""GPU branch sweep of the training and glue kernels whose launch code picks a path by shape or alignment: every path of each
entry point against torch in float64 on the same fp32 inputs, so that a failing full-size gradient test
(tests/test_gpu_fullsize_training.py) can be pinned on one kernel.  Each case names the branch it reaches and the C condition
(train.hip / glue.hip launch code) it satisfies.  fp32 tolerances are written at each check: a sum of k-deep fp32 addition
chains over terms t_i is within gamma(k) * sum |t_i| of the exact sum, gamma(k) = k u / (1 - k u), u = 2^-24.  Where the
inputs are small integers every partial sum is exact in fp32, and the result must equal the float64 one bit for bit."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _gamma(k):
    return k * U / (1.0 - k * U)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _L():
    from set_amd import _lib
    return _lib.lib()


def _check(rc, name):
    from set_amd import _lib
    _lib.check(rc, name)


_ALIVE = []  # device tensors whose raw address went to a launch: a temporary freed before its kernel ran could be handed out again


@pytest.fixture(autouse=True)
def _keep_launch_operands():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _p(t):
    from set_amd.ops import _p as p
    if t is not None:
        _ALIVE.append(t)
    return p(t)


def _s():
    from set_amd.ops import _stream
    return _stream()


def _shifted(t, off, dev):
    """t copied to dev, starting `off` floats into its own allocation (off = 1: a 4-byte storage offset)."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rows_sum_depth(rows):
    # rows_sum.h: four interleaved chains over rows / ROWS_RG (16) rows per group, pairwise combine (2), 16 groups in order
    return -(-rows // 64) + 2 + 16


# ------------------------------------------------------------------------------------------------------------------------
# LayerNorm over channels: backward (three block shapes, with / without `add`; the partial-row scratch is required) and
# forward (register / loop path)
# ------------------------------------------------------------------------------------------------------------------------
LN_BWD = [
    # B, C, T, add
    (3, 80, 70, False),     # 16x16 / 256 threads: C <= 256 && B * ceil(T/32) = 9 < 256
    (3, 192, 70, True),     # 16x16 / 256 threads, `add` (pre-LN residual)
    (2, 256, 45, True),     # 16x16 / 256 threads, C = 256 = 16 groups x RC 16 (cq <= RC)
    (16, 80, 509, False),   # 32x16 / 512 threads: C <= 256 && B * ceil(T/32) = 16 * 16 = 256 >= n_cu
    (32, 192, 250, True),   # 32x16 / 512 threads: 32 * 8 = 256 >= n_cu, `add`
    (32, 192, 250, False),  # 32x16 / 512 threads without `add`
    (16, 256, 509, True),   # 32x16 / 512 threads at C = 256 (cq = 16 = RC)
    (2, 257, 70, False),    # 32x8 loop: C > 256 -> 8 groups, cq = 33 > RC 32 (the register path of <32, 8, 32> never runs)
    (3, 384, 45, True),     # 32x8 loop, `add`, cq = 48
    (2, 384, 33, False),    # 32x8 loop, one tile and a frame (T = 33)
    (16, 384, 509, True),   # 32x8 loop at a grid that would take the 512-thread shape if C <= 256
]


def _ln_ref(x, gam, mask, dy, add, eps=1e-5):
    """float64 LayerNorm-over-channels backward: dx (+ add), dgamma, dbeta, and per-element / per-channel error bounds."""
    x, gam, mask, dy = x.double(), gam.double(), mask.double(), dy.double()
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    dym = dy * mask[:, None]
    G = dym * gam[None, :, None]
    s1, s2 = G.mean(1, keepdim=True), (G * xh).mean(1, keepdim=True)
    dx = rstd * (G - s1 - xh * s2)
    # the kernel's per-frame sums run over <= ceil(C / CG) channels in a thread and CG (<= 16) groups in LDS; mean, rstd, s1 and
    # s2 each carry <= (C + 16) u relative error of their |terms| sums, x-hat and G a few roundings: 4 (C + 32) u is a safe bar
    k = 4 * (C + 32)
    bdx = _gamma(k) * rstd * (G.abs() + G.abs().mean(1, keepdim=True) + xh.abs() * (G * xh).abs().mean(1, keepdim=True))
    if add is not None:
        dx = dx + add.double()
        bdx = bdx + U * (dx.abs() + add.double().abs())
    dgam = (dym * xh).sum((0, 2))
    dbet = dym.sum((0, 2))
    # dgamma terms dy x-hat: x-hat carries k u (|x-hat| + |mean| rstd) absolute error (|mean| rstd < 1 for these inputs)
    return dx, dgam, dbet, bdx, (dym.abs() * (xh.abs() + 1.0)).sum((0, 2)), k


@pytest.mark.parametrize("case", LN_BWD)
def test_layernorm_ch_bwd_every_block_shape(dev, case):
    B, C, T, with_add = case
    g = torch.Generator().manual_seed(B * 1000 + C + T)
    x = torch.randn(B, C, T, generator=g) * 2.0 + 0.5
    gam = torch.randn(C, generator=g) * 0.3 + 1.0
    mask = (torch.rand(B, T, generator=g) > 0.15).float()
    mask[:, -1] = 1.0  # the last frame of every utterance (the last partial row of the last block) contributes
    dy = _ints(g, (B, C, T), -3, 3)  # integer gradients: dbeta = sum of integers, exact in fp32 in any order
    add = torch.randn(B, C, T, generator=g) if with_add else None
    dx_ref, dg_ref, db_ref, bdx, dg_abs, k = _ln_ref(x, gam, mask, dy, add)
    xd, gd, md, dyd = x.to(dev), gam.to(dev), mask.to(dev), dy.to(dev)
    dx = torch.empty_like(xd)
    dg0, db0 = torch.randn(C, generator=g), _ints(g, (C,), -4, 4)  # dgamma / dbeta are accumulated (+=)
    dg, db = dg0.to(dev), db0.to(dev)
    L = _L()
    tiles = (T + 15) // 16 if (C <= 256 and B * ((T + 31) // 32) < 256) else (T + 31) // 32
    n_part = L.set_layernorm_ch_bwd_scratch(B, C, T)
    assert n_part >= tiles * B * 2 * C
    part = torch.full((n_part,), float("nan"), device=dev)  # every row the partial sum reads must have been written
    if add is None:
        _check(L.set_layernorm_ch_bwd(_p(xd), _p(gd), _p(md), _p(dyd), _p(dx), _p(dg), _p(db), _p(part), B, C, T, 1e-5, _s()),
               "set_layernorm_ch_bwd")
    else:
        _check(L.set_layernorm_ch_bwd_add(_p(xd), _p(gd), _p(md), _p(dyd), _p(add.to(dev)), _p(dx), _p(dg), _p(db), _p(part), B, C, T,
                                          1e-5, _s()), "set_layernorm_ch_bwd_add")
    torch.cuda.synchronize()
    err = (dx.cpu().double() - dx_ref).abs()
    assert bool((err <= bdx + 1e-30).all()), (case, float((err / (bdx + 1e-30)).max()))
    # dbeta: integer terms, every partial sum exact -> bit-equal to the float64 sum
    assert torch.equal(db.cpu().double(), db_ref + db0.double()), (case, float((db.cpu().double() - db_ref - db0.double()).abs().max()))
    # dgamma: per-term error of x-hat (k u) plus a 5-level lane tree, the partial-row column sum (B * tiles rows) and the +=
    rows = B * tiles
    depth = k + 5 + _rows_sum_depth(rows) + 1
    bdg = _gamma(depth) * (dg_abs + dg0.double().abs()) + 1e-30
    derr = (dg.cpu().double() - dg_ref - dg0.double()).abs()
    assert bool((derr <= bdg).all()), (case, float((derr / bdg).max()))


LN_FWD = [
    # B, C, T
    (3, 80, 70),     # register path: cq = ceil(C / LN_CG 8) = 10 <= LN_RC 32
    (2, 256, 45),    # register path at the edge: cq = 32 = LN_RC
    (2, 257, 33),    # loop path: cq = 33 > LN_RC
    (4, 384, 101),   # loop path, T not a multiple of LN_FT 32
]


@pytest.mark.parametrize("case", LN_FWD)
@pytest.mark.parametrize("masked", [False, True])
def test_layernorm_ch_forward_register_and_loop_paths(dev, case, masked):
    B, C, T = case
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(B, C, T, generator=g) * 2.0 + 0.5
    gam, bet = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.1
    mask = (torch.rand(B, T, generator=g) > 0.2).float() if masked else None
    xx = x.double()
    mean = xx.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xx - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (xx - mean) * rstd
    want = xh * gam.double()[None, :, None] + bet.double()[None, :, None]
    # mean / variance: <= (C + 8)-deep sums (bar 4 (C + 32) u on |x-hat| |gamma|), then three roundings of the affine map
    bound = _gamma(4 * (C + 32)) * (xh.abs() + 1.0) * gam.double().abs()[None, :, None] + 3 * U * (want.abs() + bet.double().abs()[None, :, None])
    if mask is not None:
        want, bound = want * mask.double()[:, None], bound * mask.double()[:, None]
    out = torch.full((B, C, T), float("nan"), device=dev)
    _check(_L().set_layernorm_ch(_p(x.to(dev)), _p(gam.to(dev)), _p(bet.to(dev)), _p(None if mask is None else mask.to(dev)), _p(out),
                                 B, C, T, 1e-5, _s()), "set_layernorm_ch")
    torch.cuda.synchronize()
    err = (out.cpu().double() - want).abs()
    assert bool((err <= bound + 1e-30).all()), float((err / (bound + 1e-30)).max())


# ------------------------------------------------------------------------------------------------------------------------
# reductions with a capped grid: set_weighted_sum_det (1024 blocks), set_sumsq_det (2048 blocks), set_channel_sum_det slices
# ------------------------------------------------------------------------------------------------------------------------
N_FLAT = 23837795  # the spec_denoiser flat parameter count (the gradient-norm reduction of every optimizer step); asserted against the
                   # model in test_gpu_fullsize_training.py::test_clipped_adamw_update_on_the_full_flat_buffer_matches_torch
WSUM_N = [
    (1, 1),          # one block
    (255, 1),        # one partial block
    (262144, 80),    # blocks = n / 256 = 1024: exactly at the cap, one element per thread
    (262145, 80),    # blocks > 1024 -> capped at 1024: grid-stride loop, the last element on a second pass of block 0
    (2048000, 80),   # B=32 L1/SSIM frame sums (32 * 800 * 80): capped, ~8 elements per thread
    (N_FLAT, 1),     # the flat parameter count
]


def _wsum_depth(n, cap):
    blocks = min(cap, -(-n // 256))
    return -(-n // (blocks * 256)) + 8 + _rows_sum_depth(blocks) + 1, blocks


@pytest.mark.parametrize("n,inner", WSUM_N)
def test_weighted_sum_det_below_at_and_above_the_block_cap(dev, n, inner):
    from set_amd import autograd_ops as A
    g = torch.Generator().manual_seed(n % 100003)
    L = _L()
    scratch = torch.full((1024 + 64,), float("nan"), device=dev)
    # integers with sum |x w| < 2^24: every partial sum exact -> bit-equal to the float64 sum
    x = _ints(g, (n,), -1, 1) * (torch.rand(n, generator=g) < 0.6).float()
    w = _ints(g, (-(-n // inner),), 0, 1)
    for ww in (w, None):
        want = float((x.double() * (ww.double().repeat_interleave(inner)[:n] if ww is not None else 1.0)).sum())
        out = torch.full((1,), 3.0, device=dev)  # accumulated (+=)
        _check(L.set_weighted_sum_det(_p(x.to(dev)), _p(None if ww is None else ww.to(dev)), _p(out), n, inner, _p(scratch), _s()),
               "set_weighted_sum_det")
        torch.cuda.synchronize()
        assert float(out) == want + 3.0, (n, ww is None, float(out), want)
    # random floats: within gamma(depth) sum |x w|
    xf, wf = torch.randn(n, generator=g), torch.rand(-(-n // inner), generator=g)
    terms = xf.double() * wf.double().repeat_interleave(inner)[:n]
    depth, _ = _wsum_depth(n, 1024)
    got = A._sum(xf.to(dev), wf.to(dev), inner, arena=False)
    torch.cuda.synchronize()
    assert abs(float(got) - float(terms.sum())) <= _gamma(depth + 1) * float(terms.abs().sum()), (n, float(got), float(terms.sum()))


SUMSQ_N = [
    1,          # one block
    255,        # one partial block
    524288,     # blocks = 2048: exactly at the cap
    524289,     # above the cap: capped at 2048, grid-stride loop
    2048000,    # capped, ~4 elements per thread
    N_FLAT,     # the flat parameter buffer: ~46 elements per thread
]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_det_below_at_and_above_the_block_cap(dev, n):
    from set_amd import autograd_ops as A
    g = torch.Generator().manual_seed(n % 100019)
    L = _L()
    scratch = torch.full((2048 + 64,), float("nan"), device=dev)
    # {-1, 0, 1} with < 2^24 nonzeros: integer partial sums, exact
    x = _ints(g, (n,), -1, 1) * (torch.rand(n, generator=g) < 0.6).float()
    out = torch.full((1,), 5.0, device=dev)  # accumulated (+=)
    _check(L.set_sumsq_det(_p(x.to(dev)), _p(out), n, _p(scratch), _s()), "set_sumsq_det")
    torch.cuda.synchronize()
    assert float(out) == float((x.double() ** 2).sum()) + 5.0, (n, float(out))
    xf = torch.randn(n, generator=g) * 1e-3
    want = float((xf.double() ** 2).sum())
    depth, _ = _wsum_depth(n, 2048)
    got = float(A.grad_sumsq(xf.to(dev)))
    assert abs(got - want) <= _gamma(depth + 1) * want, (n, got, want)  # all terms >= 0


CHSUM = [
    # B, C, T
    (1, 192, 77),     # slices = min(B, ceil(2048 / C)) = 1
    (4, 192, 100),    # slices = B = 4 (ceil(2048 / 192) = 11 > B)
    (8, 512, 33),     # slices = ceil(2048 / 512) = 4, between 1 and B
    (32, 80, 800),    # slices = 26 of B = 32: the mel-level shape at the bench size
    (3, 4096, 5),     # C > 2048: slices = 1
]


@pytest.mark.parametrize("case", CHSUM)
def test_channel_sum_det_slice_counts(dev, case):
    B, C, T = case
    g = torch.Generator().manual_seed(B + C + T)
    x = _ints(g, (B, C, T), -4, 4)  # integer terms: exact
    out0 = _ints(g, (C,), -2, 2)
    out = out0.to(dev)
    scratch = torch.full((2048 + C + 64,), float("nan"), device=dev)
    _check(_L().set_channel_sum_det(_p(x.to(dev)), _p(out), B, C, T, _p(scratch), _s()), "set_channel_sum_det")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), x.double().sum((0, 2)) + out0.double())


# ------------------------------------------------------------------------------------------------------------------------
# set_scatter_rows_det: segment counts, both modes, channel tails, padding / clamping, runs across segment boundaries
# ------------------------------------------------------------------------------------------------------------------------
SCATTER = [
    # B, T, C, n_rows, mode, padding_idx, pattern
    (3, 200, 80, 40, 0, -1, "random"),    # S = T / 128 = 1 (< 2 -> 1), C = 80: a 64-channel block + a 16-lane tail
    (2, 130, 100, 30, 0, 0, "clamp"),     # S = 1, padding_idx = 0, indices < 0 clamped to 0 (skipped) and >= n_rows to n_rows - 1
    (4, 800, 192, 300, 0, 5, "runs"),     # S = 6 (seg = 134 = 16 * 8 + 6: 8-frame batches + tail), runs across segment borders
    (2, 800, 80, 256, 0, -1, "bins"),     # S = 6, a new row every frame (pitch bins)
    (2, 1100, 80, 100, 0, 3, "runs"),     # S = min(8, 1100 / 128) = 8, seg = 138
    (2, 2000, 64, 50, 0, -1, "random"),   # S = 8 (capped: 2000 / 128 = 15), C = 64 exactly one block
    (3, 200, 80, 40, 1, -1, "sorted"),    # mode 1 (alignment gather), S = 1: row = idx - 1, idx == 0 and idx > n_rows skipped
    (4, 800, 192, 100, 1, -1, "sorted"),  # mode 1, S = 6, runs of one phoneme across segment borders
    (2, 1030, 100, 77, 1, -1, "sorted"),  # mode 1, S = 8, C = 100
]


def _scatter_idx(g, B, T, n_rows, pattern):
    if pattern == "random":
        return torch.randint(0, n_rows, (B, T), generator=g)
    if pattern == "clamp":
        return torch.randint(-3, n_rows + 4, (B, T), generator=g)
    if pattern == "bins":
        return torch.randint(0, n_rows, (B, T), generator=g)
    if pattern == "runs":  # long runs of one row, boundaries anywhere (also exactly on the segment borders)
        lens = torch.randint(1, 300, (B, T), generator=g)
        idx = torch.empty(B, T, dtype=torch.int64)
        for b in range(B):
            t, r = 0, 0
            while t < T:
                k = int(lens[b, r % T])
                idx[b, t:t + k] = int(torch.randint(0, n_rows, (1,), generator=g))
                t, r = t + k, r + 1
        return idx
    # sorted 1-based alignment with a zero-padded tail and a few indices beyond n_rows
    idx = torch.sort(torch.randint(1, n_rows + 1, (B, T), generator=g), dim=1).values
    idx[:, -T // 10:] = 0
    idx[0, :3] = n_rows + 1
    return idx


@pytest.mark.parametrize("case", SCATTER)
def test_scatter_rows_det_segments_modes_and_rows(dev, case):
    B, T, C, n_rows, mode, pad, pattern = case
    L = _L()
    assert L.set_scatter_rows_segments(T) == (1 if T < 256 else min(8, T // 128))
    S = L.set_scatter_rows_segments(T)
    g = torch.Generator().manual_seed(B * T + C)
    idx = _scatter_idx(g, B, T, n_rows, pattern)
    doutT = _ints(g, (B, T, C), -8, 8) / 8.0  # eighths: every partial sum exact
    scale = 0.5
    n_tab = n_rows if mode == 0 else B * n_rows
    tab0 = _ints(g, (n_tab, C), -4, 4) / 4.0  # accumulated (+=)
    want = tab0.double().clone()
    d = doutT.double() * scale
    for b in range(B):
        if mode == 0:
            r = idx[b].clamp(0, n_rows - 1)
            keep = r != pad
            want.index_add_(0, r[keep], d[b][keep])
        else:
            keep = (idx[b] > 0) & (idx[b] <= n_rows)
            want.index_add_(0, b * n_rows + idx[b][keep] - 1, d[b][keep])
    tab = tab0.to(dev)
    scratch = torch.full((B * S * n_rows * C + 64,), float("nan"), device=dev)  # zeroed by the call
    _check(L.set_scatter_rows_det(_p(idx.to(dev)), _p(doutT.to(dev)), _p(tab), B, T, C, n_rows, scale, pad, mode, _p(scratch), _s()),
           "set_scatter_rows_det")
    torch.cuda.synchronize()
    got = tab.cpu().double()
    assert torch.equal(got, want), (case, float((got - want).abs().max()))
    if mode == 0 and pad >= 0:
        assert torch.equal(got[pad], tab0[pad].double())


# ------------------------------------------------------------------------------------------------------------------------
# duration / pitch loss sums (ordered partials) and their second-pass gradients
# ------------------------------------------------------------------------------------------------------------------------
DUR = [
    # B, T, T_txt, sil_ids
    (3, 77, 19, (1, 2, 3)),       # one block per utterance, T_txt < 256
    (32, 800, 100, (1, 2, 3)),    # the bench size: 32 blocks (ordered partials, 32 rows)
    (4, 1000, 300, (1, 2, 3)),    # T_txt = 300 > 256 threads: the stride-256 token loops take a second pass
    (2, 50, 7, tuple(range(80))), # every token silent: n_words = 0 (word sums 0)
]


def _dur_sums_ref(dur, mel2ph, txt, word_id, n_words):
    B, T_txt = dur.shape
    dg = torch.zeros(B, T_txt + 1, dtype=torch.float64)
    dg.scatter_add_(1, mel2ph.clamp(0, T_txt), torch.ones_like(mel2ph, dtype=torch.float64))
    np_ = (txt != 0).double()
    dgt = dg[:, 1:] * np_
    l1, l2 = torch.log(dur.double() + 1), torch.log(dgt + 1)
    s0, s1 = ((l1 - l2) ** 2 * np_).sum(), np_.sum()
    wp = torch.zeros(B, n_words + 1, dtype=torch.float64).scatter_add_(1, word_id, dur.double())[:, 1:]
    wg = torch.zeros(B, n_words + 1, dtype=torch.float64).scatter_add_(1, word_id, dgt)[:, 1:]
    wm = (wg > 0).double()
    w1, w2 = torch.log(wp + 1), torch.log(wg + 1)
    s2, s3 = ((w1 - w2) ** 2 * wm).sum(), wm.sum()
    # per term: two logf (<= 2 ulp each) and a word sum (<= T_txt-deep) -> |d| <= 8 u (|l1| + |l2|) + T_txt u; squared and
    # summed in a <= ceil(T_txt / 256) + 8 deep chain per utterance, then over B utterances in the partial-row sum
    e0 = (2 * (l1 - l2).abs() * 8 * U * (l1.abs() + l2.abs()) * np_).sum()
    e2 = (2 * (w1 - w2).abs() * (8 * U * (w1.abs() + w2.abs()) + T_txt * U) * wm).sum()
    depth = -(-max(T_txt, n_words) // 256) + 8 + _rows_sum_depth(B) + 2
    f = [float(v.detach()) for v in (s0, s1, s2, s3, e0, e2)]
    return f[:4], [f[4] + _gamma(depth) * f[0], 0.0, f[5] + _gamma(depth) * f[2], 0.0], (s0, s1, s2, s3)


@pytest.mark.parametrize("case", DUR)
def test_dur_loss_sums_and_gradients(dev, case):
    from set_amd import autograd_ops as A
    from set_amd.synthetic import synthetic_inputs
    B, T, T_txt, sil_ids = case
    inp = synthetic_inputs(B, T, T_txt, seed=77 + T, pad_tail=True)
    g = torch.Generator().manual_seed(T_txt)
    dur = torch.rand(B, T_txt, generator=g) * 8
    txt = inp["txt_tokens"].clone()
    txt[:, -2:] = 0  # padded tokens
    mel2ph = inp["mel2ph"]
    sil = torch.zeros_like(txt, dtype=torch.bool)
    for i in sil_ids:
        sil |= txt == i
    sil = sil.long()
    word_id = (sil.cumsum(-1) * (1 - sil)).contiguous()
    n_words = int(word_id.max())
    assert (n_words == 0) == (len(sil_ids) == 80)
    want, bound, _ = _dur_sums_ref(dur, mel2ph, txt, word_id, n_words)
    L = _L()
    sums = torch.zeros(4, device=dev)
    scratch = torch.full((4 * B + 64,), float("nan"), device=dev)
    _check(L.set_dur_loss_sums_det(_p(dur.to(dev)), _p(mel2ph.to(dev)), _p(txt.to(dev)), _p(word_id.to(dev)), _p(sums), B, T, T_txt,
                                   n_words, _p(scratch), _s()), "set_dur_loss_sums_det")
    torch.cuda.synchronize()
    got = sums.cpu().tolist()
    for k in range(4):
        assert abs(got[k] - want[k]) <= bound[k] + 1e-30, (case, k, got[k], want[k])   # [1], [3]: integer counts, exact
    if n_words == 0:
        assert got[2] == 0.0 and got[3] == 0.0
    # second pass: d(pdur + wdur) / d dur against float64 autograd of the same sums (O.dur_losses' formulas; the oracle itself
    # builds its ground-truth durations in fp32)
    ld = dur.double().clone().requires_grad_(True)
    with torch.enable_grad():
        _, _, (s0, s1, s2, s3) = _dur_sums_ref(ld, mel2ph, txt, word_id, n_words)
        pd = s0 / s1 * 0.1
        (pd + (s2 / s3 * 1.0 if n_words > 0 else 0.0)).backward()
    dd = dur.clone().to(dev).requires_grad_(True)
    with torch.enable_grad():
        pd2, wd2 = A.dur_losses(dd, mel2ph.to(dev), txt.to(dev), word_id.to(dev), n_words, 0.1, 1.0)
        (pd2 + wd2 if n_words > 0 else pd2).backward()
    torch.cuda.synchronize()
    assert abs(float(pd2) - float(pd)) <= 0.1 * (bound[0] / want[1] + 2 * U * float(pd) / 0.1) + 1e-30
    # per element: 2 (l1 - l2) / (d + 1) / S with the log difference to 8 u (|l1| + |l2|) (+ the word sum's T_txt u), then ~4 roundings
    dgt = torch.zeros(B, T_txt + 1, dtype=torch.float64).scatter_add_(1, mel2ph.clamp(0, T_txt), torch.ones_like(mel2ph, dtype=torch.float64))[:, 1:]
    npd = (txt != 0).double()
    l1, l2 = torch.log(dur.double() + 1), torch.log(dgt * npd + 1)
    bnd = 0.1 * 2 * npd * (8 * U * (l1.abs() + l2.abs()) + 4 * U * (l1 - l2).abs()) / (dur.double() + 1) / want[1]
    if n_words > 0:  # the word term of the token's word: 2 (w1 - w2) / (wp + 1) / S3, wp a <= T_txt-term sum of positive durations
        wp = torch.zeros(B, n_words + 1, dtype=torch.float64).scatter_add_(1, word_id, dur.double())
        wg = torch.zeros(B, n_words + 1, dtype=torch.float64).scatter_add_(1, word_id, dgt * npd)
        wpt, wgt = wp.gather(1, word_id), wg.gather(1, word_id)
        w1, w2 = torch.log(wpt + 1), torch.log(wgt + 1)
        on = ((word_id > 0) & (wgt > 0)).double()
        bnd = bnd + on * 2 * ((8 * U * (w1.abs() + w2.abs()) + T_txt * U) + 4 * U * (w1 - w2).abs()) / (wpt + 1) / want[3]
        bnd = bnd + 2 * U * ld.grad.abs()  # the sum of the two terms
    err = (dd.grad.cpu().double() - ld.grad).abs()
    assert bool((err <= bnd + 1e-30).all()), (case, float((err / (bnd + 1e-30)).max()))


PITCH = [
    # B, T
    (3, 77),     # one block (B * T = 231 < 256)
    (5, 333),    # 7 blocks, the last one partial
    (32, 800),   # the bench size: 100 blocks of ordered partials
]


@pytest.mark.parametrize("case", PITCH)
def test_pitch_loss_sums_and_gradients(dev, case):
    from set_amd import autograd_ops as A
    from set_amd.synthetic import synthetic_inputs
    B, T = case
    inp = synthetic_inputs(B, T, 20, seed=91 + T, pad_tail=True)
    g = torch.Generator().manual_seed(T)
    pp = torch.randn(B, T, 2, generator=g) * 2
    pp[..., 0] += 8.0  # f0 prediction around the f0 values
    f0, uv, mel2ph = inp["f0"], inp["uv"], inp["mel2ph"]
    npd = (mel2ph != 0).double()
    nv = npd * (uv == 0).double()
    lg, fp = pp[..., 1].double(), pp[..., 0].double()
    bce = torch.clamp(lg, min=0) - lg * uv.double() + torch.log1p(torch.exp(-lg.abs()))
    l1 = (fp - f0.double()).abs()
    want = [float((bce * npd).sum()), float(npd.sum()), float((l1 * nv).sum()), float(nv.sum())]
    nb = -(-B * T // 256)
    depth = 6 + 2 + _rows_sum_depth(nb) + 1  # 64-lane tree, 4 waves in order, the partial rows
    # per term: bce from max / mul / log1pf(expf) (<= 8 u of |max| + |x u| + log1p), |fp - f0| one rounding
    e0 = float((8 * U * (lg.abs() + 1.0) * npd).sum()) + _gamma(depth) * float((bce.abs() * npd).sum())
    e2 = float((U * l1 * nv).sum()) + _gamma(depth) * want[2]
    bound = [e0, 0.0, e2, 0.0]
    L = _L()
    sums = torch.zeros(4, device=dev)
    scratch = torch.full((4 * nb + 64,), float("nan"), device=dev)
    ppd = pp.transpose(1, 2).contiguous().to(dev)
    _check(L.set_pitch_loss_sums_det(_p(ppd), _p(f0.to(dev)), _p(uv.to(dev)), _p(mel2ph.to(dev)), _p(sums), B, T, _p(scratch), _s()),
           "set_pitch_loss_sums_det")
    torch.cuda.synchronize()
    got = sums.cpu().tolist()
    for k in range(4):
        assert abs(got[k] - want[k]) <= bound[k] + 1e-30, (case, k, got[k], want[k])
    lpp = pp.double().clone().requires_grad_(True)
    with torch.enable_grad():
        uvl, f0l = O.pitch_losses(lpp, f0.double(), uv.double(), mel2ph, 1.0, 1.0)
        (uvl + f0l).backward()
    dpp = ppd.clone().requires_grad_(True)
    with torch.enable_grad():
        u2, f2 = A.pitch_losses(dpp, f0.to(dev), uv.to(dev), mel2ph.to(dev), 1.0, 1.0)
        (u2 + f2).backward()
    torch.cuda.synchronize()
    gref = lpp.grad.transpose(1, 2)
    gg = dpp.grad.cpu().double()
    # f0 row: sign * nv / S3 (the sign of an fp32 difference is exact), 3 roundings; uv row: (sigmoid(x) - u) / S1, sigmoid to 4 u
    assert bool(((gg[:, 0] - gref[:, 0]).abs() <= 3 * U * gref[:, 0].abs() + 1e-30).all())
    b_uv = (8 * U * (torch.sigmoid(lg) + uv.double()) * npd / want[1])
    assert bool(((gg[:, 1] - gref[:, 1]).abs() <= b_uv + 1e-30).all()), float(((gg[:, 1] - gref[:, 1]).abs() / (b_uv + 1e-30)).max())


# ------------------------------------------------------------------------------------------------------------------------
# SSIM loss (set_ssim_filter / _map / _bwd) at frame counts below the window, off the 16-frame tile and at T = 800
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(2, 7), (3, 77), (2, 800)])   # H < 11 (window larger than the image), H % 16 != 0, H = 800
def test_ssim_loss_at_window_and_tile_edges(dev, B, H):
    """Bars of test_losses_forward_backward (loss 2e-5, gradient 5e-4 of the largest entry): the SSIM map is local (an 11 x 11
    window of second moments of values ~ bias 6, where (E[x^2] - mu^2) cancels ~ 36 / sigma^2 of its fp32 rounding), so its
    per-element error does not grow with H, and the loss is a weighted mean of the map."""
    from set_amd import autograd_ops as A
    g = torch.Generator().manual_seed(B * H)
    M = 80
    pred = torch.randn(B, H, M, generator=g) * 0.5 - 3.0
    target = torch.clamp(torch.randn(B, H, M, generator=g) * 1.5 - 3.0, -6, 1.5)
    target[0, -max(1, H // 7):] = 0  # silent frames: weight 0
    lp = pred.double().clone().requires_grad_(True)
    with torch.enable_grad():
        ref = _ssim_loss64(lp, target.double())
        ref.backward()
    dp = pred.clone().to(dev).requires_grad_(True)
    w = A.frame_weights(target.to(dev))
    with torch.enable_grad():
        got = A.ssim_loss(dp, target.to(dev), w)
        got.backward()
    torch.cuda.synchronize()
    assert abs(float(got) - float(ref)) < 2e-5 * max(1.0, abs(float(ref))), (float(got), float(ref))
    assert _relmax(dp.grad, lp.grad) < 5e-4


def _ssim_loss64(pred, target, bias=6.0, window_size=11, sigma=1.5):
    """O.ssim_loss in float64 throughout (the oracle builds its window in fp32)."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float64)
    g = (g / g.sum()).unsqueeze(1)
    window = g.mm(g.t())[None, None]
    p = window_size // 2
    img1, img2 = pred[:, None] + bias, target[:, None] + bias
    mu1, mu2 = F.conv2d(img1, window, padding=p), F.conv2d(img2, window, padding=p)
    s1 = F.conv2d(img1 * img1, window, padding=p) - mu1 ** 2
    s2 = F.conv2d(img2 * img2, window, padding=p) - mu2 ** 2
    s12 = F.conv2d(img1 * img2, window, padding=p) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean(1)
    w = O.weights_nonzero_speech(target)
    return ((1 - m) * w).sum() / w.sum()


def _relmax(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------------
# elementwise kernels with a 16-byte path: vector path (T % 4 == 0 / n % 4 == 0 and 16-byte aligned operands) and the one-
# element path (T % 4 != 0, or an operand at a 4-byte storage offset): the same bits, within an fp64 bound of torch
# ------------------------------------------------------------------------------------------------------------------------
EW_SHAPES = [
    # B, C, T, off
    (2, 96, 100, 0),   # vector path: T % 4 == 0, aligned
    (2, 96, 101, 0),   # one-element path: T % 4 != 0
    (2, 96, 100, 1),   # one-element path: every operand 4 bytes off 16-byte alignment
]


@pytest.mark.parametrize("B,C,T,off", EW_SHAPES)
def test_add_chan_mask_and_conv_epilogue_bwd_paths(dev, B, C, T, off):
    g = torch.Generator().manual_seed(T + off)
    x, add = torch.randn(B, C, T, generator=g), torch.randn(B, C, generator=g)
    mask = (torch.rand(B, T, generator=g) > 0.3).float()
    y = torch.randn(B, C, T, generator=g)
    L = _L()
    res = {}
    for o in sorted({off, 1}):  # this case's layout, and always the one-element form for the bit comparison
        xd, md, yd = _shifted(x, o, dev), _shifted(mask, o, dev), _shifted(y, o, dev)
        ad = add.to(dev)
        out = _shifted(torch.zeros(B, C, T), o, dev)
        _check(L.set_add_chan_mask(_p(xd), _p(ad), _p(md), _p(out), B, C, T, _s()), "set_add_chan_mask")
        out2 = _shifted(torch.zeros(B, C, T), o, dev)
        _check(L.set_add_chan_mask(_p(xd), None, _p(md), _p(out2), B, C, T, _s()), "set_add_chan_mask")
        gr = _shifted(torch.zeros(B, C, T), o, dev)
        _check(L.set_conv_epilogue_bwd(_p(xd), _p(yd), _p(md), _p(gr), B, C, T, 1, 0.75, _s()), "set_conv_epilogue_bwd")  # relu
        gn = _shifted(torch.zeros(B, C, T), o, dev)
        _check(L.set_conv_epilogue_bwd(_p(xd), None, None, _p(gn), B, C, T, 0, 1.0 / 3.0, _s()), "set_conv_epilogue_bwd")
        gm = _shifted(torch.zeros(B, C, T), o, dev)
        _check(L.set_conv_epilogue_bwd(_p(xd), None, _p(md), _p(gm), B, C, T, 0, 0.75, _s()), "set_conv_epilogue_bwd")  # mask alone
        gy = _shifted(torch.zeros(B, C, T), o, dev)
        _check(L.set_conv_epilogue_bwd(_p(xd), _p(yd), None, _p(gy), B, C, T, 1, 1.0, _s()), "set_conv_epilogue_bwd")  # relu alone
        torch.cuda.synchronize()
        res[o] = [t.cpu() for t in (out, out2, gr, gn, gm, gy)]
    for a, b in zip(res[off], res[1]):
        assert torch.equal(a, b)
    xx, mm = x.double(), mask.double()[:, None]
    want = [(xx + add.double()[:, :, None]) * mm, xx * mm, xx * mm * (y.double() > 0) * 0.75, xx * (1.0 / 3.0),
            xx * mm * 0.75, xx * (y.double() > 0)]
    bounds = [2 * U * (xx.abs() + add.double().abs()[:, :, None]) * mm, U * xx.abs() * mm, 3 * U * xx.abs() * 0.75, 2 * U * xx.abs() / 3.0,
              3 * U * xx.abs() * 0.75, U * xx.abs()]
    for got, w_, b_ in zip(res[off], want, bounds):
        assert bool(((got.double() - w_).abs() <= b_ + 1e-30).all())


ACTS = [("relu", 1), ("gelu", 2), ("tanh", 3), ("softplus", 4), ("mish", 5)]


@pytest.mark.parametrize("n,off", [(4000, 0), (4001, 0), (4000, 1)])  # vector: n % 4 == 0 && aligned; one-element: n % 4 != 0 / 4 bytes off
@pytest.mark.parametrize("act", ACTS, ids=[a[0] for a in ACTS])
def test_activation_forward_backward_paths(dev, act, n, off):
    from set_amd import _lib
    name, code = act
    assert _lib.ACT[name] == code
    g = torch.Generator().manual_seed(n + off + code)
    z = torch.randn(n, generator=g) * 3
    z[:8] = torch.tensor([0.0, -0.0, 25.0, -25.0, 20.0, 19.5, -7.0, 7.0])  # softplus / mish switch at 20, saturated gelu / tanh
    dy = torch.randn(n, generator=g)
    L = _L()
    res = {}
    for o in sorted({off, 1}):
        zd, dyd = _shifted(z, o, dev), _shifted(dy, o, dev)
        y, dz, dzs = (_shifted(torch.zeros(n), o, dev) for _ in range(3))
        _check(L.set_act_fwd(_p(zd), _p(y), n, code, 0.0, _s()), "set_act_fwd")
        _check(L.set_act_bwd(_p(zd), _p(dyd), _p(dz), n, code, 0.0, _s()), "set_act_bwd")
        _check(L.set_act_bwd_scaled(_p(zd), _p(dyd), _p(dzs), n, code, 0.0, 0.2, _s()), "set_act_bwd_scaled")
        torch.cuda.synchronize()
        res[o] = [t.cpu() for t in (y, dz, dzs)]
    for a, b in zip(res[off], res[1]):
        assert torch.equal(a, b), name
    zz = z.double().clone().requires_grad_(True)
    fn = {"relu": F.relu, "gelu": F.gelu, "tanh": torch.tanh, "softplus": F.softplus, "mish": O.mish}[name]
    with torch.enable_grad():
        f = fn(zz)
        (f * dy.double()).sum().backward()
    want_y, want_dz = f.detach(), zz.grad
    # a composition of <= 4 libm calls (<= 2 ulp each) and a few roundings, amplified by at most |z| (1 + erf / tanh saturation,
    # the sigmoid inside softplus'): 64 u (|f| + |z|) forward, 64 u |dy| (1 + z^2) backward; the scaled form adds one rounding
    ya = z.double().abs()
    by = 64 * U * (want_y.abs() + ya)
    bdz = 64 * U * dy.double().abs() * (1.0 + ya * ya)
    assert bool(((res[off][0].double() - want_y).abs() <= by + 1e-30).all()), name
    assert bool(((res[off][1].double() - want_dz).abs() <= bdz + 1e-30).all()), name
    assert bool(((res[off][2].double() - 0.2 * want_dz).abs() <= 0.2 * bdz + U * 0.2 * want_dz.abs() + 1e-30).all()), name


GATE_SHAPES = [
    # B, C, T, off
    (2, 96, 100, 0),   # vector path: C * T % 4 == 0, aligned
    (2, 96, 101, 0),   # vector path although T % 4 != 0: the condition is on C * T (= 9696)
    (2, 5, 7, 0),      # one-element path: C * T = 35, % 4 != 0
    (2, 96, 100, 1),   # one-element path: every operand 4 bytes off 16-byte alignment
]


@pytest.mark.parametrize("B,C,T,off", GATE_SHAPES)
def test_gate_and_res_skip_bwd_paths(dev, B, C, T, off):
    """set_gate_bwd / set_res_skip_bwd: 16-byte form when C * T % 4 == 0 and the operands are aligned."""
    g = torch.Generator().manual_seed(C * T + off)
    y, dzz = torch.randn(B, 2 * C, T, generator=g), torch.randn(B, C, T, generator=g)
    dxo, dsk = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
    L = _L()
    res = {}
    for o in sorted({off, 1}):
        yy, dd, a, b = (_shifted(t, o, dev) for t in (y, dzz, dxo, dsk))
        dy, dx, do = _shifted(torch.zeros(B, 2 * C, T), o, dev), _shifted(torch.zeros(B, C, T), o, dev), _shifted(torch.zeros(B, 2 * C, T), o, dev)
        _check(L.set_gate_bwd(_p(yy), _p(dd), _p(dy), B, C, T, _s()), "set_gate_bwd")
        _check(L.set_res_skip_bwd(_p(a), _p(b), _p(dx), _p(do), B, C, T, _s()), "set_res_skip_bwd")
        torch.cuda.synchronize()
        res[o] = [t.cpu() for t in (dy, dx, do)]
    for u_, v_ in zip(res[off], res[1]):
        assert torch.equal(u_, v_)
    s_, th = torch.sigmoid(y[:, :C].double()), torch.tanh(y[:, C:].double())
    dzd = dzz.double()
    want = torch.cat([dzd * th * s_ * (1 - s_), dzd * s_ * (1 - th * th)], 1)
    # sigmoid / tanh to a few ulp, then <= 4 products / differences: 32 u of the products' magnitude
    bnd = 32 * U * torch.cat([dzd.abs() * s_, dzd.abs() * s_], 1)
    assert bool(((res[off][0].double() - want).abs() <= bnd + 1e-30).all())
    assert bool(((res[off][1].double() - dxo.double() / math.sqrt(2.0)).abs() <= 2 * U * dxo.double().abs()).all())
    want_o = torch.cat([dxo.double() / math.sqrt(2.0), dsk.double()], 1)
    assert bool(((res[off][2].double() - want_o).abs() <= 2 * U * want_o.abs()).all())


@pytest.mark.parametrize("n,off", [(1 << 16, 0), ((1 << 16) + 3, 0), (1 << 16, 1)])  # vector: aligned and q*4+3 < n; tail / offset: one-element
def test_dropout_paths(dev, n, off):
    """set_dropout: the keep mask is a function of (seed, offset, element index) alone -- the same bits on either path --
    and a kept element is x * fl(1 / (1 - p)) rounded once."""
    g = torch.Generator().manual_seed(n + off)
    x = torch.randn(n, generator=g)
    p = 0.2
    L = _L()
    res = {}
    for o in sorted({off, 1}):
        y = _shifted(torch.zeros(n), o, dev)
        _check(L.set_dropout(_p(_shifted(x, o, dev)), _p(y), n, p, 11, 5, _s()), "set_dropout")
        torch.cuda.synchronize()
        res[o] = y.cpu()
    assert torch.equal(res[off], res[1])
    y = res[off]
    one = torch.tensor(1.0, dtype=torch.float32)
    inv = one / (one - torch.tensor(p, dtype=torch.float32))  # 1.0f / (1.0f - p) as the kernel rounds it
    kept = y != 0
    assert torch.equal(y[kept], x[kept] * inv)
    assert abs(float(kept.float().mean()) - (1 - p)) < 6 * math.sqrt(p * (1 - p) / n)  # six standard deviations of the keep rate
