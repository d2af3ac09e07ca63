"""GPU checks of the random streams of csrc/philox.h against the float64 / integer model of philox_models.py (which test_philox_reference.py
pins to the published Random123 known answers): every consumer outside the reverse loop -- set_randn, set_posterior_step without eps,
set_dropout, set_residual_dropout, set_conv_epilogue_bwd_dropout -- and the seed delta of set_rng_seed_delta.  Keep decisions and everything
derived from them are bit for bit; normals lie within philox_models.normal_bound, which is derived from the number formats except for K_NORMAL.

K_NORMAL: the installed ROCm states no ulp errors for the device logf / sqrtf / sincosf (neither its HIP headers nor its documents), so it
was measured on the MI355X: over every case of this file the largest k with |got - z64| = r 2^-21 + k 2^-24 max(r, |z64|) was 0.0 (each
test prints it as "measured k"): the angle term alone covered every error, the largest being 0.864 of r 2^-21 (1.5e-6 absolute).  Twice
the measurement would allow nothing for the functions themselves, which the angle term does not account for, so the allowance is what
correctly rounded functions would need, K_NORMAL = 4: half an ulp (2^-24 relative) each for logf and sqrtf, of which the square root
halves the first (0.75 together), one for sin / cos of the rounded angle, one for the product, rounded up; the largest error seen is
0.576 of that bound.  A wrong word, pairing or counter is off by order 1, a factor 10^5 beyond the bound."""
import numpy as np
import pytest
import torch

import philox_models as PM
from raw_abi import L, Sent, bits, check, stream, to_dev

pytestmark = pytest.mark.gpu

K_NORMAL = 4.0
U = 2.0 ** -24
PS = [0.0, 0.1, 0.2, 0.5, 0.999]
SEEN = {"k": 0.0, "frac": 0.0, "angle": 0.0}


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _randn(dev, seed, offset, n, off=0):
    out = Sent((n,), dev, off=off)
    check(L().set_randn(out.ptr, n, seed, offset, stream()), "set_randn")
    return out.get()


def _check_normals(got, seed, offset, what):
    z, r = PM.randn_stream(seed, offset, len(got))
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - z)
    scale = U * np.maximum(r, np.abs(z))
    k = float(np.max(np.where(scale > 0, np.maximum(err - r * 2.0 ** -21, 0.0) / np.where(scale > 0, scale, 1.0), 0.0)))
    frac = float((err / np.maximum(PM.normal_bound(z, r, K_NORMAL), 1e-300)).max())
    SEEN["k"], SEEN["frac"] = max(SEEN["k"], k), max(SEEN["frac"], frac)
    angle = float(np.max(np.where(r > 0, err / np.where(r > 0, r * 2.0 ** -21, 1.0), 0.0)))
    SEEN["angle"] = max(SEEN["angle"], angle)
    print("measured k (%s) = %.3f, largest error %.3e, / bound %.3f, / angle term %.3f" % (what, k, err.max(), frac, angle))
    assert (err <= PM.normal_bound(z, r, K_NORMAL)).all(), (what, k, float(err.max()))


# ---- 1. set_randn ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,offset,n", PM.STREAMS, ids=[s[0] for s in PM.STREAMS])
def test_randn_is_the_pinned_stream(dev, name, seed, offset, n):
    got = _randn(dev, seed, offset, n)
    _check_normals(got, seed, offset, name)
    if name == "known_answer_quad":  # the quad of the first Random123 vector
        assert tuple(int(w) for w in PM.words(0, 0, 1)[0]) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert np.array_equal(bits(_randn(dev, seed, offset, n, off=1)), bits(got))  # the output's alignment does not matter


# ---- 2. Box-Muller extremes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,k,what", PM.EXTREMES, ids=["c%d_w%d_%s" % e for e in PM.EXTREMES])
def test_randn_at_the_box_muller_extremes(dev, ctr, k, what):
    got = _randn(dev, 0, ctr, 4)
    _check_normals(got, 0, ctr, "extreme %d word %d %s" % (ctr, k, what))
    if what == "ones" and k in (0, 2):  # u = 1: radius 0, both elements of the pair are exactly +-0
        assert not (bits(got[k:k + 2]) & 0x7FFFFFFF).any(), got


# ---- 3. one stream however it is cut ------------------------------------------------------------------------------------------------------
def test_randn_offset_continues_the_stream(dev):
    n, k = 1027, 100  # 4 k = 400 elements: the split lies inside the first block of 256 quads
    whole = _randn(dev, 7, 0, n + 4 * k)
    assert np.array_equal(bits(_randn(dev, 7, k, n)), bits(whole[4 * k:]))
    hi = 2 ** 32 - 50  # and across the 32-bit carry of the counter
    whole = _randn(dev, 7, hi, n + 4 * k)
    assert np.array_equal(bits(_randn(dev, 7, hi + k, n)), bits(whole[4 * k:]))


# ---- 4. set_posterior_step without eps ------------------------------------------------------------------------------------------------------
POSTERIOR = [(4, 37), (3, 37), (5, 413)]  # B per_batch % 4 = 0, 3, 1; per_batch % 4 = 1: quads straddle rows; 517 quads: three blocks


def _posterior(dev, x0, xt, coef, eps, seed, offset, in_place):
    B, pb = x0.shape
    xt_s = Sent((B, pb), dev).fill(xt)
    out = xt_s if in_place else Sent((B, pb), dev)
    ops = [to_dev(x0, dev), to_dev(coef, dev), None if eps is None else to_dev(eps, dev)]
    check(L().set_posterior_step(ops[0].data_ptr(), xt_s.ptr, None if eps is None else ops[2].data_ptr(), ops[1].data_ptr(),
                                 0 if coef.shape[0] == 1 else 4, out.ptr, B, pb, seed, offset, stream()), "set_posterior_step")
    res = out.get()
    if not in_place:
        assert np.array_equal(bits(xt_s.get()), bits(xt))
    return res


@pytest.mark.parametrize("B,pb", POSTERIOR)
@pytest.mark.parametrize("shared", [False, True], ids=["coefB4", "coef14"])
def test_posterior_step_draws_set_randns_numbers(dev, B, pb, shared):
    rng = np.random.default_rng(1000 * B + pb)
    x0, xt = (rng.standard_normal((B, pb)).astype(np.float32) for _ in range(2))
    coef = np.stack([rng.uniform(0.1, 0.9, B), rng.uniform(0.1, 0.9, B), rng.uniform(-6.0, 0.0, B), (np.arange(B) != 1).astype(np.float64)],
                    axis=1).astype(np.float32)  # row 1: t == 0, no noise
    if shared:
        coef = coef[:1]
    seed, offset = 0xDEADBEEF12345678, 2 ** 32 - 3  # both key words; the counter's carry inside the call
    eps = _randn(dev, seed, offset, B * pb).reshape(B, pb)
    _check_normals(eps.reshape(-1), seed, offset, "posterior eps")
    res = {}
    for in_place in (True, False):
        drawn = _posterior(dev, x0, xt, coef, None, seed, offset, in_place)
        given = _posterior(dev, x0, xt, coef, eps, seed, offset, in_place)
        assert np.array_equal(bits(drawn), bits(given)), (in_place, "the kernel's own draw is not set_randn's")
        res[in_place] = drawn
    assert np.array_equal(bits(res[True]), bits(res[False]))
    # float64 on the same fp32 operands.  The kernel rounds: each product of the mean (1 u of the term each, u = 2^-24 relative), their sum
    # (1 u), expf of the exact 0.5 lv (taken as within 2 ulp = 4 u), its product with eps (1 u; nz is 0 or 1: exact) and the last sum (1 u):
    # to first order at most 8 u (|c1 x0| + |c2 x_t| + |s eps|)
    c = np.broadcast_to(coef.astype(np.float64), (B, 4))
    t1, t2 = c[:, 0:1] * x0, c[:, 1:2] * xt
    t3 = c[:, 3:4] * np.exp(0.5 * c[:, 2:3]) * eps.astype(np.float64)
    err = np.abs(res[True] - (t1 + t2 + t3))
    bound = 8 * U * (np.abs(t1) + np.abs(t2) + np.abs(t3))
    print("posterior: largest error / bound = %.3f" % float((err / bound).max()))
    assert (err <= bound).all()
    if not shared:
        assert np.array_equal(bits(res[True][1]), bits((coef[1, 0] * x0[1] + coef[1, 1] * xt[1]) + np.float32(0.0) * eps[1]))  # the t == 0 row


# ---- 5. dropout keep masks ------------------------------------------------------------------------------------------------------------------
def _nonzero(rng, shape):
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape)).astype(np.float32)


def _inv(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))  # 1.0f / (1.0f - p) as the kernels round it


def _dropout(dev, x, p, seed, offset, off=0):
    n = len(x)
    xs, y = Sent((n,), dev, off=off).fill(x), Sent((n,), dev, off=off)
    check(L().set_dropout(xs.ptr, y.ptr, n, float(np.float32(p)), seed, offset, stream()), "set_dropout")
    return y.get()


def _check_dropout(y, x, keep, p, what):
    assert np.array_equal(y != 0, keep), (what, "keep mask", int(((y != 0) != keep).sum()))
    assert np.array_equal(bits(y), bits(np.where(keep, x * _inv(p), np.float32(0.0)))), (what, "values")
    if p == 0.0:
        assert np.array_equal(bits(y), bits(x))


@pytest.mark.parametrize("name,seed,offset,n", PM.STREAMS, ids=[s[0] for s in PM.STREAMS])
def test_dropout_keep_mask_is_the_pinned_stream(dev, name, seed, offset, n):
    x = _nonzero(np.random.default_rng(n), (n,))
    for p in PS:
        keep = PM.dropout_keep(seed, offset, n, p)
        for off in (0, 1):  # 0: whole quads as one 16-byte access, the tail one by one; 1: the one-element path throughout
            _check_dropout(_dropout(dev, x, p, seed, offset, off), x, keep, p, (name, p, off))
    if n >= 1023:  # another stream than the normals': the noise words at the same (seed, offset) would keep other elements
        noise_keep = (PM.words(seed, offset, (n + 3) // 4).reshape(-1)[:n] >> np.uint32(8)) >= float(np.float32(0.5)) * 2.0 ** 24
        assert not np.array_equal(noise_keep, PM.dropout_keep(seed, offset, n, 0.5))


RES_SHAPES = [(1, 1, 5), (2, 3, 37), (3, 5, 71)]  # n = 5, 222 (n % 4 = 2), 1065 (267 quads: two blocks)


def _residual(dev, x, z, mask, p, seed, offset):
    B, C, T = x.shape
    ops = [to_dev(x, dev), to_dev(z, dev), None if mask is None else to_dev(mask, dev)]
    y = Sent((B, C, T), dev)
    check(L().set_residual_dropout(ops[0].data_ptr(), ops[1].data_ptr(), None if mask is None else ops[2].data_ptr(), y.ptr, B, C, T,
                                   float(np.float32(p)), seed, offset, stream()), "set_residual_dropout")
    return y.get()


def _residual_bwd(dev, dy, mask, p, seed, offset):
    B, C, T = dy.shape
    ops = [to_dev(dy, dev), None if mask is None else to_dev(mask, dev)]
    g2, gz = Sent((B, C, T), dev), Sent((B, C, T), dev)
    check(L().set_conv_epilogue_bwd_dropout(ops[0].data_ptr(), None if mask is None else ops[1].data_ptr(), g2.ptr, gz.ptr, B, C, T,
                                            float(np.float32(p)), seed, offset, stream()), "set_conv_epilogue_bwd_dropout")
    return g2.get(), gz.get()


@pytest.mark.parametrize("name,seed,offset,_n", PM.STREAMS, ids=[s[0] for s in PM.STREAMS])
def test_residual_dropout_forward_and_backward_share_the_pinned_mask(dev, name, seed, offset, _n):
    i = [s[0] for s in PM.STREAMS].index(name)
    B, C, T = RES_SHAPES[i % 3]
    rng = np.random.default_rng(i)
    x, z, dy = (_nonzero(rng, (B, C, T)) for _ in range(3))  # |x|, |z| in [1, 2): a kept z / (1 - p) >= 1 always changes x
    mask = rng.choice([0.5, 1.0], (B, T)).astype(np.float32)  # never 0: a kept gradient stays nonzero
    for p in PS:
        keep = PM.dropout_keep(seed, offset, B * C * T, p).reshape(B, C, T)
        branch = np.where(keep, z * _inv(p), np.float32(0.0))
        # forward, without and with the mask: fl(x + fl(z inv)) (* m)
        y = _residual(dev, x, z, None, p, seed, offset)
        assert np.array_equal(y != x, keep), (name, p, "forward keep mask")
        assert np.array_equal(bits(y), bits(x + branch)), (name, p)
        ym = _residual(dev, x, z, mask, p, seed, offset)
        assert np.array_equal(bits(ym), bits((x + branch) * mask[:, None, :])), (name, p, "masked")
        # backward: g2 = dy (* m), gz = keep g2 inv
        for m in (None, mask):
            g = dy if m is None else dy * m[:, None, :]
            g2, gz = _residual_bwd(dev, dy, m, p, seed, offset)
            assert np.array_equal(bits(g2), bits(g)), (name, p, m is None)
            assert np.array_equal(gz != 0, keep), (name, p, "backward keep mask")  # = the forward's: what training depends on
            assert np.array_equal(gz != 0, y != x)
            assert np.array_equal(bits(gz), bits(np.where(keep, g * _inv(p), np.float32(0.0)))), (name, p, m is None)


def test_dropout_keeps_at_u_equal_p_and_drops_just_above(dev):
    seed, offset, n = 0xDEADBEEF12345678, 17 * 2 ** 28, 37
    top = (PM.dropout_words(seed, offset, n) >> np.uint32(8)).astype(np.int64)
    rng = np.random.default_rng(5)
    x, z = _nonzero(rng, (n,)), _nonzero(rng, (n,))
    for j in (0, 5, 17, 36):  # one word of each position in a quad, the partial last quad included
        assert 0 < top[j] < 2 ** 24 - 1
        for t, kept in ((top[j], True), (top[j] + 1, False)):
            p = t / 2.0 ** 24  # a multiple of 2^-24 below 1: exact in fp32
            assert float(np.float32(p)) == p and PM.dropout_keep(seed, offset, n, p)[j] == kept
            for off in (0, 1):
                assert (_dropout(dev, x, p, seed, offset, off)[j] != 0) == kept, (j, t, off)
            y = _residual(dev, x.reshape(1, 1, n), z.reshape(1, 1, n), None, p, seed, offset).reshape(-1)
            assert (y[j] != x[j]) == kept, (j, t)
            gz = _residual_bwd(dev, x.reshape(1, 1, n), None, p, seed, offset)[1].reshape(-1)
            assert (gz[j] != 0) == kept, (j, t)


# ---- 6. the seed delta ----------------------------------------------------------------------------------------------------------------------
DELTAS = [(0xFFFFFFFF, 1), (2 ** 64 - 1, 2), (7, 0x0123456789ABCDEF)]  # the carry into the high key word; the wrap; both words of the delta


@pytest.mark.parametrize("s,d", DELTAS, ids=["carry", "wrap", "wide"])
def test_seed_delta_is_added_modulo_2_64(dev, s, d):
    eff = (s + d) % 2 ** 64
    offset, n, p = 2 ** 32 - 1, 1027, 0.2
    rng = np.random.default_rng(d % 1000)
    x = _nonzero(rng, (n,))
    B, pb = 3, 37
    x0, xt = (rng.standard_normal((B, pb)).astype(np.float32) for _ in range(2))
    coef = np.stack([rng.uniform(0.1, 0.9, B), rng.uniform(0.1, 0.9, B), rng.uniform(-6.0, 0.0, B), np.ones(B)], axis=1).astype(np.float32)
    plain = _randn(dev, eff, offset, n)  # before the word is registered: the stream of s + d itself
    eps = _randn(dev, eff, offset, B * pb).reshape(B, pb)
    want_post = _posterior(dev, x0, xt, coef, eps, 0, 0, False)
    word = torch.tensor([d], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert L().set_rng_seed_delta(word.data_ptr()) == 0
    try:
        z = _randn(dev, s, offset, n)
        post = _posterior(dev, x0, xt, coef, None, s, offset, False)
        y = _dropout(dev, x, p, s, offset)
        torch.cuda.synchronize()
    finally:
        assert L().set_rng_seed_delta(None) == 0
    _check_normals(z, eff, offset, "seed %#x + delta %#x" % (s, d))
    assert np.array_equal(bits(z), bits(plain))
    assert not np.array_equal(bits(z), bits(_randn(dev, s, offset, n)))  # unregistered again: the plain seed, another stream
    assert np.array_equal(bits(post), bits(want_post))
    _check_dropout(y, x, PM.dropout_keep(eff, offset, n, p), p, "delta")


def test_report_measured_k():
    """Printed last: the largest k of this run (the module docstring holds the record)."""
    print("measured k over the file = %.3f (allowed %.1f), largest error / bound %.3f, / angle term %.3f" % (SEEN["k"], K_NORMAL, SEEN["frac"], SEEN["angle"]))
    assert SEEN["k"] <= K_NORMAL and SEEN["frac"] <= 1.0
