"""GPU edge sweep of the small kernels of csrc/glue.hip and csrc/diffusion_ops.hip against the models of glue_models.py (which
test_glue_reference.py ties to the oracle and the goldens), through the C ABI: partial tiles, sizes off the block multiple, more than one
block, optional operands absent, clamps and out-of-range indices.  Every output is a view inside a sentinel-filled buffer and nothing
around it may change.  The library is built with -ffp-contract=off, so elementwise results equal the same fp32 operations done in the same
order on the CPU bit for bit; the two ops with a transcendental (pitch_coarse's exp2f, sinusoid_embed) get a bound against float64.

K_SINUSOID: the installed ROCm states no ulp errors for the device expf / sinf / cosf, so one k for both terms of the bound
|t| f k 2^-24 + k 2^-24 was measured on the MI355X against the float64 model over the cases of test_sinusoid_embed: 1.48 (printed as
"measured k"); twice that, 2.96, is allowed."""
import itertools

import numpy as np
import pytest
import torch

import glue_models as GM
from raw_abi import L, Sent, bits, check, stream, to_dev

pytestmark = pytest.mark.gpu

K_SINUSOID_MEASURED = 1.48
K_SINUSOID = 2.0 * K_SINUSOID_MEASURED
I64 = torch.int64


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same(got, want, what=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


# ---- transposes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,S", [(1, 1, 1), (1, 1, 97), (1, 97, 1), (2, 31, 33), (2, 32, 32), (1, 33, 31), (3, 65, 80)])
@pytest.mark.parametrize("entry", ["set_transpose_btc_to_bct", "set_transpose_bct_to_btc"])
def test_transpose_partial_tiles(dev, entry, B, R, S):
    x = np.random.default_rng(R * 100 + S).standard_normal((B, R, S)).astype(np.float32)
    xd, out = to_dev(x, dev), Sent((B, S, R), dev)
    check(getattr(L(), entry)(xd.data_ptr(), out.ptr, B, R, S, stream()), entry)
    _same(out.get(), GM.transpose(x))


# ---- abs_sum_mask ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T", [(1, 1), (2, 63), (3, 64), (4, 65), (5, 130), (7, 65), (80, 130), (1, 65), (3, 130)])
def test_abs_sum_mask_small_channel_counts_and_special_columns(dev, C, T):
    """C < 4 leaves some of the four channel groups empty (c0 >= C).  A column whose only nonzero is a denormal counts as nonzero, as in
    the float64 model (and in the reference, whose sum of absolute values does not flush)."""
    x, special = GM.abs_sum_columns(C, T, 10 * C + T)
    xd, out = to_dev(x, dev), Sent((2, T), dev)
    check(L().set_abs_sum_mask(xd.data_ptr(), out.ptr, 2, C, T, stream()), "set_abs_sum_mask")
    got, want = out.get(), GM.abs_sum_mask(x)
    if 7 in special:
        assert want[1, 7] == 1.0 and got[1, 7] == 1.0, "a denormal column"
    assert want[1, 0] == 0.0 and (T < 8 or want[1, 1:8].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0])
    _same(got, want, (C, T))


# ---- embedding ------------------------------------------------------------------------------------------------------------------------------
def _embedding(dev, idx, tab, scale, acc_into=None, dev_scale=False):
    B, T = idx.shape
    n_rows, C = tab.shape
    ops = [to_dev(idx, dev), to_dev(tab, dev), to_dev(np.array([scale], dtype=np.float32), dev)]
    out = Sent((B, C, T), dev)
    if acc_into is not None:
        out.fill(acc_into)
    if dev_scale:
        rc = L().set_embedding_bct_dev_scale(ops[0].data_ptr(), ops[1].data_ptr(), out.ptr, B, T, C, n_rows, ops[2].data_ptr(),
                                             int(acc_into is not None), stream())
    else:
        rc = L().set_embedding_bct(ops[0].data_ptr(), ops[1].data_ptr(), out.ptr, B, T, C, n_rows, float(np.float32(scale)),
                                   int(acc_into is not None), stream())
    check(rc, "set_embedding_bct")
    return out.get()


@pytest.mark.parametrize("B,T,C", [(2, 37, 5), (3, 97, 1)])  # 370 and 291 elements: two blocks, neither a multiple of 256
def test_embedding_scale_entries_accumulate_padding_and_clamp(dev, B, T, C):
    rng = np.random.default_rng(B * T)
    n_rows, scale = 11, 1.7
    tab = rng.standard_normal((n_rows, C)).astype(np.float32)
    tab[0] = 0.0  # padding_idx = 0: nn.Embedding keeps that row zero
    idx = rng.integers(0, n_rows, (B, T))
    idx[:, 3] = 0
    base = rng.standard_normal((B, C, T)).astype(np.float32)
    for dev_scale in (False, True):  # the device-scale entry gives the float entry's bits
        _same(_embedding(dev, idx, tab, scale, None, dev_scale), GM.embedding_bct(idx, tab, scale), dev_scale)
        acc = _embedding(dev, idx, tab, scale, base, dev_scale)
        _same(acc, GM.embedding_bct(idx, tab, scale, base), ("accumulate", dev_scale))  # two roundings: fl(out + fl(sc tab))
        _same(acc[:, :, 3], base[:, :, 3])                                             # the padding row adds nothing
    assert not _embedding(dev, idx, tab, scale)[:, :, 3].any()
    # the clamp (memory safety only; the Python wrapper's range check is tested in test_abi_and_host.py): -3 reads row 0, n_rows + 2 the last
    tab2 = rng.standard_normal((n_rows, C)).astype(np.float32)
    bad = idx.copy()
    bad[:, 1], bad[:, 2] = -3, n_rows + 2
    got = _embedding(dev, bad, tab2, scale)
    _same(got, GM.embedding_bct(bad, tab2, scale))
    _same(got[:, :, 1], np.broadcast_to(np.float32(scale) * tab2[0], (B, C)).copy())
    _same(got[:, :, 2], np.broadcast_to(np.float32(scale) * tab2[n_rows - 1], (B, C)).copy())


# ---- index_mask, expand_states --------------------------------------------------------------------------------------------------------------
def _mel2ph(rng, B, T, Tt):
    m = rng.integers(0, Tt + 1, (B, T))
    m[:, :5] = [0, 1, Tt, Tt + 1, -1][:min(T, 5)]
    return m


def test_index_mask_off_the_block_multiple(dev):
    idx = _mel2ph(np.random.default_rng(0), 2, 150, 7)  # 300 elements
    out = Sent((2, 150), dev)
    d = to_dev(idx, dev)
    check(L().set_index_mask(d.data_ptr(), out.ptr, idx.size, stream()), "set_index_mask")
    _same(out.get(), GM.index_mask(idx))


@pytest.mark.parametrize("C", [1, 3])
def test_expand_states_out_of_range_indices_give_zero(dev, C):
    rng = np.random.default_rng(C)
    B, Tt, T = 2, 7, 131  # 262 / 786 elements
    enc = rng.standard_normal((B, C, Tt)).astype(np.float32)
    m2p = _mel2ph(rng, B, T, Tt)
    ops, out = [to_dev(enc, dev), to_dev(m2p, dev)], Sent((B, C, T), dev)
    check(L().set_expand_states(ops[0].data_ptr(), ops[1].data_ptr(), out.ptr, B, C, Tt, T, stream()), "set_expand_states")
    got = out.get()
    _same(got, GM.expand_states(enc, m2p))
    assert not bits(got[:, :, [0, 3, 4]]).any()  # mel2ph 0, T_txt + 1 and -1: +0.0
    _same(got[:, :, 1], enc[:, :, 0])
    _same(got[:, :, 2], enc[:, :, Tt - 1])


# ---- masked_dur -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tt,T", [(1, 1), (255, 255), (256, 257), (257, 700), (1000, 257), (1000, 700)])
def test_masked_dur_beyond_one_block_of_tokens(dev, Tt, T):
    rng = np.random.default_rng(Tt + T)
    B = 4
    m2p = np.sort(rng.integers(0, Tt + 1, (B, T)), 1)
    tm = rng.choice([0.0, 0.0, 1.0, 0.5], (B, T)).astype(np.float32)  # 0.5 truncates to keep = 0, as the reference's .long() does
    tm[1], tm[2] = 1.0, 0.5                                           # a fully masked utterance, and one of halves
    tm[3] = 0.0
    txt = rng.integers(0, 4, (B, Tt))                                 # padding tokens inside the text
    ops, out = [to_dev(m2p, dev), to_dev(tm, dev), to_dev(txt, dev)], Sent((B, Tt), dev, I64)
    check(L().set_masked_dur(ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), out.ptr, B, T, Tt, stream()), "set_masked_dur")
    got, want = out.get(), GM.masked_dur(m2p, tm, txt)
    _same(got, want)
    assert not got[1].any() and not got[2].any()
    assert np.array_equal(got[3], np.bincount(m2p[3], minlength=Tt + 1)[1:] * (txt[3] != 0))


# ---- dur_total, length_regulate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tt", [1, 257, 1000])
def test_length_regulate_rounding_zero_totals_and_long_texts(dev, Tt):
    from set_amd import ops
    dur, txt = GM.dur_cases(Tt, Tt)
    if Tt == 1:
        dur[2, 0], txt[2, 0] = 2.5, 3  # some utterance has frames
    B = 3
    d, t = to_dev(dur, dev), to_dev(txt, dev)
    total = Sent((B,), dev, I64)
    check(L().set_dur_total(d.data_ptr(), t.data_ptr(), total.ptr, B, Tt, stream()), "set_dur_total")
    want = GM.length_regulate(dur, txt)
    tot = total.get()
    assert np.array_equal(tot, GM.dur_total(dur, txt)) and tot[1] == 0 and tot.max() > 0
    T_out = int(tot.max())
    out = Sent((B, T_out), dev, I64)
    check(L().set_length_regulate(d.data_ptr(), t.data_ptr(), out.ptr, B, Tt, T_out, stream()), "set_length_regulate")
    got = out.get()
    _same(got, want)
    assert not got[1].any()  # total 0 beside totals > 0: a row of zeros
    for b in range(B):
        assert np.array_equal(got[b, :tot[b]], np.repeat(np.arange(1, Tt + 1), GM.round_dur(dur, txt)[b]))
    _same(ops.length_regulate(d, t).cpu().numpy(), want)
    # all totals 0: [B, 0], and no launch
    none = ops.length_regulate(to_dev(np.where(txt == 0, dur, np.float32(0.5)).astype(np.float32), dev), t)
    assert tuple(none.shape) == (B, 0) and none.dtype == I64


def test_length_regulate_half_to_even(dev):
    from set_amd import ops
    dur = np.array([[0, 0.5, 1.5, 2.5, 3.49, 3.51, 0.5, 0]], dtype=np.float32)
    got = ops.length_regulate(to_dev(dur, dev), to_dev(np.ones((1, 8), dtype=np.int64), dev)).cpu().numpy()
    assert got.tolist() == [[3, 3, 4, 4, 5, 5, 5, 6, 6, 6, 6]]  # 0, 0, 2, 2, 3, 4, 0, 0 frames


# ---- pitch_coarse ---------------------------------------------------------------------------------------------------------------------------
FLAGS = list(itertools.product([False, True], [False, True], [False, True], [False, True], ["denorm", "coarse", "both"]))


def test_pitch_coarse_flag_matrix(dev):
    rng = np.random.default_rng(6)
    n = 300
    f0 = rng.uniform(4.5, 11.0, n).astype(np.float32)
    f0[:9] = [-1e30, -3.0, 0.0, 4.999, 5.0, 10.5, 10.51, 50.0, 1e30]
    uv = rng.standard_normal(n).astype(np.float32)
    tm = (rng.random(n) > 0.7).astype(np.float32)
    pad = rng.integers(0, 3, n)
    d = {k: to_dev(v, dev) for k, v in dict(f0=f0, uv=uv, tm=tm, pad=pad).items()}
    worst = 0.0
    for has_uv, logit, has_tm, has_pad, want in FLAGS:
        den = Sent((n,), dev) if want != "coarse" else None
        co = Sent((n,), dev, I64) if want != "denorm" else None
        check(L().set_pitch_coarse(d["f0"].data_ptr(), d["uv"].data_ptr() if has_uv else None, d["tm"].data_ptr() if has_tm else None,
                                   d["pad"].data_ptr() if has_pad else None, int(logit), den.ptr if den else None, co.ptr if co else None,
                                   n, stream()), "set_pitch_coarse")
        ref_den, ref_bins = GM.pitch_coarse(f0, uv if has_uv else None, tm if has_tm else None, pad if has_pad else None, logit)
        what = (has_uv, logit, has_tm, has_pad, want)
        if co:
            _same(co.get(), ref_bins, what)
        if den:
            got = den.get()
            assert np.array_equal(got == 0, ref_den == 0), what
            worst = max(worst, float(np.abs(got - ref_den).max()))
            assert np.abs(got - ref_den).max() < 1e-3, what  # Hz: exp2f against float64 at up to 900 (ulp 6e-5)
    print("pitch_coarse: largest denormalised f0 error %.3e Hz" % worst)


# ---- q_sample -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,T", [(1, 1), (80, 37), (1, 37), (80, 1)])
@pytest.mark.parametrize("masked", [False, True])
def test_q_sample_shapes_and_nonpad(dev, M, T, masked):
    rng = np.random.default_rng(M + T)
    B = 3
    x, eps = (rng.standard_normal((B, M, T)).astype(np.float32) for _ in range(2))
    ab = rng.uniform(0.1, 1.0, (B, 2)).astype(np.float32)
    nonpad = rng.choice([0.0, 1.0], (B, T)).astype(np.float32) if masked else None
    ops = [to_dev(a, dev) for a in (x, eps, ab)] + [to_dev(nonpad, dev) if masked else None]
    out = Sent((B, M, T), dev)
    check(L().set_q_sample(ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr() if masked else None, out.ptr,
                           B, M, T, stream()), "set_q_sample")
    _same(out.get(), GM.q_sample(x, eps, ab, nonpad))


# ---- sum_scale, blend_mask, mul_one_minus_mask ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_sum_scale_with_operands_absent(dev, n):
    rng = np.random.default_rng(n)
    a, b, c = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    dv = [to_dev(v, dev) for v in (a, b, c)]
    for hb, hc in itertools.product([True, False], repeat=2):
        out = Sent((n,), dev)
        check(L().set_sum_scale(dv[0].data_ptr(), dv[1].data_ptr() if hb else None, dv[2].data_ptr() if hc else None, out.ptr, 3.0, n,
                                stream()), "set_sum_scale")
        _same(out.get(), GM.sum_scale(a, b if hb else None, c if hc else None, 3.0), (n, hb, hc))


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_blend_and_mul_one_minus_mask_inner_sizes(dev, n):
    rng = np.random.default_rng(n + 1)
    a, b = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    da, db = to_dev(a, dev), to_dev(b, dev)
    for inner in sorted({1, 80, n}):
        m = rng.choice([0.0, 1.0, 0.25], -(-n // inner)).astype(np.float32)
        dm = to_dev(m, dev)
        out = Sent((n,), dev)
        check(L().set_blend_mask(da.data_ptr(), db.data_ptr(), dm.data_ptr(), out.ptr, n, inner, stream()), "set_blend_mask")
        _same(out.get(), GM.blend_mask(a, b, m, inner), (n, inner))
        out = Sent((n,), dev)
        check(L().set_mul_one_minus_mask(da.data_ptr(), dm.data_ptr(), out.ptr, n, inner, stream()), "set_mul_one_minus_mask")
        _same(out.get(), GM.mul_one_minus_mask(a, m, inner), (n, inner))


# ---- sinusoid_embed -------------------------------------------------------------------------------------------------------------------------
def test_sinusoid_embed(dev):
    """|got - float64| <= |t| f k 2^-24 + k 2^-24: the error of expf and the rounding of the angle t f, carried through the angle (the slope
    of sin / cos is at most 1), plus the error of sinf / cosf itself."""
    worst = 0.0
    for dim, n in itertools.product([4, 6, 256], [1, 100, 257]):
        t = np.resize(np.array([999, 0, 1, 99, 500.5, 37], dtype=np.float32), n)
        td, out = to_dev(t, dev), Sent((dim, n), dev)
        check(L().set_sinusoid_embed(td.data_ptr(), out.ptr, dim, n, stream()), "set_sinusoid_embed")
        want, ang = GM.sinusoid_embed(t, dim)
        got = out.get()
        unit = 2.0 ** -24 * (ang + 1.0)
        k = float((np.abs(got - want) / unit).max())
        worst = max(worst, k)
        assert (np.abs(got - want) <= K_SINUSOID * unit).all(), (dim, n, k)
        zero = t == 0
        assert not bits(got[:dim // 2, zero]).any() and (got[dim // 2:, zero] == 1.0).all()  # t = 0: sin +0.0, cos 1
    print("sinusoid_embed: measured k = %.3f (allowed %.1f)" % (worst, K_SINUSOID))
