"""CPU checks of tests/glue_models.py against the repository's oracle functions and goldens, so that the GPU tests of
test_gpu_glue_branches.py need nothing but the models."""
import numpy as np
import torch

import glue_models as GM
from conftest import load_golden
from oracle import oracle as O


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_expand_states_and_masks():
    rng = np.random.default_rng(0)
    B, C, Tt, T = 2, 3, 7, 19
    enc = rng.standard_normal((B, C, Tt)).astype(np.float32)
    m2p = rng.integers(0, Tt + 1, (B, T))
    ref = O.expand_states(_t(enc).transpose(1, 2), _t(m2p)).transpose(1, 2).numpy()
    assert np.array_equal(GM.expand_states(enc, m2p), ref)
    out = GM.expand_states(enc, np.array([[0, 1, Tt, Tt + 1, -1]] * B))
    assert not out[:, :, [0, 3, 4]].any() and np.array_equal(out[:, :, 1], enc[:, :, 0]) and np.array_equal(out[:, :, 2], enc[:, :, Tt - 1])
    assert GM.index_mask(np.array([-1, 0, 1, 5])).tolist() == [0.0, 0.0, 1.0, 1.0]
    x = rng.standard_normal((B, 5, T)).astype(np.float32)
    assert np.array_equal(GM.transpose(x), _t(x).transpose(1, 2).contiguous().numpy())
    x, special = GM.abs_sum_columns(5, 65, 1)
    m = GM.abs_sum_mask(x)
    assert m[1, :8].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0] and m[0].all() and special == list(range(8))
    assert np.array_equal(np.delete(m, 7, 1), np.delete((_t(x).abs().sum(1) > 0).float().numpy(), 7, 1))


def test_embedding():
    rng = np.random.default_rng(1)
    idx, tab = rng.integers(0, 11, (2, 9)), rng.standard_normal((11, 5)).astype(np.float32)
    ref = torch.nn.functional.embedding(_t(idx), _t(tab)).transpose(1, 2)
    assert np.array_equal(GM.embedding_bct(idx, tab, 1.7), (np.float32(1.7) * ref).numpy())
    out = rng.standard_normal((2, 5, 9)).astype(np.float32)
    assert np.array_equal(GM.embedding_bct(idx, tab, 1.7, out), (_t(out) + np.float32(1.7) * ref).numpy())
    assert np.array_equal(GM.embedding_bct(np.array([[-3, 13]]), tab), tab[[0, 10]].T[None])


def test_masked_dur():
    rng = np.random.default_rng(2)
    B, T, Tt = 3, 61, 9
    m2p = np.sort(rng.integers(0, Tt + 1, (B, T)), 1)
    tm = (rng.random((B, T)) > 0.6).astype(np.float32)
    tm[2] = 1.0
    txt = rng.integers(0, 4, (B, Tt))
    ref = (O.mel2token_to_dur(_t(m2p) * (1 - _t(tm)).long(), Tt) * (_t(txt) != 0).float()).long().numpy()
    assert np.array_equal(GM.masked_dur(m2p, tm, txt), ref) and not ref[2].any()
    half = np.full((1, 4), 0.5, dtype=np.float32)  # (1 - 0.5).long() = 0: nothing is kept
    assert not GM.masked_dur(np.array([[1, 1, 2, 2]]), half, np.ones((1, 2), dtype=np.int64)).any()


def test_length_regulate():
    g = load_golden("length_regulator")
    txt = (~g["pad"]).astype(np.int64)
    assert np.array_equal(GM.length_regulate(g["dur"], txt), g["mel2ph"])
    for Tt in (1, 257):
        dur, txt = GM.dur_cases(Tt, Tt)
        ref = O.length_regulator(_t(dur), _t(txt == 0)).numpy()
        got = GM.length_regulate(dur, txt)
        assert np.array_equal(got, ref) and np.array_equal(GM.dur_total(dur, txt), (ref > 0).sum(1))
        assert GM.dur_total(dur, txt)[1] == 0 and not got[1].any()
    d = GM.round_dur(np.array([[0, 0.5, 1.5, 2.5, 3.49, 3.51]], dtype=np.float32), np.ones((1, 6), dtype=np.int64))
    assert d.tolist() == [[0, 0, 2, 2, 3, 4]]


def test_pitch_coarse():
    rng = np.random.default_rng(3)
    n = 300
    f0 = rng.uniform(4.5, 11.0, n).astype(np.float32)
    uv = rng.standard_normal(n).astype(np.float32)
    tm = (rng.random(n) > 0.7).astype(np.float32)
    pad = rng.integers(0, 3, n)
    den, bins = GM.pitch_coarse(f0, uv, tm, pad)
    ref_den = O.denorm_f0(_t(f0) * (1 - _t(tm)), _t(uv) * (1 - _t(tm)), _t(pad == 0))
    assert np.abs(den - ref_den.numpy()).max() < 1e-3
    assert np.array_equal(bins, O.f0_to_coarse(ref_den).numpy())
    den, bins = GM.pitch_coarse(f0, None)
    ref_den = O.denorm_f0(_t(f0), None)
    assert np.abs(den - ref_den.numpy()).max() < 1e-3 and np.array_equal(bins, O.f0_to_coarse(ref_den).numpy())
    den, bins = GM.pitch_coarse(f0, uv, tm, None, uv_from_logit=True)  # the raw logit decides, also under the mask
    assert ((den == 0) == (uv > 0)).all() and (bins[uv > 0] == 1).all()
    fo = np.array([-1e30, -3.0, 0.0, 4.999, 5.0, 10.5, 10.51, 50.0, 1e30], dtype=np.float32)
    assert GM.pitch_coarse(fo)[1].tolist() == [1, 1, 1, 1, 1, 255, 255, 255, 255]


def test_diffusion_elementwise():
    rng = np.random.default_rng(4)
    B, M, T = 3, 5, 37
    tab, _ = O.diffusion_tables(8)
    t = torch.tensor([0, 3, 7])
    x0, xt, eps = (rng.standard_normal((B, 1, M, T)).astype(np.float32) for _ in range(3))
    ab = torch.stack([tab["sqrt_alphas_cumprod"][t], tab["sqrt_one_minus_alphas_cumprod"][t]], -1).numpy()
    got = GM.q_sample(x0[:, 0], eps[:, 0], ab)
    assert np.array_equal(got, O.q_sample(tab, _t(x0), t, _t(eps)).numpy()[:, 0])
    nonpad = (rng.random((B, T)) > 0.3).astype(np.float32)
    assert np.array_equal(GM.q_sample(x0[:, 0], eps[:, 0], ab, nonpad), got * nonpad[:, None, :])
    coef = torch.stack([tab["posterior_mean_coef1"][t], tab["posterior_mean_coef2"][t], tab["posterior_log_variance_clipped"][t],
                        (t != 0).float()], -1).numpy()
    ref = O.q_posterior_sample(tab, _t(x0), _t(xt), t, _t(eps)).numpy()
    assert np.abs(GM.posterior64(x0, xt, coef, eps) - ref).max() < 1e-6
    a, b, c = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    assert np.array_equal(GM.sum_scale(a, b, c, 3.0), (((_t(a) + _t(b)) + _t(c)) / 3.0).numpy())
    assert np.array_equal(GM.sum_scale(a, None, c, 3.0), ((_t(a) + _t(c)) / 3.0).numpy())
    m = (rng.random(125) > 0.5).astype(np.float32)
    ref = _t(a).view(125, 8) * (1 - _t(m)[:, None]) + _t(b).view(125, 8) * _t(m)[:, None]
    assert np.array_equal(GM.blend_mask(a, b, m, 8), ref.view(-1).numpy())
    assert np.array_equal(GM.mul_one_minus_mask(a, m, 8), (_t(a).view(125, 8) * (1 - _t(m)[:, None])).view(-1).numpy())


def test_sinusoid_embed():
    """Against the reference's formula in fp32 torch (diffnet.py: exp(arange(half) * -(ln 1e4 / (half - 1))), t[:, None] * emb, cat(sin, cos))."""
    import math
    t = np.array([0, 1, 99, 999, 500.5], dtype=np.float32)
    for dim in (4, 6, 256):
        half = dim // 2
        emb = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
        emb = _t(t)[:, None] * emb[None, :]
        ref = torch.cat((emb.sin(), emb.cos()), dim=-1).T.numpy()
        got, ang = GM.sinusoid_embed(t, dim)
        assert got.shape == (dim, len(t)) and np.abs(got - ref).max() < 2e-4 * max(1.0, ang.max() / 999)  # fp32 angles up to 999: ulp 6e-5
        assert (got[:half, 0] == 0).all() and (got[half:, 0] == 1).all()
