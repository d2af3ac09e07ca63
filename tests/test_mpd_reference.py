"""CPU checks of the multi-period discriminator's test model (tests/mpd_models.py) and of the host side of its entry points.

The float64 model is held live to torch's own F.pad(reflect) + Conv2d + leaky_relu + autograd in float64 -- scores, maps, losses and
d/d y_hat -- and to the reference's own MultiPeriodDiscriminator and loss functions: through the recording tests/golden/mpd_reference.npz
(tools/make_mpd_golden.py), and live through oracle/ref_import.py where the reference checkout is present.  Further: the layout maps, the
H_out rule, the mirror rule of the fold, the exactness budget of the integer cases, the bars and the share of undecided entries, the
documented order of the list losses, and the refusals of the entry points (no GPU needed: they come before any device call)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mpd_models as MM
from conftest import load_golden

GOLD_SEED_W, GOLD_SEED_Y, GOLD_B, GOLD_T = 11, 12, 2, 200       # tools/make_mpd_golden.py


@pytest.fixture(autouse=True)
def _grad_mode():
    """Autograd on, whatever grad mode an earlier test module left behind."""
    with torch.enable_grad():
        yield


# ---- torch float64 restatement ----------------------------------------------------------------------------------------------------------
def torch_mpd(state, y, y_hat, u_adv, u_fm, slope):
    """The reference's forward and the two generator-side losses from torch's own ops in float64; returns what MM.mpd_forward / mpd_grad
    return."""
    y = torch.from_numpy(y).double().unsqueeze(1)
    yh = torch.from_numpy(y_hat).double().unsqueeze(1).requires_grad_()
    out = dict(scores_r=[], scores_g=[], maps_r=[], maps_g=[])
    gl = fl = 0.0
    for i, p in enumerate(MM.PERIODS):
        res = []
        for x in (y, yh):
            b, c, t = x.shape
            if t % p:
                x = F.pad(x, (0, p - t % p), "reflect")
            x = x.view(b, c, -1, p)
            fmap = []
            for j in range(6):
                pre = "discriminators.%d.%s." % (i, "convs.%d" % j if j < 5 else "conv_post")
                v, g, bias = (state[pre + k].double() for k in ("weight_v", "weight_g", "bias"))
                w = torch._weight_norm(v, g, 0)
                x = F.conv2d(x, w, bias, stride=(3 if j < 4 else 1, 1), padding=(2 if j < 5 else 1, 0))
                if j < 5:
                    x = F.leaky_relu(x, slope)
                fmap.append(x)
            res.append((torch.flatten(x, 1, -1), fmap))
        (sr, fr), (sg, fg) = res
        out["scores_r"].append(sr)
        out["scores_g"].append(sg)
        out["maps_r"].append(fr)
        out["maps_g"].append(fg)
        gl = gl + torch.mean((1 - sg) ** 2)
        for r, g in zip(fr, fg):
            fl = fl + torch.mean(torch.abs(r - g))
    gl, fl = gl / len(MM.PERIODS), fl * 2
    (grad,) = torch.autograd.grad(u_adv * gl + u_fm * fl, yh)
    out.update(gen_loss=gl, fm_loss=fl, grad=grad[:, 0])
    return out


@pytest.mark.parametrize("channels,T", [(MM.NARROW, 23), (MM.NARROW, 97), (MM.FULL, 97)])
def test_model_matches_torch_float64(channels, T):
    state = MM.seeded_state(3, channels)
    y, y_hat = MM.waves(4, 2, T)
    B = 2
    fw = MM.mpd_forward(y, y_hat, MM.state_numpy(state), slope=0.1)
    ref = torch_mpd(state, y, y_hat, 0.7, 2.5, 0.1)
    n = lambda t: t.detach().numpy()  # noqa: E731
    for i, p in enumerate(MM.PERIODS):
        Rg = B * p
        np.testing.assert_allclose(fw["scores_g"][i], n(ref["scores_g"][i]), rtol=0, atol=1e-12)
        np.testing.assert_allclose(fw["scores_r"][i], n(ref["scores_r"][i]), rtol=0, atol=1e-12)
        for j in range(6):
            got_r, got_g = MM.rows_to_map(fw["maps"][i][j][:Rg], B, p), MM.rows_to_map(fw["maps"][i][j][Rg:], B, p)
            assert got_g.shape == tuple(ref["maps_g"][i][j].shape)
            np.testing.assert_allclose(got_r, n(ref["maps_r"][i][j]), rtol=0, atol=1e-12)
            np.testing.assert_allclose(got_g, n(ref["maps_g"][i][j]), rtol=0, atol=1e-12)
    assert abs(float(fw["gen_loss"]) - float(ref["gen_loss"])) < 1e-13 and abs(float(fw["fm_loss"]) - float(ref["fm_loss"])) < 1e-12
    grad = MM.mpd_grad(fw, 0.7, 2.5)
    np.testing.assert_allclose(grad, n(ref["grad"]), rtol=0, atol=1e-12 * max(1.0, float(np.abs(grad).max())))
    assert float(np.abs(grad).max()) > 1e-4


def _check_recording(rec, fw, B):
    for i, p in enumerate(MM.PERIODS):
        Rg = B * p
        np.testing.assert_allclose(fw["scores_r"][i], rec["score_r_%d" % i], rtol=0, atol=1e-12)
        np.testing.assert_allclose(fw["scores_g"][i], rec["score_g_%d" % i], rtol=0, atol=1e-12)
        for j in range(6):
            for tag, rows in (("r", fw["maps"][i][j][:Rg]), ("g", fw["maps"][i][j][Rg:])):
                m = MM.rows_to_map(rows, B, p)
                assert list(m.shape) == list(rec["map_shapes_%d" % i][j])
                np.testing.assert_allclose([m.mean(), np.abs(m).mean()], rec["map_stats_%s_%d" % (tag, i)][j], rtol=0, atol=1e-12)
    for k, name in (("gen_loss", "generator_loss"), ("fm_loss", "feature_loss"), ("disc_r_loss", "disc_r_loss"), ("disc_g_loss", "disc_g_loss")):
        assert abs(float(fw[k]) - float(rec[name])) < 1e-12, name


def test_model_matches_the_reference():
    """The recording of the reference's own module and loss functions (B = 2, T = 200, float64) -- and, where the checkout is present,
    the same comparison live (oracle/ref_import.py unchanged; weights from the same torch seed on both sides)."""
    y, y_hat = MM.waves(GOLD_SEED_Y, GOLD_B, GOLD_T)
    fw = MM.mpd_forward(y, y_hat, MM.state_numpy(MM.seeded_state(GOLD_SEED_W)), slope=0.1)
    _check_recording(load_golden("mpd_reference"), fw, GOLD_B)
    from oracle import ref_import
    if ref_import.available():
        import importlib
        import importlib.util
        import os
        ref_import.install()
        spec = importlib.util.spec_from_file_location("make_mpd_golden", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "make_mpd_golden.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        assert (tool.SEED_W, tool.SEED_Y, tool.B, tool.T) == (GOLD_SEED_W, GOLD_SEED_Y, GOLD_B, GOLD_T)
        _check_recording(tool.record(importlib.import_module("modules.vocoder.hifigan.hifigan")), fw, GOLD_B)


# ---- layout, lengths, the fold ----------------------------------------------------------------------------------------------------------
def test_rows_and_maps_are_one_buffer():
    B, p, Cc, H = 2, 3, 4, 5
    rows = torch.arange(B * p * Cc * H, dtype=torch.float32).view(B * p, Cc, H)
    m = rows.view(B, p, Cc, H).permute(0, 2, 3, 1)
    assert tuple(m.shape) == (B, Cc, H, p) and m.data_ptr() == rows.data_ptr()
    assert np.array_equal(m.numpy(), MM.rows_to_map(rows.numpy(), B, p))
    assert np.array_equal(MM.map_to_rows(m.numpy()), rows.numpy())
    back = m.permute(0, 3, 1, 2)
    assert back.is_contiguous() and back.data_ptr() == rows.data_ptr()
    # the score: flatten(1, -1) of [B, 1, H, p] runs over (h, w)
    x = torch.arange(B * p * H, dtype=torch.float32).view(B * p, 1, H)
    s = x.view(B, p, 1, H).permute(0, 2, 3, 1).flatten(1, -1)
    assert float(s[1, 2 * p + 1]) == float(x[1 * p + 1, 0, 2])


def test_out_len_rule_down_to_one_frame(built_lib):
    for K, s, pad in ((5, 3, 2), (5, 1, 2), (3, 1, 1), (1, 4, 0), (7, 2, 6), (5, 4, 0)):
        for H in range(1, 40):
            if H + 2 * pad < K:
                continue
            want = F.conv1d(torch.zeros(1, 1, H), torch.zeros(1, 1, K), stride=s, padding=pad).shape[2]
            assert MM.out_len(H, K, s, pad) == want == built_lib.set_sconv1d_out_len(H, K, s, pad), (H, K, s, pad)
    H, seen = 4096, []
    for _ in range(12):
        H = MM.out_len(H, 5, 3, 2)
        seen.append(H)
    assert seen[-1] == 1 and MM.out_len(1, 5, 3, 2) == 1 and MM.out_len(1, 5, 1, 2) == 1 and MM.out_len(1, 3, 1, 1) == 1


@pytest.mark.parametrize("p", MM.PERIODS)
def test_fold_mirror_rule(p):
    rng = np.random.default_rng(p)
    for T in (p + 1, 5 * p, 5 * p + 1, 6 * p - 1, 97):
        assert T % p in (0, 1, p - 1) or T == 97
        y = rng.standard_normal((2, T))
        t = torch.from_numpy(y).unsqueeze(1).requires_grad_()
        x = F.pad(t, (0, (-T) % p), "reflect") if T % p else t
        ref = x.view(2, 1, -1, p)
        rows = MM.fold(y, p)
        assert np.array_equal(MM.rows_to_map(rows, 2, p), ref.detach().numpy())
        idx = MM.fold_index(T, p)
        assert (idx[:T] == np.arange(T)).all() and (idx[T:] < T - 1).all() and len(set(idx[T:])) == len(idx[T:])
        # the gradient: torch's autograd through pad + view against fold_bwd with a one-tap identity layer
        g = rng.standard_normal(ref.shape)
        (want,) = torch.autograd.grad(ref, t, torch.from_numpy(g))
        got = MM.fold_bwd(MM.map_to_rows(g), np.ones((1, 1)), 2, T, p, 1, 0)
        np.testing.assert_allclose(got, want[:, 0].numpy(), rtol=0, atol=1e-15)


def test_layer_model_against_torch_conv1d():
    rng = np.random.default_rng(0)
    for (s, K, pad, cin, cout, H, R) in MM.sconv_cases()[::3]:
        x, W, b = rng.standard_normal((R, cin, H)), rng.standard_normal((cout, cin, K)), rng.standard_normal(cout)
        xt = torch.from_numpy(x).requires_grad_()
        z = F.conv1d(xt, torch.from_numpy(W), torch.from_numpy(b), stride=s, padding=pad)
        out = F.leaky_relu(z, 0.3)
        got = MM.conv_rows(x, W, b, s, pad, 0.3)
        np.testing.assert_allclose(got, out.detach().numpy(), rtol=0, atol=1e-11)
        dz = rng.standard_normal(z.shape)
        (want,) = torch.autograd.grad(z, xt, torch.from_numpy(dz))
        f_in, add = rng.standard_normal(x.shape), rng.standard_normal(x.shape)
        gate = MM.gate_of(f_in, 0.3)
        got = MM.dgrad_rows(dz, W, H, s, pad, gate, add)
        np.testing.assert_allclose(got, (want.numpy() + add) * gate, rtol=0, atol=1e-11)
        # gate(0) = slope, as torch's leaky_relu backward
        zt = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        (g0,) = torch.autograd.grad(F.leaky_relu(zt, 0.3).sum(), zt)
        assert (g0.numpy() == MM.gate_of(np.zeros(3), 0.3)).all()


def test_integer_cases_are_exact_and_cover_the_tiles():
    cases = MM.sconv_cases()
    assert {c[0] for c in cases} == {1, 2, 3, 4} and {c[1] for c in cases} == {1, 3, 5} and {c[6] for c in cases} == {1, 3}
    assert {(c[3], c[4]) for c in cases} == set(MM.CHANNEL_PAIRS)
    for s in (1, 2, 3, 4):
        assert {(c[3], c[4]) for c in cases if c[0] == s} == set(MM.CHANNEL_PAIRS)
        for K in (1, 3, 5):
            Hs = {c[5] for c in cases if c[0] == s and c[1] == K}
            pad = (K - 1) // 2
            assert {1, 2, 3, 4, 5} <= Hs
            assert {w + d for w in MM.DGRAD_TILES[s] for d in (-1, 0, 1)} <= Hs
            assert {w + d for w in MM.FWD_TILES for d in (-1, 0, 1)} <= {MM.out_len(h, K, s, pad) for h in Hs}
    # every product and every sum of an integer case is an integer or a multiple of the slope 0.5 below 2^24: exact in fp32
    assert max(MM.exact_budget(c[3], c[4], c[1]) for c in cases) < 2 ** 24 and MM.INT_SLOPE == 0.5
    rng = np.random.default_rng(1)
    for (s, K, pad, cin, cout, H, R) in cases[::5]:
        x, W, b = MM.int_array(rng, (R, cin, H), MM.INT_X), MM.int_array(rng, (cout, cin, K), MM.INT_W), MM.int_array(rng, (cout,), MM.INT_X)
        want = MM.conv_rows(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), s, pad, MM.INT_SLOPE)
        got = MM.conv_rows(x, W, b, s, pad, MM.INT_SLOPE, chain=True)            # the float32 mirror, one product at a time
        assert got.dtype == np.float32 and (got == want).all() and (want * 2 == np.round(want * 2)).all()
        dz, f_in = MM.int_array(rng, want.shape, MM.INT_X), MM.int_array(rng, x.shape, MM.INT_X)
        want = MM.dgrad_rows(dz.astype(np.float64), W.astype(np.float64), H, s, pad, MM.gate_of(f_in.astype(np.float64), MM.INT_SLOPE), x.astype(np.float64))
        got = MM.dgrad_rows(dz, W, H, s, pad, MM.gate_of(f_in, MM.INT_SLOPE), x, chain=True)
        assert got.dtype == np.float32 and (got == want).all()


# ---- bars and undecided entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MM.E2E))
def test_bars_and_undecided_share(case):
    """The recorded bars are the float32 mirror's errors (He-scaled Gaussian weights, y ~ 0.3 N, y_hat = y + 0.05 N; full width at
    T = 97, 200, 1024 and the narrow net, every period), and the model alone leaves at most UNDECIDED_CAP of the gate and sign entries
    of any period undecided.  The mirror is slow at full width (about half a minute for T = 1024)."""
    rec, now = MM.load_bars(case), MM.mirror_errors(case)
    assert set(rec) == set(now) == {"maps", "sign_ops", "losses", "grads", "undecided"}
    for k in ("maps", "sign_ops", "losses", "grads"):
        assert rec[k].shape == now[k].shape and (now[k] > 0).all()
        np.testing.assert_allclose(rec[k], now[k], rtol=0.05)       # the float64 side runs on the host's BLAS: last bits may move
    assert (now["undecided"] <= MM.UNDECIDED_CAP).all() and (rec["undecided"] <= MM.UNDECIDED_CAP).all(), now["undecided"]
    fw = MM.e2e_model(case)
    scale = max(float(np.abs(m).max()) for maps in fw["maps"] for m in maps)
    assert now["maps"].max() < 1e-5 * max(scale, 1.0)               # fp32 errors, not a broken mirror
    assert now["grads"].max() < 1e-4 * float(np.abs(MM.mpd_grad(fw, *MM.U_PAIRS[1])).max())


# ---- the list losses --------------------------------------------------------------------------------------------------------------------
def test_list_loss_order_model():
    rng = np.random.default_rng(2)
    for n in (1, 255, 2048, 2049, 5000, 300 * 2048 + 7):
        t = np.abs(rng.standard_normal(n))
        got = MM.loss_item_sum(t)
        assert abs(got - math.fsum(t)) <= 1e-12 * max(1.0, math.fsum(t))
    a, b = rng.standard_normal((3, 5)).astype(np.float32), rng.standard_normal((3, 5)).astype(np.float32)
    b[0] = a[0]
    want = 2 * np.abs(a.astype(np.float64) - b).mean()
    assert abs(float(MM.multi_loss([(a, b, MM.L1, 0)], 2.0, 1)[0]) - want) <= 1e-7 * want
    one = np.asarray([[0.25]], np.float32)
    assert MM.multi_loss([(one, None, MM.SQ1, 0), (one, None, MM.SQ0, 1)], 1.0, 2).tolist() == [0.5625, 0.0625]
    g = MM.multi_loss_grad(a, b, MM.L1, 1.5, 2.0)
    assert (g[0] == 0).all() and set(np.unique(np.abs(g[1:]))) == {np.float32(1.5 * 2.0 / 15)}
    ta = torch.from_numpy(a).requires_grad_()
    (tg,) = torch.autograd.grad(1.5 * 2 * (torch.from_numpy(b) - ta).abs().mean(), ta)
    np.testing.assert_allclose(g, tg.numpy(), rtol=1e-6, atol=0)
    for mode, fn in ((MM.SQ1, lambda t: ((1 - t) ** 2).mean()), (MM.SQ0, lambda t: (t ** 2).mean())):
        ta = torch.from_numpy(a).requires_grad_()
        (tg,) = torch.autograd.grad(0.5 * fn(ta), ta)
        np.testing.assert_allclose(MM.multi_loss_grad(a, None, mode, 1.0, 0.5), tg.numpy(), rtol=1e-6, atol=1e-9)


def test_loss_item_dims_merge_in_memory_order():
    from set_amd import ops
    B, p, Cc, H = 2, 3, 4, 5
    buf = torch.zeros(2 * B * p, Cc, H)
    r, g = (t.view(B, p, Cc, H).permute(0, 2, 3, 1) for t in (buf[:B * p], buf[B * p:]))
    assert ops._loss_dims(g, r) == ([1, 1, 1, B * p * Cc * H], [0, 0, 0, 1], [0, 0, 0, 1])     # a map against a map: one run
    e, sa, sb = ops._loss_dims(g, r.contiguous())
    assert e == [1, B, p, Cc * H] and sa == [0, p * Cc * H, Cc * H, 1] and sb == [0, Cc * H * p, 1, p]
    assert ops._loss_dims(torch.zeros(1, 1), None) == ([1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0])
    with pytest.raises(ValueError, match="overlap"):
        ops._loss_dims(torch.zeros(3, 1).expand(3, 4), None)
    with pytest.raises(ValueError, match="four"):
        ops._loss_dims(torch.zeros(3, 3, 3, 3, 3)[::2, ::2, ::2, ::2, ::2], None)                # five dims, none mergeable
    assert ops.MULTI_LOSS_WORDS == MM.LOSS_WORDS and ops.MULTI_LOSS_CHUNK == MM.LOSS_CHUNK and ops.LOSS_MODES == dict(l1=MM.L1, sq1=MM.SQ1, sq0=MM.SQ0)


# ---- the entry points refuse before any device call -------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(built_lib):
    from set_amd import _lib
    L = built_lib
    buf = (C.c_float * 64)()
    q = C.cast(buf, C.c_void_p)
    one = C.c_float(0.1)
    INV, UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
    ok = dict(R=1, Cin=4, Cout=4, H=8, K=5, s=3, pad=2)

    def fwd(x=q, w=q, out=q, act=1, **kw):
        a = dict(ok, **kw)
        return L.set_sconv1d_fwd(x, w, q, out, a["R"], a["Cin"], a["Cout"], a["H"], a["K"], a["s"], a["pad"], act, one, None)

    def dgrad(dz=q, w=q, out=q, **kw):
        a = dict(ok, **kw)
        return L.set_sconv1d_dgrad(dz, w, None, None, out, a["R"], a["Cin"], a["Cout"], a["H"], a["K"], a["s"], a["pad"], one, None)

    for call, name in ((fwd, b"set_sconv1d_fwd"), (dgrad, b"set_sconv1d_dgrad")):
        assert call(None) == INV and name in L.set_last_error()
        assert call(w=None) == INV and call(out=None) == INV
        for bad in (dict(R=0), dict(Cin=0), dict(Cout=-1), dict(H=0), dict(K=0), dict(K=8), dict(s=0), dict(s=5), dict(pad=-1), dict(pad=5),
                    dict(H=1, K=5, pad=1)):
            assert call(**bad) == INV, (name, bad)
        assert call(Cin=1 << 15, H=1 << 15) == UNS and b"2 GiB" in L.set_last_error()
        assert call(Cout=1 << 16, H=1 << 15) == UNS
    assert fwd(act=2) == INV
    assert L.set_sconv1d_out_len(0, 5, 3, 2) == INV and L.set_sconv1d_out_len(8, 5, 5, 2) == INV and L.set_sconv1d_out_len(8, 5, 3, 2) == 3

    def fold_fwd(y=q, yh=q, w=q, out=q, B=2, T=16, p=3, Cc=4, K=5, s=3, pad=2, act=1):
        return L.set_mpd_fold_conv_fwd(y, yh, w, q, out, B, T, p, Cc, K, s, pad, act, one, None)

    def fold_bwd(dz=q, w=q, g=q, B=2, T=16, p=3, Cc=4, K=5, s=3, pad=2):
        return L.set_mpd_fold_conv_bwd(dz, w, g, B, T, p, Cc, K, s, pad, None)

    assert fold_fwd(None) == INV and fold_fwd(yh=None) == INV and fold_fwd(w=None) == INV and fold_fwd(out=None) == INV
    assert b"set_mpd_fold_conv_fwd" in L.set_last_error()
    assert fold_bwd(None) == INV and fold_bwd(w=None) == INV and fold_bwd(g=None) == INV and b"set_mpd_fold_conv_bwd" in L.set_last_error()
    for call in (fold_fwd, fold_bwd):
        for bad in (dict(B=0), dict(T=3), dict(T=2), dict(p=0), dict(Cc=0), dict(K=8), dict(K=0), dict(s=0), dict(s=5), dict(pad=5), dict(pad=-1)):
            assert call(**bad) == INV, bad
    assert fold_fwd(act=3) == INV
    words = (C.c_int64 * 18)()
    t = C.cast(words, C.c_void_p)
    assert L.set_multi_loss_fwd(None, 1, 1, one, 1, q, q, None) == INV and b"set_multi_loss_fwd" in L.set_last_error()
    assert L.set_multi_loss_fwd(t, 1, 1, one, 1, None, q, None) == INV and L.set_multi_loss_fwd(t, 1, 1, one, 1, q, None, None) == INV
    assert L.set_multi_loss_fwd(t, 0, 1, one, 1, q, q, None) == INV and L.set_multi_loss_fwd(t, 2, 1, one, 1, q, q, None) == INV
    assert L.set_multi_loss_fwd(t, 1, 1, one, 0, q, q, None) == INV and L.set_multi_loss_fwd(t, 1, 1, one, 5, q, q, None) == INV
    assert L.set_multi_loss_bwd(None, 1, 1, one, q, None) == INV and L.set_multi_loss_bwd(t, 1, 1, one, None, None) == INV
    assert L.set_multi_loss_bwd(t, 0, 0, one, q, None) == INV and b"set_multi_loss_bwd" in L.set_last_error()


def test_module_parameters_and_refusals_without_a_gpu():
    import set_amd  # noqa: F401
    from set_amd.discriminators import DiscriminatorP, MultiPeriodDiscriminator, feature_loss
    mpd = MultiPeriodDiscriminator()
    state = MM.seeded_state(5)
    assert list(mpd.state_dict()) == list(state) and all(tuple(v.shape) == tuple(state[k].shape) for k, v in mpd.state_dict().items())
    mpd.load_state_dict(state, strict=True)
    assert [d.period for d in mpd.discriminators] == list(MM.PERIODS)
    assert not any(q.requires_grad for q in mpd.parameters())
    assert tuple(mpd.discriminators[0].convs[3].weight_v.shape) == (1024, 512, 5, 1)
    assert [(m.stride[0], m.padding[0]) for m in mpd.discriminators[0].convs] == [(3, 2)] * 4 + [(1, 2)]
    for kw in (dict(use_cond=True), dict(use_spectral_norm=True)):
        with pytest.raises(NotImplementedError):
            DiscriminatorP(2, **kw)
    d = DiscriminatorP(2, channels=MM.NARROW)
    d._check_weights()
    d.conv_post.weight_g.requires_grad_(True)
    with pytest.raises(RuntimeError, match="weight gradients are not built"):
        d._check_weights()
    with torch.no_grad():
        d._check_weights()
    y = torch.zeros(2, 1, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mpd(y, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature_loss([[y]], [[y]])
