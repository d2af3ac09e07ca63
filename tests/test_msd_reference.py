"""The float64 model of the multi-scale discriminator (tests/msd_models.py) against torch's own grouped conv1d + avg_pool1d + leaky_relu
under autograd in float64, against a live torch.nn.utils.spectral_norm conv, against the recording of the reference's own module
(tests/golden/msd_reference.npz, tools/make_msd_golden.py) and live through oracle/ref_import.py where the reference checkout is present.
Further: the exactness budget and coverage of the integer case table, the recorded bars and the undecided shares, the planted faults,
the entry points' refusals and the module's parameters."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mpd_models as PM
import msd_models as MM
from conftest import load_golden

GOLD_SEED_W, GOLD_SEED_Y, GOLD_B, GOLD_T = 61, 62, 2, 333


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def torch_msd(state, groups, y, y_hat, u_adv, u_fm, train, slope=MM.SLOPE, score_only=False, maps_only=False):
    """The generator-side step in float64 torch: folded weights as constants, F.conv1d(groups), F.avg_pool1d, autograd."""
    st = {k: v.double() for k, v in state.items()}
    y, yh0 = torch.from_numpy(y).double(), torch.from_numpy(y_hat).double().requires_grad_()
    yh = yh0
    gl, fl, maps_all = 0.0, 0.0, []
    for i in range(MM.N_SCALES):
        if i:
            y, yh = F.avg_pool1d(y[:, None], 4, 2, 1)[:, 0], F.avg_pool1d(yh[:, None], 4, 2, 1)[:, 0]
        Ws = []
        for j in range(8):
            pre = MM._pre(i, j)
            if i == 0:
                W, u, v = st[pre + "weight_orig"], st[pre + "weight_u"], st[pre + "weight_v"]
                m = W.reshape(W.shape[0], -1)
                both = []
                for _call in range(2):
                    if train:
                        v = F.normalize(m.t().mv(u), dim=0, eps=1e-12)
                        u = F.normalize(m.mv(v), dim=0, eps=1e-12)
                    both.append(W / torch.dot(u, m.mv(v)))
                Ws.append(both)
            else:
                Wn = torch._weight_norm(st[pre + "weight_v"], st[pre + "weight_g"], 0)
                Ws.append([Wn, Wn])
        outs = []
        for which, x in ((0, y), (1, yh)):
            x = x[:, None]
            ms = []
            for j in range(8):
                x = F.conv1d(x, Ws[j][which], st[MM._pre(i, j) + "bias"], MM.STRIDES[j], MM.PADS[j], 1, 1 if j == 7 else groups[j])
                if j < 7:
                    x = F.leaky_relu(x, slope)
                ms.append(x)
            outs.append(ms)
        maps_all.append(outs)
        gl = gl + ((1 - outs[1][7].flatten(1)) ** 2).mean()
        for r, g in zip(*outs):
            fl = fl + (r.detach() - g).abs().mean()
    gl, fl = gl / MM.N_SCALES, fl * 2
    total = (0 if maps_only else u_adv * gl) + (0 if score_only else u_fm * fl)
    (grad,) = torch.autograd.grad(total, yh0)
    return maps_all, float(gl), float(fl), grad.numpy()


@pytest.mark.parametrize("T", [83, 333])
@pytest.mark.parametrize("train", [False, True])
def test_model_matches_torch_float64(T, train):
    state = MM.seeded_state(7, MM.NARROW, MM.NARROW_GROUPS)
    y, y_hat = MM.waves(8, 2, T)
    fw = MM.msd_forward(y, y_hat, MM.state_numpy(state), MM.NARROW_GROUPS, train, slope=MM.SLOPE)
    for kw in (dict(), dict(score_only=True), dict(maps_only=True)):            # both gradient paths, and their sum
        maps, gl, fl, grad = torch_msd(state, MM.NARROW_GROUPS, y, y_hat, 4.0, 2.5, train, **kw)
        want = MM.msd_grad(fw, 4.0, 2.5, **kw)
        assert np.abs(grad - want).max() <= 1e-12 and np.abs(want).max() > 1e-6, kw
    for i in range(MM.N_SCALES):
        for j in range(8):
            assert np.abs(maps[i][0][j].detach().numpy() - fw["real"][i][j]).max() <= 1e-12
            assert np.abs(maps[i][1][j].detach().numpy() - fw["gen"][i][j]).max() <= 1e-12
    assert abs(gl - fw["gen_loss"]) <= 1e-12 and abs(fl - fw["fm_loss"]) <= 1e-12


@pytest.mark.parametrize("T", [2, 3, 4, 5, 64, 65, 333])
def test_pool_model_matches_avg_pool1d(T):
    rng = np.random.default_rng(T)
    x = rng.standard_normal((3, T))
    xt = torch.from_numpy(x).requires_grad_()
    want = F.avg_pool1d(xt[:, None], 4, 2, 1)[:, 0]
    got = MM.pool(x)
    assert got.shape == tuple(want.shape) == (3, MM.pool_len(T)) and np.abs(got - want.detach().numpy()).max() <= 1e-15
    g = rng.standard_normal(got.shape)
    add = rng.standard_normal(x.shape)
    (gx,) = torch.autograd.grad(want, xt, torch.from_numpy(g))
    assert np.abs(MM.pool_bwd(g, T) - gx.numpy()).max() <= 1e-15
    assert np.abs(MM.pool_bwd(g, T, add) - (add + gx.numpy())).max() <= 1e-15
    if T > 2:
        assert np.abs(MM.pool(x, edge_count=True) - got).max() > 1e-3          # the planted fault is visible


def test_layer_model_against_torch_grouped_conv1d():
    rng = np.random.default_rng(3)
    for (cig, cog, G, K, s, pad, H) in ((3, 5, 4, 41, 2, 20, 50), (8, 16, 3, 40, 4, 39, 9), (1, 1, 16, 5, 3, 0, 20), (17, 33, 1, 15, 1, 14, 7)):
        x = rng.standard_normal((2, cig * G, H))
        W = rng.standard_normal((cog * G, cig, K))
        b = rng.standard_normal(cog * G)
        xt = torch.from_numpy(x).requires_grad_()
        want = F.leaky_relu(F.conv1d(xt, torch.from_numpy(W), torch.from_numpy(b), s, pad, 1, G), 0.1)
        got = MM.gconv_rows(x, W, b, s, pad, G, 0.1)
        assert np.abs(got - want.detach().numpy()).max() <= 1e-12
        chain = MM.gconv_rows(x, W, b, s, pad, G, 0.1, chain=True)
        assert np.abs(got - chain).max() <= 1e-12
        dz = rng.standard_normal(got.shape)
        pre = F.conv1d(xt, torch.from_numpy(W), None, s, pad, 1, G)
        (gx,) = torch.autograd.grad(pre, xt, torch.from_numpy(dz))
        for ch in (False, True):
            assert np.abs(MM.gdgrad_rows(dz, W, H, s, pad, G, chain=ch) - gx.numpy()).max() <= 1e-12
    W1 = rng.standard_normal((6, 1, 15))
    dz = rng.standard_normal((2, 6, 40))
    assert np.abs(MM.wave_conv_bwd(dz, W1, 7) - MM.wave_conv_bwd(dz, W1, 7, chain=True)).max() <= 1e-12


@pytest.mark.parametrize("groups", [1, 4])
def test_spectral_norm_model_matches_torch(groups):
    torch.manual_seed(groups)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(8, 12, 41, 2, padding=20, groups=groups)).double()
    assert set(conv.state_dict()) == {"bias", "weight_orig", "weight_u", "weight_v"}
    W = conv.weight_orig.detach().numpy().copy()
    u, v = conv.weight_u.numpy().copy(), conv.weight_v.numpy().copy()
    x = torch.randn(1, 8, 30, dtype=torch.float64)
    conv.eval()
    conv(x)
    assert np.abs(conv.weight.detach().numpy() - MM.sn_fold(W, u, v)).max() <= 1e-12         # eval: the stored u, v, no iteration
    assert np.array_equal(conv.weight_u.numpy(), u)
    conv.train()
    for _it in range(2):
        conv(x)
        u, v = MM.sn_iterate(W, u, v)
        assert np.abs(conv.weight_u.numpy() - u).max() <= 1e-12 and np.abs(conv.weight_v.numpy() - v).max() <= 1e-12
        assert np.abs(conv.weight.detach().numpy() - MM.sn_fold(W, u, v)).max() <= 1e-12
        assert abs(float(torch.dot(conv.weight_u, conv.weight_orig.reshape(12, -1).mv(conv.weight_v))) - MM.sn_sigma(W, u, v)) <= 1e-12


def _check_recording(rec, mode, fw):
    for i in range(MM.N_SCALES):
        np.testing.assert_allclose(fw["scores_r"][i], rec["%s.score_r_%d" % (mode, i)], rtol=0, atol=1e-12)
        np.testing.assert_allclose(fw["scores_g"][i], rec["%s.score_g_%d" % (mode, i)], rtol=0, atol=1e-12)
        for j in range(8):
            for tag, m in (("r", fw["real"][i][j]), ("g", fw["gen"][i][j])):
                assert list(m.shape) == list(rec["%s.map_shapes_%d" % (mode, i)][j])
                np.testing.assert_allclose([m.mean(), np.abs(m).mean()], rec["%s.map_stats_%s_%d" % (mode, tag, i)][j], rtol=0, atol=1e-12)
    assert abs(float(fw["gen_loss"]) - float(rec[mode + ".generator_loss"])) <= 1e-12
    assert abs(float(fw["fm_loss"]) - float(rec[mode + ".feature_loss"])) <= 1e-12
    if mode == "train":
        for k, v in fw["after"].items():
            np.testing.assert_allclose(v, rec["train.after." + k], rtol=0, atol=1e-12)


def test_model_matches_the_reference():
    """The recording of the reference's own MultiScaleDiscriminator in eval() and in train() (B = 2, T = 333, float64) -- and, where
    the checkout is present, the same comparison live."""
    y, y_hat = MM.waves(GOLD_SEED_Y, GOLD_B, GOLD_T)
    state = MM.state_numpy(MM.seeded_state(GOLD_SEED_W))
    fws = {mode: MM.msd_forward(y, y_hat, state, MM.FULL_GROUPS, mode == "train", slope=0.1) for mode in ("eval", "train")}
    rec = load_golden("msd_reference")
    for mode, fw in fws.items():
        _check_recording(rec, mode, fw)
    from oracle import ref_import
    if ref_import.available():
        import importlib
        import importlib.util
        import os
        ref_import.install()
        spec = importlib.util.spec_from_file_location("make_msd_golden", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "make_msd_golden.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        assert (tool.SEED_W, tool.SEED_Y, tool.B, tool.T) == (GOLD_SEED_W, GOLD_SEED_Y, GOLD_B, GOLD_T)
        live = tool.record(importlib.import_module("modules.vocoder.hifigan.hifigan"))
        for mode, fw in fws.items():
            _check_recording(live, mode, fw)


def test_integer_cases_are_exact_and_cover_the_table():
    cases = MM.gconv_cases()
    assert len(cases) <= 400
    assert {c[:2] for c in cases} == set(MM.GROUP_PAIRS) and {c[2] for c in cases} == set(MM.GROUPS)
    assert {c[3] for c in cases} == set(MM.KS) and {c[4] for c in cases} == set(MM.STRIDES_ALL) and {c[7] for c in cases} == set(MM.RS)
    assert {c[5] for c in cases} >= {0, 20} and any(c[5] == c[3] - 1 and c[3] > 1 for c in cases)
    assert {(c[:2], c[4]) for c in cases} == {(p, s) for p in MM.GROUP_PAIRS for s in MM.STRIDES_ALL}
    assert {(c[3], c[4]) for c in cases} == {(K, s) for K in MM.KS for s in MM.STRIDES_ALL}
    for b in range(4):                                             # bias, activation, f_in, add: each with and without
        assert {c[8 + b] for c in cases} == {False, True}
    for tile in MM.GCONV_TILES:                                    # H_out around every forward tile width, H_in around every dgrad tile
        houts = {MM.out_len(c[6], c[3], c[4], c[5]) for c in cases if MM.tile_of(c[1]) == tile}
        assert houts >= {1, tile - 1, tile, tile + 1, 2 * tile + 3}, (tile, sorted(houts))
        for s in MM.STRIDES_ALL:
            hins = {c[6] for c in cases if MM.tile_of(c[0]) == tile and c[4] == s}
            assert hins & {s * tile - 1, s * tile, s * tile + 1}, (tile, s)
    assert max(MM.exact_budget(c[0], c[1], c[3]) for c in cases) < 2 ** 24
    assert 2 * (MM.INT_X * MM.INT_W * 128 * 15 + MM.INT_X) < 2 ** 24      # the wave conv's backward at C = 128, K = 15
    assert {MM.tile_of(c) for c in (1, 32, 33, 64, 65, 200)} == set(MM.GCONV_TILES)


def test_tile_widths_and_lengths_match_the_library(built_lib):
    from set_amd import _lib, ops
    L = _lib.lib()
    assert tuple(ops.GCONV_TILES) == MM.GCONV_TILES and (ops.GCONV_KMAX, ops.WAVE_CONV_KMAX) == (MM.GCONV_KMAX, MM.WAVE_KMAX)
    for rows in (1, 16, 32, 33, 64, 65, 1024):
        assert L.set_gconv1d_tile(rows) == MM.tile_of(rows)
    for H, K, s, pad in ((1, 41, 4, 20), (333, 41, 2, 20), (5, 40, 3, 39), (7, 1, 1, 0)):
        assert L.set_gconv1d_out_len(H, K, s, pad) == MM.out_len(H, K, s, pad)
    assert L.set_gconv1d_out_len(5, 42, 1, 0) < 0 and L.set_gconv1d_out_len(5, 5, 5, 0) < 0 and L.set_gconv1d_out_len(5, 5, 1, 5) < 0
    for T in (2, 3, 4, 5, 333):
        assert L.set_avgpool4s2_out_len(T) == MM.pool_len(T)
    assert L.set_avgpool4s2_out_len(1) == 0
    assert L.set_packed_gconv_weight_size(256, 128, 41, 16) == 16 * L.set_packed_conv_weight_size(16, 8, 41)
    assert L.set_packed_gconv_weight_size(256, 128, 41, 3) < 0


def test_entry_points_refuse_bad_arguments(built_lib):
    from set_amd import _lib
    L = _lib.lib()
    p = 4096                                                           # never dereferenced: every call is refused before a launch
    assert L.set_gconv1d_fwd(p, p, None, p, 1, 8, 8, 3, 10, 5, 1, 2, 0, 0.0, None) == _lib.E_INVALID      # groups divide neither
    assert L.set_gconv1d_fwd(p, p, None, p, 1, 8, 8, 2, 10, 42, 1, 2, 0, 0.0, None) == _lib.E_INVALID     # K > 41
    assert L.set_gconv1d_fwd(p, p, None, p, 1, 8, 8, 2, 10, 5, 5, 2, 0, 0.0, None) == _lib.E_INVALID      # s > 4
    assert L.set_gconv1d_fwd(p, p, None, p, 1, 8, 8, 2, 3, 41, 1, 0, 0, 0.0, None) == _lib.E_INVALID      # no output frame
    assert L.set_gconv1d_fwd(None, p, None, p, 1, 8, 8, 2, 10, 5, 1, 2, 0, 0.0, None) == _lib.E_INVALID
    assert L.set_gconv1d_dgrad(p, p, None, None, p, 1, 8, 8, 2, 10, 5, 1, 5, 0.0, None) == _lib.E_INVALID  # pad >= K
    assert L.set_gconv1d_dgrad(p, None, None, None, p, 1, 8, 8, 2, 10, 5, 1, 2, 0.0, None) == _lib.E_INVALID
    assert L.set_wave_conv_fwd(p, p, p, None, p, 1, 10, 4, 17, 8, 0, 0.0, None) == _lib.E_INVALID          # K > 15
    assert L.set_wave_conv_fwd(p, p, p, None, p, 1, 10, 4, 15, 6, 0, 0.0, None) == _lib.E_INVALID          # not a same-length conv
    assert L.set_wave_conv_bwd(p, p, p, 1, 0, 4, 15, 7, None) == _lib.E_INVALID
    assert L.set_avgpool4s2_fwd(p, p, 1, 1, None) == _lib.E_INVALID
    assert L.set_avgpool4s2_bwd(p, None, p, 0, 8, None) == _lib.E_INVALID


E2E_CPU = [c for c in MM.E2E if not c.startswith("full_1024")] + ["full_1024_train"]


@pytest.mark.parametrize("case", E2E_CPU)
def test_bars_and_undecided_share(case):
    """The recorded bars are the float32 mirror's errors, and the model alone leaves at most UNDECIDED_CAP of the gate and sign entries
    of any scale undecided (full_1024_eval shares its shapes with full_1024_train and is checked by the recording only)."""
    rec, now = MM.load_bars(case), MM.mirror_errors(case)
    assert set(rec) == set(now) == {"maps", "sign_ops", "losses", "grads", "undecided"}
    for k in ("maps", "sign_ops", "losses", "grads"):
        assert rec[k].shape == now[k].shape and (now[k] > 0).all()
        np.testing.assert_allclose(rec[k], now[k], rtol=0.05)
    assert (now["undecided"] <= MM.UNDECIDED_CAP).all() and (rec["undecided"] <= MM.UNDECIDED_CAP).all(), now["undecided"]
    fw = MM.e2e_model(case)
    scale = max(float(np.abs(m).max()) for maps in fw["gen"] for m in maps)
    assert now["maps"].max() < 1e-5 * max(scale, 1.0)
    assert now["grads"].max() < 1e-4 * float(np.abs(MM.msd_grad(fw, *MM.U_PAIRS[1])).max())


def test_every_recorded_case_stays_under_the_cap():
    for case in MM.E2E:
        rec = MM.load_bars(case)
        assert (rec["undecided"] <= MM.UNDECIDED_CAP).all() and all((rec[k] > 0).all() for k in ("maps", "sign_ops", "losses", "grads"))


FAULTS = [dict(group_shift=1), dict(reverse_taps=True), dict(pad=19), dict(edge_count=True), dict(gen_uses_real_sigma=True)]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: next(iter(f)))
def test_planted_faults_exceed_the_bar(fault):
    case = "narrow_333_train"
    fw, bars = MM.e2e_model(case), MM.load_bars(case)
    state, y, y_hat = MM.e2e_inputs(case)
    bad = MM.msd_forward(y, y_hat, MM.state_numpy(state), MM.E2E[case][1], True, faults=fault)
    worst = max(np.abs(b - a).max() / (MM.BAR_FACTOR * bars["maps"][i][j]) for i in range(MM.N_SCALES)
                for j, (a, b) in enumerate(zip(fw["gen"][i], bad["gen"][i])))
    assert worst > 10, worst
    g_bad = MM.msd_grad(bad, *MM.U_PAIRS[1])
    assert np.abs(g_bad - MM.msd_grad(fw, *MM.U_PAIRS[1])).max() > 10 * MM.BAR_FACTOR * bars["grads"][1]


def test_planted_gate_at_zero_exceeds_the_bar():
    """gate(0) = 1 instead of slope: Gaussian maps hold no exact zero, so the fault is planted where the kernels' tests look for it,
    on an integer grid whose f_in has exact zeros."""
    rng = np.random.default_rng(9)
    dz = MM.int_array(rng, (2, 32, 20), MM.INT_X).astype(np.float64)
    W = MM.int_array(rng, (32, 8, 41), MM.INT_W).astype(np.float64)
    f_in = MM.int_array(rng, (2, 16, 39), MM.INT_X).astype(np.float64)
    f_in.reshape(-1)[::5] = 0
    good = MM.gdgrad_rows(dz, W, 39, 2, 20, 2, gate=MM.gate_of(f_in, MM.INT_SLOPE))
    bad = MM.gdgrad_rows(dz, W, 39, 2, 20, 2, gate=np.where(f_in == 0, 1.0, MM.gate_of(f_in, MM.INT_SLOPE)))
    assert np.abs(good - bad).max() >= 0.5                            # an integer grid is compared bit for bit: any difference shows


def test_module_parameters_and_refusals_without_a_gpu():
    import set_amd  # noqa: F401
    from set_amd.discriminators import DiscriminatorS, MultiScaleDiscriminator
    msd = MultiScaleDiscriminator()
    state = MM.seeded_state(5)
    assert list(msd.state_dict()) == list(state) and all(tuple(v.shape) == tuple(state[k].shape) for k, v in msd.state_dict().items())
    msd.load_state_dict(state, strict=True)
    assert not any(q.requires_grad for q in msd.parameters())
    d0, d1 = msd.discriminators[0], msd.discriminators[1]
    assert set(k.split(".")[-1] for k in d0.state_dict()) == {"bias", "weight_orig", "weight_u", "weight_v"}
    assert set(k.split(".")[-1] for k in d1.state_dict()) == {"bias", "weight_g", "weight_v"}
    assert tuple(d1.convs[3].weight_v.shape) == (512, 16, 41) and tuple(d0.conv_post.weight_orig.shape) == (1, 1024, 3)
    assert [(m.kernel_size[0], m.stride[0], m.padding[0], m.groups) for m in d0.convs] == list(zip(MM.KERNELS, MM.STRIDES, MM.PADS, MM.FULL_GROUPS))
    with pytest.raises(NotImplementedError):
        MultiScaleDiscriminator(use_cond=True)
    with pytest.raises(NotImplementedError):
        DiscriminatorS(use_cond=True, upsample_rates=[4, 4, 16])
    d = DiscriminatorS(channels=MM.NARROW, groups=MM.NARROW_GROUPS)
    d._check_weights()
    d.conv_post.weight_g.requires_grad_(True)
    with pytest.raises(RuntimeError, match="weight gradients are not built"):
        d._check_weights()
    with torch.no_grad():
        d._check_weights()
    d._check_length(1)                                                # every layer keeps one frame alive (2 pad >= K - 1): only the pools need more
    with pytest.raises(ValueError, match="without an output frame"):
        d._check_length(0)
    y = torch.zeros(2, 1, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        msd(y, y)
    # the float64 model's state and the module's agree in names and shapes for the narrow net as well
    narrow = MultiScaleDiscriminator(channels=MM.NARROW, groups=MM.NARROW_GROUPS)
    narrow.load_state_dict(MM.seeded_state(6, MM.NARROW, MM.NARROW_GROUPS), strict=True)
    assert PM.UNDECIDED_CAP == MM.UNDECIDED_CAP
