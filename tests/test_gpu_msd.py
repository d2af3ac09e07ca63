"""The multi-scale discriminator on the GPU (csrc/msd.hip, set_amd.discriminators) against the float64 model of tests/msd_models.py.

Raw calls write into sentinel-filled guarded buffers (tests/raw_abi.py); the module runs with NaN-filled outputs and scratch.  Integer
cases are compared bit for bit (every product and sum is exact; +0 and -0 are one value); Gaussian cases within BAR_FACTOR times the
float32 mirror's error.  Every test prints the largest error / bar ratio of its stages (`-s` shows them; profiles/msd_gpu_accuracy.log
is that output)."""
import numpy as np
import pytest
import torch

import mpd_models as PM
import msd_models as MM
from raw_abi import L, Sent, bits, check, stream, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def same_bits(got, want):
    got, want = np.asarray(got, np.float32) + np.float32(0), np.asarray(want, np.float32) + np.float32(0)
    return got.shape == want.shape and bool((bits(got) == bits(want)).all())


def grouped_weight(W, groups):
    from set_amd import ops
    return ops.GroupedConvWeight(to_dev(W, DEV), W.shape[0], W.shape[1] * groups, W.shape[2], groups)


def raw_fwd(x, gw, bias, s, pad, slope, off=0):
    R, Cin, H = x.shape
    Ho = L().set_gconv1d_out_len(H, gw.K, s, pad)
    assert Ho == MM.out_len(H, gw.K, s, pad)
    out = Sent((R, gw.Cout, Ho), DEV, off=off)
    xd, bd = to_dev(x, DEV), (None if bias is None else to_dev(bias, DEV))
    check(L().set_gconv1d_fwd(xd.data_ptr(), gw.packed().data_ptr(), None if bd is None else bd.data_ptr(), out.ptr, R, Cin, gw.Cout, gw.groups, H,
                              gw.K, s, pad, int(slope is not None), float(slope or 0.0), stream()), "set_gconv1d_fwd")
    return out.get()


def raw_dgrad(dz, gw, H_in, s, pad, f_in, add, slope, off=0):
    R = dz.shape[0]
    out = Sent((R, gw.Cin, H_in), DEV, off=off)
    dzd = to_dev(dz, DEV)
    fd, ad = (None if f_in is None else to_dev(f_in, DEV)), (None if add is None else to_dev(add, DEV))
    check(L().set_gconv1d_dgrad(dzd.data_ptr(), gw.packed_transposed().data_ptr(), None if fd is None else fd.data_ptr(),
                                None if ad is None else ad.data_ptr(), out.ptr, R, gw.Cin, gw.Cout, gw.groups, H_in, gw.K, s, pad, float(slope),
                                stream()), "set_gconv1d_dgrad")
    return out.get()


# ---- the grouped conv pair, integer operands: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", MM.GROUP_PAIRS, ids=lambda p: "%dto%d" % p)
def test_gconv_integer_cases_bit_for_bit(pair):
    cases = [c for c in MM.gconv_cases() if c[:2] == pair]
    assert len(cases) >= 8
    assert (L().set_gconv1d_tile(pair[0]), L().set_gconv1d_tile(pair[1])) == (MM.tile_of(pair[0]), MM.tile_of(pair[1]))
    zero_gates = 0
    for n, (cig, cog, G, K, s, pad, H, R, use_bias, use_act, use_gate, use_add) in enumerate(cases):
        rng = np.random.default_rng(1000 * cig + 10 * cog + n)
        x = MM.int_array(rng, (R, cig * G, H), MM.INT_X)
        W = MM.int_array(rng, (cog * G, cig, K), MM.INT_W)
        b = MM.int_array(rng, (cog * G,), MM.INT_X) if use_bias else None
        gw = grouped_weight(W, G)
        tag = (cig, cog, G, K, s, pad, H, R, use_bias, use_act, use_gate, use_add)
        slope = MM.INT_SLOPE if use_act else None
        want = MM.gconv_rows(x.astype(np.float64), W.astype(np.float64), None if b is None else b.astype(np.float64), s, pad, G, slope)
        assert same_bits(raw_fwd(x, gw, b, s, pad, slope, off=n % 2), want), ("fwd", tag)
        Ho = want.shape[2]
        dz = MM.int_array(rng, (R, cog * G, Ho), MM.INT_X)
        f_in = MM.int_array(rng, (R, cig * G, H), MM.INT_X)
        f_in.reshape(-1)[::5] = 0                                   # exact zeros: gate(0) = slope
        add = MM.int_array(rng, (R, cig * G, H), MM.INT_X)
        gate = MM.gate_of(f_in.astype(np.float64), MM.INT_SLOPE) if use_gate else None
        zero_gates += int(use_gate)
        want = MM.gdgrad_rows(dz.astype(np.float64), W.astype(np.float64), H, s, pad, G, gate, add.astype(np.float64) if use_add else None)
        got = raw_dgrad(dz, gw, H, s, pad, f_in if use_gate else None, add if use_add else None, MM.INT_SLOPE, off=(n + 1) % 2)
        assert same_bits(got, want), ("dgrad", tag)
    assert zero_gates > 0


@pytest.mark.parametrize("cin,cout,groups,s", MM.MSD_LAYER_SHAPES)
@pytest.mark.parametrize("H", [64, 77])
def test_gconv_gaussian_within_the_mirror_bar(cin, cout, groups, s, H):
    rng = np.random.default_rng(cin + cout + H + s)
    R, K, pad = 2, 41, 20
    cig = cin // groups
    x = rng.standard_normal((R, cin, H)).astype(np.float32)
    W = (rng.standard_normal((cout, cig, K)) * (2.0 / (cig * K)) ** 0.5).astype(np.float32)
    b = (0.05 * rng.standard_normal(cout)).astype(np.float32)
    gw = grouped_weight(W, groups)
    x64, W64, b64 = x.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    want = MM.gconv_rows(x64, W64, b64, s, pad, groups, MM.SLOPE)
    bar = MM.bar(want, MM.gconv_rows(x, W, b, s, pad, groups, MM.SLOPE, chain=True))
    got = raw_fwd(x, gw, b, s, pad, MM.SLOPE)
    err = float(np.abs(got - want).max())
    print("gconv fwd   %4d -> %4d g %2d H %3d s %d: err %.3e bar %.3e ratio %.3f" % (cin, cout, groups, H, s, err, bar, err / bar))
    assert 0 < bar < 1e-4 and err <= bar
    Ho = want.shape[2]
    dz = rng.standard_normal((R, cout, Ho)).astype(np.float32)
    f_in = rng.standard_normal((R, cin, H)).astype(np.float32)
    add = rng.standard_normal((R, cin, H)).astype(np.float32)
    gate64 = MM.gate_of(f_in.astype(np.float64), MM.SLOPE)
    want = MM.gdgrad_rows(dz.astype(np.float64), W64, H, s, pad, groups, gate64, add.astype(np.float64))
    bar = MM.bar(want, MM.gdgrad_rows(dz, W, H, s, pad, groups, gate64.astype(np.float32), add, chain=True))
    got = raw_dgrad(dz, gw, H, s, pad, f_in, add, MM.SLOPE)
    err = float(np.abs(got - want).max())
    print("gconv dgrad %4d -> %4d g %2d H %3d s %d: err %.3e bar %.3e ratio %.3f" % (cin, cout, groups, H, s, err, bar, err / bar))
    assert 0 < bar < 1e-4 and err <= bar


# ---- the first layer on the waveforms ----------------------------------------------------------------------------------------------------
def _wave_calls(y, y_hat, W, b, pad, slope, dz, off):
    B, T = y.shape
    Cc, K = W.shape[0], W.shape[2]
    out = Sent((2 * B, Cc, T), DEV, off=off)
    yd, yhd, Wd, bd = (to_dev(a, DEV) for a in (y, y_hat, W, b))
    check(L().set_wave_conv_fwd(yd.data_ptr(), yhd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.ptr, B, T, Cc, K, pad, int(slope is not None),
                                float(slope or 0.0), stream()), "set_wave_conv_fwd")
    alone = Sent((B, Cc, T), DEV, off=1 - off)
    check(L().set_wave_conv_fwd(yhd.data_ptr(), None, Wd.data_ptr(), bd.data_ptr(), alone.ptr, B, T, Cc, K, pad, int(slope is not None),
                                float(slope or 0.0), stream()), "set_wave_conv_fwd")
    g = Sent((B, T), DEV, off=1 - off)
    dzd = to_dev(dz, DEV)
    check(L().set_wave_conv_bwd(dzd.data_ptr(), Wd.data_ptr(), g.ptr, B, T, Cc, K, pad, stream()), "set_wave_conv_bwd")
    return out.get(), alone.get(), g.get()


@pytest.mark.parametrize("T", MM.WAVE_T)
def test_wave_conv_integer_cases_bit_for_bit(T):
    for n, (Cc, K) in enumerate(((128, 15), (5, 3), (12, 1), (9, 7))):
        rng = np.random.default_rng(100 * T + n)
        B, pad = 2, (K - 1) // 2
        y, y_hat = MM.int_array(rng, (B, T), MM.INT_X), MM.int_array(rng, (B, T), MM.INT_X)
        W, b = MM.int_array(rng, (Cc, 1, K), MM.INT_W), MM.int_array(rng, (Cc,), MM.INT_X)
        dz = MM.int_array(rng, (B, Cc, T), MM.INT_X)
        out, alone, g = _wave_calls(y, y_hat, W, b, pad, MM.INT_SLOPE, dz, n % 2)
        want = MM.wave_conv(np.concatenate([y, y_hat]).astype(np.float64), W.astype(np.float64), b.astype(np.float64), pad, MM.INT_SLOPE)
        assert same_bits(out, want) and same_bits(alone, want[B:]), ("wave fwd", T, Cc, K)
        assert same_bits(g, MM.wave_conv_bwd(dz.astype(np.float64), W.astype(np.float64), pad)), ("wave bwd", T, Cc, K)


def test_wave_conv_gaussian_within_the_mirror_bar():
    rng = np.random.default_rng(11)
    B, T, Cc, K, pad = 2, 333, 128, 15, 7
    y, y_hat = MM.waves(12, B, T)
    W = (rng.standard_normal((Cc, 1, K)) * (2.0 / K) ** 0.5).astype(np.float32)
    b = (0.05 * rng.standard_normal(Cc)).astype(np.float32)
    dz = rng.standard_normal((B, Cc, T)).astype(np.float32)
    out, _alone, g = _wave_calls(y, y_hat, W, b, pad, MM.SLOPE, dz, 0)
    wav = np.concatenate([y, y_hat])
    want = MM.wave_conv(wav.astype(np.float64), W.astype(np.float64), b.astype(np.float64), pad, MM.SLOPE)
    bar = MM.bar(want, MM.wave_conv(wav, W, b, pad, MM.SLOPE, chain=True))
    err = float(np.abs(out - want).max())
    print("wave fwd: err %.3e bar %.3e ratio %.3f" % (err, bar, err / bar))
    assert 0 < bar < 1e-5 and err <= bar
    want = MM.wave_conv_bwd(dz.astype(np.float64), W.astype(np.float64), pad)
    bar = MM.bar(want, MM.wave_conv_bwd(dz, W, pad, chain=True))
    err = float(np.abs(g - want).max())
    print("wave bwd: err %.3e bar %.3e ratio %.3f" % (err, bar, err / bar))
    assert 0 < bar < 1e-3 and err <= bar


# ---- the pool ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", MM.POOL_T)
def test_pool_bit_for_bit_in_the_documented_order(T):
    rng = np.random.default_rng(T)
    B = 3
    x = rng.standard_normal((B, T)).astype(np.float32)
    To = MM.pool_len(T)
    assert L().set_avgpool4s2_out_len(T) == To
    out = Sent((B, To), DEV, off=T % 2)
    xd = to_dev(x, DEV)
    check(L().set_avgpool4s2_fwd(xd.data_ptr(), out.ptr, B, T, stream()), "set_avgpool4s2_fwd")
    assert (bits(out.get()) == bits(MM.pool(x))).all()
    g = rng.standard_normal((B, To)).astype(np.float32)
    add = rng.standard_normal((B, T)).astype(np.float32)
    gd, ad = to_dev(g, DEV), to_dev(add, DEV)
    for a_np, a_dev in ((None, None), (add, ad)):
        gin = Sent((B, T), DEV, off=(T + 1) % 2)
        check(L().set_avgpool4s2_bwd(gd.data_ptr(), None if a_dev is None else a_dev.data_ptr(), gin.ptr, B, T, stream()), "set_avgpool4s2_bwd")
        assert (bits(gin.get()) == bits(MM.pool_bwd(g, T, a_np).astype(np.float32))).all(), (T, a_np is None)


# ---- the module, end to end ------------------------------------------------------------------------------------------------------------
_MODULES = {}


def _module(case):
    """The module of a case with its seeded buffers restored (a training forward moves weight_u / weight_v)."""
    from set_amd.discriminators import MultiScaleDiscriminator
    channels, groups, _B, _T, train = MM.E2E[case][:5]
    key = case.rsplit("_", 1)[0]
    if key not in _MODULES:
        _MODULES[key] = MultiScaleDiscriminator(channels=channels, groups=groups).to(DEV)
    msd = _MODULES[key]
    msd.load_state_dict(MM.e2e_inputs(case)[0], strict=True)             # the reference's key names
    return msd.train(train)


def _run(case, rows=None, squeeze=False):
    from set_amd.discriminators import feature_loss, generator_loss
    _state, y, y_hat = MM.e2e_inputs(case)
    if rows is not None:
        y, y_hat = y[rows], y_hat[rows]
    yd, yh = to_dev(y, DEV), to_dev(y_hat, DEV)
    if not squeeze:
        yd, yh = yd.unsqueeze(1), yh.unsqueeze(1)
    yh.requires_grad_()
    rs, gs, fr, fg = _module(case)(yd, yh, sentinel=NAN)
    gl, fl = generator_loss(gs), feature_loss(fr, fg)
    return yh, rs, gs, fr, fg, gl, fl


@pytest.mark.parametrize("case", list(MM.E2E))
def test_msd_end_to_end_against_the_model(case):
    _channels, _groups, B, T, train = MM.E2E[case][:5]
    fw, bars = MM.e2e_model(case), MM.load_bars(case)
    yh, rs, gs, fr, fg, gl, fl = _run(case)
    msd = _MODULES[case.rsplit("_", 1)[0]]
    after = {k: v.detach().cpu().numpy() for k, v in msd.state_dict().items()}
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    ratios = dict(score=0.0, maps=0.0, loss=0.0, grad=0.0)
    decisions, flips, entries = [], 0, 0
    for i in range(MM.N_SCALES):
        assert tuple(gs[i].shape) == tuple(rs[i].shape) == tuple(fw["scores_g"][i].shape)
        assert not rs[i].requires_grad and gs[i].requires_grad
        ratios["score"] = max(ratios["score"], np.abs(n(gs[i]) - fw["scores_g"][i]).max() / (MM.BAR_FACTOR * bars["maps"][i][7]),
                              np.abs(n(rs[i]) - fw["scores_r"][i]).max() / (MM.BAR_FACTOR * bars["maps"][i][7]))
        gates, signs = [], []
        for j in range(8):
            want_r, want_g = fw["real"][i][j], fw["gen"][i][j]
            got_r, got_g = n(fr[i][j]), n(fg[i][j])
            assert got_r.shape == want_r.shape == got_g.shape and not fr[i][j].requires_grad
            ratios["maps"] = max(ratios["maps"], np.abs(got_r - want_r).max() / (MM.BAR_FACTOR * bars["maps"][i][j]),
                                 np.abs(got_g - want_g).max() / (MM.BAR_FACTOR * bars["maps"][i][j]))
            # the decisions the GPU took on its own maps; they may differ from the model's only where the operand is within the bar of 0
            sg = np.sign(got_g - got_r).astype(np.float64)
            differ = sg != fw["signs"][i][j]
            assert (np.abs(fw["sign_ops"][i][j][differ]) <= MM.BAR_FACTOR * bars["sign_ops"][i][j]).all(), ("sign", i, j)
            flips, entries = flips + int(differ.sum()), entries + differ.size
            signs.append(sg)
            if j < 7:
                gt = MM.gate_of(got_g, MM.SLOPE).astype(np.float64)
                differ = gt != fw["gates"][i][j]
                assert (np.abs(fw["gate_ops"][i][j][differ]) <= MM.BAR_FACTOR * bars["maps"][i][j]).all(), ("gate", i, j)
                flips, entries = flips + int(differ.sum()), entries + differ.size
                gates.append(gt)
        decisions.append((gates, signs))
    assert flips <= MM.UNDECIDED_CAP * entries, (flips, entries)
    # The losses are means over maps that have just been held to their bars b = BAR_FACTOR x the mirror's error, so their bound follows
    # from those (a single scalar's mirror error is one draw and no yardstick): |fm - model| <= 2 sum over the maps of mean(|dr| + |dg|)
    # <= 4 sum b;  |gen - model| <= (1 / 3) sum over the scales of (2 max |1 - g| + b) b;  plus the result's own fp32 rounding.
    b_maps = MM.BAR_FACTOR * bars["maps"]
    fm_bound = 4.0 * float(b_maps.sum()) + 2.0 ** -23 * abs(float(fw["fm_loss"]))
    gen_bound = sum((2.0 * float(np.abs(1 - fw["gen"][i][7]).max()) + b_maps[i][7]) * b_maps[i][7] for i in range(MM.N_SCALES)) / MM.N_SCALES \
        + 2.0 ** -23 * abs(float(fw["gen_loss"]))
    ratios["loss"] = max(abs(float(gl.detach()) - float(fw["gen_loss"])) / gen_bound, abs(float(fl.detach()) - float(fw["fm_loss"])) / fm_bound)
    g_adv, g_fm = MM.msd_grad(fw, 1.0, 0.0, decisions), MM.msd_grad(fw, 0.0, 1.0, decisions)
    for k, (ua, uf) in enumerate(MM.U_PAIRS):
        total = gl * ua + fl * uf
        (g1,) = torch.autograd.grad(total, yh, retain_graph=True)
        (g2,) = torch.autograd.grad(total, yh, retain_graph=True)          # a second backward: bit for bit
        assert tuple(g1.shape) == (B, 1, T) and torch.equal(g1, g2) and bool(torch.isfinite(g1).all())
        want = ua * g_adv + uf * g_fm
        ratios["grad"] = max(ratios["grad"], np.abs(n(g1)[:, 0] - want).max() / (MM.BAR_FACTOR * bars["grads"][k]))
    uv = 0.0
    for k, v in fw["after"].items():                                      # weight_u / weight_v: moved by a training forward only
        uv = max(uv, float(np.abs(after[k] - v).max() / np.abs(v).max()))
    assert uv <= 1e-5, uv
    print("msd %-16s flips %d of %d; u / v rel %.1e; err / bar: %s" % (case, flips, entries, uv, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(0 <= v <= 1.0 for v in ratios.values()), ratios
    # a second run from restored buffers gives the same bits
    yh2, rs2, gs2, fr2, fg2, gl2, fl2 = _run(case)
    assert torch.equal(gl, gl2) and torch.equal(fl, fl2)
    assert all(torch.equal(a, b) for a, b in zip(gs + [m for d in fg for m in d], gs2 + [m for d in fg2 for m in d]))
    (ga,) = torch.autograd.grad(gl * MM.LAMBDA_ADV + fl * 2.5, yh)
    (gb,) = torch.autograd.grad(gl2 * MM.LAMBDA_ADV + fl2 * 2.5, yh2)
    assert torch.equal(ga, gb)


def test_eval_folds_once_and_training_moves_the_buffers():
    msd = _module("narrow_333_eval")
    d0 = msd.discriminators[0]
    _run("narrow_333_eval")
    first = [c._slot.value for c in d0._convs] + [c._slot.value for c in msd.discriminators[1]._convs]
    _state, y, y_hat = MM.e2e_inputs("narrow_333_eval")
    yd, yh = to_dev(y, DEV), to_dev(y_hat, DEV)
    with torch.no_grad():
        msd(yd, yh)
    again = [c._slot.value for c in d0._convs] + [c._slot.value for c in msd.discriminators[1]._convs]
    assert all(a is b and a[0] is b[0] and a[1] is b[1] for a, b in zip(first, again))          # the cache's identity: no re-fold, no re-pack
    u0 = d0.convs[2].weight_u.clone()
    msd.train()
    with torch.no_grad():
        msd(yd, yh)
    assert not torch.equal(u0, d0.convs[2].weight_u)
    msd.eval()
    with torch.no_grad():
        msd(yd, yh)
    assert d0._convs[2]._slot.value is not first[2]                                            # new u, v: a new fold


def test_a_row_of_a_batch_equals_that_row_alone():
    for case in ("narrow_333_eval", "narrow_333_train"):
        _yh, rs, gs, fr, fg, gl, fl = _run(case)
        _yh1, rs1, gs1, fr1, fg1, gl1, fl1 = _run(case, rows=slice(1, 2))
        for i in range(MM.N_SCALES):
            assert torch.equal(gs[i][1:2], gs1[i]) and torch.equal(rs[i][1:2], rs1[i])
            for j in range(8):
                assert torch.equal(fg[i][j][1:2], fg1[i][j]) and torch.equal(fr[i][j][1:2], fr1[i][j])
        assert float(gl) != float(gl1) and float(fl) != float(fl1)


def test_two_and_three_dimensional_inputs_agree():
    a = _run("narrow_333_eval")
    b = _run("narrow_333_eval", squeeze=True)
    assert torch.equal(a[5], b[5]) and torch.equal(a[6], b[6])
    (ga,) = torch.autograd.grad(a[5] + a[6], a[0])
    (gb,) = torch.autograd.grad(b[5] + b[6], b[0])
    assert tuple(ga.shape) == (2, 1, 333) and tuple(gb.shape) == (2, 333) and torch.equal(ga[:, 0], gb)


def test_loss_functions_take_the_msd_maps():
    from set_amd.discriminators import discriminator_loss
    _yh, rs, gs, fr, fg, gl, fl = _run("narrow_333_eval")
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    want = PM.multi_loss([(n(g), n(r), PM.L1, 0) for dr, dg in zip(fr, fg) for r, g in zip(dr, dg)], 2.0, 1)
    assert bits(n(fl).reshape(1)) == bits(want)
    want = PM.multi_loss([(n(o), None, PM.SQ1, 0) for o in gs], 1.0 / 3, 1)
    assert bits(n(gl).reshape(1)) == bits(want)
    dr, dg = discriminator_loss(rs, [g.detach() for g in gs])
    want = PM.multi_loss([(n(o), None, PM.SQ1, 0) for o in rs] + [(n(o), None, PM.SQ0, 1) for o in gs], 1.0 / 3, 2)
    assert bits(n(dr).reshape(1)) == bits(want[:1]) and bits(n(dg).reshape(1)) == bits(want[1:])


def test_both_discriminators_in_one_backward():
    from set_amd.discriminators import MultiPeriodDiscriminator, feature_loss, generator_loss
    msd = _module("narrow_333_eval")
    mpd = MultiPeriodDiscriminator(channels=PM.NARROW)
    mpd.load_state_dict(PM.seeded_state(3, PM.NARROW), strict=True)
    mpd = mpd.to(DEV)
    _state, y, y_hat = MM.e2e_inputs("narrow_333_eval")
    yd = to_dev(y, DEV).unsqueeze(1)

    def step(which):
        yh = to_dev(y_hat, DEV).unsqueeze(1).requires_grad_()
        tot = 0
        for d in which:
            _, g, fr, fg = d(yd, yh, sentinel=NAN)
            tot = tot + generator_loss(g) * 4.0 + feature_loss(fr, fg)
        tot.backward()
        return yh.grad
    both, gp, gs = step((mpd, msd)), step((mpd,)), step((msd,))
    assert torch.equal(both, gp + gs) and float(gs.abs().max()) > 0 and float(gp.abs().max()) > 0


def test_module_refusals_on_the_gpu():
    from set_amd.discriminators import DiscriminatorS, MultiScaleDiscriminator
    msd = _module("narrow_333_eval")
    y = torch.zeros(2, 1, 64, device=DEV)
    with pytest.raises(ValueError, match="y is data"):
        msd(y.clone().requires_grad_(), y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        msd(y.cpu(), y)
    with pytest.raises(TypeError):
        msd(y.double(), y.double())
    with pytest.raises(ValueError):
        msd(y, torch.zeros(2, 1, 65, device=DEV))
    with pytest.raises(ValueError, match="pool of scale 2"):
        msd(y[:, :, :3], y[:, :, :3])
    rs, gs, _fr, _fg = msd(y[:, :, :4], y[:, :, :4])                      # the shortest waveform every scale accepts
    assert [tuple(s.shape) for s in gs] == [(2, 1)] * 3 and [tuple(m[0].shape) for m in _fg] == [(2, 12, 4), (2, 12, 2), (2, 12, 1)]
    d = DiscriminatorS(channels=MM.NARROW, groups=MM.NARROW_GROUPS).to(DEV)
    d.convs[2].weight_v.requires_grad_(True)
    with pytest.raises(RuntimeError, match="weight gradients are not built"):
        d(y, y)
    with torch.no_grad():
        sr, sg, mr, mg = d(y, y)
    assert tuple(sr.shape) == tuple(sg.shape) and len(mr) == len(mg) == 8 and torch.equal(sr, sg)
    with pytest.raises(NotImplementedError):
        MultiScaleDiscriminator(use_cond=True)


def test_readme_one_liner_shape():
    from set_amd.discriminators import MultiScaleDiscriminator, feature_loss, generator_loss
    d = MultiScaleDiscriminator().cuda()
    assert all(k in d.state_dict() for k in MM.seeded_state(1, MM.NARROW, MM.NARROW_GROUPS))
    torch.manual_seed(0)
    y = 0.3 * torch.randn(2, 1, 8192).cuda()
    y_ = (y + 0.02 * torch.randn_like(y)).requires_grad_()
    _, g, fr, fg = d(y, y_)
    (generator_loss(g) + feature_loss(fr, fg)).backward()
    assert tuple(y_.grad.shape) == (2, 1, 8192) and bool(torch.isfinite(y_.grad).all()) and float(y_.grad.abs().max()) > 0
