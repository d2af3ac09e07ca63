"""The multi-period discriminator on the GPU (csrc/sconv.hip, set_amd.discriminators) against the float64 model of tests/mpd_models.py.

Raw calls write into sentinel-filled guarded buffers (tests/raw_abi.py); the module runs with NaN-filled outputs and scratch.  Integer
cases are compared bit for bit (every product and sum is exact; +0 and -0 are one value); Gaussian cases within BAR_FACTOR times the
float32 mirror's error.  Every test prints the largest error / bar ratio of its stages (`-s` shows them; profiles/mpd_gpu_accuracy.log
is that output).

Which losses legitimately differ between a batch and its rows alone: every loss is a mean over the whole batch, so a row alone gives
another number (the maps and scores of a row do not depend on the batch, bit for bit)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mpd_models as MM
from raw_abi import L, Sent, bits, check, stream, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _grad_mode():
    """Autograd on, whatever grad mode an earlier test module left behind."""
    with torch.enable_grad():
        yield


def same_bits(got, want):
    """Bit for bit, with -0 and +0 as one value."""
    got, want = np.asarray(got, np.float32) + np.float32(0), np.asarray(want, np.float32) + np.float32(0)
    return got.shape == want.shape and bool((bits(got) == bits(want)).all())


def conv_weight(W):
    from set_amd import ops
    return ops.ConvWeight(to_dev(W, DEV), W.shape[0], W.shape[1], W.shape[2])


def raw_fwd(x, cw, bias, s, pad, slope, off=0):
    R, Cin, H = x.shape
    Ho = L().set_sconv1d_out_len(H, cw.K, s, pad)
    assert Ho == MM.out_len(H, cw.K, s, pad)
    out = Sent((R, cw.Cout, Ho), DEV, off=off)
    xd, bd = to_dev(x, DEV), (None if bias is None else to_dev(bias, DEV))
    check(L().set_sconv1d_fwd(xd.data_ptr(), cw.packed().data_ptr(), None if bd is None else bd.data_ptr(), out.ptr, R, Cin, cw.Cout, H, cw.K, s, pad,
                              int(slope is not None), float(slope or 0.0), stream()), "set_sconv1d_fwd")
    return out.get()


def raw_dgrad(dz, cw, H_in, s, pad, f_in, add, slope, off=0):
    R = dz.shape[0]
    out = Sent((R, cw.Cin, H_in), DEV, off=off)
    dzd = to_dev(dz, DEV)
    fd, ad = (None if f_in is None else to_dev(f_in, DEV)), (None if add is None else to_dev(add, DEV))
    check(L().set_sconv1d_dgrad(dzd.data_ptr(), cw.transposed().packed().data_ptr(), None if fd is None else fd.data_ptr(),
                                None if ad is None else ad.data_ptr(), out.ptr, R, cw.Cin, cw.Cout, H_in, cw.K, s, pad, float(slope), stream()),
          "set_sconv1d_dgrad")
    return out.get()


# ---- the two GEMM kernels, integer operands: bit for bit ---------------------------------------------------------------------------------
STRIDE_KERNEL = [(s, K) for s in (1, 2, 3, 4) for K in (1, 3, 5)]


@pytest.mark.parametrize("s,K", STRIDE_KERNEL)
def test_sconv_integer_cases_bit_for_bit(s, K):
    cases = [c for c in MM.sconv_cases() if c[0] == s and c[1] == K]
    assert len(cases) >= 10
    for n, (_s, _K, pad, cin, cout, H, R) in enumerate(cases):
        rng = np.random.default_rng(1000 * s + 100 * K + n)
        x = MM.int_array(rng, (R, cin, H), MM.INT_X)
        W = MM.int_array(rng, (cout, cin, K), MM.INT_W)
        b = MM.int_array(rng, (cout,), MM.INT_X)
        cw = conv_weight(W)
        tag = (s, K, pad, cin, cout, H, R)
        want = MM.conv_rows(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), s, pad, MM.INT_SLOPE)
        assert same_bits(raw_fwd(x, cw, b, s, pad, MM.INT_SLOPE, off=n % 2), want), ("fwd", tag)
        want = MM.conv_rows(x.astype(np.float64), W.astype(np.float64), None, s, pad, None)
        assert same_bits(raw_fwd(x, cw, None, s, pad, None, off=(n + 1) % 2), want), ("fwd plain", tag)
        Ho = want.shape[2]
        dz = MM.int_array(rng, (R, cout, Ho), MM.INT_X)
        f_in = MM.int_array(rng, (R, cin, H), MM.INT_X)          # exact zeros are frequent: gate(0) = slope
        add = MM.int_array(rng, (R, cin, H), MM.INT_X)
        f_in.reshape(-1)[::5] = 0
        for use_gate in (False, True):
            for use_add in (False, True):
                gate = MM.gate_of(f_in.astype(np.float64), MM.INT_SLOPE) if use_gate else None
                want = MM.dgrad_rows(dz.astype(np.float64), W.astype(np.float64), H, s, pad, gate, add.astype(np.float64) if use_add else None)
                got = raw_dgrad(dz, cw, H, s, pad, f_in if use_gate else None, add if use_add else None, MM.INT_SLOPE, off=n % 2)
                assert same_bits(got, want), ("dgrad", use_gate, use_add, tag)


GAUSS = [(512, 1024, 20, 3, 5, 2), (128, 512, 200, 3, 5, 2), (512, 1024, 20, 1, 5, 2), (1024, 1, 20, 1, 3, 1)]


@pytest.mark.parametrize("cin,cout,H,s,K,pad", GAUSS)
def test_sconv_gaussian_within_the_mirror_bar(cin, cout, H, s, K, pad):
    rng = np.random.default_rng(cin + cout + H + s)
    R = 2
    x = rng.standard_normal((R, cin, H)).astype(np.float32)
    W = (rng.standard_normal((cout, cin, K)) * (2.0 / (cin * K)) ** 0.5).astype(np.float32)
    b = (0.05 * rng.standard_normal(cout)).astype(np.float32)
    cw = conv_weight(W)
    x64, W64, b64 = x.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    want = MM.conv_rows(x64, W64, b64, s, pad, MM.SLOPE)
    bar = MM.bar(want, MM.conv_rows(x, W, b, s, pad, MM.SLOPE, chain=True))
    got = raw_fwd(x, cw, b, s, pad, MM.SLOPE)
    err = float(np.abs(got - want).max())
    print("sconv fwd   %4d -> %4d H %3d s %d: err %.3e bar %.3e ratio %.3f" % (cin, cout, H, s, err, bar, err / bar))
    assert 0 < bar < 1e-4 and err <= bar
    Ho = want.shape[2]
    dz = rng.standard_normal((R, cout, Ho)).astype(np.float32)
    f_in = rng.standard_normal((R, cin, H)).astype(np.float32)   # the gate operand is an input here: both sides decide on the same value
    add = rng.standard_normal((R, cin, H)).astype(np.float32)
    gate64 = MM.gate_of(f_in.astype(np.float64), MM.SLOPE)
    want = MM.dgrad_rows(dz.astype(np.float64), W64, H, s, pad, gate64, add.astype(np.float64))
    bar = MM.bar(want, MM.dgrad_rows(dz, W, H, s, pad, gate64.astype(np.float32), add, chain=True))
    got = raw_dgrad(dz, cw, H, s, pad, f_in, add, MM.SLOPE)
    err = float(np.abs(got - want).max())
    print("sconv dgrad %4d -> %4d H %3d s %d: err %.3e bar %.3e ratio %.3f" % (cin, cout, H, s, err, bar, err / bar))
    assert 0 < bar < 1e-4 and err <= bar


# ---- the folded first layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", MM.PERIODS)
def test_fold_layer_integer_cases_bit_for_bit(p):
    for n, T in enumerate((p + 1, 97, 200, 1024)):
        for (s, K, pad, Cc) in ((3, 5, 2, 32), (1, 3, 1, 5), (2, 5, 0, 8)) if T != 1024 else ((3, 5, 2, 32),):
            H_in = -(-T // p)
            if H_in + 2 * pad < K:
                continue
            rng = np.random.default_rng(100 * p + 10 * n + s)
            B = 2
            y, y_hat = MM.int_array(rng, (B, T), MM.INT_X), MM.int_array(rng, (B, T), MM.INT_X)
            W = MM.int_array(rng, (Cc, 1, K), MM.INT_W)
            b = MM.int_array(rng, (Cc,), MM.INT_X)
            Ho = MM.out_len(H_in, K, s, pad)
            out = Sent((2 * B * p, Cc, Ho), DEV, off=n % 2)
            yd, yhd, Wd, bd = (to_dev(a, DEV) for a in (y, y_hat, W, b))
            check(L().set_mpd_fold_conv_fwd(yd.data_ptr(), yhd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.ptr, B, T, p, Cc, K, s, pad, 1,
                                            MM.INT_SLOPE, stream()), "set_mpd_fold_conv_fwd")
            x = np.concatenate([MM.fold(y.astype(np.float64), p), MM.fold(y_hat.astype(np.float64), p)])
            want = MM.conv_rows(x, W.astype(np.float64), b.astype(np.float64), s, pad, MM.INT_SLOPE)
            assert same_bits(out.get(), want), ("fold fwd", p, T, s, K, pad)
            dz = MM.int_array(rng, (B * p, Cc, Ho), MM.INT_X)
            g = Sent((B, T), DEV, off=(n + 1) % 2)
            dzd = to_dev(dz, DEV)
            check(L().set_mpd_fold_conv_bwd(dzd.data_ptr(), Wd.data_ptr(), g.ptr, B, T, p, Cc, K, s, pad, stream()), "set_mpd_fold_conv_bwd")
            want = MM.fold_bwd(dz.astype(np.float64), W.astype(np.float64), B, T, p, s, pad)
            if T % p:  # a sample and its mirror both contribute
                tail = MM.fold_index(T, p)[T:]
                assert len(tail) == p - T % p and (tail < T - 1).all()
            assert same_bits(g.get(), want), ("fold bwd", p, T, s, K, pad)


# ---- the list losses -------------------------------------------------------------------------------------------------------------------
def _loss_items(rng):
    """[(a tensor, b tensor or None, mode, slot)] on the device: a contiguous pair with ties, a pair with permuted strides, a one-element
    item, an item of three chunks and one of more than 256 chunks."""
    def dev(shape, scale=1.0):
        return to_dev((scale * rng.standard_normal(shape)).astype(np.float32), DEV)
    a0, b0 = dev((3, 5, 7)), dev((3, 5, 7))
    b0.view(-1)[::3] = a0.view(-1)[::3]                                   # a == b ties: sign(0) = 0
    a1, b1 = dev((2, 3, 4, 5)).permute(0, 2, 3, 1), dev((3, 2, 5, 4)).permute(1, 3, 2, 0)   # two views of [2, 4, 5, 3]: walked in a's memory
    a2 = dev((1, 1))                                                      # order, b keeps four strided dims (nothing merges)
    a3 = dev((5000,))
    a4 = dev((300, 2048), 0.5)
    return [(a0, b0, MM.L1, 0), (a1, b1, MM.L1, 0), (a2, None, MM.SQ1, 1), (a3, None, MM.SQ0, 1), (a4, None, MM.SQ1, 0)]


def test_multi_loss_forward_and_backward_bit_for_bit():
    from set_amd import ops
    rng = np.random.default_rng(5)
    items = _loss_items(rng)
    assert items[1][0].shape == items[1][1].shape and not items[1][0].is_contiguous()
    a_list, b_list = [it[0] for it in items], [it[1] for it in items]
    modes, slots = [it[2] for it in items], [it[3] for it in items]
    scale, n_slots = 0.7, 2
    grads = [torch.full(a.shape, NAN, device=DEV).as_strided(a.shape, a.stride()) if i != 3 else None for i, a in enumerate(a_list)]
    grads[1] = torch.full((2, 3, 4, 5), NAN, device=DEV).permute(0, 2, 3, 1)
    table, chunks, host = ops.multi_loss_items(a_list, b_list, modes, slots, grads)
    assert tuple(host.shape) == (5, MM.LOSS_WORDS) and chunks == 1 + 1 + 1 + 3 + 300
    assert host[1, 4:8].tolist() == [2, 3, 4, 5] and host[1, 12:16].tolist() == [20, 40, 1, 4]   # nothing merges
    part = torch.full((chunks,), NAN, dtype=torch.float64, device=DEV)
    loss = Sent((n_slots,), DEV)
    check(L().set_multi_loss_fwd(table.data_ptr(), len(items), chunks, scale, n_slots, part.data_ptr(), loss.ptr, stream()), "set_multi_loss_fwd")
    # the numpy restatement walks each item in the table's element order: row-major over the extents of `host`
    def in_order(t, row, which):
        e = [int(v) for v in host[row, 4:8]]
        st = [int(v) for v in host[row, 8 + 4 * which:12 + 4 * which]]
        return torch.as_strided(t, e, st, t.storage_offset()).cpu().numpy()
    model_items = [(in_order(a, i, 0), None if b is None else in_order(b, i, 1), m, sl) for i, (a, b, m, sl) in enumerate(items)]
    want = MM.multi_loss(model_items, scale, n_slots)
    got = loss.get()
    assert (bits(got) == bits(want)).all(), (got, want)
    u = to_dev(np.asarray([1.25, -0.5], np.float32), DEV)
    check(L().set_multi_loss_bwd(table.data_ptr(), len(items), chunks, scale, u.data_ptr(), stream()), "set_multi_loss_bwd")
    for i, (a, b, m, sl) in enumerate(model_items):
        if grads[i] is None:
            continue
        g = in_order(grads[i], i, 0)
        want_g = MM.multi_loss_grad(a, b, m, [1.25, -0.5][sl], scale)
        assert same_bits(g, want_g), i
        if m == MM.L1 and i == 0:
            assert (g.reshape(-1)[::3] == 0).all()                        # the ties


def test_loss_functions_and_their_gradients():
    from set_amd.discriminators import discriminator_loss, feature_loss, generator_loss
    rng = np.random.default_rng(6)
    mk = lambda *s: to_dev(rng.standard_normal(s).astype(np.float32), DEV)  # noqa: E731
    fr = [[mk(2, 3, 5, 2), mk(2, 1, 4, 2)], [mk(2, 3, 3, 3)]]
    fg = [[mk(2, 3, 5, 2).requires_grad_(), mk(2, 1, 4, 2).requires_grad_()], [mk(2, 3, 3, 3).requires_grad_()]]
    outs = [mk(2, 8).requires_grad_(), mk(2, 9).requires_grad_()]
    reals = [mk(2, 8).requires_grad_(), mk(2, 9).requires_grad_()]
    fl, gl = feature_loss(fr, fg), generator_loss(outs)
    dr, dg = discriminator_loss(reals, outs)
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    flat_r, flat_g = [t for d in fr for t in d], [t for d in fg for t in d]
    want = MM.multi_loss([(n(g), n(r), MM.L1, 0) for r, g in zip(flat_r, flat_g)], 2.0, 1)
    assert bits(n(fl).reshape(1)) == bits(want)
    want = MM.multi_loss([(n(o), None, MM.SQ1, 0) for o in outs], 0.5, 1)
    assert bits(n(gl).reshape(1)) == bits(want)
    want = MM.multi_loss([(n(o), None, MM.SQ1, 0) for o in reals] + [(n(o), None, MM.SQ0, 1) for o in outs], 0.5, 2)
    assert bits(n(dr).reshape(1)) == bits(want[:1]) and bits(n(dg).reshape(1)) == bits(want[1:])
    (3.0 * fl + 0.25 * gl).backward()
    for r, g in zip(flat_r, flat_g):
        assert same_bits(n(g.grad), MM.multi_loss_grad(n(g), n(r), MM.L1, 3.0, 2.0))
    for o in outs:
        assert same_bits(n(o.grad), MM.multi_loss_grad(n(o), None, MM.SQ1, 0.25, 0.5))
        o.grad = None
    (dr + 2.0 * dg).backward()
    for o, r in zip(outs, reals):
        assert same_bits(n(o.grad), MM.multi_loss_grad(n(o), None, MM.SQ0, 2.0, 0.5))
        assert same_bits(n(r.grad), MM.multi_loss_grad(n(r), None, MM.SQ1, 1.0, 0.5))
    # torch's own autograd on the same values agrees to fp32 rounding
    ref = 2 * sum((r - g.detach()).abs().mean() for r, g in zip(flat_r, flat_g))
    assert abs(float(ref) - float(fl)) <= 1e-5 * abs(float(ref))


# ---- the module, end to end ------------------------------------------------------------------------------------------------------------
_MODULES = {}


def _module(case):
    from set_amd.discriminators import MultiPeriodDiscriminator
    if case not in _MODULES:
        channels = MM.E2E[case][0]
        mpd = MultiPeriodDiscriminator(channels=channels)
        mpd.load_state_dict(MM.e2e_inputs(case)[0], strict=True)         # the reference's key names
        _MODULES[case] = mpd.to(DEV)
    return _MODULES[case]


def _run(case, rows=None):
    from set_amd.discriminators import feature_loss, generator_loss
    _state, y, y_hat = MM.e2e_inputs(case)
    if rows is not None:
        y, y_hat = y[rows], y_hat[rows]
    yd = to_dev(y, DEV).unsqueeze(1)
    yh = to_dev(y_hat, DEV).unsqueeze(1).requires_grad_()
    rs, gs, fr, fg = _module(case)(yd, yh, sentinel=NAN)
    gl, fl = generator_loss(gs), feature_loss(fr, fg)
    return yh, rs, gs, fr, fg, gl, fl


@pytest.mark.parametrize("case", MM.GPU_E2E)
def test_mpd_end_to_end_against_the_model(case):
    channels, B, T, _sw, _sy = MM.E2E[case]
    fw, bars = MM.e2e_model(case), MM.load_bars(case)
    yh, rs, gs, fr, fg, gl, fl = _run(case)
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    ratios = dict(score=0.0, maps=0.0, loss=0.0, grad=0.0)
    decisions, flips, entries = [], 0, 0
    for i, p in enumerate(MM.PERIODS):
        Rg = B * p
        assert tuple(gs[i].shape) == tuple(rs[i].shape) == tuple(fw["scores_g"][i].shape)
        assert not rs[i].requires_grad and gs[i].requires_grad
        ratios["score"] = max(ratios["score"], np.abs(n(gs[i]) - fw["scores_g"][i]).max() / (MM.BAR_FACTOR * bars["maps"][i][5]),
                              np.abs(n(rs[i]) - fw["scores_r"][i]).max() / (MM.BAR_FACTOR * bars["maps"][i][5]))
        gates, signs = [], []
        for j in range(6):
            want_r, want_g = MM.rows_to_map(fw["maps"][i][j][:Rg], B, p), MM.rows_to_map(fw["maps"][i][j][Rg:], B, p)
            got_r, got_g = n(fr[i][j]), n(fg[i][j])
            assert got_r.shape == want_r.shape == got_g.shape and not fr[i][j].requires_grad
            ratios["maps"] = max(ratios["maps"], np.abs(got_r - want_r).max() / (MM.BAR_FACTOR * bars["maps"][i][j]),
                                 np.abs(got_g - want_g).max() / (MM.BAR_FACTOR * bars["maps"][i][j]))
            rows_r, rows_g = MM.map_to_rows(got_r), MM.map_to_rows(got_g)
            # the decisions the GPU took on its own maps; they may differ from the model's only where the operand is within the bar of 0
            sg = np.sign(rows_g - rows_r).astype(np.float64)
            differ = sg != fw["signs"][i][j]
            assert (np.abs(fw["sign_ops"][i][j][differ]) <= MM.BAR_FACTOR * bars["sign_ops"][i][j]).all(), ("sign", p, j)
            flips, entries = flips + int(differ.sum()), entries + differ.size
            signs.append(sg)
            if j < 5:
                gt = MM.gate_of(rows_g, MM.SLOPE).astype(np.float64)
                differ = gt != fw["gates"][i][j]
                assert (np.abs(fw["gate_ops"][i][j][differ]) <= MM.BAR_FACTOR * bars["maps"][i][j]).all(), ("gate", p, j)
                flips, entries = flips + int(differ.sum()), entries + differ.size
                gates.append(gt)
        decisions.append((gates, signs))
    assert flips <= MM.UNDECIDED_CAP * entries, (flips, entries)
    ratios["loss"] = max(abs(float(gl) - float(fw["gen_loss"])) / (MM.BAR_FACTOR * bars["losses"][0]),
                         abs(float(fl) - float(fw["fm_loss"])) / (MM.BAR_FACTOR * bars["losses"][1]))
    # a_p = generator_loss * lambda_adv and fm_f, backward for both upstream pairs; the model's backward takes the GPU's decisions
    g_adv, g_fm = MM.mpd_grad(fw, 1.0, 0.0, decisions), MM.mpd_grad(fw, 0.0, 1.0, decisions)
    for k, (ua, uf) in enumerate(MM.U_PAIRS):
        total = gl * ua + fl * uf
        (g1,) = torch.autograd.grad(total, yh, retain_graph=True)
        (g2,) = torch.autograd.grad(total, yh, retain_graph=True)
        assert tuple(g1.shape) == (B, 1, T) and torch.equal(g1, g2) and bool(torch.isfinite(g1).all())
        want = ua * g_adv + uf * g_fm
        ratios["grad"] = max(ratios["grad"], np.abs(n(g1)[:, 0] - want).max() / (MM.BAR_FACTOR * bars["grads"][k]))
    print("mpd %-10s flips %d of %d; err / bar: %s" % (case, flips, entries, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(0 <= v <= 1.0 for v in ratios.values()), ratios
    # a second run gives the same bits
    yh2, rs2, gs2, fr2, fg2, gl2, fl2 = _run(case)
    assert torch.equal(gl, gl2) and torch.equal(fl, fl2)
    assert all(torch.equal(a, b) for a, b in zip(gs + [m for d in fg for m in d], gs2 + [m for d in fg2 for m in d]))
    (ga,) = torch.autograd.grad(gl * MM.LAMBDA_ADV + fl * 2.5, yh)
    (gb,) = torch.autograd.grad(gl2 * MM.LAMBDA_ADV + fl2 * 2.5, yh2)
    assert torch.equal(ga, gb)


def test_a_row_of_a_batch_equals_that_row_alone():
    case = "narrow_200"
    _yh, rs, gs, fr, fg, gl, fl = _run(case)
    _yh1, rs1, gs1, fr1, fg1, gl1, fl1 = _run(case, rows=slice(1, 2))
    for i in range(len(MM.PERIODS)):
        assert torch.equal(gs[i][1:2], gs1[i]) and torch.equal(rs[i][1:2], rs1[i])
        for j in range(6):
            assert torch.equal(fg[i][j][1:2], fg1[i][j]) and torch.equal(fr[i][j][1:2], fr1[i][j])
    assert float(gl) != float(gl1) and float(fl) != float(fl1)            # means over another batch: they differ, legitimately


def test_module_refusals_on_the_gpu():
    from set_amd.discriminators import DiscriminatorP, MultiPeriodDiscriminator
    mpd = _module("narrow_200")
    y = torch.zeros(2, 1, 64, device=DEV)
    with pytest.raises(ValueError, match="y is data"):
        mpd(y.clone().requires_grad_(), y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mpd(y.cpu(), y)
    with pytest.raises(TypeError):
        mpd(y.double(), y.double())
    with pytest.raises(ValueError):
        mpd(y, torch.zeros(2, 1, 65, device=DEV))
    with pytest.raises(ValueError, match="reflect pad"):
        mpd(y[:, :, :11], y[:, :, :11])
    d = DiscriminatorP(3, channels=MM.NARROW).to(DEV)
    d.convs[2].weight_v.requires_grad_(True)
    with pytest.raises(RuntimeError, match="weight gradients are not built"):
        d(y, y)
    with torch.no_grad():
        sr, sg, mr, mg = d(y, y)                                          # no grad mode: nothing to refuse
    assert tuple(sr.shape) == tuple(sg.shape) and len(mr) == len(mg) == 6 and torch.equal(sr, sg)
    with pytest.raises(NotImplementedError):
        MultiPeriodDiscriminator(use_cond=True)


def test_issue_one_liner_shape():
    from set_amd.discriminators import MultiPeriodDiscriminator, feature_loss, generator_loss
    d = _module("full_97")
    torch.manual_seed(0)
    y = 0.3 * torch.randn(2, 1, 8192, device=DEV)
    y_ = (y + 0.02 * torch.randn_like(y)).requires_grad_()
    _, g, fr, fg = d(y, y_)
    (generator_loss(g) + feature_loss(fr, fg)).backward()
    assert tuple(y_.grad.shape) == (2, 1, 8192) and bool(torch.isfinite(y_.grad).all()) and float(y_.grad.abs().max()) > 0
    assert isinstance(d, MultiPeriodDiscriminator)
