"""The float64 models of the discriminator step (tests/disc_step_models.py) held to float64 torch autograd on weight_norm /
spectral_norm Conv2d / Conv1d(groups) modules with discriminator_loss, to finite differences (the two fold backwards), and to themselves:
the Python mirror of the slice plan against the library, the case tables, the exactness budget of the integer cases, the float32
mirror, the planted faults the bars must separate, and the share of gate decisions the model alone leaves undecided.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm, weight_norm

import disc_step_models as DM
import mpd_models as PM
import msd_models as SM

REL = 1e-12


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---- torch modules written from the published architecture (HiFi-GAN's discriminators), float64 ----------------------------------------
class TorchP(nn.Module):
    def __init__(self, period, channels):
        super().__init__()
        self.period = period
        ch = [1] + list(channels)
        self.convs = nn.ModuleList([weight_norm(nn.Conv2d(ch[i], ch[i + 1], (5, 1), (3 if i < 4 else 1, 1), padding=(2, 0))) for i in range(5)])
        self.conv_post = weight_norm(nn.Conv2d(ch[5], 1, (3, 1), 1, padding=(1, 0)))

    def forward(self, x):
        b, c, t = x.shape
        if t % self.period:
            x = F.pad(x, (0, self.period - t % self.period), "reflect")
        x = x.view(b, c, -1, self.period)
        for layer in self.convs:
            x = F.leaky_relu(layer(x), PM.SLOPE)
        return torch.flatten(self.conv_post(x), 1, -1)


class TorchS(nn.Module):
    def __init__(self, spectral, channels, groups):
        super().__init__()
        norm = spectral_norm if spectral else weight_norm
        ch = [1] + list(channels)
        self.convs = nn.ModuleList([norm(nn.Conv1d(ch[j], ch[j + 1], SM.KERNELS[j], SM.STRIDES[j], groups=groups[j], padding=SM.PADS[j]))
                                    for j in range(7)])
        self.conv_post = norm(nn.Conv1d(ch[7], 1, 3, 1, padding=1))

    def forward(self, x):
        for layer in self.convs:
            x = F.leaky_relu(layer(x), SM.SLOPE)
        return torch.flatten(self.conv_post(x), 1, -1)


class TorchDisc(nn.Module):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        if kind == "mpd":
            self.discriminators = nn.ModuleList([TorchP(p, PM.NARROW) for p in PM.PERIODS])
        else:
            self.discriminators = nn.ModuleList([TorchS(i == 0, DM.MSD_NARROW, DM.MSD_NARROW_GROUPS) for i in range(3)])
        self.pool = nn.AvgPool1d(4, 2, padding=1)

    def forward(self, y, y_hat):
        rs, gs = [], []
        for i, d in enumerate(self.discriminators):
            if self.kind == "msd" and i:
                y, y_hat = self.pool(y), self.pool(y_hat)
            rs.append(d(y))
            gs.append(d(y_hat))
        return rs, gs


def torch_step(case, u_r, u_f):
    kind, _B, _T, train, _sw, _sy = DM.E2E[case]
    state, y, y_hat = DM.e2e_inputs(case)
    net = TorchDisc(kind).double()
    net.load_state_dict({k: torch.from_numpy(v).double() for k, v in state.items()}, strict=True)
    net.train(train)
    rs, gs = net(torch.from_numpy(y).double()[:, None], torch.from_numpy(y_hat).double()[:, None])
    r = sum(((1 - a) ** 2).mean() for a in rs) / len(rs)
    f = sum((a ** 2).mean() for a in gs) / len(gs)
    (u_r * r + u_f * f).backward()
    return {k: q.grad.numpy() for k, q in net.named_parameters()}, r.item(), f.item()


@pytest.mark.parametrize("case", ["mpd_333", "msd_333_eval", "msd_333_train", "msd_1024_train"])
def test_step_model_matches_float64_autograd(case):
    fw = DM.e2e_forward(case)
    for u_r, u_f in DM.U_PAIRS:
        want, r, f = torch_step(case, u_r, u_f)
        got = DM.e2e_step(fw, case, u_r, u_f)
        assert set(got) == set(want)
        assert abs(float(fw["disc_r_loss"]) - r) <= REL * abs(r) and abs(float(fw["disc_g_loss"]) - f) <= REL * abs(f)
        worst = max(rel_err(got[k].reshape(want[k].shape), want[k]) for k in want)
        print("%s u = (%g, %g): worst relative error of a parameter's gradient %.2e" % (case, u_r, u_f, worst))
        assert worst <= REL


@pytest.mark.parametrize("run", DM.GOLDEN_RUNS, ids=lambda r: r[0])
def test_step_model_matches_the_recorded_reference(run):
    """The reference's own discriminators and discriminator_loss at full size (tests/golden/disc_step_reference.npz), and the reference
    itself where its checkout is present."""
    import os
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_step_reference.npz"))
    got, losses = DM.golden_model(run)
    name = run[0]
    keys = [k[len(name) + 6:] for k in rec.files if k.startswith(name + ".grad.")]
    assert set(keys) == set(got) and len(keys) > 30
    worst = 0.0
    for k in keys:
        want = rec["%s.grad.%s" % (name, k)]
        worst = max(worst, float(np.abs(got[k] - want).max() / want[1]))         # relative to the gradient's L2 norm
    print("%s: worst error of a recorded value / its gradient's norm %.2e" % (name, worst))
    assert worst <= REL
    assert np.abs(np.asarray(losses) - rec[name + ".losses"]).max() <= REL * np.abs(rec[name + ".losses"]).max()
    from oracle import ref_import
    if ref_import.available():
        import importlib
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
        ref_import.install()
        tool = importlib.import_module("make_disc_step_golden")
        live = tool.record(importlib.import_module("modules.vocoder.hifigan.hifigan"), only=name)
        for k in keys:
            assert np.abs(live["%s.grad.%s" % (name, k)] - got[k]).max() <= REL * got[k][1], k


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cig,cog,G,K,s,pad,H,R", [(8, 16, 3, 41, 2, 20, 77, 3), (33, 17, 2, 5, 3, 0, 40, 2), (1, 8, 1, 3, 4, 1, 9, 1),
                                                   (16, 32, 2, 1, 1, 0, 12, 3), (72, 1, 1, 3, 1, 1, 10, 3)])
def test_wgrad_model_matches_autograd(cig, cog, G, K, s, pad, H, R):
    rng = np.random.default_rng(K + H)
    x = rng.standard_normal((R, cig * G, H))
    Ho = DM.out_len(H, K, s, pad)
    dz = rng.standard_normal((R, cog * G, Ho))
    W = torch.zeros(cog * G, cig, K, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cog * G, dtype=torch.float64, requires_grad=True)
    out = F.conv1d(torch.from_numpy(x), W, b, stride=s, padding=pad, groups=G)
    out.backward(torch.from_numpy(dz))
    dW, db = DM.gconv_wgrad(dz, x, K, s, pad, G)
    assert rel_err(dW, W.grad.numpy()) <= REL and rel_err(db, b.grad.numpy()) <= REL
    # the float32 mirror, at several slice counts, is the model up to float32 rounding -- and not exactly it
    for slices in (1, 2, 5):
        mW, mb = DM.gconv_wgrad_mirror(x=x.astype(np.float32), dz=dz.astype(np.float32), K=K, s=s, pad=pad, groups=G, slices=slices)
        w32, b32 = DM.gconv_wgrad(dz.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64), K, s, pad, G)
        assert rel_err(mW, w32) < 1e-5 and rel_err(mb, b32) < 1e-6


@pytest.mark.parametrize("p", PM.PERIODS)
def test_first_layer_models_match_autograd(p):
    rng = np.random.default_rng(p)
    B, T, C, K, s, pad = 2, 10 * p + 3, 6, 5, 3, 2
    y, y_hat = rng.standard_normal((B, T)), rng.standard_normal((B, T))
    net = TorchP(p, (C, 1, 1, 1, 1)).double()
    conv = net.convs[0]
    xs = []
    for w in (y, y_hat):
        x = torch.from_numpy(w)[:, None]
        if T % p:
            x = F.pad(x, (0, p - T % p), "reflect")
        xs.append(x.view(B, 1, -1, p))
    Wt = torch.zeros(C, 1, K, 1, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(torch.cat(xs), Wt, bt, stride=conv.stride, padding=conv.padding)       # [2 B, C, H_out, p]
    g = torch.from_numpy(rng.standard_normal(tuple(out.shape)))
    out.backward(g)
    dz = g.permute(0, 3, 1, 2).reshape(2 * B * p, C, -1).numpy()                          # rows (sig B + b) p + w
    dW, db = DM.fold_wgrad(dz, y, y_hat, p, K, s, pad)
    assert rel_err(dW, Wt.grad.numpy().reshape(C, K)) <= REL and rel_err(db, bt.grad.numpy()) <= REL
    # the MSD's first layer
    Wt = torch.zeros(C, 1, 15, dtype=torch.float64, requires_grad=True)
    wavs = np.concatenate([y, y_hat])
    out = F.conv1d(torch.from_numpy(wavs)[:, None], Wt, padding=7)
    g = rng.standard_normal(tuple(out.shape))
    out.backward(torch.from_numpy(g))
    dW, _db = DM.wave_wgrad(g, wavs, 15, 7)
    assert rel_err(dW, Wt.grad.numpy().reshape(C, 15)) <= REL


def test_fold_backwards_match_finite_differences_and_autograd():
    rng = np.random.default_rng(5)
    n0, shape = 6, (6, 3, 5)
    g, v, Cm = rng.standard_normal((n0, 1, 1)) + 2, rng.standard_normal(shape), rng.standard_normal(shape)
    f = lambda g_, v_: float((Cm * SM.wn_fold(g_, v_)).sum())  # noqa: E731
    dg, dv = DM.wn_fold_bwd(Cm, g, v)
    eps = 1e-6
    for idx in [(0, 0, 0), (3, 0, 0), (5, 0, 0)]:
        e = np.zeros_like(g)
        e[idx] = eps
        assert abs((f(g + e, v) - f(g - e, v)) / (2 * eps) - dg[idx]) <= 1e-7 * max(1, abs(dg[idx]))
    for idx in [(0, 0, 0), (2, 1, 4), (5, 2, 3)]:
        e = np.zeros_like(v)
        e[idx] = eps
        assert abs((f(g, v + e) - f(g, v - e)) / (2 * eps) - dv[idx]) <= 1e-7 * max(1, abs(dv[idx]))
    W = rng.standard_normal(shape)
    u, vv = rng.standard_normal(n0), rng.standard_normal(15)
    u, vv = u / np.linalg.norm(u), vv / np.linalg.norm(vv)
    fs = lambda W_: float((Cm * SM.sn_fold(W_, u, vv)).sum())  # noqa: E731
    dWo = DM.sn_fold_bwd(Cm, W, u, vv)
    for idx in [(0, 0, 0), (2, 1, 4), (5, 2, 3)]:
        e = np.zeros_like(W)
        e[idx] = eps
        assert abs((fs(W + e) - fs(W - e)) / (2 * eps) - dWo[idx]) <= 1e-7 * max(1, abs(dWo[idx]))
    # and exactly (1e-12) against autograd
    Wt = torch.from_numpy(W).requires_grad_(True)
    sig = torch.dot(torch.from_numpy(u), torch.mv(Wt.reshape(n0, -1), torch.from_numpy(vv)))
    ((Wt / sig) * torch.from_numpy(Cm)).sum().backward()
    assert rel_err(dWo, Wt.grad.numpy()) <= REL
    gt, vt = torch.from_numpy(g).requires_grad_(True), torch.from_numpy(v).requires_grad_(True)
    (torch._weight_norm(vt, gt, 0) * torch.from_numpy(Cm)).sum().backward()
    assert rel_err(dg, gt.grad.numpy()) <= REL and rel_err(dv, vt.grad.numpy()) <= REL
    # the planted faults of the folds are far outside float32 rounding
    assert rel_err(DM.wn_fold_bwd(Cm, g, v, fault="proj")[1], dv) > 1e-3
    assert rel_err(DM.sn_fold_bwd(Cm, W, u, vv, fault="sigma_const"), dWo) > 1e-3


# ---- the plan, the case tables, the exactness budget ------------------------------------------------------------------------------------
def test_plan_mirror_matches_the_library(built_lib):
    L = built_lib
    shapes = [(R, cig * G, cog * G, G, H, K, s, (K - 1) // 2) for (cig, cog, G) in DM.WGRAD_TRIPLES for R in (1, 3, 128, 1408)
              for H, K, s in ((10, 5, 3), (21, 5, 3), (77, 41, 2), (8192, 41, 4), (2731, 5, 1))]
    shapes += [(128, cin, cout, G, 2048, K, s, (K - 1) // 2) for cin, cout, G, K, s in DM.MPD_PAIRS + DM.MSD_PAIRS]
    seen = set()
    for n_cu in (1, 64, 256, 304):
        for sh in shapes:
            got = L.set_gconv1d_wgrad_plan(*sh, n_cu)
            assert got == DM.plan(*sh, n_cu), (sh, n_cu, got)
            seen.add(got)
            assert L.set_gconv1d_wgrad_scratch_floats(*sh, 3) == 3 * sh[2] * (sh[1] // sh[3]) * sh[5]
    assert 1 in seen and DM.MAX_SLICES in seen and len(seen) > 4
    assert L.set_gconv1d_wgrad_plan(1, 4, 4, 1, 10, DM.KMAX + 1, 1, 0, 8) < 0 and L.set_gconv1d_wgrad_plan(1, 4, 4, 3, 10, 3, 1, 0, 8) < 0
    assert L.set_gconv1d_wgrad_scratch_floats(1, 4, 4, 1, 10, 3, 1, 0, DM.MAX_SLICES + 1) < 0


def test_case_table_covers_the_grid_and_stays_exact():
    cases = DM.wgrad_cases()
    assert 100 <= len(cases) <= 400
    col = lambda i: {c[i] for c in cases}  # noqa: E731
    assert {c[:3] for c in cases} == set(DM.WGRAD_TRIPLES)
    assert col(3) == set(DM.WGRAD_KS) and col(4) == {1, 2, 3, 4} and col(7) == {1, 3} and col(8) == set(DM.WGRAD_SLICES)
    assert col(9) == {False, True} and col(10) == {False, True}
    for s in (1, 2, 3, 4):
        for K in DM.WGRAD_KS:
            sub = [c for c in cases if c[3] == K and c[4] == s]
            assert {c[5] for c in sub} == {0, (K - 1) // 2}
            J = {c[7] * DM.out_len(c[6], K, s, c[5]) for c in sub}
            assert J & {DM.CHUNK - 1, DM.CHUNK - 2} and J & {DM.CHUNK, DM.CHUNK + 1} and max(J) > DM.CHUNK + 1, (s, K, sorted(J))
            assert any(c[7] == 3 and DM.out_len(c[6], K, s, c[5]) <= 10 for c in sub)          # several short rows in one chunk
            if s > 1:
                assert any((c[6] + 2 * c[5] - K) % s for c in sub)
    # a forced slice count beyond the chunks leaves slices empty; one that does not divide them leaves the last one short
    empties = [c for c in cases if c[8] == 5 and -(-c[7] * DM.out_len(c[6], c[3], c[4], c[5]) // DM.CHUNK) < 5]
    assert empties
    for cig, cog, G, K, s, pad, H, R, _sl, _acc, _db in cases:
        # + 1 row of magnitude INT_X^2 R H_out for the accumulate operand
        assert 2 * DM.exact_budget(R, DM.out_len(H, K, s, pad), cig, K) < 2 ** 24


def test_wgrad_faults_are_outside_the_bar():
    """Each planted fault moves the weight gradient by far more than BAR_FACTOR x the float32 mirror's error."""
    rng = np.random.default_rng(9)
    R, cin, cout, G, K, s, pad, H = 2, 32, 32, 2, 5, 2, 2, 77
    x = rng.standard_normal((R, cin, H)).astype(np.float32)
    dz = rng.standard_normal((R, cout, DM.out_len(H, K, s, pad))).astype(np.float32)
    x64, d64 = x.astype(np.float64), dz.astype(np.float64)
    want, _ = DM.gconv_wgrad(d64, x64, K, s, pad, G)
    b = DM.bar(want, DM.gconv_wgrad_mirror(dz, x, K, s, pad, G, 2)[0])
    assert 0 < b < 1e-4
    for fault in ("tap", "phase", "last_slice", "real_rows"):
        got, _ = DM.gconv_wgrad(d64, x64, K, s, pad, G, fault=fault, slices=2)
        assert np.abs(got - want).max() > 100 * b, fault


@pytest.mark.parametrize("case", ["mpd_333", "msd_333_train", "msd_333_eval"])
def test_step_faults_are_outside_the_bars(case):
    """A step that leaves the real rows out moves every parameter's gradient beyond its bar; one that treats sigma as a constant moves
    every weight_orig's."""
    fw, bars = DM.e2e_forward(case), DM.grad_bars(DM.load_bars(case), 0)
    want = DM.e2e_step(fw, case)
    order = list(want)
    for fault in ("real_rows",) + (("sigma_const",) if case.startswith("msd") else ()):
        got = DM.e2e_step(fw, case, fault=fault)
        hit = [k for k in order if fault == "real_rows" or k.endswith("weight_orig")]
        assert len(hit) >= 8
        for k in hit:
            assert np.abs(got[k] - want[k]).max() > bars[order.index(k)], (fault, k)


# ---- gate decisions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(DM.E2E))
def test_recorded_bars_and_undecided_share(case):
    """The recorded mirror errors exist for every parameter and the share of gate entries the model alone leaves undecided stays under
    the cap, for the real and for the generated rows."""
    bars = DM.load_bars(case)
    state, _y, _y_hat = DM.e2e_inputs(case)
    n_par = len([k for k in state if not k.endswith(("weight_u",)) and not (k.endswith("weight_v") and k.replace("weight_v", "weight_orig") in state)])
    for n in range(len(DM.U_PAIRS)):
        assert bars["grads%d" % n].shape == (n_par,) and (bars["grads%d" % n] > 0).all()
    und = bars["undecided"]
    print("%s: undecided share real %.2e generated %.2e (cap %.0e)" % (case, und[0], und[1], DM.UNDECIDED_CAP))
    assert und.shape == (2,) and (und < DM.UNDECIDED_CAP).all()


def test_recorded_bars_are_the_mirrors():
    """One case recomputed live: the recording is what the mirror gives."""
    case = "msd_333_eval"
    live, rec = DM.mirror_errors(case), DM.load_bars(case)
    assert set(live) == set(rec)
    for k in live:
        assert np.array_equal(np.asarray(live[k]), rec[k]), k
