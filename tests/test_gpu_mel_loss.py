"""GPU checks of the HiFi-GAN mel loss and its waveform gradient (csrc/mel_loss.hip through set_amd.vocoder_losses), launch by launch and
end to end, against the float64 model of mel_loss_models.py.  The bars are 4 x the error of a float32 mirror of the same matrix form
(derived and printed per fixture; test_mel_loss_reference.py asserts the conditions they stand on).  Every output and scratch buffer
starts as NaN, so an element a kernel leaves out shows.  Shapes: the smallest at which tiles, mirrors and chunks can go wrong."""
import numpy as np
import pytest
import torch

import mel_loss_models as LM
from mel_loss_models import FLOOR, HOP, N_FFT, PAD
CASES = LM.ALL_CASES

pytestmark = pytest.mark.gpu
NAN = float("nan")
MEASURED = {}


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _grad_mode():
    """The module differentiates: whatever grad mode an earlier test module left behind, these tests run with it enabled."""
    with torch.enable_grad():
        yield


_FN = {}


def _fn(name):
    from set_amd.vocoder_losses import MelSpectrogramLoss
    if name not in _FN:
        bk = LM.bank(name)
        _FN[name] = MelSpectrogramLoss(bk.hp, mel_basis=bk.mel_basis)
        assert (_FN[name].fe.bin_lo, _FN[name].fe.bin_hi) == (bk.bin_lo, bk.bin_hi)
    return _FN[name]


def _images(fn, dev):
    return fn._images.get((dev,), lambda old: fn._build_images(dev))


def _front(fn):
    from set_amd.melspec import FLAVOURS
    f = FLAVOURS["hifigan"]
    return dict(fn._geometry(), reflect=f["reflect"], clamp_input=f["clamp_input"], mag_eps=f["mag_eps"], sentinel=NAN)


def _note(key, err, bar):
    MEASURED[key] = max(MEASURED.get(key, (0.0, 0.0)), (err / bar if bar else 0.0, err))
    assert err <= bar, (key, err, bar)


def _t(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name,B,n", CASES)
def test_launch_by_launch(dev, name, B, n):
    from set_amd import ops
    d, fn = LM.derived(name, B, n), _fn(name)
    bars, p = d["bars"], d["parts"]
    table, basis, basis_t, itable = _images(fn, dev)
    y_hat, y = _t(d["y_hat"], dev), _t(d["y"], dev)
    # launch 1: the linear mel, and its finished form against set_log_mel
    mel_hat, mel_y = ops.mel_linear(y_hat, table, basis, **_front(fn)), ops.mel_linear(y, table, basis, **_front(fn))
    mh, my = mel_hat.cpu().numpy(), mel_y.cpu().numpy()
    assert np.isfinite(mh).all() and np.isfinite(my).all() and mh.shape == p["mel_hat"].shape
    e_mel = float(max(np.abs(mh - p["mel_hat"]).max(), np.abs(my - p["mel_y"]).max()))
    # launch 2: loss and mel gradient
    loss, g_mel, log_hat, log_y = ops.mel_loss_fwd(mel_hat, mel_y, floor=FLOOR, log_scale=1.0, return_logs=True, sentinel=NAN)
    assert torch.equal(log_hat, fn.fe(y_hat)) and torch.equal(log_y, fn.fe(y))           # bit for bit set_log_mel's
    rl, rg = LM.loss_launch_f32(mh, log_hat.cpu().numpy(), log_y.cpu().numpy())
    assert np.array_equal(_bits(loss), np.array([rl]).view(np.uint32))                      # the documented order, bit for bit
    assert np.array_equal(_bits(g_mel), rg.view(np.uint32))
    e_loss = abs(float(loss) - d["loss"])
    dec = ~d["undecided"]
    e_g = float(np.abs(g_mel.cpu().numpy().astype(np.float64) / dec.size - p["g_mel"])[dec].max())
    # launch 3..5: the spectral backward, inverse and fold on a given mel gradient; the input carries the clamp probe
    w = d["w_probe"]
    _, beyond, at = LM.clamp_probe(d["y_hat"])
    g_wav = ops.mel_loss_bwd(_t(w, dev), _t(d["g_given"], dev), table, basis_t, itable, mag_eps=LM.MAG_EPS, sentinel=NAN,
                             **fn._geometry()).cpu().numpy()
    assert np.isfinite(g_wav).all() and g_wav.shape == (B, n)
    e_w = float(np.abs(g_wav - d["gw_given"]).max())
    assert not g_wav[0, beyond].any() and np.all(g_wav[0, at] != 0)                        # the clamp mask, exact on the input bits
    print("%s B=%d N=%d: linear mel %.3e (bar %.3e), loss %.3e (%.3e), g_mel %.3e (%.3e), g_wav of a given g_mel %.3e (%.3e)" % (
        name, B, n, e_mel, bars["mel"], e_loss, bars["loss"], e_g, bars["g_mel"], e_w, bars["g_wav"]))
    _note("linear mel", e_mel, bars["mel"])
    _note("loss", e_loss, bars["loss"])
    _note("g_mel", e_g, bars["g_mel"])
    _note("g_wav given g_mel", e_w, bars["g_wav"])


def _run(fn, y_hat, y, **kw):
    a = y_hat.clone().requires_grad_(True)
    loss = fn(a, y, sentinel=NAN, **kw)
    return a, loss


@pytest.mark.parametrize("name,B,n", CASES)
def test_end_to_end(dev, name, B, n):
    from set_amd import ops
    d, fn = LM.derived(name, B, n), _fn(name)
    y_hat, y = _t(d["y_hat"], dev), _t(d["y"], dev)
    a, loss = _run(fn, y_hat, y)
    assert loss.shape == () and loss.requires_grad
    loss.backward(retain_graph=True)
    g = a.grad.clone()
    assert g.shape == (B, n) and torch.isfinite(g).all()
    _note("loss (end to end)", abs(float(loss.detach()) - d["loss"]), d["bars"]["loss"])
    # the model with the GPU's own sign / floor choice at the undecided entries (both are admissible there), its own everywhere else
    table, basis, _, _ = _images(fn, dev)
    gm = ops.mel_loss_fwd(ops.mel_linear(y_hat, table, basis, **_front(fn)), ops.mel_linear(y, table, basis, **_front(fn)), floor=FLOOR,
                          log_scale=1.0)[1].cpu().numpy()
    und = d["undecided"]
    assert und.mean() <= LM.UNDECIDED_CAP
    p = d["parts"]
    _, g_mel, _, _ = LM.loss_and_g_mel(p["mel_hat"], p["mel_y"], np.float64, sign=np.where(und, np.sign(gm), np.nan),
                                       passed=np.where(und, (gm != 0).astype(np.int64), -1))
    ref = LM.wave_grad(d["y_hat"], g_mel, d["bank"], np.float64)
    err = float(np.abs(g.cpu().numpy() - ref).max())
    print("%s B=%d N=%d: gradient %.3e (bar %.3e), max |gradient| %.3e, undecided %.2e" % (name, B, n, err, d["bars"]["grad"],
                                                                                           np.abs(ref).max(), und.mean()))
    _note("gradient (end to end)", err, d["bars"]["grad"])
    # a second backward: the same bits
    a.grad = None
    loss.backward()
    assert torch.equal(a.grad, g)
    # a second forward + backward: the same bits
    a2, loss2 = _run(fn, y_hat, y)
    loss2.backward()
    assert torch.equal(loss2, loss) and torch.equal(a2.grad, g)
    # the task's lambda_mel: the upstream scalar scales the gradient, one rounding
    a3, loss3 = _run(fn, y_hat, y)
    (loss3 * 45.0).backward()
    want = g.cpu().numpy().astype(np.float64) * 45.0
    assert np.all(np.abs(a3.grad.cpu().numpy() - want) <= 0.5 * np.spacing(np.abs(want).astype(np.float32)))
    # [B, 1, N] in, [B, 1, N] out
    a4 = y_hat.clone()[:, None, :].requires_grad_(True)
    l4, m_hat, m_y = fn(a4, y[:, None, :], return_mels=True, sentinel=NAN)
    l4.backward()
    assert a4.grad.shape == (B, 1, n) and torch.equal(a4.grad[:, 0], g) and torch.equal(l4, loss)
    assert torch.equal(m_hat, fn.fe(y_hat)) and torch.equal(m_y, fn.fe(y)) and not m_hat.requires_grad
    if B > 1:
        # a row alone, rescaled by the element counts, is the row's gradient within the batch to one rounding of that rescale (the
        # division by the count is the last operation: before it the row's bits do not depend on the batch)
        for r in range(B):
            ar, lr = _run(fn, y_hat[r:r + 1], y[r:r + 1])
            lr.backward()
            want = ar.grad.cpu().numpy().astype(np.float64)[0] / B
            got = g[r].cpu().numpy()
            # half an ulp from each of the two divisions, the first carried over as a relative error: at most 1.5 ulp
            assert np.all(np.abs(got - want) <= 1.5 * np.spacing(np.abs(got))), (r, float(np.abs(got - want).max()))


def test_exact_cases(dev):
    fn = _fn("mel80")
    n = 16 * HOP + 100
    y_hat, y = (np.array(v, copy=True) for v in LM.pair(2, n, seed=2))
    # equal inputs: loss 0.0, gradient exactly zero everywhere
    a, loss = _run(fn, _t(y, dev), _t(y, dev))
    loss.backward()
    assert float(loss.detach()) == 0.0 and not a.grad.cpu().numpy().any() and torch.isfinite(a.grad).all()
    # a silent stretch under the floor, samples beyond and at the clamp's ends
    y_hat[1, 3 * HOP:11 * HOP] = 0.0
    y_hat, beyond, at = LM.clamp_probe(y_hat)                                              # (row 0)
    a, loss = _run(fn, _t(y_hat, dev), _t(y, dev))
    loss.backward()
    g = a.grad.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(float(loss.detach()))                               # every sentinel overwritten
    silent = [t for t in range(LM.n_frames(n)) if t * HOP - PAD >= 3 * HOP and t * HOP - PAD + N_FFT <= 11 * HOP]
    lo, hi = silent[0] * HOP - PAD + N_FFT - HOP, silent[-1] * HOP - PAD + HOP
    assert hi > lo and not g[1, lo:hi].any() and g[1, :lo - N_FFT].all()                   # under silent frames only: exactly 0
    assert not g[0, beyond].any() and np.all(g[0, at] != 0)
    # N = 1000: the padded samples beyond the last frame (mirror samples only, test_mel_loss_reference) add exactly nothing
    from set_amd import ops
    table, basis, basis_t, itable = _images(fn, dev)
    w = LM.pair(1, 1000, seed=1000 % 97)[0]
    gm = LM.given_g_mel(1, 1000, 80)
    got = ops.mel_loss_bwd(_t(w, dev), _t(gm, dev), table, basis_t, itable, mag_eps=LM.MAG_EPS, sentinel=NAN, **fn._geometry()).cpu().numpy()
    g_p = LM.padded_grad(w[0], gm[0], LM.bank("mel80"), np.float64)
    assert (LM.fold(np.where(np.arange(g_p.size) >= 1536, 1.0, 0.0), 1000) > 0).any() and np.isfinite(got).all()
    assert np.abs(got[0] - LM.fold(g_p[:1536], 1000)).max() <= LM.derived("mel80", 1, 1000)["bars"]["g_wav"]


def test_refusals(dev):
    from set_amd.vocoder_losses import MelSpectrogramLoss, mel_l1_loss
    fn = _fn("mel80")
    z = torch.zeros(2, 4096, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(z.cpu(), z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(z, z.cpu())
    with pytest.raises(TypeError):
        fn(z.double(), z)
    with pytest.raises(TypeError):
        fn(z, z.half())
    with pytest.raises(ValueError, match="y is data"):
        fn(z, z.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        fn(torch.zeros(2, 384, device=dev), torch.zeros(2, 384, device=dev))               # N <= pad
    assert float(fn(torch.zeros(2, 385, device=dev), torch.zeros(2, 385, device=dev))) == 0.0
    with pytest.raises(ValueError):
        fn(z, z[:1])
    with pytest.raises(ValueError):
        fn(z[:, None, None], z[:, None, None])
    for over in ({"hop_size": 128}, {"fft_size": 2048, "win_size": 2048}, {"audio_num_mel_bins": 128}):
        with pytest.raises(ValueError):
            MelSpectrogramLoss(dict(LM.HP, **over))
        with pytest.raises(ValueError):
            mel_l1_loss(z, z, dict(LM.HP, **over))
    # the C entries' own refusals: another padding than (n_fft - hop) / 2, a floor of 0
    from set_amd import ops
    from set_amd._lib import SetAmdError
    table, basis, basis_t, itable = _images(fn, dev)
    with pytest.raises(SetAmdError, match="set_mel_loss_bwd"):
        ops.mel_loss_bwd(z, torch.zeros(2, 17, 80, device=dev), table, basis_t, itable, mag_eps=LM.MAG_EPS, **dict(fn._geometry(), pad=512))
    with pytest.raises(SetAmdError, match="set_mel_loss_fwd"):
        ops.mel_loss_fwd(torch.ones(2, 16, 80, device=dev), torch.ones(2, 16, 80, device=dev), floor=0.0, log_scale=1.0)
    with pytest.raises(ValueError):
        ops.mel_loss_bwd(z, torch.zeros(2, 15, 80, device=dev), table, basis_t, itable, mag_eps=LM.MAG_EPS, **fn._geometry())
    a = z.clone().requires_grad_(True)
    with torch.no_grad():
        assert not fn(a, z).requires_grad
    y_hat, y = (_t(v, dev) for v in LM.pair(1, 512, seed=512 % 97))
    assert torch.equal(mel_l1_loss(y_hat, y, LM.HP), fn(y_hat, y))                          # the functional form, same configuration


def test_report_measured_errors():
    """Printed last: the largest error seen per quantity, as a share of its bar (profiles/mel_loss_gpu_accuracy.log quotes them)."""
    for k, (share, err) in sorted(MEASURED.items()):
        print("measured %s: %.3e at %.2f of its bar" % (k, err, share))
    assert all(share <= 1.0 for share, _ in MEASURED.values())
