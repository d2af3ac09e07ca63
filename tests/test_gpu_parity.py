"""GPU parity tests (run on the MI355X box with `-m gpu`): every HIP kernel and the whole path, through the
C ABI, against the CPU oracle on the same seeded inputs and against the committed golden vectors.

Bars: bit-exact for integer/index tensors; fp32 tolerances written next to each check
(north_star: |dmel| < 1e-4 on the final mel)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import base_hparams, load_golden
from oracle import oracle as O
from oracle import weights as Wt

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _maxdiff(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


def test_mfma_fragment_layout(dev):
    from set_amd import ops
    assert ops.selftest_mfma() == 0.0  # exact: small integers/8ths in fp32


# ----------------------------------------------------------------------------------------------------
# generic conv: naive and MFMA vs torch CPU
# ----------------------------------------------------------------------------------------------------
CONV_CASES = [
    # B, Cin, Cout, K, dil, T, extras
    (2, 80, 256, 1, 1, 64, dict(act="relu")),
    (2, 256, 80, 1, 1, 70, dict()),
    (1, 256, 256, 1, 1, 33, dict(pro="div", pro_param=math.sqrt(20.0), act="relu")),
    (2, 192, 384, 5, 1, 50, dict(alpha=5 ** -0.5, act="gelu")),
    (2, 384, 192, 1, 1, 50, dict(res=True, mask=True)),
    (1, 192, 192, 3, 1, 16, dict(mask=True)),
    (3, 7, 33, 3, 2, 29, dict(chan_add=True, res=True)),
    (2, 192, 1, 1, 1, 40, dict(act="softplus", mask=True)),
    (2, 192, 2, 1, 1, 300, dict()),
    (1, 32, 32, 11, 5, 257, dict(pro="lrelu", pro_param=0.1, res=True)),
    (1, 64, 1, 7, 1, 130, dict(pro="lrelu", pro_param=0.01, act="tanh")),
    (2, 256, 1024, 1, 1, 5, dict(act="mish")),
    (1, 256, 512, 3, 4, 90, dict(chan_add=True, res=True)),
    (2, 16, 48, 3, 1, 64, dict(accumulate=True)),
    (2, 512, 256, 3, 1, 130, dict()),                                  # two 256-channel LDS chunks, RB=2
    (1, 300, 200, 7, 3, 97, dict(pro="lrelu", pro_param=0.1, res=True)),  # ragged channels, two chunks
    (2, 512, 192, 1, 1, 64, dict()),
    (1, 128, 128, 11, 5, 300, dict(pro="lrelu", pro_param=0.1)),       # halo 50
    # epilogue paths: batched operands on full row blocks (v1), 4-frame vectors with a partial 16-row group and a
    # ragged tail tile (v2), previous-output accumulation, leaky-ReLU epilogue
    (2, 96, 96, 3, 1, 256, dict(res=True, mask=True, act="relu")),
    (2, 200, 200, 3, 1, 192, dict(res=True, act="relu")),
    (2, 128, 128, 3, 1, 260, dict(res=True, mask=True, accumulate=True)),
    (1, 32, 32, 7, 1, 1000, dict(res=True, accumulate=True, act="lrelu", act_param=0.2)),
    (2, 64, 64, 3, 3, 300, dict(pro="lrelu", pro_param=0.1, res=True, mask=True, alpha=0.5)),
]


def _conv_ref(x, w, b, K, dil, ex, res, mask, add, prev):
    xin = x
    if add is not None:
        xin = xin + add[:, :, None]
    if ex.get("pro") == "lrelu":
        xin = F.leaky_relu(xin, ex["pro_param"])
    elif ex.get("pro") == "div":
        xin = xin / ex["pro_param"]
    pad = dil * (K - 1) // 2
    # the bias / chan_add must not leak into the zero padding: pad AFTER the prologue
    y = F.conv1d(F.pad(xin, (pad, pad)), w, b, dilation=dil)
    y = y * ex.get("alpha", 1.0)
    act = ex.get("act", "none")
    y = {"none": lambda v: v, "relu": F.relu, "gelu": F.gelu, "tanh": torch.tanh, "softplus": F.softplus,
         "mish": O.mish, "lrelu": lambda v: F.leaky_relu(v, ex.get("act_param", 0.0))}[act](y)
    if res is not None:
        y = y + res
    if mask is not None:
        y = y * mask[:, None, :]
    if prev is not None:
        y = prev + y
    return y


@pytest.mark.parametrize("impl", ["naive", "mfma", "mfma2"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv1d_vs_torch(dev, impl, case):
    from set_amd import ops
    B, Cin, Cout, K, dil, T, ex = case
    g = torch.Generator().manual_seed(1000 + Cin * 7 + Cout + K)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, K, generator=g) / math.sqrt(Cin * K)
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, Cout, T, generator=g) if ex.get("res") else None
    mask = (torch.rand(B, T, generator=g) > 0.3).float() if ex.get("mask") else None
    add = torch.randn(B, Cin, generator=g) if ex.get("chan_add") else None
    prev = torch.randn(B, Cout, T, generator=g) if ex.get("accumulate") else None
    ref = _conv_ref(x, w, b, K, dil, ex, res, mask, add, prev)
    wd = w.to(dev)
    cw = ops.ConvWeight(lambda: wd, Cout, Cin, K)
    out = prev.clone().to(dev) if prev is not None else None
    kw = {k: ex[k] for k in ("pro", "pro_param", "act", "act_param", "alpha") if k in ex}
    y = ops.conv1d(x.to(dev), cw, b.to(dev), dil=dil, pad=dil * (K - 1) // 2, res=None if res is None else res.to(dev),
                   mask=None if mask is None else mask.to(dev), in_chan_add=None if add is None else add.to(dev),
                   out=out, accumulate=prev is not None, impl=impl, **kw)
    torch.cuda.synchronize()
    assert _maxdiff(y, ref) < 2e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("impl", ["naive", "mfma"])
@pytest.mark.parametrize("cfg", [(2, 64, 32, 8, 4, 24), (1, 32, 16, 4, 2, 37), (1, 512, 256, 16, 8, 12),
                                 (2, 16, 8, 7, 3, 10)])
def test_conv_transpose_polyphase(dev, impl, cfg):
    from set_amd import ops
    B, Cin, Cout, k, u, T = cfg
    g = torch.Generator().manual_seed(77 + k)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cin, Cout, k, generator=g) / math.sqrt(Cin * k / u)
    b = torch.randn(Cout, generator=g) * 0.1
    P = (k - u) // 2
    ref = F.conv_transpose1d(F.leaky_relu(x, 0.1), w, b, stride=u, padding=P)
    wd = w.to(dev)
    y = ops.conv_transpose1d(x.to(dev), lambda: wd, b.to(dev), Cin, Cout, k, u, P, pro="lrelu", pro_param=0.1,
                             impl=impl)
    torch.cuda.synchronize()
    assert y.shape == ref.shape
    assert _maxdiff(y, ref) < 2e-5 * max(1.0, float(ref.abs().max()))


# ----------------------------------------------------------------------------------------------------
# glue kernels
# ----------------------------------------------------------------------------------------------------
def test_glue_kernels(dev):
    from set_amd import ops
    g = torch.Generator().manual_seed(5)
    B, C, T, Tt = 3, 192, 70, 21
    x = torch.randn(B, C, T, generator=g)
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    mask = (torch.rand(B, T, generator=g) > 0.2).float()
    ref = O.layer_norm_ch(x, gam, bet) * mask[:, None, :]
    assert _maxdiff(ops.layernorm_ch(x.to(dev), gam.to(dev), bet.to(dev), mask.to(dev)), ref) < 1e-5
    idx = torch.randint(0, 50, (B, T), generator=g)
    tab = torch.randn(50, C, generator=g)
    e = ops.embedding_bct(idx.to(dev), tab.to(dev), scale=math.sqrt(C))
    assert _maxdiff(e, (math.sqrt(C) * F.embedding(idx, tab)).transpose(1, 2)) == 0.0
    e2 = ops.embedding_bct(idx.to(dev), tab.to(dev), out=x.to(dev).clone(), accumulate=True)
    assert _maxdiff(e2, x + F.embedding(idx, tab).transpose(1, 2)) == 0.0
    xz = x.clone()
    xz[:, :, 5:9] = 0
    assert _maxdiff(ops.abs_sum_mask(xz.to(dev)), (xz.abs().sum(1) > 0).float()) == 0.0
    assert _maxdiff(ops.index_mask(idx.to(dev)), (idx > 0).float()) == 0.0
    enc = torch.randn(B, C, Tt, generator=g)
    m2p = torch.sort(torch.randint(0, Tt + 1, (B, T), generator=g), dim=1).values
    ref = O.expand_states(enc.transpose(1, 2), m2p).transpose(1, 2)
    assert _maxdiff(ops.expand_states(enc.to(dev), m2p.to(dev)), ref) == 0.0
    add = torch.randn(B, C, generator=g)
    assert _maxdiff(ops.add_chan_mask(x.to(dev), add.to(dev), mask.to(dev)), (x + add[:, :, None]) * mask[:, None]) == 0.0
    bt = torch.randn(B, T, 80, generator=g)
    assert _maxdiff(ops.btc_to_bct(bt.to(dev)), bt.transpose(1, 2)) == 0.0
    assert _maxdiff(ops.bct_to_btc(x.to(dev)), x.transpose(1, 2)) == 0.0
    a, b_, c = (torch.randn(1000, generator=g) for _ in range(3))
    assert _maxdiff(ops.sum_div(a.to(dev), b_.to(dev), c.to(dev), 3.0), ((a + b_) + c) / 3.0) == 0.0
    m1 = (torch.rand(B, T, generator=g) > 0.5).float()
    assert _maxdiff(ops.mul_one_minus_mask(bt.to(dev), m1.to(dev), 80), bt * (1 - m1[:, :, None])) == 0.0
    bt2 = torch.randn(B, T, 80, generator=g)
    assert _maxdiff(ops.blend_mask(bt.to(dev), bt2.to(dev), m1.to(dev), 80),
                    bt * (1 - m1[:, :, None]) + bt2 * m1[:, :, None]) == 0.0


def test_integer_bookkeeping_bit_exact(dev):
    from set_amd import ops
    inp = Wt.synthetic_inputs(4, 120, 30, seed=9, pad_tail=True)
    tm = inp["time_mel_masks"].squeeze(-1)
    ref_md = (O.mel2token_to_dur(inp["mel2ph"] * (1 - inp["time_mel_masks"]).squeeze(-1).long(), 30)
              * (inp["txt_tokens"] != 0).float()).long()
    md = ops.masked_dur(inp["mel2ph"].to(dev), tm.contiguous().to(dev), inp["txt_tokens"].to(dev))
    assert torch.equal(md.cpu(), ref_md)
    pad = inp["mel2ph"] == 0
    ref_den = O.denorm_f0(inp["f0"] * (1 - tm), inp["uv"] * (1 - tm), pad)
    ref_bins = O.f0_to_coarse(ref_den)
    den, bins = ops.pitch_coarse(inp["f0"].to(dev), inp["uv"].to(dev), tmask=tm.contiguous().to(dev),
                                 mel2ph_pad=inp["mel2ph"].to(dev))
    assert torch.equal(bins.cpu(), ref_bins)
    assert _maxdiff(den, ref_den) < 1e-3  # Hz; exp2f vs torch pow(2, x)
    # the bin function against the REFERENCE run committed as tests/golden/pitch_edges.npz (oracle/make_pitch_edges.py: the reference's
    # own functions on every fp32 in [5.0, 10.5], recorded as runs of equal bins + every value within 8 ulp of a run boundary): the
    # edge neighbourhoods, then EVERY fp32 of the sweep (8.9 M values) against the run table -- no mismatch allowed.  (Not against
    # torch-CPU at test time: its pow / log are not correctly rounded and differ BETWEEN host CPUs -- the same oracle code gave
    # 3 other bins of 8.9 M on the GPU box's host than in the container the reference ran in; the committed run is the pin.)
    ge = load_golden("pitch_edges")
    fe = torch.from_numpy(ge["f0_bits"].view(np.float32).copy())
    _, bins = ops.pitch_coarse(fe.to(dev), None)
    assert torch.equal(bins.cpu(), torch.from_numpy(ge["bins"].astype(np.int64)))
    lo, hi = int(np.float32(5.0).view(np.uint32)), int(np.float32(10.5).view(np.uint32))
    allbits = np.arange(lo, hi + 1, dtype=np.uint32)
    want = ge["run_bin"].astype(np.int64)[np.searchsorted(ge["run_bits"], allbits, side="right") - 1]
    _, bins = ops.pitch_coarse(torch.from_numpy(allbits.view(np.float32).copy()).to(dev), None)
    assert int((bins.cpu() != torch.from_numpy(want)).sum()) == 0
    fo = torch.tensor([-1e30, -3.0, 0.0, 4.999, 5.0, 10.5, 10.51, 50.0, 1e30])
    _, bins = ops.pitch_coarse(fo.to(dev), None)
    assert bins.cpu().tolist() == [1, 1, 1, 1, 1, 255, 255, 255, 255]
    g = load_golden("length_regulator")
    txt = torch.from_numpy((~g["pad"]).astype(np.int64))
    out = ops.length_regulate(torch.from_numpy(g["dur"]).to(dev), txt.to(dev))
    assert torch.equal(out.cpu(), torch.from_numpy(g["mel2ph"]))


def test_posterior_qsample_randn(dev):
    from set_amd import ops
    g = torch.Generator().manual_seed(3)
    B, M, T = 3, 80, 37
    tab, _ = O.diffusion_tables(8)
    x0, xt, eps = (torch.randn(B, 1, M, T, generator=g) for _ in range(3))
    t = torch.tensor([0, 3, 7])
    ref = O.q_posterior_sample(tab, x0, xt, t, eps)
    coef = torch.stack([tab["posterior_mean_coef1"][t], tab["posterior_mean_coef2"][t],
                        tab["posterior_log_variance_clipped"][t], (t != 0).float()], -1).contiguous()
    out = torch.empty(B, 1, M, T, device=dev)
    ops.posterior_step(x0.to(dev), xt.to(dev), coef.to(dev), eps=eps.to(dev), out=out)
    assert _maxdiff(out, ref) < 1e-6
    ab = torch.stack([tab["sqrt_alphas_cumprod"][t], tab["sqrt_one_minus_alphas_cumprod"][t]], -1).contiguous()
    assert _maxdiff(ops.q_sample(x0.to(dev), eps.to(dev), ab.to(dev)), O.q_sample(tab, x0, t, eps)) < 1e-6
    z = ops.randn((1 << 20,), dev, seed=7)
    z2 = ops.randn((1 << 20,), dev, seed=7)
    assert torch.equal(z, z2) and not torch.equal(z, ops.randn((1 << 20,), dev, seed=8))
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1.0) < 5e-3
    assert abs(float((z ** 4).mean()) - 3.0) < 0.05


# ----------------------------------------------------------------------------------------------------
# DiffNet: fused layer kernel vs unfused kernels vs golden layer traces
# ----------------------------------------------------------------------------------------------------
def _build_model(dev, manifest, wseed, steps, variant="masked", **over):
    from set_amd.diffnet import DiffNet
    from set_amd import spec_denoiser as SD
    hp = base_hparams(timesteps=steps, **over)
    cls = SD.GaussianDiffusionNormal if variant == "normal" else SD.GaussianDiffusion
    m = cls(list(range(80)), 80, DiffNet(80, hp), timesteps=steps, time_scale=1, loss_type="l1",
                          spec_min=[], spec_max=[], hp=hp)
    W = Wt.seeded_weights(Wt.load_manifest(manifest), wseed)
    missing, unexpected = m.load_state_dict(W, strict=False)
    assert not unexpected and all(Wt.is_buffer(k) for k in missing)
    return m.to(dev).eval(), W


def _case_inputs(g, dev):
    m = g["meta"]
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=m["pad_tail"])
    noises = torch.stack(Wt.synthetic_noises(m["B"], m["T"], m["steps"], seed=m["iseed"] + 1))
    return {k: v.to(dev) for k, v in inp.items()}, noises.to(dev)


def test_diffnet_single_pass_fused_vs_unfused_vs_oracle(dev):
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    dn = model.denoise_fn
    gen = torch.Generator().manual_seed(11)
    B, T = 2, 100  # T not a multiple of the 64-frame tile
    spec = torch.randn(B, 1, 80, T, generator=gen)
    cond = torch.randn(B, 192, T, generator=gen)
    t = torch.tensor([3, 0])
    ref = O.diffnet_forward(W, spec, t, cond)
    dn.impl = "fused"
    y_f = dn(spec.to(dev), t.to(dev), cond.to(dev))
    dn.impl = "unfused"
    y_u = dn(spec.to(dev), t.to(dev), cond.to(dev))
    torch.cuda.synchronize()
    assert _maxdiff(y_u, ref) < 2e-5
    assert _maxdiff(y_f, ref) < 2e-5
    assert _maxdiff(y_f, y_u) < 2e-5


def test_fused_layer_matches_golden_layer_trace(dev):
    """First executed step of infer_tiny: per-layer (x, skip) after layers 0, 1 and 19 from the reference."""
    from set_amd import ops
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    dn = model.denoise_fn
    ret, cond = model.conditioner(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"],
                                  inp["ref_mels"], inp["f0"], inp["uv"])
    steps = m["steps"]
    ids = torch.arange(steps, device=dev)
    dtab = dn.step_table(ids.float())
    condproj = dn.cond_projections(cond)
    x = noises[0, :, 0].contiguous()
    h = ops.conv1d(x, dn._w_in, dn.input_projection.bias.data, act="relu")
    B, C, T = h.shape
    skip = torch.empty_like(h)
    nxt = torch.empty_like(h)
    sid = steps - 1
    for l, layer in enumerate(dn.residual_layers):
        w1p, w2p = layer.fused_weights()
        ops.diffnet_layer(h, condproj[:, l * 512:(l + 1) * 512].data_ptr(), condproj.stride(0),
                          dtab.data_ptr() + 4 * (l * C * steps + sid), 0, steps, w1p, layer.dilated_conv.bias.data,
                          w2p, layer.output_projection.bias.data, nxt, skip, layer.dilation, l == 0)
        h, nxt = nxt, h
        if l in (0, 1, 19):
            torch.cuda.synchronize()
            assert _maxdiff(h, g["layer%d_x" % l]) < 2e-5, l
    # golden skip is the per-layer skip output; ours is the running sum -> check the final sum via x0
    hs = ops.conv1d(skip, dn._w_skip, dn.skip_projection.bias.data, pro="div", pro_param=math.sqrt(20.0), act="relu")
    x0 = ops.conv1d(hs, dn._w_outp, dn.output_projection.bias.data)
    assert _maxdiff(x0[:, None], g["x0_step0"]) < 2e-5


# ----------------------------------------------------------------------------------------------------
# whole path vs golden (reference outputs)
# ----------------------------------------------------------------------------------------------------
FULL = [("infer_tiny", "spec_denoiser", {}), ("infer_pad", "spec_denoiser", {}),
        ("infer_ragged", "spec_denoiser", {}),  # round 5: T = 77, T_txt = 19, three padded tails -- sizes that are multiples of nothing
        ("infer_short", "spec_denoiser", {}),   # round 5: T = 7, T_txt = 3 -- shorter than every tile, halo and MFMA threshold
        ("infer_predpitch", "spec_denoiser", {}), ("infer_drift100", "spec_denoiser", {}),
        ("infer_dil", "spec_denoiser_dil", {}), ("infer_c64", "spec_denoiser_c64", {}),
        ("infer_nopitch", "spec_denoiser_nopitch", {}),  # egs/spec_denoiser_libritts.yaml: use_pitch_embed false
        ("infer_normal", "spec_denoiser_normal", {})]    # egs/spec_denoiser_wo_masked_predictor.yaml


@pytest.mark.parametrize("case,manifest,_", FULL)
def test_full_inference_matches_reference(dev, case, manifest, _):
    g = load_golden(case)
    m = g["meta"]
    model, W = _build_model(dev, manifest, m["wseed"], m["steps"], variant=m.get("variant", "masked"), **m["overrides"])
    inp, noises = _case_inputs(g, dev)
    ret = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                inp["f0"], inp["uv"], infer=True, noises=noises, **m["flags"])
    torch.cuda.synchronize()
    # integer / index tensors: bit exact
    assert torch.equal(ret["mel2ph"].cpu(), torch.from_numpy(g["mel2ph"]))
    if "masked_dur" in g:
        assert torch.equal(ret["masked_dur"].cpu(), torch.from_numpy(g["masked_dur"]))
    else:  # `normal` variant: no masked predictor inputs, no dur_embed (modules/tts/fs.py)
        assert "masked_dur" not in ret and "fs.dur_embed.weight" not in model.state_dict()
    # conditioner floats
    assert _maxdiff(ret["decoder_inp"], g["decoder_inp"]) < 2e-5
    assert _maxdiff(ret["dur"], g["dur"]) < 2e-5
    if "pitch_pred" in g:
        if "masked_pitch" in g:
            assert torch.equal(ret["masked_pitch"].cpu(), torch.from_numpy(g["masked_pitch"]))
        assert torch.equal(ret["pitch"].cpu(), torch.from_numpy(g["pitch"]))
        assert _maxdiff(ret["pitch_pred"], g["pitch_pred"]) < 5e-5
        assert _maxdiff(ret["f0_denorm"], g["f0_denorm"]) < 1e-3
    else:  # no pitch block (fs.py:97-99 skipped): the reference returns none of the pitch keys
        assert not ({"pitch_pred", "pitch", "masked_pitch", "f0_denorm", "f0_denorm_pred"} & set(ret))
        assert not any(k.startswith("fs.pitch_") for k in model.state_dict())
    # the bar: |dmel| < 1e-4 (fp32) after the whole reverse loop
    d = _maxdiff(ret["mel_out"], g["mel_out"])
    mcd = O.mel_mcd(ret["mel_out"].cpu().numpy(), g["mel_out"])
    print("%s: max|dmel| = %.3e  mel-MCD = %.3e" % (case, d, mcd))
    assert d < 1e-4
    assert mcd < 1e-3


def test_unfused_loop_matches_fused(dev):
    g = load_golden("infer_pad")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    model.denoise_fn.impl = "unfused"
    r_u = model(*args, infer=True, noises=noises)
    model.denoise_fn.impl = "fused"
    r_f = model(*args, infer=True, noises=noises)
    assert _maxdiff(r_u["mel_out"], g["mel_out"]) < 1e-4
    assert _maxdiff(r_f["mel_out"], r_u["mel_out"]) < 1e-4


def test_persistent_stack_bit_identical_to_layer_launches(dev):
    """set_diffnet_stack (task queue + ready flags across CUs/XCDs) must reproduce L per-layer launches bit for bit,
    repeatedly, at the full benchmark size (uneven load, L1-warm consumers: every tile re-reads buffers it read two
    layers earlier) and at ragged sizes; sync_ws[1] (timeout flag) must stay 0."""
    from set_amd import ops
    for (B, T, L, dcl, reps) in ((32, 800, 20, 1, 6), (3, 130, 5, 3, 3), (1, 50, 2, 1, 2)):
        g = torch.Generator().manual_seed(B * 1000 + T)
        x0 = torch.randn(B, 256, T, generator=g).to(dev)
        cp = (torch.randn(B, L * 512, T, generator=g) * 0.5).to(dev)
        dtab = torch.randn(L * 256, 3, generator=g).to(dev)
        w1 = torch.empty(L, 512 * 768, device=dev)
        w2 = torch.empty(L, 512 * 256, device=dev)
        bd = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
        bo = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
        for l in range(L):
            wd = (torch.randn(512, 256, 3, generator=g) / 27.7).to(dev)
            wo = (torch.randn(512, 256, 1, generator=g) / 16.0).to(dev)
            ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        col = 1
        # reference: L launches of the per-layer kernel
        h, nxt, skip_ref = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        for l in range(L):
            ops.diffnet_layer(h, cp[:, l * 512:(l + 1) * 512].data_ptr(), cp.stride(0),
                              dtab.data_ptr() + 4 * (l * 256 * 3 + col), 0, 3, w1[l], bd[l], w2[l], bo[l], nxt, skip_ref,
                              1 << (l % dcl), l == 0)
            h, nxt = nxt, h
        x_ref = h.clone()
        torch.cuda.synchronize()
        for rep in range(reps):
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4 * col, 0, 3, 256 * 3, ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo), dcl)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            assert int(ws[0]) >= L * B * ((T + 63) // 64)
            assert torch.equal(skip, skip_ref), (B, T, rep)
            assert torch.equal(xb if L % 2 else xa, x_ref), (B, T, rep)


def test_row_split_stack_bit_identical_to_layer_launches(dev, monkeypatch):
    """Small batches: every 32-frame tile of set_diffnet_stack is computed by four co-operating blocks (one 32-row block
    per wave, z exchanged through L2, two counter rendezvous per layer).  Same accumulation chains as the per-layer
    kernel -> bit-identical, run after run (a stale z or neighbour read would change bits), at one utterance of the
    benchmark length, at ragged lengths, with dilations 1..8, and the time-out flag stays 0."""
    from set_amd import ops
    for (B, T, L, dcl, reps) in ((1, 800, 20, 1, 8), (4, 800, 20, 1, 3), (2, 333, 6, 4, 3), (1, 31, 3, 2, 2), (5, 200, 4, 3, 2),
                                 (1, 1548, 3, 1, 1), (1, 1, 2, 1, 1)):
        g = torch.Generator().manual_seed(B * 1000 + T + 7)
        x0 = torch.randn(B, 256, T, generator=g).to(dev)
        cp = (torch.randn(B, L * 512, T, generator=g) * 0.5).to(dev)
        dtab = torch.randn(L * 256, 3, generator=g).to(dev)
        w1 = torch.empty(L, 512 * 768, device=dev)
        w2 = torch.empty(L, 512 * 256, device=dev)
        bd = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
        bo = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
        for l in range(L):
            wd = (torch.randn(512, 256, 3, generator=g) / 27.7).to(dev)
            wo = (torch.randn(512, 256, 1, generator=g) / 16.0).to(dev)
            ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        w1s, w2s = ops.split_images(w1, w2)
        packs = ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo, w1s=w1s, w2s=w2s)
        col = 2
        h, nxt, skip_ref = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        for l in range(L):
            ops.diffnet_layer(h, cp[:, l * 512:(l + 1) * 512].data_ptr(), cp.stride(0),
                              dtab.data_ptr() + 4 * (l * 256 * 3 + col), 0, 3, w1[l], bd[l], w2[l], bo[l], nxt, skip_ref,
                              1 << (l % dcl), l == 0)
            h, nxt = nxt, h
        x_ref = h.clone()
        monkeypatch.setenv("SET_AMD_SPLIT", "2")
        assert ops.stack_variant(B, T, dcl, x3_mode=0) == 3
        for rep in range(reps):
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4 * col, 0, 3, 256 * 3, packs, dcl)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            assert torch.equal(skip, skip_ref), (B, T, rep)
            assert torch.equal(xb if L % 2 else xa, x_ref), (B, T, rep)
        monkeypatch.delenv("SET_AMD_SPLIT")
    # too many tiles for co-residency: the queue kernels take over
    assert ops.stack_variant(8, 800, 1) != 3


def test_row_split_f16x2_stack_bit_identical_to_split_operand_kernel(dev, monkeypatch):
    """Small batches with two-piece fp16 images: the row-split scheme runs on the split operands (one accumulator per wave,
    z exchanged already split).  Same products in the same order per accumulator as the throughput kernel -> bit-identical
    to it, run after run, at one utterance of the benchmark length, ragged lengths, dilations 1..8; no time-out."""
    from set_amd import ops
    for (B, T, L, dcl, reps) in ((1, 800, 20, 1, 6), (2, 333, 6, 4, 3), (1, 31, 3, 2, 2), (3, 200, 4, 3, 2), (1, 1548, 3, 1, 1),
                                 (1, 1, 2, 1, 1)):
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, B * 1000 + T + 3, 2)
        col = 2

        def run():
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4 * col, 0, 3, 256 * 3, packs, dcl)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            return (xb if L % 2 else xa).clone(), skip.clone()

        monkeypatch.setenv("SET_AMD_SPLIT", "0")
        monkeypatch.setenv("SET_AMD_X3", "2")
        assert ops.stack_variant(B, T, dcl, x3_mode=2) == 5
        x_ref, s_ref = run()
        monkeypatch.setenv("SET_AMD_SPLIT", "2")
        assert ops.stack_variant(B, T, dcl, x3_mode=2) == 3
        for rep in range(reps):
            x, sk = run()
            assert torch.equal(sk, s_ref), (B, T, rep)
            assert torch.equal(x, x_ref), (B, T, rep)
        monkeypatch.setenv("SET_AMD_SPLIT_F32", "1")  # the fp32-pipe row-split kernel on the same inputs: fp32 rounding apart
        x32, s32 = run()
        assert _maxdiff(x32, x_ref) < 1e-5 * max(1.0, float(x_ref.abs().max()))
        monkeypatch.delenv("SET_AMD_SPLIT_F32")
    monkeypatch.delenv("SET_AMD_SPLIT")
    monkeypatch.delenv("SET_AMD_X3")


def test_row_split_timeout_is_reported(dev, monkeypatch):
    """Same error contract as the queue kernels: a part that never publishes (SET_AMD_FAULT_TILE) makes its neighbours
    give up after the spin limit, every block leaves, the reverse loop raises; the next call works."""
    from set_amd._lib import SetAmdError
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    monkeypatch.setenv("SET_AMD_SPLIT", "2")
    monkeypatch.setenv("SET_AMD_FAULT_TILE", "0")
    with pytest.raises(SetAmdError, match="timed out"):
        model(*args, infer=True, noises=noises)
    monkeypatch.delenv("SET_AMD_FAULT_TILE")
    ok = model(*args, infer=True, noises=noises)["mel_out"]
    assert _maxdiff(ok, g["mel_out"]) < 1e-4


def _random_stack(dev, B, T, L, seed, x3_mode=3):
    """Random layer stack: unpacked weights (for references) + every packed image set_diffnet_stack can use."""
    from set_amd import ops
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 256, T, generator=g).to(dev)
    cp = (torch.randn(B, L * 512, T, generator=g) * 0.5).to(dev)
    dtab = torch.randn(L * 256, 3, generator=g).to(dev)
    w1 = torch.empty(L, 512 * 768, device=dev)
    w2 = torch.empty(L, 512 * 256, device=dev)
    wx3 = ops.SplitOperandImages(L, x3_mode, dev)
    bd = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
    bo = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
    wds, wos = [], []
    for l in range(L):
        wd = (torch.randn(512, 256, 3, generator=g) / 27.7).to(dev)
        wo = (torch.randn(512, 256, 1, generator=g) / 16.0).to(dev)
        ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        wx3.pack(l, wd, wo)
        wds.append(wd), wos.append(wo)
    w1s, w2s = ops.split_images(w1, w2)
    packs = ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo, w1s=w1s, w2s=w2s, wx3=wx3)
    return x0, cp, dtab, packs, wds, wos, bd, bo


@pytest.mark.parametrize("x3_mode", [2, 3])
def test_x3_stack_matches_fp32_stack_and_fp64(dev, monkeypatch, x3_mode):
    """The split-operand kernel (every fp32 operand = two fp16 / three bf16 pieces, three / six 16-bit MFMAs per product,
    fp32 accumulate) against the fp32-MFMA direct kernel on the same weights: equal to fp32 rounding, run-to-run
    bit-identical, no time-out; and against an fp64 evaluation of the same layers (diffnet.py:60-81): its error is not
    larger than the fp32 kernel's (bf16x3) / than 1.5 x the fp32 kernel's (f16x2) -- an fp32-equivalent path, not a
    reduced-precision one."""
    from set_amd import ops
    import torch.nn.functional as F
    for (B, T, L, dcl, reps) in ((32, 800, 20, 1, 3), (3, 203, 5, 3, 2), (2, 65, 3, 1, 2), (1, 1, 2, 1, 1), (5, 66, 8, 4, 2),
                                 (2, 1548, 2, 2, 1), (2, 800, 20, 1, 1)):  # the last one: full depth and length, vs fp64
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, B * 1000 + T + 11, x3_mode)
        col = 1

        def run(x3):
            monkeypatch.setenv("SET_AMD_X3", x3)
            monkeypatch.setenv("SET_AMD_SPLIT", "0")
            assert ops.stack_variant(B, T, dcl, have_wino=False, x3_mode=x3_mode) == (
                (7 - x3_mode) if x3 == "2" else (0 if B * ((T + 63) // 64) >= 768 else 1))
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4 * col, 0, 3, 256 * 3, packs, dcl)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            return (xb if L % 2 else xa).clone(), skip.clone()

        x_ref, s_ref = run("0")
        first = None
        for rep in range(reps):
            x, sk = run("2")
            assert _maxdiff(x, x_ref) < 1e-5 * max(1.0, float(x_ref.abs().max())), (B, T)
            assert _maxdiff(sk, s_ref) < 1e-5 * max(1.0, float(s_ref.abs().max())), (B, T)
            if first is None:
                first = (x, sk)
            assert torch.equal(x, first[0]) and torch.equal(sk, first[1]), (B, T, rep)
        if B * T <= 2048:  # fp64 evaluation on the device
            xd, skd = x0.double(), torch.zeros_like(x0, dtype=torch.float64)
            for l in range(L):
                d = 1 << (l % dcl)
                dv = dtab[l * 256:(l + 1) * 256, col].double()[None, :, None]
                y = F.conv1d(xd + dv, wds[l].double(), bd[l].double(), padding=d, dilation=d) + cp[:, l * 512:(l + 1) * 512].double()
                z = torch.sigmoid(y[:, :256]) * torch.tanh(y[:, 256:])
                o = F.conv1d(z, wos[l].double(), bo[l].double())
                xd, skd = (xd + o[:, :256]) / 2 ** 0.5, skd + o[:, 256:]
            e32 = max(float((x_ref.double() - xd).abs().max()), float((s_ref.double() - skd).abs().max()))
            e3 = max(float((first[0].double() - xd).abs().max()), float((first[1].double() - skd).abs().max()))
            print("stack (%d, %d, L=%d): max err vs fp64: fp32 kernel %.3e, split-operand kernel (mode %d) %.3e" % (
                B, T, L, e32, x3_mode, e3))
            assert e3 < (1.0 if x3_mode == 3 else 1.5) * e32 + 1e-7, (B, T, e3, e32)
    monkeypatch.delenv("SET_AMD_X3")
    monkeypatch.delenv("SET_AMD_SPLIT")


@pytest.mark.parametrize("x3_mode", [2, 3])
def test_x3_stack_tile_widths_agree_bit_for_bit(dev, monkeypatch, x3_mode):
    """The split-operand kernel with 32-frame tiles (batches that leave most CUs without a 64-frame tile) computes every
    output element with the same products in the same order as with 64-frame tiles: bit-identical."""
    from set_amd import ops
    monkeypatch.setenv("SET_AMD_X3", "2")
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_X3_WINO", "0")  # the direct form on both widths (round 6: 64-frame tiles default to the Winograd form of GEMM 1)
    for (B, T, L, dcl) in ((8, 800, 20, 1), (3, 203, 5, 3), (1, 1, 2, 1), (5, 66, 8, 4), (2, 1548, 2, 2)):
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, B * 100 + T + 9, x3_mode)
        outs = []
        for tile in ("64", "32"):
            monkeypatch.setenv("SET_AMD_X3_TILE", tile)
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, dcl)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0
            outs.append(((xb if L % 2 else xa).clone(), skip.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (B, T)
    monkeypatch.delenv("SET_AMD_X3_TILE")


@pytest.mark.parametrize("x3_mode", [2, 3])
def test_x3_stack_worker_counts_agree_bit_for_bit(dev, monkeypatch, x3_mode):
    """The persistent split-operand kernel with its default worker count against 7 workers and 512 workers (more workers than
    CUs): the same images, the same products in the same order per accumulator -- bit-identical, for both tile widths, ragged
    lengths and utterance boundaries inside a tile (the dependency protocol must not depend on who runs which task)."""
    from set_amd import ops
    monkeypatch.setenv("SET_AMD_X3", "2")
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    for (B, T, L, dcl, tile) in ((8, 800, 20, 1, "64"), (3, 203, 5, 1, "32"), (1, 1, 2, 1, "64"), (5, 66, 8, 2, "64"),
                                 (2, 1548, 3, 1, "32"), (32, 800, 4, 1, "64")):
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, B * 100 + T + 11, x3_mode)
        monkeypatch.setenv("SET_AMD_X3_TILE", tile)
        outs = []
        for grid in (None, "7", "512"):
            if grid is None:
                monkeypatch.delenv("SET_AMD_STACK_GRID", raising=False)
            else:
                monkeypatch.setenv("SET_AMD_STACK_GRID", grid)
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, dcl)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0
            outs.append(((xb if L % 2 else xa).clone(), skip.clone()))
        for o in outs[1:]:
            assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), (B, T)
    for k in ("SET_AMD_X3_TILE", "SET_AMD_STACK_GRID"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("split", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("case", ["infer_tiny", "infer_pad", "infer_ragged", "infer_short", "infer_drift100", "infer_dil"])
def test_full_inference_matches_reference_with_split_operand_kernel_forced(dev, monkeypatch, case, split):
    """The parity bar (|dmel| < 1e-4 against the reference's output, 100-step drift case included) with every DiffNet
    stack pass on the split-operand kernel (these small batches would otherwise take the row-split fp32 kernel)."""
    monkeypatch.setenv("SET_AMD_X3", "2")
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_SPLIT_OPERAND", split)
    g = load_golden(case)
    m = g["meta"]
    manifest = "spec_denoiser_dil" if case == "infer_dil" else "spec_denoiser"
    model, W = _build_model(dev, manifest, m["wseed"], m["steps"], **m["overrides"])
    inp, noises = _case_inputs(g, dev)
    ret = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                inp["f0"], inp["uv"], infer=True, noises=noises, persistent=True, **m["flags"])
    torch.cuda.synchronize()
    d = _maxdiff(ret["mel_out"], g["mel_out"])
    monkeypatch.setenv("SET_AMD_X3", "0")
    ret0 = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                 inp["f0"], inp["uv"], infer=True, noises=noises, persistent=True, **m["flags"])
    d0 = _maxdiff(ret0["mel_out"], g["mel_out"])
    print("%s: max|dmel| vs the reference: split-operand kernel (%s) %.3e, fp32 kernel %.3e" % (case, split, d, d0))
    assert d < 1e-4
    assert _maxdiff(ret["mel_out"], ret0["mel_out"]) < 5e-5


def test_f16x2_range_guard_is_loud(dev, monkeypatch):
    """fp16 pieces cover |x| < 65504: an activation beyond 32768 must raise (sticky error word 2), never overflow silently;
    the bf16x3 splitting has fp32's range and runs the same input."""
    from set_amd import ops
    B, T, L = 2, 130, 2
    for mode in (2, 3):
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, 99, mode)
        x0[1, 7, 60] = 5.0e4
        monkeypatch.setenv("SET_AMD_X3", "2")
        monkeypatch.setenv("SET_AMD_SPLIT", "0")
        xa, xb, skip = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        from set_amd import _lib
        a_err = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, 1, err_flag=a_err)
        torch.cuda.synchronize()
        assert int(ws[1]) == 0
        assert int(a_err) == (2 if mode == 2 else 0)
        if mode == 3:
            assert torch.isfinite(xa).all() and torch.isfinite(skip).all()
    monkeypatch.delenv("SET_AMD_X3")
    monkeypatch.delenv("SET_AMD_SPLIT")


def test_f16x2_range_fallback_repeats_the_loop_on_bf16x3(dev, monkeypatch):
    """End to end: weights that drive the residual stream beyond the fp16 range make the two-piece kernel flag the loop;
    GaussianDiffusion.forward then repeats it from x_T with the three-piece bf16 splitting (fp32 range) and returns exactly
    what a run pinned to that splitting returns -- never an overflowed mel."""
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"])
    with torch.no_grad():
        model.denoise_fn.input_projection.weight.mul_(2.0e5)
    from set_amd import ops
    ops.bump_weights_epoch()
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_X3", "2")
    monkeypatch.setenv("SET_AMD_SPLIT_OPERAND", "bf16x3")
    ref = model(*args, infer=True, noises=noises)["mel_out"]
    monkeypatch.setenv("SET_AMD_SPLIT_OPERAND", "f16x2")
    with pytest.warns(UserWarning, match="fp16 split range"):
        out = model(*args, infer=True, noises=noises)["mel_out"]
    assert torch.isfinite(out).all()
    # (with activations of 1e5 the net is ill-conditioned -- kernels with different rounding drift apart -- so the check is
    # against the kernel the fallback is supposed to have run, bit for bit)
    assert torch.equal(out, ref)


def test_split_operand_timeout_is_reported(dev, monkeypatch):
    from set_amd._lib import SetAmdError
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    monkeypatch.setenv("SET_AMD_X3", "2")
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_FAULT_TILE", "0")
    with pytest.raises(SetAmdError, match="timed out"):
        model(*args, infer=True, noises=noises)
    monkeypatch.delenv("SET_AMD_FAULT_TILE")
    ok = model(*args, infer=True, noises=noises)["mel_out"]
    assert _maxdiff(ok, g["mel_out"]) < 1e-4


def test_winograd_stack_matches_direct_stack(dev, monkeypatch):
    """The Winograd F(2,3) persistent kernel (4 GEMMs over output pairs, filter transform folded into the packed
    weights) against the direct persistent kernel on the same weights: equal to fp32 rounding (not bit for bit: the
    summation order differs), run-to-run bit-identical, no dependency time-out.  (32, 800, 20) takes the Winograd
    path by default (more 64-frame tiles than CUs); the small ragged cases force it (odd T, one-frame tail tile)."""
    from set_amd import ops
    # even T >= 64: cross-utterance tiling (boundaries inside tiles at offsets 32, 2, 62, 0/64 ...); odd / short T: per
    # utterance tiles
    for (B, T, L, reps) in ((32, 800, 20, 4), (3, 203, 5, 2), (2, 65, 3, 2), (1, 1, 2, 1), (5, 66, 4, 2), (4, 64, 3, 2),
                            (7, 126, 3, 2), (3, 1548, 2, 1), (6, 96, 3, 2)):
        g = torch.Generator().manual_seed(B * 1000 + T)
        x0 = torch.randn(B, 256, T, generator=g).to(dev)
        cp = (torch.randn(B, L * 512, T, generator=g) * 0.5).to(dev)
        dtab = torch.randn(L * 256, 3, generator=g).to(dev)
        w1 = torch.empty(L, 512 * 768, device=dev)
        w2 = torch.empty(L, 512 * 256, device=dev)
        w1w = torch.empty(L, 512 * 256 * 4, device=dev)
        w2w = torch.empty(L, 512 * 256, device=dev)
        bd = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
        bo = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
        for l in range(L):
            wd = (torch.randn(512, 256, 3, generator=g) / 27.7).to(dev)
            wo = (torch.randn(512, 256, 1, generator=g) / 16.0).to(dev)
            ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
            ops.pack_diffnet_layer_wino(wd, wo, w1w[l], w2w[l])
        packs = ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo, w1w=w1w, w2w=w2w)

        def run(mode):
            monkeypatch.setenv("SET_AMD_WINO", mode)
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, 1)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            return (xb if L % 2 else xa).clone(), skip.clone(), int(ws[0])

        x_ref, s_ref, _ = run("0")
        first = None
        for rep in range(reps):
            x, sk, claimed = run("2")
            assert claimed >= L * min(B * ((T + 63) // 64), (B * T + 63) // 64)  # per-utterance or concatenated tiling
            assert _maxdiff(x, x_ref) < 1e-5 * max(1.0, float(x_ref.abs().max())), (B, T)
            assert _maxdiff(sk, s_ref) < 1e-5 * max(1.0, float(s_ref.abs().max())), (B, T)
            if first is None:
                first = (x, sk)
            assert torch.equal(x, first[0]) and torch.equal(sk, first[1]), (B, T, rep)
    # dilated stacks (dilation_cycle_length 2..4: d = 1, 2, 4, 8 per layer): the F(2,3) pairing runs over frames d apart
    for dcl, Ld in ((2, 4), (3, 6), (4, 8)):
        monkeypatch.setenv("SET_AMD_WINO", "2")
        xa, xb, skip = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        pk = ops.StackImages(**{k: (p[:Ld] if p is not None else None) for k, p in packs._asdict().items()})
        ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, pk, dcl)
        monkeypatch.setenv("SET_AMD_WINO", "0")
        ya, yb, skip2 = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        ops.diffnet_stack(ya, yb, skip2, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, pk, dcl)
        torch.cuda.synchronize()
        assert _maxdiff(skip, skip2) < 1e-5 * max(1.0, float(skip2.abs().max())), dcl
        assert _maxdiff(xa if Ld % 2 == 0 else xb, ya if Ld % 2 == 0 else yb) < 1e-5 * max(1.0, float(ya.abs().max())), dcl


def test_dependency_timeout_is_reported_not_swallowed(dev, monkeypatch):
    """Error behaviour of the persistent kernel: if a producer tile is never published (test hook SET_AMD_FAULT_TILE)
    its consumers give up after the spin limit, every block drains, and the reverse loop raises instead of returning
    a mel computed from garbage.  The next call (hook removed) works again."""
    from set_amd._lib import SetAmdError
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    monkeypatch.setenv("SET_AMD_WINO", "2")
    monkeypatch.setenv("SET_AMD_FAULT_TILE", "0")
    with pytest.raises(SetAmdError, match="timed out"):
        model(*args, infer=True, noises=noises)
    monkeypatch.delenv("SET_AMD_FAULT_TILE")
    ok = model(*args, infer=True, noises=noises)["mel_out"]
    assert _maxdiff(ok, g["mel_out"]) < 1e-4


def test_winograd_stack_soak_is_bit_stable(dev, monkeypatch):
    """The publish protocol of the Winograd kernel (agent-scope write-through stores + vmcnt drain + relaxed flag store,
    acquire on the consumer side) under many launches and different worker counts: every run must be bit-identical
    to the first one -- a stale read of a neighbour tile would show up as a different result -- and no dependency wait
    may time out."""
    from set_amd import ops
    B, T, L = 32, 800, 20
    g = torch.Generator().manual_seed(4242)
    x0 = torch.randn(B, 256, T, generator=g).to(dev)
    cp = (torch.randn(B, L * 512, T, generator=g) * 0.5).to(dev)
    dtab = torch.randn(L * 256, 1, generator=g).to(dev)
    w1 = torch.empty(L, 512 * 768, device=dev)
    w2 = torch.empty(L, 512 * 256, device=dev)
    w1w = torch.empty(L, 512 * 256 * 4, device=dev)
    w2w = torch.empty(L, 512 * 256, device=dev)
    bd = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
    bo = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
    for l in range(L):
        wd = (torch.randn(512, 256, 3, generator=g) / 27.7).to(dev)
        wo = (torch.randn(512, 256, 1, generator=g) / 16.0).to(dev)
        ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        ops.pack_diffnet_layer_wino(wd, wo, w1w[l], w2w[l])
    packs = ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo, w1w=w1w, w2w=w2w)
    ref = None
    n_runs = 0
    for grid in (None, "256", "200", "131", "64"):
        if grid is None:
            monkeypatch.delenv("SET_AMD_STACK_GRID", raising=False)
        else:
            monkeypatch.setenv("SET_AMD_STACK_GRID", grid)
        for rep in range(40 if grid is None else 12):
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr(), 0, 1, 256, packs, 1)
            if rep % 8 == 0:
                torch.cuda.synchronize()
                assert int(ws[1]) == 0, "dependency wait timed out"
            out = (xa, skip)
            if ref is None:
                torch.cuda.synchronize()
                ref = (xa.clone(), skip.clone())
                assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all()
            else:
                assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]), (grid, rep)
            n_runs += 1
    monkeypatch.delenv("SET_AMD_STACK_GRID", raising=False)
    assert n_runs == 88


@pytest.mark.parametrize("case", ["infer_tiny", "infer_pad", "infer_ragged", "infer_short", "infer_drift100", "infer_dil"])
def test_full_inference_matches_reference_with_winograd_forced(dev, monkeypatch, case):
    """The parity bar (|dmel| < 1e-4 against the reference's output) with every DiffNet stack pass on the Winograd
    kernel (small batches would otherwise use the direct kernel)."""
    monkeypatch.setenv("SET_AMD_WINO", "2")
    g = load_golden(case)
    m = g["meta"]
    manifest = "spec_denoiser_dil" if case == "infer_dil" else "spec_denoiser"
    model, W = _build_model(dev, manifest, m["wseed"], m["steps"], **m["overrides"])
    inp, noises = _case_inputs(g, dev)
    ret = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                inp["f0"], inp["uv"], infer=True, noises=noises, persistent=True, **m["flags"])
    torch.cuda.synchronize()
    d = _maxdiff(ret["mel_out"], g["mel_out"])
    print("%s (winograd): max|dmel| = %.3e" % (case, d))
    assert d < 1e-4
    monkeypatch.setenv("SET_AMD_WINO", "0")
    ret0 = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                 inp["f0"], inp["uv"], infer=True, noises=noises, persistent=True, **m["flags"])
    assert _maxdiff(ret["mel_out"], ret0["mel_out"]) < 5e-5


@pytest.mark.parametrize("case", ["infer_pad", "infer_tiny"])
def test_fused_step_boundary_equals_separate_kernels(dev, monkeypatch, case):
    """One launch per step for skip-projection + output-projection + posterior update + next input projection
    (T % 4 == 0) against the four separate kernels: same arithmetic order -> bit-identical, with explicit noise and
    with the on-device Philox stream (same quad numbering)."""
    g = load_golden(case)
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    assert m["T"] % 4 == 0
    out = {}
    monkeypatch.setenv("SET_AMD_BOUNDARY_X2", "0")  # the fp32 MFMA boundary kernel (the split-operand one: next test)
    for mode in ("1", "0"):
        monkeypatch.setenv("SET_AMD_FUSED_BOUNDARY", mode)
        out[mode] = (model(*args, infer=True, noises=noises)["mel_out"], model(*args, infer=True, seed=11)["mel_out"],
                     model(*args, infer=True, noises=noises, persistent=False)["mel_out"])
    assert _maxdiff(out["1"][0], g["mel_out"]) < 1e-4
    for a, b in zip(out["1"], out["0"]):
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("case", ["infer_pad", "infer_tiny", "infer_drift100"])
def test_split_operand_step_boundary(dev, monkeypatch, case):
    """The fused step boundary on two-piece fp16 operands (what the loop runs whenever the layer stack does) against the
    fp32 MFMA boundary kernel on the same stack kernel, and against the reference: same parity bar, explicit noise and the
    Philox stream (identical noise either way)."""
    g = load_golden(case)
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    for forced in ("0", "2"):  # row-split kernel (small batch) and the throughput kernel
        monkeypatch.setenv("SET_AMD_SPLIT", "2" if forced == "0" else "0")
        monkeypatch.setenv("SET_AMD_X3", forced if forced == "2" else "1")
        monkeypatch.setenv("SET_AMD_BOUNDARY_X2", "1")
        a, ap = model(*args, infer=True, noises=noises)["mel_out"], model(*args, infer=True, seed=11)["mel_out"]
        monkeypatch.setenv("SET_AMD_BOUNDARY_X2", "0")
        b, bp = model(*args, infer=True, noises=noises)["mel_out"], model(*args, infer=True, seed=11)["mel_out"]
        assert not torch.equal(a, b)  # (the switch does switch kernels)
        assert _maxdiff(a, b) < 2e-5 and _maxdiff(ap, bp) < 2e-5
        assert _maxdiff(a, g["mel_out"]) < 1e-4


def test_loop_persistent_equals_per_layer_launches(dev, monkeypatch):
    """fp32-pipe kernels pinned (SET_AMD_X3=0, SET_AMD_SPLIT_F32=1): the persistent loop, with and without utterance
    groups, is bit-identical to one launch per layer.  The default kernels (split operands) agree to fp32 rounding."""
    g = load_golden("infer_pad")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    dflt = model(*args, infer=True, noises=noises, persistent=True)["mel_out"]
    monkeypatch.setenv("SET_AMD_X3", "0")
    monkeypatch.setenv("SET_AMD_SPLIT_F32", "1")
    a = model(*args, infer=True, noises=noises, persistent=False)["mel_out"]
    b = model(*args, infer=True, noises=noises, persistent=True)["mel_out"]
    c = model(*args, infer=True, noises=noises, persistent=True, n_groups=2)["mel_out"]
    assert torch.equal(a, b) and torch.equal(a, c)
    assert _maxdiff(a, g["mel_out"]) < 1e-4
    assert _maxdiff(dflt, g["mel_out"]) < 1e-4 and _maxdiff(dflt, a) < 2e-5


def test_utterance_groups_do_not_change_results(dev):
    """set_diffusion_loop(n_groups=g): chains on auxiliary streams, bit-identical output incl. the Philox noise."""
    g = load_golden("infer_pad")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
            inp["uv"])
    base = model(*args, infer=True, noises=noises, n_groups=1)["mel_out"]
    assert _maxdiff(base, g["mel_out"]) < 1e-4
    for ng in (2, 3):
        assert torch.equal(model(*args, infer=True, noises=noises, n_groups=ng)["mel_out"], base)
    p1 = model(*args, infer=True, seed=5, n_groups=1)["mel_out"]
    p3 = model(*args, infer=True, seed=5, n_groups=3, want_layer_spans=True)
    assert torch.equal(p3["mel_out"], p1) and len(p3["layer_span_ms"]) == m["steps"] and p3["loop_ms"] > 0
    assert not torch.equal(model(*args, infer=True, seed=6, n_groups=3)["mel_out"], p1)


def test_train_branch_forward(dev):
    g = load_golden("train_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"])
    inp = {k: v.to(dev) for k, v in Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True).items()}
    ret = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
                inp["uv"], infer=False, t=torch.from_numpy(g["t"]).to(dev), noises=torch.from_numpy(g["eps"]).to(dev))
    assert _maxdiff(ret["x_t"][:, None], g["x_t"]) < 1e-6
    assert _maxdiff(ret["mel_out"], g["mel_out"]) < 5e-5


def test_task_run_model_paste(dev):
    from set_amd import hparams as H
    from set_amd import tasks
    g = load_golden("infer_tiny")
    m = g["meta"]
    H.hparams.clear()
    H.hparams.update(base_hparams(timesteps=m["steps"]))
    task = tasks.SpeechDenoiserTask(build_vocoder=False)
    task.build_model()
    W = Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), m["wseed"])
    task.model.load_state_dict(W, strict=False)
    task.model.to(dev).eval()
    inp, noises = _case_inputs(g, dev)
    sample = dict(txt_tokens=inp["txt_tokens"], mels=inp["ref_mels"], mel2ph=inp["mel2ph"], f0=inp["f0"], uv=inp["uv"],
                  time_mel_masks=inp["time_mel_masks"].squeeze(-1), spk_embed=inp["spk_embed"])
    out = task.run_model(sample, infer=True, noises=noises)
    tm = inp["time_mel_masks"].cpu()
    ref = torch.from_numpy(g["mel_out"]) * tm + inp["ref_mels"].cpu() * (1 - tm)
    assert _maxdiff(out["mel_out"], ref) < 1e-4


# ----------------------------------------------------------------------------------------------------
# HiFi-GAN
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h", [("hifigan_tiny", Wt.HIFIGAN_TINY), ("hifigan_tiny_rb2", Wt.HIFIGAN_TINY_RB2),
                                    ("hifigan_v1", Wt.HIFIGAN_V1), ("hifigan_v1_long", Wt.HIFIGAN_V1),
                                    ("hifigan_v2", Wt.HIFIGAN_V2), ("hifigan_v3", Wt.HIFIGAN_V3)])
@pytest.mark.parametrize("impl", ["auto", "naive", "mfma"])
def test_hifigan_matches_reference(dev, name, h, impl, monkeypatch):
    """`hifigan_v1_long` = the V1 generator at T=220 (56,320 samples): many tiles per stage, every dilation x kernel halo
    crosses tile borders.  `auto` is the SHIPPED path -- what `HifiGanGenerator.forward` runs when
    nobody pins a kernel: the two-piece fp16 conv kernel / fused ResBlock kernels, the all-phase transposed convs, and the
    fp32 MFMA kernel only for the shapes those do not take -- against the reference's own waveforms;
    the fp16 range flag must stay clear (a set flag would mean the forward silently fell back to the fp32 kernels)."""
    from set_amd import ops
    from set_amd.hifigan import HifiGanGenerator
    # hifigan_v2 / hifigan_v3: the paper's other two generator shapes at T = 200 -- C0 = 128 (stages of 64 / 32 / 16 / 8
    # channels) and ResBlock2 with rates [8, 8, 4], kernels [3, 5, 7], dilations [[1, 2], [2, 6], [3, 12]] -- reference-generated
    if impl == "naive" and (name.endswith("_long") or name in ("hifigan_v2", "hifigan_v3")):
        pytest.skip("the one-thread-per-output cross-check kernel is exercised by the short cases")
    if impl == "auto":
        assert ops._DEFAULT_IMPL == "auto"
        monkeypatch.delenv("SET_AMD_VOCODER_SPLIT", raising=False)
        ops.conv_x2_range_flag(reset=True)
    else:
        monkeypatch.setattr(ops, "_DEFAULT_IMPL", impl)
    g = load_golden(name)
    gen = HifiGanGenerator(h)
    gen.load_state_dict(Wt.seeded_weights(Wt.load_manifest(g["meta"].get("manifest", name)), g["meta"]["wseed"]), strict=True)
    gen.to(dev).eval()
    if impl == "auto":
        # the shipped forward with the kernel picks recorded: the split-operand kernels must actually have run
        picks = []
        real_pick, real_pair = ops._pick_impl, ops.resblock_pair

        def spy(*a, **k):
            r = real_pick(*a, **k)
            picks.append(r)
            return r

        def spy_pair(*a, **k):
            picks.append("f16x2")  # the fused ResBlock pair: the same arithmetic, one launch (csrc/resblock_x2.hip)
            return real_pair(*a, **k)
        monkeypatch.setattr(ops, "_pick_impl", spy)
        monkeypatch.setattr(ops, "resblock_pair", spy_pair)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the range fallback warns: it must not happen
            wav = gen(torch.from_numpy(g["mel"]).to(dev))
        torch.cuda.synchronize()
        assert not ops.conv_x2_range_flag(reset=True)
        assert "f16x2" in picks, picks
    else:
        wav = gen(torch.from_numpy(g["mel"]).to(dev))
        torch.cuda.synchronize()
    assert wav.shape == g["wav"].shape
    assert _maxdiff(wav, g["wav"]) < 1e-4


def test_hifigan_v1_full_batch_checks_two_utterances_against_oracle(dev):
    """BASELINE configs[3] vocoder shape (B=64, T=800, V1): the whole batch must be finite and bounded by tanh, two
    utterances (first and last) must match the oracle run on exactly those rows, and an utterance's waveform must not
    depend on the batch it rides in (no cross-sample op in the generator)."""
    from set_amd.hifigan import HifiGanGenerator
    W = Wt.seeded_weights(Wt.load_manifest("hifigan_v1"), 23)
    gen = HifiGanGenerator(Wt.HIFIGAN_V1)
    gen.load_state_dict(W, strict=True)
    gen.to(dev).eval()
    B, T = 64, 800
    rng = np.random.default_rng(991)
    mel = torch.from_numpy(np.clip(rng.normal(-3.0, 1.5, size=(B, 80, T)), -6.0, 1.5).astype(np.float32))
    wav = gen(mel.to(dev))
    torch.cuda.synchronize()
    assert wav.shape == (B, 1, T * 256) and torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0
    rows = [0, B - 1]
    ref = O.hifigan_forward(W, Wt.HIFIGAN_V1, mel[rows])
    assert _maxdiff(wav[rows], ref) < 1e-4
    alone = gen(mel[rows].to(dev))
    assert torch.equal(alone, wav[rows])


def test_vocoder_wrapper_spec2wav(dev, tmp_path):
    import yaml
    from set_amd import hparams as H
    from set_amd import vocoder_infer
    g = load_golden("hifigan_tiny")
    d = tmp_path / "voc"
    d.mkdir()
    yaml.safe_dump(Wt.HIFIGAN_TINY, open(d / "config.yaml", "w"))
    torch.save({"state_dict": {"model_gen": Wt.seeded_weights(Wt.load_manifest("hifigan_tiny"), g["meta"]["wseed"])}},
               d / "model_ckpt_steps_0.ckpt")
    H.hparams.clear()
    H.hparams.update(base_hparams(vocoder_ckpt=str(d)))
    voc = vocoder_infer.get_vocoder_cls("HifiGAN")()
    wav = voc.spec2wav(g["mel"][0].T)  # [T,80] numpy in, numpy out
    assert wav.dtype == np.float32 and wav.shape == (g["wav"].shape[-1],)
    assert np.abs(wav - g["wav"][0, 0]).max() < 1e-4


# ----------------------------------------------------------------------------------------------------
# BASELINE size (B=32, T=800): size-independent properties + a 2-step oracle check
# ----------------------------------------------------------------------------------------------------
def test_full_size_properties(dev, monkeypatch):
    from set_amd import parallel
    B, T, Tt, steps = 32, 800, 100, 2
    model, W = _build_model(dev, "spec_denoiser", 31, steps)
    inp = Wt.synthetic_inputs(B, T, Tt, seed=1234, pad_tail=True)
    noises = torch.stack(Wt.synthetic_noises(B, T, steps, seed=77))
    di = {k: v.to(dev) for k, v in inp.items()}

    def run(d, nz):
        return model(d["txt_tokens"], d["time_mel_masks"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"],
                     infer=True, noises=nz.to(dev))

    full = run(di, noises)
    again = run(di, noises)
    assert torch.equal(full["mel_out"], again["mel_out"])  # deterministic
    assert torch.isfinite(full["mel_out"]).all()
    # sharding invariance (what the multi-GPU path relies on): rank r of 2 computes rows r::2.  B=32 and a 16-utterance
    # shard both run the split-operand stack kernel (64-frame tiles; tiles are cut from the batch's block list, so a tile of
    # the full batch may straddle two utterances where the shard's does not): the two agree to fp32 rounding by default,
    # and bit for bit with the fp32 direct kernel pinned (SET_AMD_WINO=0: per-utterance tiles).
    for r in range(2):
        sh = parallel.shard_batch(di, r, 2)
        part = run(sh, noises[:, r::2].contiguous())
        assert _maxdiff(part["mel_out"], full["mel_out"][r::2]) < 2e-5
        assert torch.equal(part["mel2ph"], full["mel2ph"][r::2])
    monkeypatch.setenv("SET_AMD_WINO", "0")
    full_d = run(di, noises)
    assert _maxdiff(full_d["mel_out"], full["mel_out"]) < 2e-5
    for r in range(2):
        part = run(parallel.shard_batch(di, r, 2), noises[:, r::2].contiguous())
        assert torch.equal(part["mel_out"], full_d["mel_out"][r::2])
    monkeypatch.delenv("SET_AMD_WINO")
    # oracle on the first 4 utterances (the CPU finishes this in seconds)
    sub = {k: v[:4] for k, v in inp.items()}
    oret = O.gaussian_diffusion_infer(W, steps, sub, [n[:4] for n in noises])
    assert _maxdiff(full["mel_out"][:4], oret["mel_out"]) < 1e-4
    assert torch.equal(full["pitch"][:4].cpu(), oret["pitch"])


def test_config3_batch64_diffusion_plus_vocoder_vs_oracle(dev):
    """BASELINE configs[3] (batched inference + HiFi-GAN vocoder at B=64, T=800) end to end at full size with explicit
    noise (2 denoise steps: the oracle finishes two utterances in seconds): conditioner + reverse loop on the kernels a
    64-utterance batch selects, then the V1 generator on the pasted mels exactly as `run_vocoder` batches them
    (inference/tts/base_tts_infer.py:44-47).  First and last utterance against the oracle: integer tensors bit-exact,
    |dmel| < 1e-4, |dwav| < 1e-4 on the oracle's own mel and 5e-4 through both stages; the batch is deterministic and an
    utterance does not depend on the batch it rides in."""
    from set_amd import ops
    from set_amd.hifigan import HifiGanGenerator
    B, T, Tt, steps = 64, 800, 100, 2
    model, W = _build_model(dev, "spec_denoiser", 31, steps)
    inp = Wt.synthetic_inputs(B, T, Tt, seed=6464, pad_tail=True)
    noises = torch.stack(Wt.synthetic_noises(B, T, steps, seed=78))
    di = {k: v.to(dev) for k, v in inp.items()}

    def run(d, nz):
        return model(d["txt_tokens"], d["time_mel_masks"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"],
                     infer=True, noises=nz.to(dev))

    assert ops.stack_variant(B, T, 1) == 5  # the split-operand throughput kernel is what this batch runs
    full = run(di, noises)
    again = run(di, noises)
    assert torch.equal(full["mel_out"], again["mel_out"]) and torch.isfinite(full["mel_out"]).all()
    rows = [0, B - 1]
    sub = {k: v[rows] for k, v in inp.items()}
    oret = O.gaussian_diffusion_infer(W, steps, sub, [n[rows] for n in noises])
    assert _maxdiff(full["mel_out"][rows], oret["mel_out"]) < 1e-4
    for k in ("mel2ph", "pitch", "masked_dur"):
        assert torch.equal(full[k][rows].cpu(), oret[k]), k
    # the vocoder leg on the batch of edited mels
    Wg = Wt.seeded_weights(Wt.load_manifest("hifigan_v1"), 23)
    gen = HifiGanGenerator(Wt.HIFIGAN_V1)
    gen.load_state_dict(Wg, strict=True)
    gen.to(dev).eval()
    mel_bct = full["mel_out"].transpose(1, 2).contiguous()
    wav = gen(mel_bct)
    torch.cuda.synchronize()
    assert wav.shape == (B, 1, T * 256) and torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0
    assert not ops.conv_x2_range_flag(reset=True)
    ref_same_mel = O.hifigan_forward(Wg, Wt.HIFIGAN_V1, mel_bct[rows].cpu())
    assert _maxdiff(wav[rows], ref_same_mel) < 1e-4
    ref_chain = O.hifigan_forward(Wg, Wt.HIFIGAN_V1, oret["mel_out"].transpose(1, 2).contiguous())
    assert _maxdiff(wav[rows], ref_chain) < 5e-4
    assert torch.equal(gen(mel_bct[rows].contiguous()), wav[rows])


def test_full_size_100_steps_split_operand_vs_fp32_pipe(dev, monkeypatch):
    """The benchmark configuration itself (B=32, T=800, 100 denoise steps, on-device Philox noise): the default kernels
    (fp32 operands as two fp16 pieces on the 16-bit MFMA pipe) against the same loop on the fp32 MFMA pipe.  100 steps of
    feedback do not amplify the difference: the two mels agree to a few 1e-6 (bar 5e-5, half the parity bar), and the
    three-piece bf16 splitting agrees with both."""
    from set_amd import ops
    B, T, Tt, steps = 32, 800, 100, 100
    model, W = _build_model(dev, "spec_denoiser", 77, steps)
    inp = {k: v.to(dev) for k, v in Wt.synthetic_inputs(B, T, Tt, seed=4321, pad_tail=True).items()}

    def run():
        return model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"],
                     inp["uv"], infer=True, seed=5)["mel_out"]

    assert ops.stack_variant(B, T, 1) == 5
    m2 = run()
    monkeypatch.setenv("SET_AMD_SPLIT_OPERAND", "bf16x3")
    m3 = run()
    monkeypatch.delenv("SET_AMD_SPLIT_OPERAND")
    monkeypatch.setenv("SET_AMD_X3", "0")
    m32 = run()
    monkeypatch.delenv("SET_AMD_X3")
    assert torch.isfinite(m2).all()
    d2, d3 = _maxdiff(m2, m32), _maxdiff(m3, m32)
    print("B=32 T=800 100 steps: max|dmel| vs the fp32-pipe loop: f16x2 %.3e, bf16x3 %.3e" % (d2, d3))
    assert d2 < 5e-5 and d3 < 5e-5


# ----------------------------------------------------------------------------------------------------
# round 6: the metric's own shape against the REFERENCE (tests/golden/infer_full800.npz: T = 800, T_txt = 100, 100 steps, B = 2 with one
# padded tail, generated by oracle/make_golden.full800_case from /root/reference; spec_denoiser.py:178-184)
# ----------------------------------------------------------------------------------------------------
FULL800_PATHS = {
    "default": {},                                                                                   # B = 2: row-split f16x2 kernel
    "f16x2": {"SET_AMD_X3": "2", "SET_AMD_SPLIT": "0", "SET_AMD_SPLIT_OPERAND": "f16x2"},            # throughput kernel, 64-frame tiles
    "bf16x3": {"SET_AMD_X3": "2", "SET_AMD_SPLIT": "0", "SET_AMD_SPLIT_OPERAND": "bf16x3"},
    "winograd": {"SET_AMD_WINO": "2"},                                                               # fp32 MFMA pipe
}


def _full800(dev):
    g = load_golden("infer_full800")
    m = g["meta"]
    assert (m["B"], m["T"], m["steps"]) == (2, 800, 100)
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"], **m["overrides"])
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=True)
    noises = torch.stack(Wt.synthetic_noises(m["B"], m["T"], m["steps"], seed=m["iseed"] + 1))
    return g, model, inp, noises


def _run800(model, inp, noises, dev, **kw):
    d = {k: v.to(dev) for k, v in inp.items()}
    ret = model(d["txt_tokens"], d["time_mel_masks"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"], infer=True,
                noises=noises.to(dev), **kw)
    torch.cuda.synchronize()
    return ret


@pytest.mark.parametrize("path", sorted(FULL800_PATHS))
def test_full800_100_steps_matches_reference(dev, monkeypatch, path):
    """13 tiles of 64 frames per utterance, the halo hand-off between them exercised over all 100 steps, on every stack kernel family:
    |dmel| < 1e-4 against the reference's own output, integer tensors bit-exact."""
    for k, v in FULL800_PATHS[path].items():
        monkeypatch.setenv(k, v)
    g, model, inp, noises = _full800(dev)
    ret = _run800(model, inp, noises, dev, **({} if path == "default" else {"persistent": True}))
    for k in ("mel2ph", "masked_dur", "pitch", "masked_pitch"):
        assert torch.equal(ret[k].cpu(), torch.from_numpy(g[k])), k
    d = _maxdiff(ret["mel_out"], g["mel_out"])
    mcd = O.mel_mcd(ret["mel_out"].cpu().numpy(), g["mel_out"])
    print("infer_full800 [%s]: max|dmel| = %.3e  mel-MCD = %.3e" % (path, d, mcd))
    assert d < 1e-4 and mcd < 1e-3


def test_full800_inside_a_batch_of_32_matches_reference(dev):
    """The same two utterances as rows 5 and 18 of a B = 32 batch -- the metric's configuration: the throughput kernel on 64-frame tiles cut
    from the batch's block list (400 tiles, several of them straddling two utterances), 100 steps.  The rows must still match the
    reference's output for those utterances (< 1e-4), and the other 30 rows must not matter."""
    from set_amd import ops
    g, model, inp2, noises2 = _full800(dev)
    B, T, Tt, steps = 32, 800, 100, 100
    rows = [5, 18]
    inp = Wt.synthetic_inputs(B, T, Tt, seed=9001, pad_tail=True)
    for k in inp:
        inp[k][rows] = inp2[k]
    gen = torch.Generator(device=dev).manual_seed(9002)
    noises = torch.randn(steps + 1, B, 1, 80, T, device=dev, generator=gen)
    noises[:, rows] = noises2.to(dev)
    assert ops.stack_variant(B, T, 1) == 5
    ret = _run800(model, inp, noises, dev)
    for k in ("mel2ph", "masked_dur", "pitch", "masked_pitch"):
        assert torch.equal(ret[k][rows].cpu(), torch.from_numpy(g[k])), k
    d = _maxdiff(ret["mel_out"][rows], g["mel_out"])
    mcd = O.mel_mcd(ret["mel_out"][rows].cpu().numpy(), g["mel_out"])
    print("infer_full800 inside B=32: max|dmel| = %.3e  mel-MCD = %.3e" % (d, mcd))
    assert d < 1e-4 and mcd < 1e-3
    assert torch.isfinite(ret["mel_out"]).all()


@pytest.mark.parametrize("row", [0, 1])
def test_full800_single_utterance_matches_reference(dev, row):
    """BASELINE configs[0]'s shape on the GPU: ONE utterance, T = 800, 100 steps, through the kernel a batch of one selects (row-split)."""
    from set_amd import ops
    g, model, inp, noises = _full800(dev)
    assert ops.stack_variant(1, 800, 1) != 5
    one = {k: v[row:row + 1].contiguous() for k, v in inp.items()}
    ret = _run800(model, one, noises[:, row:row + 1].contiguous(), dev)
    assert torch.equal(ret["mel2ph"].cpu(), torch.from_numpy(g["mel2ph"][row:row + 1]))
    d = _maxdiff(ret["mel_out"], g["mel_out"][row:row + 1])
    print("infer_full800 row %d alone: max|dmel| = %.3e" % (row, d))
    assert d < 1e-4


def test_cached_step_table_and_conditioner_weights_follow_the_weights(dev):
    """Round 6: the reverse loop keeps its table of step offsets (DiffNet.step_table_all: a function of the step MLP and the layers' diffusion
    projections only) across calls.  A second loop reuses it (same object, same mel); an in-place change of ONE of the 44 tensors (version
    counter), a load_state_dict and an optimizer-style epoch bump each rebuild it, and the loop then equals a freshly built model's."""
    from set_amd import ops
    g = load_golden("infer_tiny")
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"], **m["overrides"])
    inp, noises = _case_inputs(g, dev)
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"])
    a = model(*args, infer=True, noises=noises, **m["flags"])["mel_out"].clone()
    dn = model.denoise_fn
    t0 = dn._dtab.value
    b = model(*args, infer=True, noises=noises, **m["flags"])["mel_out"].clone()
    assert dn._dtab.value is t0 and torch.equal(a, b)
    assert _maxdiff(a, g["mel_out"]) < 1e-4
    with torch.no_grad():
        dn.residual_layers[3].diffusion_projection.bias.add_(0.25)   # in place: version counter
    c = model(*args, infer=True, noises=noises, **m["flags"])["mel_out"].clone()
    assert dn._dtab.value is not t0 and not torch.equal(a, c)
    fresh, _ = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"], **m["overrides"])
    with torch.no_grad():
        fresh.denoise_fn.residual_layers[3].diffusion_projection.bias.add_(0.25)
    assert torch.equal(c, fresh(*args, infer=True, noises=noises, **m["flags"])["mel_out"])
    t1 = dn._dtab.value
    model.load_state_dict({k: v.to(dev) for k, v in W.items()}, strict=False)   # back to the golden's weights (copy_: version counters)
    d = model(*args, infer=True, noises=noises, **m["flags"])["mel_out"].clone()
    assert dn._dtab.value is not t1 and torch.equal(d, a)
    t2 = dn._dtab.value
    ops.bump_weights_epoch()                                                     # what FlatAdamW.step does after its in-place kernel
    e = model(*args, infer=True, noises=noises, **m["flags"])["mel_out"]
    assert dn._dtab.value is not t2 and torch.equal(e, a)
    # the stacked conditioner projection of the loop (DiffNet.cond_projections: one launch for all layers) follows its layers the same way and
    # equals the per-layer launches bit for bit
    cond = torch.randn(2, dn.encoder_hidden, 64, device=dev)
    one = dn.cond_projections(cond).clone()
    with torch.enable_grad():
        per_layer = dn.cond_projections(cond)
    assert torch.equal(one, per_layer)
    w_all = dn._cond_all.value
    with torch.no_grad():
        dn.residual_layers[7].conditioner_projection.weight.mul_(1.5)
    two = dn.cond_projections(cond)
    with torch.enable_grad():
        per_layer = dn.cond_projections(cond)
    assert dn._cond_all.value is not w_all and torch.equal(two, per_layer) and not torch.equal(one, two)


def test_fp32_loop_after_a_bf16_loop_equals_a_fresh_models(dev):
    """The table of step offsets is computed with fp32 operands whichever loop asks for it first: a bf16-operand loop on a model leaves
    no bf16-rounded table behind for a later fp32 (parity) loop on the same model.  40 steps: wide enough for the bf16 conv kernel."""
    from set_amd import ops
    over = dict(residual_layers=20, residual_channels=256, dilation_cycle_length=1)
    model, _ = _build_model(dev, "spec_denoiser", 11, 40, **over)
    inp = {k: v.to(dev) for k, v in Wt.synthetic_inputs(2, 64, 16, seed=101).items()}
    args = (inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"])
    ops.set_compute_dtype("bf16")
    try:
        model(*args, infer=True, seed=5)
    finally:
        ops.set_compute_dtype("f32")
    got = model(*args, infer=True, seed=5)["mel_out"]
    fresh, _ = _build_model(dev, "spec_denoiser", 11, 40, **over)
    assert torch.equal(got, fresh(*args, infer=True, seed=5)["mel_out"])


def test_hifigan_fold_follows_a_weight_load(dev):
    """The folded weight-norm weights follow load_state_dict (it copies into the same storage): after a forward on one set of weights and
    a load of another, the generator equals a fresh one built with the second set, bit for bit."""
    from set_amd.hifigan import HifiGanGenerator
    man = Wt.load_manifest("hifigan_tiny")
    mel = torch.randn(1, 80, 40, generator=torch.Generator().manual_seed(3)).to(dev)

    def gen(seed):
        g = HifiGanGenerator(Wt.HIFIGAN_TINY)
        g.load_state_dict(Wt.seeded_weights(man, seed))
        return g.to(dev).eval()
    g = gen(21)
    first = g(mel).clone()
    g.load_state_dict(Wt.seeded_weights(man, 22))
    second = g(mel)
    assert not torch.equal(first, second)
    assert torch.equal(second, gen(22)(mel))


@pytest.mark.parametrize("form", ["2", "3"])
def test_x3v_winograd_split_operand_stack(dev, monkeypatch, form):
    """Round 6: the Winograd F(2,3) form of GEMM 1 on the two-piece fp16 operands (diffnet_stack_x3v_kernel; SET_AMD_X3_WINO=2 / =3: 64- / 96-frame
    tiles = 2 / 3 column blocks, GEMM 1 on the 16-wide matrix instruction; 3/4 of the layer's MFMAs) against the direct split-operand
    kernel and the fp32-pipe kernel on the same weights -- equal to fp32 rounding; run to run and for 7 / 512 workers bit-identical; against an
    fp64 evaluation of the same layers its error stays within 2 x the fp32 kernel's.
    Shapes: the metric's batch, tiles whose column blocks lie in different utterances or end in a partial block (every column block of a tile
    carries its own utterance and halo frames), T = 66 (a block that holds two frames), T = 2."""
    from set_amd import ops
    import torch.nn.functional as F
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_X3_TILE", "64")
    for (B, T, L, reps) in ((32, 800, 20, 2), (3, 204, 5, 2), (2, 66, 3, 2), (5, 70, 4, 1), (1, 2, 2, 1), (2, 800, 20, 1)):
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, B * 1000 + T + 17, 2)

        def run(x3, wino, grid=None):
            monkeypatch.setenv("SET_AMD_X3", x3)
            monkeypatch.setenv("SET_AMD_X3_WINO", wino)
            if grid is None:
                monkeypatch.delenv("SET_AMD_STACK_GRID", raising=False)
            else:
                monkeypatch.setenv("SET_AMD_STACK_GRID", grid)
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, 1)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            return (xb if L % 2 else xa).clone(), skip.clone()

        x32, s32 = run("0", "0")
        xd2, sd2 = run("2", "0")
        xw, sw = run("2", form)
        tol = 1e-5 * max(1.0, float(x32.abs().max()))
        assert _maxdiff(xw, x32) < tol and _maxdiff(sw, s32) < 1e-5 * max(1.0, float(s32.abs().max())), (B, T)
        assert _maxdiff(xw, xd2) < tol, (B, T)
        for rep in range(reps - 1):
            x, sk = run("2", form)
            assert torch.equal(x, xw) and torch.equal(sk, sw), (B, T, rep)
        for grid in ("7", "512"):
            x, sk = run("2", form, grid)
            assert torch.equal(x, xw) and torch.equal(sk, sw), (B, T, grid)
        if B * T <= 2048:
            xd, skd = x0.double(), torch.zeros_like(x0, dtype=torch.float64)
            for l in range(L):
                dv = dtab[l * 256:(l + 1) * 256, 1].double()[None, :, None]
                y = F.conv1d(xd + dv, wds[l].double(), bd[l].double(), padding=1) + cp[:, l * 512:(l + 1) * 512].double()
                z = torch.sigmoid(y[:, :256]) * torch.tanh(y[:, 256:])
                o = F.conv1d(z, wos[l].double(), bo[l].double())
                xd, skd = (xd + o[:, :256]) / 2 ** 0.5, skd + o[:, 256:]
            e32 = max(float((x32.double() - xd).abs().max()), float((s32.double() - skd).abs().max()))
            ed = max(float((xd2.double() - xd).abs().max()), float((sd2.double() - skd).abs().max()))
            ew = max(float((xw.double() - xd).abs().max()), float((sw.double() - skd).abs().max()))
            print("stack (%d, %d, L=%d): max err vs fp64: fp32 kernel %.3e, split-operand direct %.3e, split-operand Winograd %.3e" % (B, T, L, e32, ed, ew))
            assert ew < 2.0 * e32 + 1e-7, (B, T, ew, e32)


@pytest.mark.parametrize("form", ["0", "2", "3"])
def test_split_operand_stack_on_heavy_tailed_weights_and_activations(dev, monkeypatch, form):
    """Every fixture of this suite draws Gaussian weights -- the benign case for the two-piece fp16 splitting (real checkpoints are external
    downloads).  Here the layers get what trained conv stacks show: heavy-tailed weights (Student-t, 3 degrees of freedom: a few entries
    20 - 50 x the typical one, so the per-layer power-of-two scale leaves most weights' low pieces near the subnormal range), per-channel gains over
    two decades, and activations with isolated outliers of a few hundred.  Criterion as for the Gaussian stacks: the error of the split-operand
    kernel (direct form, Winograd form on 64- / 96-frame tiles) against an fp64 evaluation stays within 2 x the native fp32-MFMA kernel's."""
    from set_amd import ops
    import torch.nn.functional as F
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_X3_TILE", "64")
    B, T, L = 2, 192, 4
    g = torch.Generator().manual_seed(909)

    def student_t(*shape):
        z = torch.randn(*shape, generator=g)
        chi = (torch.randn(3, *shape, generator=g) ** 2).sum(0) / 3.0
        return z / chi.sqrt()

    x0 = torch.randn(B, 256, T, generator=g)
    x0[torch.rand(B, 256, T, generator=g) < 2e-3] *= 300.0
    x0 = x0.to(dev)
    cp = (torch.randn(B, L * 512, T, generator=g) * 0.5).to(dev)
    dtab = torch.randn(L * 256, 3, generator=g).to(dev)
    w1 = torch.empty(L, 512 * 768, device=dev)
    w2 = torch.empty(L, 512 * 256, device=dev)
    wx3 = ops.SplitOperandImages(L, 2, dev)
    bd = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
    bo = (torch.randn(L, 512, generator=g) * 0.1).to(dev)
    wds, wos = [], []
    for l in range(L):
        gain = torch.exp(torch.randn(512, 1, 1, generator=g) * 1.2)           # per-output-channel gains over ~two decades
        wd = (student_t(512, 256, 3) * gain / 60.0).to(dev)
        wo = (student_t(512, 256, 1) * torch.exp(torch.randn(512, 1, 1, generator=g)) / 40.0).to(dev)
        ops.pack_diffnet_layer(wd, wo, w1[l], w2[l])
        wx3.pack(l, wd, wo)
        wds.append(wd), wos.append(wo)
    w1s, w2s = ops.split_images(w1, w2)
    packs = ops.StackImages(w1p=w1, w2p=w2, b_dil=bd, b_out=bo, w1s=w1s, w2s=w2s, wx3=wx3)

    def run(x3, wino):
        monkeypatch.setenv("SET_AMD_X3", x3)
        monkeypatch.setenv("SET_AMD_X3_WINO", wino)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
        ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, 1, err_flag=err)
        torch.cuda.synchronize()
        assert int(ws[1]) == 0 and int(err) == 0, (int(ws[1]), int(err))   # no time-out, no activation beyond the fp16 range
        return (xb if L % 2 else xa).clone(), skip.clone()

    x32, s32 = run("0", "0")
    xs, ss = run("2", form)
    xd, skd = x0.double(), torch.zeros_like(x0, dtype=torch.float64)
    for l in range(L):
        dv = dtab[l * 256:(l + 1) * 256, 1].double()[None, :, None]
        y = F.conv1d(xd + dv, wds[l].double(), bd[l].double(), padding=1) + cp[:, l * 512:(l + 1) * 512].double()
        z = torch.sigmoid(y[:, :256]) * torch.tanh(y[:, 256:])
        o = F.conv1d(z, wos[l].double(), bo[l].double())
        xd, skd = (xd + o[:, :256]) / 2 ** 0.5, skd + o[:, 256:]
    scale = max(float(xd.abs().max()), float(skd.abs().max()))
    e32 = max(float((x32.double() - xd).abs().max()), float((s32.double() - skd).abs().max()))
    es = max(float((xs.double() - xd).abs().max()), float((ss.double() - skd).abs().max()))
    print("heavy-tailed stack, form %s: max |value| %.1f, max err vs fp64: fp32 kernel %.3e, split-operand %.3e" % (form, scale, e32, es))
    assert es < 2.0 * e32 + 1e-7 * scale, (form, es, e32)


@pytest.mark.parametrize("form", ["2", "3"])
def test_x3v_shape_sweep_against_the_direct_form(dev, monkeypatch, form):
    """The Winograd kernel on shapes around its tile geometry: T below one column block, at / one pair past the 32-, 64- and 96-frame
    boundaries, the reference's max_frames (1548), batches whose column-block count is not a multiple of the tile's 2 / 3 blocks -- against
    the direct split-operand kernel on the same images (fp32 rounding apart), NaN-filled outputs so that an unwritten element shows."""
    from set_amd import ops
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_X3_TILE", "64")
    monkeypatch.setenv("SET_AMD_X3", "2")
    L = 3
    for (B, T) in ((1, 30), (1, 32), (2, 34), (3, 62), (1, 64), (2, 94), (1, 96), (3, 98), (2, 130), (5, 190), (1, 1548), (7, 258), (4, 4)):
        x0, cp, dtab, packs, wds, wos, bd, bo = _random_stack(dev, B, T, L, 31 * B + T, 2)
        outs = {}
        for wino in ("0", form):
            monkeypatch.setenv("SET_AMD_X3_WINO", wino)
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, 1)
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
            outs[wino] = ((xb if L % 2 else xa).clone(), skip.clone())
        (xd, sd), (xw, sw) = outs["0"], outs[form]
        assert bool(torch.isfinite(xw).all()) and bool(torch.isfinite(sw).all()), (B, T)
        assert _maxdiff(xw, xd) < 1e-5 * max(1.0, float(xd.abs().max())), (B, T, _maxdiff(xw, xd))
        assert _maxdiff(sw, sd) < 1e-5 * max(1.0, float(sd.abs().max())), (B, T, _maxdiff(sw, sd))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
def test_second_device_computes_what_the_first_does(dev, monkeypatch):
    """Launch-time state is set up once per device (csrc/common.h): the SSIM window in __constant__ memory, the LDS opt-ins of the x3v
    stack kernel and the bf16 conv, the CU count behind the kernel choice.  The same seeded inputs on cuda:0 and then cuda:1 give the
    same bits, SSIM backward (autograd's device thread) included."""
    from set_amd import autograd_ops as A, ops
    for k in ("SET_AMD_X3", "SET_AMD_SPLIT", "SET_AMD_WINO", "SET_AMD_SPLIT_OPERAND", "SET_AMD_STACK_NCB", "SET_AMD_X3_WINO",
              "SET_AMD_X3_TILE", "SET_AMD_STACK_GRID"):
        monkeypatch.delenv(k, raising=False)

    def run(d):
        out = {}
        with torch.cuda.device(d):
            g = torch.Generator().manual_seed(7)
            pred = (torch.randn(3, 60, 80, generator=g) * 0.5 - 3.0).to(d).requires_grad_(True)
            target = torch.clamp(torch.randn(3, 60, 80, generator=g) * 1.5 - 3.0, -6, 1.5).to(d)
            with torch.enable_grad():
                loss = A.ssim_loss(pred, target, A.frame_weights(target))
                loss.backward()
            out["ssim"], out["ssim_grad"] = loss.detach(), pred.grad
            assert ops.stack_x3_winograd(32, 800, 1) == 3  # the x3v kernel, 96-frame tiles
            x0, cp, dtab, packs, *_ = _random_stack(d, 32, 800, 4, 41, 2)
            xa, xb, skip = x0.clone(), torch.full_like(x0, float("nan")), torch.full_like(x0, float("nan"))
            ws = ops.diffnet_stack(xa, xb, skip, cp, dtab.data_ptr() + 4, 0, 3, 256 * 3, packs, 1)
            out["stack_x"], out["stack_skip"] = xa, skip
            x = torch.randn(2, 256, 300, generator=g).to(d)
            wd = (torch.randn(512, 256, 3, generator=g) / 27.7).to(d)
            cw = ops.ConvWeight(lambda: wd, 512, 256, 3)
            out["conv_bf16"] = ops.conv1d(x, cw, torch.randn(512, generator=g).to(d), pad=1,
                                          in_chan_add=torch.randn(2, 256, generator=g).to(d), impl="bf16")
            torch.cuda.synchronize()
            assert int(ws[1]) == 0, "dependency wait timed out"
        return {k: v.cpu() for k, v in out.items()}

    first, second = run(torch.device("cuda:0")), run(torch.device("cuda:1"))
    for k in first:
        assert torch.equal(first[k], second[k]), k


@pytest.mark.parametrize("form", ["2", "3"])
@pytest.mark.parametrize("case", ["infer_full800", "infer_tiny", "infer_pad", "infer_ragged", "infer_drift100"])
def test_full_inference_matches_reference_with_x3v_forced(dev, monkeypatch, case, form):
    """The parity bar (|dmel| < 1e-4 against the reference's own output; the T = 800 x 100-step and the 100-step drift cases included) with
    every DiffNet stack pass on the split-operand kernel's Winograd form (odd T: the launch falls back to the direct form)."""
    monkeypatch.setenv("SET_AMD_X3", "2")
    monkeypatch.setenv("SET_AMD_SPLIT", "0")
    monkeypatch.setenv("SET_AMD_X3_TILE", "64")
    monkeypatch.setenv("SET_AMD_X3_WINO", form)
    g = load_golden(case)
    m = g["meta"]
    model, W = _build_model(dev, "spec_denoiser", m["wseed"], m["steps"], **m["overrides"])
    inp, noises = _case_inputs(g, dev)
    ret = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                inp["f0"], inp["uv"], infer=True, noises=noises, persistent=True, **m["flags"])
    torch.cuda.synchronize()
    d = _maxdiff(ret["mel_out"], g["mel_out"])
    print("%s (split-operand Winograd, form %s): max|dmel| = %.3e" % (case, form, d))
    assert d < 1e-4


# ----------------------------------------------------------------------------------------------------
# ragged / extreme shapes vs the oracle (no golden: the oracle itself is pinned by tests/test_oracle_golden.py)
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,Tt,steps,pad", [(1, 5, 2, 3, False), (2, 31, 7, 2, True), (1, 33, 9, 2, False),
                                              (3, 65, 11, 2, True), (1, 1548, 120, 1, True), (5, 200, 40, 2, True)])
def test_ragged_and_extreme_shapes_vs_oracle(dev, monkeypatch, B, T, Tt, steps, pad):
    """T below / across the 32- and 64-frame tile sizes, B=1, the reference's max_frames (1548), padded tails: the default
    kernels (split operands) against the oracle to 1e-4; with the fp32-pipe kernels pinned the persistent and per-layer
    loops agree bit for bit."""
    model, W = _build_model(dev, "spec_denoiser", 40 + T, steps)
    inp = Wt.synthetic_inputs(B, T, Tt, seed=T, pad_tail=pad)
    noises = Wt.synthetic_noises(B, T, steps, seed=T + 1)
    d = {k: v.to(dev) for k, v in inp.items()}
    nz = torch.stack(noises).to(dev)
    args = (d["txt_tokens"], d["time_mel_masks"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"])
    a = model(*args, infer=True, noises=nz, persistent=True)
    monkeypatch.setenv("SET_AMD_X3", "0")
    monkeypatch.setenv("SET_AMD_SPLIT_F32", "1")
    a32 = model(*args, infer=True, noises=nz, persistent=True)
    b = model(*args, infer=True, noises=nz, persistent=False)
    monkeypatch.delenv("SET_AMD_X3")
    monkeypatch.delenv("SET_AMD_SPLIT_F32")
    assert torch.equal(a32["mel_out"], b["mel_out"])
    assert _maxdiff(a["mel_out"], b["mel_out"]) < 2e-5
    oret = O.gaussian_diffusion_infer(W, steps, inp, noises)
    assert torch.equal(a["mel2ph"].cpu(), oret["mel2ph"]) and torch.equal(a["pitch"].cpu(), oret["pitch"])
    assert torch.equal(a["masked_dur"].cpu(), oret["masked_dur"])
    assert _maxdiff(a["decoder_inp"], oret["decoder_inp"]) < 2e-5
    assert _maxdiff(a["mel_out"], oret["mel_out"]) < 1e-4


@pytest.mark.parametrize("B,T,Tt,steps", [(6, 1548, 120, 1), (3, 65, 11, 2), (1, 5, 2, 2), (5, 70, 9, 2), (3, 128, 20, 2)])
def test_winograd_forced_ragged_and_max_length_vs_oracle(dev, monkeypatch, B, T, Tt, steps):
    """The Winograd stack kernel at the reference's max_frames (1548 = 24 full tiles + a 12-frame tail, odd pair
    count in the tail), across a tile boundary by one frame, and on a 5-frame utterance: vs the oracle to 1e-4."""
    monkeypatch.setenv("SET_AMD_WINO", "2")
    model, W = _build_model(dev, "spec_denoiser", 50 + T, steps)
    inp = Wt.synthetic_inputs(B, T, Tt, seed=T + 3, pad_tail=True)
    noises = Wt.synthetic_noises(B, T, steps, seed=T + 4)
    d = {k: v.to(dev) for k, v in inp.items()}
    nz = torch.stack(noises).to(dev)
    a = model(d["txt_tokens"], d["time_mel_masks"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"],
              infer=True, noises=nz, persistent=True)
    n_or = B if T <= 128 else 2  # the oracle on (the first) utterances (seconds on the CPU even at T=1548)
    sub = {k: v[:n_or] for k, v in inp.items()}
    oret = O.gaussian_diffusion_infer(W, steps, sub, [n[:n_or] for n in noises])
    assert torch.equal(a["mel2ph"][:n_or].cpu(), oret["mel2ph"])
    assert _maxdiff(a["mel_out"][:n_or], oret["mel_out"]) < 1e-4
    assert torch.isfinite(a["mel_out"]).all()


def test_all_padding_and_all_masked_utterances(dev):
    """Degenerate inputs: one utterance fully padded (mel2ph == 0 everywhere), one fully masked, one unmasked."""
    steps, B, T, Tt = 2, 3, 48, 10
    model, W = _build_model(dev, "spec_denoiser", 77, steps)
    inp = Wt.synthetic_inputs(B, T, Tt, seed=9)
    inp["mel2ph"][0] = 0
    inp["ref_mels"][0] = 0
    inp["f0"][0] = 0
    inp["uv"][0] = 0
    inp["time_mel_masks"][0] = 0
    inp["time_mel_masks"][1] = 1
    inp["time_mel_masks"][2] = 0
    noises = Wt.synthetic_noises(B, T, steps, seed=10)
    d = {k: v.to(dev) for k, v in inp.items()}
    ret = model(d["txt_tokens"], d["time_mel_masks"], d["mel2ph"], d["spk_embed"], d["ref_mels"], d["f0"], d["uv"],
                infer=True, noises=torch.stack(noises).to(dev))
    oret = O.gaussian_diffusion_infer(W, steps, inp, noises)
    assert torch.isfinite(ret["mel_out"]).all()
    assert torch.equal(ret["masked_dur"].cpu(), oret["masked_dur"]) and torch.equal(ret["pitch"].cpu(), oret["pitch"])
    assert _maxdiff(ret["mel_out"], oret["mel_out"]) < 1e-4


def test_infer_cli_end_to_end(dev, tmp_path, monkeypatch):
    """`--infer` path: binarised test set (written by the reference's builder) -> StutterSpeechDataset -> edit the
    masked span -> HiFi-GAN -> wav files + meta.csv, through set_hparams / run_task like tasks/run.py."""
    import os
    import yaml
    from scipy.io import wavfile
    from conftest import GOLDEN, ROOT
    from set_amd import hparams as H
    from set_amd import tasks
    monkeypatch.chdir(tmp_path)
    voc = tmp_path / "voc"
    voc.mkdir()
    yaml.safe_dump(Wt.HIFIGAN_TINY_RB2, open(voc / "config.yaml", "w"))
    torch.save({"state_dict": {"model_gen": Wt.seeded_weights(Wt.load_manifest("hifigan_tiny_rb2"), 22)}},
               voc / "model_ckpt_steps_0.ckpt")
    cfg = os.path.join(ROOT, "speech-editing-toolkit_amd", "egs", "spec_denoiser.yaml")
    H.set_hparams(config=cfg, exp_name="e2e", print_hparams=False,
                  hparams_str="timesteps=4,binary_data_dir=%s,vocoder_ckpt=%s" % (os.path.join(GOLDEN, "binary_tiny"), voc))
    H.hparams["infer"] = True
    # a "trained" checkpoint in the reference layout
    torch.manual_seed(0)
    task0 = tasks.SpeechDenoiserTask(build_vocoder=False)
    sd = task0.build_model().state_dict()  # incl. the 16 schedule buffers, as in a reference checkpoint
    sd.update(Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), 5))
    os.makedirs("checkpoints/e2e", exist_ok=True)
    torch.save({"state_dict": {"model": sd}, "global_step": 1234}, "checkpoints/e2e/model_ckpt_steps_1234.ckpt")
    task = tasks.SpeechDenoiserTask()
    assert task.vocoder is not None
    res = task.test()
    assert len(res) == 3
    gen = "checkpoints/e2e/generated_1234_"
    meta = open(os.path.join(gen, "meta.csv")).read().strip().split("\n")
    assert len(meta) == 4 and meta[1].startswith("utt0,hello world 0")
    hop = 4 * 4  # HIFIGAN_TINY_RB2 upsampling
    for r, T in zip(res, (40, 56, 33)):
        sr, wav = wavfile.read(r["files"]["P"])
        assert sr == 22050 and wav.shape == (T * hop,) and wav.dtype == np.int16 and np.abs(wav).max() > 0
        assert r["mel_pred"].shape == (T, 80) and np.isfinite(r["mel_pred"]).all()
        assert set(r["files"]) == {"P", "P_SEG", "G", "G_SEG"}
    # unmasked frames are pasted from the ground truth (spec_denoiser.py:53)
    from set_amd import data as D
    ds = D.IndexedDataset(os.path.join(GOLDEN, "binary_tiny", "test"))
    assert np.abs(res[0]["mel_pred"] - ds[0]["mel"]).min(axis=1).max() < 1e5  # sanity: comparable ranges
