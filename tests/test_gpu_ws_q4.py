"""The channel-quad ("q4") layout of the reverse loop's x and skip workspaces (SetDiffnetStackArgs.xs_q4, SetDiffLoopArgs.ws_q4;
csrc/common.h q4f_index): element (b, c, t) of a [B][256][T] buffer at float b 256 T + ((c >> 2) T + t) 4 + (c & 3).  Only addresses
change -- the same values go through the same arithmetic in the same order -- so every comparison here is bit for bit against the plain
layout after de-interleaving on the host; any difference is a bug.  Structs are filled by hand, every buffer is a view at offset G inside
a sentinel-filled buffer whose guards are checked.

  stack  diffnet_stack_x3v_kernel<2 | 3, Q4> against <2 | 3, plain>: B = 3, T = 68 (a 4-frame last column block; tiles of 64 and 96 frames
         that straddle utterances; halo frames at utterance ends) with L = 3 and L = 2 (both ping-pong parities), B = 1, T = 64 (exact
         tiles), B = 2, T = 34.  skip starts as NaN: layer 0 must not read it.  xs_q4 on a plan that is not x3v returns SET_E_INVALID.
  loop   set_diffusion_loop with ws_q4 = 1 against 0: B = 3, T = 68, M = 80, L = 2; steps = 2 (the boundary writes q4 xin_next, the next
         stack reads it) and steps = 1 (last-step branch); explicit and Philox noise.  SET_AMD_WS_Q4=0 or a plan that does not qualify
         keeps plain workspaces, equal to the flag-off run.
  model  one GaussianDiffusion forward (B = 2, T = 64, 4 steps): mel_out with the default equals mel_out with SET_AMD_WS_Q4=0."""
import ctypes as C
import math

import pytest
import torch

import test_loop_reference as R
import test_gpu_loop_branches as LB
from test_gpu_conv_branches import SENTINEL, _ALIVE, _L, _keep_launch_operands, _p, _s, dev  # noqa: F401
from test_gpu_stack_branches import _images

pytestmark = pytest.mark.gpu

G = 64  # guard floats in front of and behind every view (256 bytes: the views stay 16-byte aligned)
DC = 256
SWITCHES = tuple(sorted(set(LB.SWITCHES) | {"SET_AMD_WS_Q4", "SET_AMD_SPLIT_OPERAND", "SET_AMD_STACK_GRID"}))
X3V = {"SET_AMD_X3": "2", "SET_AMD_X3_TILE": "64", "SET_AMD_SPLIT": "0"}  # (SPLIT=0: these batches are small enough for the row-split kernel)
WIDTHS = ("2", "3")  # SET_AMD_X3_WINO: 64- and 96-frame tiles


def _setenv(monkeypatch, env):
    for n in SWITCHES:
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)


def to_q4(x):
    """[B][256][T] -> the same elements in channel-quad order (a [B][64][T][4] array, flat)."""
    B, _, T = x.shape
    return x.reshape(B, DC // 4, 4, T).permute(0, 1, 3, 2).contiguous().reshape(B, DC, T)


def from_q4(x):
    B, _, T = x.shape
    return x.reshape(B, DC // 4, T, 4).permute(0, 1, 3, 2).contiguous().reshape(B, DC, T)


def test_host_layout_helpers_match_the_index_formula():
    B, T = 2, 6
    x = torch.arange(B * DC * T, dtype=torch.float32).view(B, DC, T)
    q = to_q4(x).flatten()
    for b, c, t in ((0, 0, 0), (0, 3, 5), (0, 4, 0), (1, 255, 5), (1, 129, 2)):
        assert q[b * DC * T + ((c >> 2) * T + t) * 4 + (c & 3)] == x[b, c, t]
    assert torch.equal(from_q4(to_q4(x)), x)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guards(buf, name):
    assert bool((buf[:G] == SENTINEL).all()) and bool((buf[-G:] == SENTINEL).all()), "%s: a guard was written" % name


# ------------------------------------------------------------------------------------------------------------------------
# the stack kernel
# ------------------------------------------------------------------------------------------------------------------------
def _stack_operands(B, T, L, dcl=1):
    g = torch.Generator().manual_seed(1000 * B + 10 * T + L)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(B=B, T=T, L=L, dcl=dcl, Wd=rn(L, 512, DC, 3) / 27.7, bd=rn(L, 512) * 0.1, Wo=rn(L, 512, DC, 1) / 16, bo=rn(L, 512) * 0.1,
                cp=rn(B, L * 512, T) * 0.5, x0=rn(B, DC, T), tab=rn(L * DC, 1))


def _stack_launch(dev, o, packs, q4):
    """One set_diffnet_stack launch; returns (rc, the whole xa / xb / skip buffers on the CPU, sync_ws, error word)."""
    from set_amd import _lib, ops
    B, T, L = o["B"], o["T"], o["L"]
    n = B * DC * T
    cpu = {k: torch.full((G + n + G,), SENTINEL) for k in ("xa", "xb", "skip")}
    cpu["xa"][G:-G] = (to_q4(o["x0"]) if q4 else o["x0"]).flatten()
    cpu["xb"][G:-G] = float("nan")
    cpu["skip"][G:-G] = float("nan")
    d = {k: v.to(dev) for k, v in cpu.items()}
    cp, tab = o["cp"].to(dev).contiguous(), o["tab"].to(dev).contiguous()
    ws = torch.full((ops.sync_ws_size(B, T) + 16,), -1, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _lib.SetDiffnetStackArgs()
    _ALIVE.append(ops._set_images(a, packs, B, T, o["dcl"], dev))
    a.xa, a.xb, a.skip = (_p(d[k]) + 4 * G for k in ("xa", "xb", "skip"))
    a.condproj, a.dstep = _p(cp), _p(tab)
    a.cp_bs, a.cp_ls = L * 512 * T, 512 * T
    a.d_bs, a.d_cs, a.d_ls = 0, 1, DC
    a.B, a.T, a.L, a.dilation_cycle_length = B, T, L, o["dcl"]
    a.sync_ws, a.err_flag = _p(ws), _p(err)
    a.xs_q4 = int(q4)
    rc = _L().set_diffnet_stack(C.byref(a), _s())
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in d.items()}
    return rc, cpu, out, ws.cpu(), int(err.item())


STACK_CASES = [(3, 68, 3), (3, 68, 2), (1, 64, 2), (2, 34, 2)]


@pytest.mark.parametrize("B,T,L", STACK_CASES, ids=["B%d_T%d_L%d" % c for c in STACK_CASES])
def test_stack_q4_equals_plain(dev, monkeypatch, B, T, L):
    from set_amd import ops
    o = _stack_operands(B, T, L)
    packs = _images(dev, o, 2)
    for wino in WIDTHS:
        _setenv(monkeypatch, dict(X3V, SET_AMD_X3_WINO=wino))
        assert ops.stack_x3_winograd(B, T, 1, x3_mode=2) == int(wino), "the forcing switches did not reach the x3v kernel"
        rc0, _, plain, ws0, err0 = _stack_launch(dev, o, packs, False)
        rc1, _, quad, ws1, err1 = _stack_launch(dev, o, packs, True)
        assert rc0 == 0 and rc1 == 0 and err0 == 0 and err1 == 0, (rc0, rc1, err0, err1)
        assert int(ws0[1]) == 0 and int(ws1[1]) == 0, "a dependency wait gave up"
        assert torch.equal(ws0, ws1), "the two layouts did not run the same tiling"
        ntiles = (B * ((T + 31) // 32) + int(wino) - 1) // int(wino)
        assert bool((ws1[4:4 + ntiles] == 8 * L).all()), ("not the x3v kernel's flags (8 waves per layer)", ws1[:4 + ntiles].tolist())
        for k in ("xa", "xb", "skip"):
            _guards(plain[k], k + " (plain)"), _guards(quad[k], k + " (q4)")
            got, want = from_q4(quad[k][G:-G].view(B, DC, T)), plain[k][G:-G].view(B, DC, T)
            assert not bool(torch.isnan(want).any()), k + ": the plain run left NaN (layer 0 read skip, or a frame was not written)"
            assert _bits_equal(got, want), (k, wino, "first difference at (b, c, t) = %s" % (got != want).nonzero()[:4].tolist())
        assert not _bits_equal(quad["skip"][G:-G], plain["skip"][G:-G]), "xs_q4 changed nothing: the q4 form did not run"


@pytest.mark.parametrize("B,T,dcl,env", [(2, 67, 1, {}), (2, 68, 2, {}), (2, 68, 1, {"SET_AMD_X3_WINO": "0"})],
                         ids=["odd_T", "dilation_cycle_2", "direct_form"])
def test_stack_q4_is_refused_on_every_other_plan(dev, monkeypatch, B, T, dcl, env):
    from set_amd import _lib, ops
    o = _stack_operands(B, T, 2, dcl)
    packs = _images(dev, o, 2)
    _setenv(monkeypatch, {**X3V, "SET_AMD_X3_WINO": "2", **env})
    assert ops.stack_x3_winograd(B, T, dcl, x3_mode=2) == 0
    rc, before, out, ws, err = _stack_launch(dev, o, packs, True)
    assert rc == _lib.E_INVALID, rc
    assert b"xs_q4" in _L().set_last_error()
    for k in ("xa", "xb", "skip"):  # nothing ran
        assert _bits_equal(out[k], before[k]), k
    assert bool((ws == -1).all())
    assert _stack_launch(dev, o, packs, False)[0] == 0  # the same launch without the flag is fine


# ------------------------------------------------------------------------------------------------------------------------
# the loop
# ------------------------------------------------------------------------------------------------------------------------
LOOP_CASE = dict(name="ws_q4_B3_M80_T68", B=3, M=80, T=68)
WS = ("ws_x0", "ws_x1", "ws_skip")


def _loop_run(dev, o, d, *, ws_q4, seed=None):
    """LB._run with the ws_q4 field: one set_diffusion_loop call, the whole buffers back on the CPU."""
    from set_amd import _lib, ops
    B, M, T, L, steps = o["B"], o["M"], o["T"], o["L"], o["steps"]
    n = dict(x=B * M * T, ws_x0=B * DC * T, ws_x1=B * DC * T, ws_skip=B * DC * T, ws_h=B * DC * T, ws_x0pred=B * M * T)
    cpu = {k: torch.full((G + v + G,), SENTINEL) for k, v in n.items()}
    cpu["x"][G:-G] = o["x_T"].flatten()
    dbuf = {k: v.to(dev) for k, v in cpu.items()}
    a = _lib.SetDiffLoopArgs()
    a.B, a.T, a.M, a.L, a.steps, a.dilation_cycle_length = B, T, M, L, steps, o["dcl"]
    for k in n:
        setattr(a, k, _p(dbuf[k]) + 4 * G)
    a.noise, a.seed = (_p(d["noise"]), 0) if seed is None else (None, int(seed))
    a.condproj, a.dstep, a.coef4 = _p(d["cp"]), _p(d["dstep"]), _p(d["coef4"])
    a.w_in_p, a.b_in = _p(d["img"]["W_in"]), _p(d["b_in"])
    a.w_skip_p, a.b_skip = _p(d["img"]["W_skip"]), _p(d["b_skip"])
    a.w_outp_p, a.b_outp = _p(d["img"]["W_out"]), _p(d["b_out"])
    a.w_in_x2, a.w_skip_x2, a.w_outp_x2 = _p(d["img_x2"]["W_in"]), _p(d["img_x2"]["W_skip"]), _p(d["img_x2"]["W_out"])
    _ALIVE.append(ops._set_images(a, d["packs"], B, T, o["dcl"], dev))
    a.persistent, a.n_groups = 1, 1
    sync_ws = torch.zeros(ops.sync_ws_size(B, T), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a.sync_ws, a.err_flag = _p(sync_ws), _p(err)
    a.ws_q4 = int(ws_q4)
    _lib.check(_L().set_diffusion_loop(C.byref(a), _s()), "set_diffusion_loop")
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in dbuf.items()}
    assert int(err.item()) == 0
    return out


@pytest.fixture(scope="module")
def loop_operands(dev):
    """Operands of the loop cases, made once and never changed: {steps: (o, device copies)}."""
    made = {}
    for steps in (2, 1):
        o = R.make_gauss(LOOP_CASE, 1, steps=steps, L=2, tag="ws_q4")
        made[steps] = (o, LB._operands(dev, o, 2))
    return made


@pytest.mark.parametrize("seed", [None, 79], ids=["eps", "philox"])
@pytest.mark.parametrize("steps", [2, 1])
def test_loop_q4_equals_plain(dev, monkeypatch, loop_operands, steps, seed):
    o, d = loop_operands[steps]
    B, T = o["B"], o["T"]
    for wino in WIDTHS:
        env = dict(X3V, SET_AMD_X3_WINO=wino)
        _setenv(monkeypatch, env)
        plain = _loop_run(dev, o, d, ws_q4=0, seed=seed)
        quad = _loop_run(dev, o, d, ws_q4=1, seed=seed)
        for k in plain:
            _guards(plain[k], k), _guards(quad[k], k)
        for k in ("x", "ws_h", "ws_x0pred"):
            assert _bits_equal(quad[k], plain[k]), (k, wino)
        assert bool((plain["ws_h"] == SENTINEL).all()), "the fused boundary did not run"
        for k in WS:
            got, want = from_q4(quad[k][G:-G].view(B, DC, T)), plain[k][G:-G].view(B, DC, T)
            assert _bits_equal(got, want), (k, wino, (got != want).nonzero()[:4].tolist())
            assert not _bits_equal(quad[k], plain[k]), k + ": ws_q4 changed nothing, the workspaces are plain"
        # the A/B switch: plain workspaces, the flag-off run bit for bit
        _setenv(monkeypatch, dict(env, SET_AMD_WS_Q4="0"))
        off = _loop_run(dev, o, d, ws_q4=1, seed=seed)
        for k in plain:
            assert _bits_equal(off[k], plain[k]), (k, wino, "SET_AMD_WS_Q4=0")


@pytest.mark.parametrize("why,env,x3_mode", [("direct form of GEMM 1", dict(X3V, SET_AMD_X3_WINO="0"), 2),
                                             ("fp32 boundary", dict(X3V, SET_AMD_X3_WINO="2", SET_AMD_BOUNDARY_X2="0"), 2),
                                             ("unfused boundary", dict(X3V, SET_AMD_X3_WINO="2", SET_AMD_FUSED_BOUNDARY="0"), 2),
                                             ("three bf16 pieces (the repeat after a range error)", dict(X3V, SET_AMD_X3_WINO="2"), 3)],
                         ids=["direct", "boundary_f32", "unfused", "bf16x3"])
def test_loop_keeps_plain_workspaces_when_the_plan_does_not_qualify(dev, monkeypatch, loop_operands, why, env, x3_mode):
    o, d = loop_operands[2]
    if x3_mode == 3:
        d = LB._operands(dev, o, 3)
    _setenv(monkeypatch, env)
    plain = _loop_run(dev, o, d, ws_q4=0)
    flagged = _loop_run(dev, o, d, ws_q4=1)
    for k in plain:
        assert _bits_equal(flagged[k], plain[k]), (k, why)


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def test_model_forward_is_the_same_with_and_without_q4(dev, monkeypatch):
    import os
    import yaml
    from set_amd.diffnet import DiffNet
    from set_amd.spec_denoiser import GaussianDiffusion
    from oracle import weights as Wt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "speech-editing-toolkit_amd", "egs", "spec_denoiser.yaml")) as f:
        hp = yaml.safe_load(f)
    steps = 4
    hp["timesteps"] = steps
    with torch.no_grad():
        model = GaussianDiffusion(list(range(80)), 80, DiffNet(80, hp), timesteps=steps, time_scale=1, loss_type="l1", spec_min=[], spec_max=[], hp=hp)
        model.load_state_dict(Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), 11), strict=False)
        model.to(dev).eval()
        inp = {k: v.to(dev) for k, v in Wt.synthetic_inputs(2, 64, 16, seed=101).items()}
        noises = torch.stack(Wt.synthetic_noises(2, 64, steps, seed=102)).to(dev)
        from set_amd import ops
        mels = {}
        for wino in WIDTHS:
            for q4 in ("1", "0"):
                _setenv(monkeypatch, dict(X3V, SET_AMD_X3_WINO=wino, SET_AMD_WS_Q4=q4))
                assert ops.stack_x3_winograd(2, 64, 1, x3_mode=2) == int(wino)
                ret = model(inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"],
                            infer=True, noises=noises)
                mels[wino, q4] = ret["mel_out"].cpu()
            assert bool(torch.isfinite(mels[wino, "1"]).all())
            assert _bits_equal(mels[wino, "1"], mels[wino, "0"]), (wino, float((mels[wino, "1"] - mels[wino, "0"]).abs().max()))
