"""INTEGRATION.md is executable documentation: these tests run its code blocks as written.

* section A (registry swap) -- build container only: the reference is imported through oracle/ref_import.py, the block is executed
  verbatim (with the checkout path filled in), the model is built through the REFERENCE's own SpeechDenoiserTask.build_tts_model
  (tasks/speech_editing/spec_denoiser.py:29-36) and a state dict produced by the reference's own classes is loaded with strict=True;
  the vocoder registry (tasks/tts/vocoder_infer/base_vocoder.py:6-18) hands out this package's wrapper.  Skipped where the reference
  checkout is absent (oracle/ref_import.py); the same block also runs against stand-ins of the two registry modules it patches, with the
  reference's state_dict layout from tests/golden/.
* section B (raw ctypes binding of one ResidualBlock.forward, diffnet.py:60-81) -- `-m gpu`: the block is executed verbatim in a namespace that
  has never imported this package (only ctypes + torch + the path of the built library) and its output is compared with the reference's own
  layer trace in tests/golden/infer_tiny.npz.
"""
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = os.path.join(ROOT, "INTEGRATION.md")


def _python_blocks():
    with open(DOC) as f:
        return re.findall(r"```python\n(.*?)```", f.read(), flags=re.S)


def test_integration_md_has_the_three_blocks():
    blocks = _python_blocks()
    assert len(blocks) == 3
    assert "DIFF_DECODERS" in blocks[0] and "REGISTERED_VOCODERS" in blocks[0]
    assert "set_diffnet_layer" in blocks[1] and "import set_amd" not in blocks[1]
    assert "set_attention" in blocks[2]


def _reference_available():
    sys.path.insert(0, ROOT)
    from oracle import ref_import
    return ref_import.available()


def test_section_a_registry_swap_on_stand_in_registries(monkeypatch):
    """Section A without the reference checkout: the block runs verbatim against stand-ins of the two reference modules it patches
    (nothing but the registry names it assigns to), the patched `GaussianDiffusion` / `DIFF_DECODERS["wavenet"]` build this package's
    model with the reference's constructor keywords, and that model has the reference's state_dict layout (tests/golden/
    manifest_spec_denoiser.json, written from the reference's own model) and loads it with strict=True."""
    import types
    from conftest import base_hparams
    from oracle import weights as Wt
    hp = base_hparams(timesteps=4)  # the schedule length the manifest was written with
    ref_task = types.ModuleType("tasks.speech_editing.spec_denoiser")
    ref_task.DIFF_DECODERS, ref_task.GaussianDiffusion, ref_task.hparams = {}, None, hp
    ref_voc = types.ModuleType("tasks.tts.vocoder_infer.base_vocoder")
    ref_voc.REGISTERED_VOCODERS = {}
    mods = {"tasks": types.ModuleType("tasks"), "tasks.speech_editing": types.ModuleType("tasks.speech_editing"),
            "tasks.speech_editing.spec_denoiser": ref_task, "tasks.tts": types.ModuleType("tasks.tts"),
            "tasks.tts.vocoder_infer": types.ModuleType("tasks.tts.vocoder_infer"), "tasks.tts.vocoder_infer.base_vocoder": ref_voc}
    for name, mod in mods.items():
        monkeypatch.setitem(sys.modules, name, mod)
        parent, _, child = name.rpartition(".")
        if parent:
            setattr(mods[parent], child, mod)
    monkeypatch.setattr(sys, "path", list(sys.path))
    ns = {}
    exec(compile(_python_blocks()[0].replace("/path/to/this/repo", ROOT), "INTEGRATION.md#A", "exec"), ns)
    from set_amd import vocoder_infer as amd_voc
    from set_amd.diffnet import DiffNet as AmdDiffNet
    from set_amd.spec_denoiser import GaussianDiffusion as AmdGD
    assert ref_voc.REGISTERED_VOCODERS == {"HifiGAN": amd_voc.HifiGAN}
    dn = ref_task.DIFF_DECODERS["wavenet"](hp)
    model = ref_task.GaussianDiffusion(phone_encoder=list(range(80)), out_dims=80, denoise_fn=dn, timesteps=4, time_scale=1,
                                       loss_type="l1", spec_min=[], spec_max=[])
    assert isinstance(model, AmdGD) and isinstance(model.denoise_fn, AmdDiffNet) and model.num_timesteps == 4
    manifest = Wt.load_manifest("spec_denoiser")
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == manifest and len(manifest) == 339
    sd = dict(model.state_dict())
    sd.update(Wt.seeded_weights(manifest, 3))
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.skipif(not _reference_available(), reason="the reference checkout is not available")
def test_section_a_registry_swap_inside_the_reference(tmp_path):
    """In a process of its own (the reference's top-level packages `utils`, `modules`, `tasks` stay out of this one)."""
    block = _python_blocks()[0].replace("/path/to/this/repo", ROOT)
    script = textwrap.dedent('''
        import sys
        sys.path.insert(0, %r)
        import torch
        from oracle import ref_import
        hp = ref_import.install(timesteps=100)
        hp.update(residual_layers=20, residual_channels=256, dilation_cycle_length=1)
        # ---- the reference's own model, built BEFORE the swap: the state dict a user's checkpoint would hold
        import tasks.speech_editing.spec_denoiser as ref_task
        tok = list(range(80))
        def bare_task():  # the task object without its dataset / vocoder set-up (speech_base.py: needs the binarised set on disk)
            t = ref_task.SpeechDenoiserTask.__new__(ref_task.SpeechDenoiserTask)
            torch.nn.Module.__init__(t)
            t.token_encoder = tok
            return t
        ref = bare_task()
        ref_task.SpeechDenoiserTask.build_tts_model(ref)
        assert type(ref.model).__module__ == "modules.speech_editing.spec_denoiser.spec_denoiser"
        with torch.no_grad():
            for p in ref.model.parameters():
                p.normal_(0.0, 0.02)
        sd = {k: v.clone() for k, v in ref.model.state_dict().items()}
        # ---- INTEGRATION.md section A, verbatim
        BLOCK
        # ---- the reference's task builds its model through the swapped registries
        task = bare_task()
        ref_task.SpeechDenoiserTask.build_tts_model(task)
        from set_amd.spec_denoiser import GaussianDiffusion as AmdGD
        from set_amd.diffnet import DiffNet as AmdDiffNet
        assert isinstance(task.model, AmdGD) and isinstance(task.model.denoise_fn, AmdDiffNet)
        assert list(task.model.state_dict().keys()) == list(sd.keys())
        missing, unexpected = task.model.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        for k, v in task.model.state_dict().items():
            assert torch.equal(v.cpu(), sd[k]), k
        assert task.model.num_timesteps == ref.model.num_timesteps == 100
        # ---- vocoder registry: get_vocoder_cls (base_vocoder.py:16-18) hands out this package's wrapper, with the reference's surface
        voc = ref_voc.get_vocoder_cls("HifiGAN")
        assert voc is amd_voc.HifiGAN and callable(getattr(voc, "spec2wav"))
        print("SECTION_A_OK", len(sd))
    ''' % ROOT).replace("BLOCK", block.rstrip())
    path = tmp_path / "section_a.py"
    path.write_text(script)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and "SECTION_A_OK 339" in r.stdout, r.stdout[-3000:]


@pytest.mark.gpu
def test_section_b_ctypes_binding_reproduces_the_reference_layer(built_lib):
    """The snippet as printed, in a namespace that never saw `set_amd`: layer 0 of the first executed step of infer_tiny."""
    import torch.nn as nn
    import torch.nn.functional as F
    from conftest import load_golden
    from oracle import oracle as O
    from oracle import weights as Wt
    dev = torch.device("cuda:0")
    lib_path = os.path.join(ROOT, "speech-editing-toolkit_amd", "libset_amd.so")
    assert os.path.exists(lib_path)
    block = _python_blocks()[1].replace("/path/to/repo/speech-editing-toolkit_amd/libset_amd.so", lib_path)
    ns = {}
    exec(compile(block, "INTEGRATION.md#B", "exec"), ns)
    ns["lib"].set_last_error.restype = __import__("ctypes").c_char_p
    assert "set_amd" not in ns and not any(k.startswith("set_amd") for k in ns)
    g = load_golden("infer_tiny")
    m = g["meta"]
    W = Wt.seeded_weights(Wt.load_manifest("spec_denoiser"), m["wseed"])
    inp = Wt.synthetic_inputs(m["B"], m["T"], m["T_txt"], seed=m["iseed"], pad_tail=m["pad_tail"])
    noises = Wt.synthetic_noises(m["B"], m["T"], m["steps"], seed=m["iseed"] + 1)
    # everything in front of the residual block comes from the CPU oracle (the checker): conditioner, input projection, step embedding
    _, cond = O.conditioner(W, inp["txt_tokens"], inp["time_mel_masks"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"], inp["uv"])
    p = "denoise_fn."
    x = F.relu(F.conv1d(noises[0][:, 0], W[p + "input_projection.weight"], W[p + "input_projection.bias"]))
    t = torch.full((m["B"],), m["steps"] - 1, dtype=torch.long)
    emb = O.step_embedding(W, t)

    class Block(nn.Module):  # the attribute names of the reference's ResidualBlock (diffnet.py:49-58)
        def __init__(self):
            super().__init__()
            self.dilated_conv = nn.Conv1d(256, 512, 3, padding=1, dilation=1)
            self.diffusion_projection = nn.Linear(256, 256)
            self.conditioner_projection = nn.Conv1d(192, 512, 1)
            self.output_projection = nn.Conv1d(256, 512, 1)

    blk = Block()
    lp = p + "residual_layers.0."
    blk.load_state_dict({k[len(lp):]: v for k, v in W.items() if k.startswith(lp)}, strict=True)
    blk.to(dev)
    with torch.no_grad():
        condproj = blk.conditioner_projection(cond.to(dev)).contiguous()
        d = blk.diffusion_projection(emb.to(dev)).contiguous()
        w1p, w2p = ns["pack"](blk)
        skip = torch.zeros(m["B"], 256, m["T"], device=dev)
        x_out = ns["residual_block_forward"](blk, x.to(dev).contiguous(), condproj, d, skip, True, w1p, w2p)
    torch.cuda.synchronize()
    dx = float((x_out.cpu() - torch.from_numpy(g["layer0_x"])).abs().max())
    ds = float((skip.cpu() - torch.from_numpy(g["layer0_skip"])).abs().max())
    print("INTEGRATION.md section B vs the reference's layer trace: |dx| %.2e |dskip| %.2e" % (dx, ds))
    assert dx < 2e-5 and ds < 2e-5
