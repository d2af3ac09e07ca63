"""Fixtures of the StutterSpeech model (tests/golden/*stutter*): the reference's own model, loss functions and autograd.

Run on a host with the reference checkout (oracle/ref_import.py finds it); never on a GPU box.  Uses oracle.make_golden's helpers
read-only.  Writes manifest_stutter_speech.json, train_losses_stutter{,_ragged}.npz, infer_stutter.npz and binary_stutter_tiny/.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402  (importing it turns autograd off globally)
from oracle import ref_import, weights as Wt  # noqa: E402

GOLD = Wt.GOLDEN_DIR
BASE = dict(residual_layers=20, residual_channels=256, dilation_cycle_length=1)


def build_ref(hp, steps):
    hp["timesteps"] = steps
    hp.update(BASE)
    from modules.speech_editing.stutter_speech import spec_denoiser as SD
    from modules.speech_editing.stutter_speech.diffnet import DiffNet
    SD.tqdm = lambda it, **kw: it
    m = SD.GaussianDiffusion(list(range(80)), 80, DiffNet(80), timesteps=steps, time_scale=1, loss_type="l1", spec_min=[], spec_max=[])
    m.eval()
    return m


def labels_for(inp, seed):
    """Raw stutter masks as the collate hands them over: 0 fluent, 1 stutter, -1 on padded frames (stutter_pad_idx); remapped here
    like tasks/speech_editing/stutter_speech.py:75-76."""
    rng = np.random.default_rng(seed)
    mel2ph = inp["mel2ph"].numpy()
    raw = (rng.random(mel2ph.shape) < 0.3).astype(np.int64)
    raw[mel2ph == 0] = -1
    m = torch.from_numpy(raw)
    lab = m.clone()
    lab[lab > 0] = 1
    lab[lab < 0] = 2
    assert set(np.unique(lab.numpy())) == {0, 1, 2}
    return m, lab


def fake_task():
    """The reference task's loss methods on an object that holds only the attributes they touch."""
    from tasks.tts.speech_base import SpeechBaseTask as S
    from tasks.speech_editing.speech_editing_base import SpeechEditingBaseTask as E
    T = type("FakeTask", (), dict(l1_loss=S.l1_loss, ssim_loss=S.ssim_loss, add_mel_loss=S.add_mel_loss, add_dur_loss=E.add_dur_loss,
                                  add_pitch_loss=E.add_pitch_loss))
    task = T()
    task.mel_losses = {"l1": 0.5, "ssim": 0.5}
    task.sil_ph = [1, 2, 3]
    task.token_encoder = type("Enc", (), {"encode": staticmethod(lambda p: [p])})()
    return task


def train_loss_case(hp, name, B, T, T_txt, steps, wseed, iseed, step):
    from modules.speech_editing.stutter_speech.stutter_predictor import MultiFocalLoss
    task = fake_task()
    model = build_ref(hp, steps)
    MG.load_seeded(model, wseed)
    inp = Wt.synthetic_inputs(B, T, T_txt, seed=iseed, pad_tail=True)
    raw, lab = labels_for(inp, iseed + 3)
    rng = np.random.default_rng(iseed + 7)
    t = torch.from_numpy(rng.integers(0, steps + 1, size=(B,), dtype=np.int64))
    eps = torch.from_numpy(rng.standard_normal(size=(B, 1, 80, T), dtype=np.float32))
    real_randint, real_rl = torch.randint, torch.randn_like
    torch.randint = lambda *a, **k: t.clone()
    torch.randn_like = lambda x, **k: eps.clone()
    try:
        with torch.enable_grad():
            out = model(inp["txt_tokens"], inp["time_mel_masks"], lab, inp["mel2ph"], inp["spk_embed"], inp["ref_mels"],
                        inp["f0"].clone(), inp["uv"].clone(), infer=False)
            tm = inp["time_mel_masks"]
            losses = {}
            task.add_mel_loss(out["mel_out"] * tm, inp["ref_mels"] * tm, losses, postfix="_coarse")
            task.add_dur_loss(out["dur"], inp["mel2ph"], inp["txt_tokens"], losses=losses)
            logits = out["stutter_predictor_out"]
            losses["ce"] = torch.nn.CrossEntropyLoss(ignore_index=2)(logits.transpose(1, 2), lab)
            losses["focal"] = MultiFocalLoss(ignore_index=2)(logits.transpose(1, 2), lab)
            task.add_pitch_loss(out, {"mel2ph": inp["mel2ph"], "f0": inp["f0"], "uv": inp["uv"]}, losses)
            w = {"ce": 8e-3 + 5e-3 * (step + 1) / 100000, "focal": 1 + 2 * (step + 1) / 100000}
            total = sum(w.get(k, 1) * v for k, v in losses.items())
            total.backward()
    finally:
        torch.randint, torch.randn_like = real_randint, real_rl
    for k, v in losses.items():
        assert np.isfinite(float(v)), k
    grads = {k: p.grad for k, p in model.named_parameters()}
    names = [k for k, _ in model.named_parameters()]
    assert all(grads[k] is not None for k in names), [k for k in names if grads[k] is None]
    norms = np.array([float(grads[k].norm()) for k in names], dtype=np.float64)
    keep = ["stutter_predictor.linear.weight", "stutter_predictor.linear.bias", "stutter_embed.weight", "mel_encoder.encoder.0.weight",
            "mel_encoder.fc_out.bias", "stutter_predictor.conv.g_prenet.bias", "stutter_predictor.conv.res_blocks.0.blocks.0.0.weight",
            "stutter_predictor.conv.res_blocks.3.blocks.1.4.bias", "stutter_predictor.conv.last_norm.weight",
            "stutter_predictor.conv.post_net1.bias"]
    out_np = dict(meta=np.array(json.dumps(dict(B=B, T=T, T_txt=T_txt, steps=steps, wseed=wseed, iseed=iseed, pad_tail=True,
                                                sil_ids=[1, 2, 3], param_names=names, global_step=step))),
                  t=t, eps=eps, raw_masks=raw, labels=lab, logits=logits.detach(), grad_norms=norms, total=total.detach(),
                  **{"loss_" + k: v.detach() for k, v in losses.items()})
    for k in keep:
        out_np["grad::" + k] = grads[k]
    MG.npz(name, **out_np)


def infer_case(hp, name, B, T, T_txt, steps, wseed, iseed):
    model = build_ref(hp, steps)
    MG.load_seeded(model, wseed)
    inp = Wt.synthetic_inputs(B, T, T_txt, seed=iseed, pad_tail=True)
    noises = Wt.synthetic_noises(B, T, steps, seed=iseed + 1)
    with MG.patched_randn(noises):
        ret = model(inp["txt_tokens"], inp["time_mel_masks"], None, inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"].clone(),
                    inp["uv"].clone(), infer=True)
    det = model.forward_stutter_predictor(inp["txt_tokens"], inp["mel2ph"], inp["spk_embed"], inp["ref_mels"], inp["f0"].clone(),
                                          inp["uv"].clone())
    MG.npz(name, meta=np.array(json.dumps(dict(B=B, T=T, T_txt=T_txt, steps=steps, wseed=wseed, iseed=iseed, pad_tail=True))),
           noises=torch.stack(noises), mel_out=ret["mel_out"], stutter_predictor_out=ret["stutter_predictor_out"], detect_logits=det)


def binary_case(hp):
    """A few items with `stutter_mel_mask` in the IndexedDataset format + the reference collater's stutter_mel_masks of one batch."""
    import shutil
    from utils.commons.indexed_datasets import IndexedDatasetBuilder as RefBuilder
    from tasks.speech_editing.dataset_utils import StutterSpeechDataset as RefDS
    d = os.path.join(GOLD, "binary_stutter_tiny")
    if os.path.exists(d):
        shutil.rmtree(d)
    os.makedirs(d)
    rng = np.random.default_rng(55)
    items = []
    for i in range(6):
        n_ph = int(rng.integers(5, 9))
        dur = rng.integers(2, 6, size=n_ph)
        T = int(dur.sum())
        mel2ph = np.repeat(np.arange(1, n_ph + 1), dur)
        f0 = np.where(rng.random(T) < 0.8, rng.uniform(90, 250, T), 0.0)
        stm = (rng.random(T) < 0.3).astype(np.int64)
        if i == 5:
            stm = stm[:-2]  # shorter than the mel: collated with the pad value
        items.append({"item_name": "stutter_%d" % i, "txt": "item %d" % i, "wav_fn": "stutter_%d.wav" % i,
                      "ph_token": np.concatenate([[3], rng.integers(6, 45, size=n_ph - 1)]).astype(np.int64), "mel": rng.standard_normal((T, 80)).astype(np.float32) - 4,
                      "spk_embed": rng.standard_normal(256).astype(np.float32), "mel2ph": mel2ph.astype(np.int64), "f0": f0,
                      "pitch": np.zeros(T, dtype=np.int64), "stutter_mel_mask": stm})
    for split, sl in (("train", slice(0, 4)), ("valid", slice(4, 6)), ("test", slice(4, 6))):
        b = RefBuilder(os.path.join(d, split))
        lens = []
        for it in items[sl]:
            b.add_item(it)
            lens.append(len(it["mel"]))
        b.finalize()
        np.save(os.path.join(d, split + "_lengths.npy"), np.array(lens))
    with open(os.path.join(d, "phone_set.json"), "w") as f:
        json.dump(["|", "<BOS>", "<EOS>"] + ["P%d" % i for i in range(40)], f)
    hp2 = dict(hp)
    hp2.update(binary_data_dir=d, infer=False, max_frames=1548, frames_multiple=1, max_input_tokens=1550, use_pitch_embed=True,
               use_spk_embed=True, pitch_type="frame", test_ids=[])
    import utils.commons.hparams as RH
    saved = dict(RH.hparams)
    RH.hparams.clear()
    RH.hparams.update(hp2)
    try:
        ds = RefDS("valid", shuffle=False)
        batch = ds.collater([ds[0], ds[1]])
    finally:
        RH.hparams.clear()
        RH.hparams.update(saved)
    MG.npz("binary_stutter_tiny_batch", stutter_mel_masks=batch["stutter_mel_masks"], mels_shape=np.array(batch["mels"].shape))


def main():
    hp = ref_import.install(timesteps=4)
    m = build_ref(hp, 4)
    man = MG.manifest_of(m)
    with open(os.path.join(GOLD, "manifest_stutter_speech.json"), "w") as f:
        json.dump(man, f)
    print("manifest: %d keys" % len(man))
    train_loss_case(hp, "train_losses_stutter", B=2, T=64, T_txt=16, steps=8, wseed=31, iseed=301, step=0)
    train_loss_case(hp, "train_losses_stutter_ragged", B=3, T=77, T_txt=19, steps=8, wseed=32, iseed=112, step=12345)
    infer_case(hp, "infer_stutter", B=2, T=77, T_txt=19, steps=4, wseed=33, iseed=303)
    binary_case(hp)


if __name__ == "__main__":
    main()
