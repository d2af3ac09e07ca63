"""Task-level operator surface of the hot path.

`SpeechEditingBaseTask` carries what both tasks share with the Trainer; `DIFF_DECODERS` and `SpeechDenoiserTask` mirror tasks/speech_editing/spec_denoiser.py:13-62 (registry,
`build_tts_model`, `run_model` incl. the `mel_out*mask + target*(1-mask)` paste), the loss functions of the task base
classes (tasks/tts/speech_base.py:219-257, speech_editing_base.py:58-108) and the hooks the Trainer counterpart
(trainer.py) drives: `configure_optimizers`, `train_dataloader` / `val_dataloader`, `_training_step`,
`validation_step`, `test`.  `start()` dispatches training or `--infer` like utils/commons/base_task.py:203-229.
"""
import importlib
import json
import os

import torch

from . import autograd_ops, ops
from .diffnet import DiffNet
from .hparams import hparams, set_hparams
from .spec_denoiser import GaussianDiffusion, GaussianDiffusionNormal
from .stutter_speech import GaussianDiffusionStutter
from .text_encoder import build_token_encoder
from .vocoder_infer import get_vocoder_cls

DIFF_DECODERS = {
    "wavenet": lambda hp: DiffNet(hp["audio_num_mel_bins"], hp),
}

# dotted task paths of the reference's yaml files -> classes of this package
TASK_ALIASES = {
    "tasks.speech_editing.spec_denoiser.SpeechDenoiserTask": "set_amd.tasks.SpeechDenoiserTask",
    "tasks.speech_editing.campnet.CampNetTask": "set_amd.tasks.CampNetTask",
    "tasks.speech_editing.spec_denoiser_normal.SpeechDenoiserNormalTask": "set_amd.tasks.SpeechDenoiserNormalTask",
    "tasks.speech_editing.stutter_speech.StutterSpeechTask": "set_amd.tasks.StutterSpeechTask",
}


class SpeechEditingBaseTask:
    """What the Trainer counterpart drives, shared by the two tasks of the path (tasks/speech_editing/
    speech_editing_base.py:16-192 over tasks/tts/speech_base.py:35-380 and utils/commons/base_task.py:24-232): phone set +
    vocoder in the constructor, `build_model`, optimizer, train / validation loaders over `StutterSpeechDataset`,
    `_training_step`, `validation_step`, the dataset-driven `test`, and `start()`.  Subclasses provide `build_tts_model`
    and `run_model`."""

    def __init__(self, build_vocoder=True):
        # phone set: <binary_data_dir>/phone_set.json through the reference's TokenTextEncoder layout
        # (tasks/tts/speech_base.py:40-44): 3 reserved ids first, so len() = 3 + the phones in the file.  Without the
        # file (synthetic batches) the dictionary is `dict_size` anonymous ids and the silence ids come from hparams.
        ph_path = os.path.join(hparams.get("binary_data_dir", "") or "", "phone_set.json")
        if os.path.exists(ph_path):
            self.token_encoder = build_token_encoder(ph_path)
            self.sil_ids = self.token_encoder.sil_ids()  # speech_editing_base.py:20
        else:
            self.token_encoder = list(range(int(hparams.get("dict_size", 80))))
            self.sil_ids = [int(i) for i in hparams.get("sil_token_ids", [1, 2, 3])]
        self._sil_lut = ops.CacheSlot()  # is_sil by token id (word_ids)
        self.vocoder = None
        if build_vocoder and os.path.exists(os.path.join(hparams.get("vocoder_ckpt", "") or "", "config.yaml")):
            self.vocoder = get_vocoder_cls(hparams["vocoder"])()
        self.model = None
        self.global_step = 0

    def build_tts_model(self):
        raise NotImplementedError

    def run_model(self, sample, infer=False, **kwargs):
        raise NotImplementedError

    def build_model(self):
        self.build_tts_model()
        if hparams.get("load_ckpt", "") != "":  # speech_base.py:143-144
            from .ckpt_utils import load_ckpt
            load_ckpt(self.model, hparams["load_ckpt"])
        return self.model

    def training_step(self, sample, optimizer, **kwargs):
        """One optimisation step: forward + losses, backward, gradient all-reduce (if distributed), clip + AdamW."""
        return _optimisation_step(self, sample, optimizer, **kwargs)

    def loss_terms(self, losses):
        """The terms training_step sums into the optimised total (every loss, unweighted)."""
        return list(losses.values())

    # ---- Trainer hooks (tasks/tts/speech_base.py:59-137,140-205; utils/commons/base_task.py:60-65) -----------------
    def configure_optimizers(self):
        """AdamW(lr, betas, weight_decay) + WarmupSchedule + clip_grad_norm as ONE fused flat optimizer
        (speech_base.py:154-170, base_task.py:129-137)."""
        from .training import FlatAdamW
        if hparams.get("scheduler", "warmup") not in ("warmup",):
            raise NotImplementedError("scheduler %r (only 'warmup' is on this path)" % hparams.get("scheduler"))
        return FlatAdamW(self.model, lr=hparams["lr"],
                         betas=(hparams["optimizer_adam_beta1"], hparams["optimizer_adam_beta2"]),
                         weight_decay=hparams["weight_decay"], clip_grad_norm=hparams["clip_grad_norm"],
                         warmup_updates=hparams["warmup_updates"])

    def _loader(self, prefix, shuffle, max_tokens, max_sentences, endless, use_batch_by_size=True):
        from .data import StutterSpeechDataset, build_batches
        from .trainer import BatchLoader, RNG_LOCK
        tr = getattr(self, "trainer", None)
        world, rank = (tr.world, tr.rank) if tr is not None else (1, 0)
        import numpy as np
        ds = StutterSpeechDataset(prefix, hparams, shuffle=shuffle)
        # the batch list is a function of hparams['seed'] alone (the reference draws it from the global numpy generator
        # seeded in start(); here the generator is seeded for this call, so validation passes or data-loader rebuilds in
        # between cannot shift it -- a resumed run gets the list of the run it continues, on every rank)
        with RNG_LOCK:  # (the prefetch worker reseeds the same global generator inside BatchLoader.fetch)
            state = np.random.get_state()
            np.random.seed(int(hparams.get("seed", 1234)))
            try:
                batches = build_batches(ds, shuffle, max_tokens, max_sentences, endless=endless,
                                        use_batch_by_size=use_batch_by_size, world=world, rank=rank)
            finally:
                np.random.set_state(state)
        return BatchLoader(ds, batches, hparams.get("seed", 1234))

    def train_dataloader(self):
        return self._loader(hparams["train_set_name"], True, hparams["max_tokens"], hparams["max_sentences"],
                            hparams["endless_ds"])

    def val_dataloader(self):
        bd = hparams.get("binary_data_dir", "") or ""
        if not os.path.exists(os.path.join(bd, hparams["valid_set_name"] + ".idx")):
            return None
        return self._loader(hparams["valid_set_name"], False, hparams["max_valid_tokens"],
                            hparams["max_valid_sentences"], False, use_batch_by_size=False)

    def _training_step(self, sample, batch_idx, optimizer_idx=-1, **kwargs):
        """speech_base.py:172-176: (sum of the losses that carry a gradient, loss dict + batch_size)."""
        losses, _ = self.run_model(sample, infer=False, **kwargs)
        with torch.enable_grad():
            total = sum(v for v in losses.values() if isinstance(v, torch.Tensor) and v.requires_grad)
        log = {k: v.detach() for k, v in losses.items()}
        log["batch_size"] = sample["txt_tokens"].shape[0]
        return total, log

    def validation_step(self, sample, batch_idx):
        """speech_base.py:193-203 without the plot / vocoder side effects: the loss dict on a validation batch."""
        losses, _ = self.run_model(sample, infer=False, tape=False, seed=batch_idx)
        losses = {k: float(v) for k, v in losses.items()}
        return {"losses": losses, "total_loss": sum(losses.values()), "nsamples": sample.get("nsamples", 1)}

    # ---- dataset-driven inference: `--infer`  (utils/commons/base_task.py:203-229, speech_editing_base.py:151-192) --
    @torch.no_grad()
    def test_step(self, sample, batch_idx, gen_dir):
        """One utterance: edit the masked region, vocode prediction (+ ground truth), write the wavs."""
        from scipy.io import wavfile
        import numpy as np
        assert sample["txt_tokens"].shape[0] == 1, "only support batch_size=1 in inference"
        out = self.run_model(sample, infer=True)
        item_name, text = sample["item_name"][0], sample["text"][0]
        mel_gt = sample["mels"][0].cpu().numpy()
        mel_pred = out["mel_out"][0].cpu().numpy()
        tm = sample["time_mel_masks"][0].cpu().numpy()
        base_fn = "[%06d][%s][%%s]" % (batch_idx, str(item_name).replace("%", "_"))
        if text is not None:
            base_fn += str(text).replace(":", "$3A")[:80]
        base_fn = base_fn.replace(" ", "_")
        written = {}
        jobs = [("P", mel_pred), ("P_SEG", mel_pred[tm == 1])]
        if hparams.get("save_gt", True):
            jobs += [("G", mel_gt), ("G_SEG", mel_gt[tm == 1])]
        for tag, mel in jobs:
            if self.vocoder is None or mel.shape[0] == 0:
                continue
            wav = self.vocoder.spec2wav(mel)
            fn = os.path.join(gen_dir, "wavs", (base_fn % tag) + ".wav")
            wavfile.write(fn, hparams["audio_sample_rate"], (np.clip(wav, -1, 1) * 32767).astype(np.int16))
            written[tag] = fn
        return {"item_name": item_name, "text": text, "wav_fn_pred": base_fn % "P", "wav_fn_gt": base_fn % "G",
                "wav_fn_orig": sample["wav_fn"][0], "mel_pred": mel_pred, "files": written}

    def test(self, max_items=None, device="cuda"):
        """Run the test set of <binary_data_dir> one utterance at a time; returns the per-item dicts and writes
        checkpoints/<exp>/generated_<step>_<gen_dir_name>/{wavs/*.wav, meta.csv} like the reference."""
        from .ckpt_utils import get_last_checkpoint, load_ckpt
        from .data import StutterSpeechDataset
        hparams["infer"] = True
        random_seed = int(hparams.get("seed", 1234))
        import random
        import numpy as np
        random.seed(random_seed)
        np.random.seed(random_seed)
        self.build_model()
        work_dir = hparams.get("work_dir") or ""
        step = 0
        if work_dir and get_last_checkpoint(work_dir)[0] is not None:
            load_ckpt(self.model, work_dir, "model")
            step = int(get_last_checkpoint(work_dir)[0].get("global_step", 0))
        self.model.to(device).eval()
        ds = StutterSpeechDataset(hparams.get("test_set_name", "test"), hparams)
        gen_dir = os.path.join(work_dir or ".", "generated_%d_%s" % (step, hparams.get("gen_dir_name", "")))
        os.makedirs(os.path.join(gen_dir, "wavs"), exist_ok=True)
        results = []
        n = len(ds) if max_items is None else min(len(ds), max_items)
        for i in range(n):
            batch = ds.collater([ds[i]])
            batch = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
            results.append(self.test_step(batch, i, gen_dir))
        with open(os.path.join(gen_dir, "meta.csv"), "w") as f:
            f.write("item_name,text,wav_fn_pred,wav_fn_gt,wav_fn_orig\n")
            for r in results:
                f.write(",".join(str(r[k]) for k in ("item_name", "text", "wav_fn_pred", "wav_fn_gt", "wav_fn_orig")) + "\n")
        return results

    @classmethod
    def start(cls):
        """utils/commons/base_task.py:203-229: seed python / numpy, build the Trainer from hparams, fit or test."""
        import random
        import numpy as np
        from .trainer import Trainer
        if hparams.get("validate") or hparams.get("debug"):
            ops.set_validate(True)  # index range checks before every embedding lookup (a wrong dictionary size fails loudly)
        random.seed(hparams.get("seed", 1234))
        np.random.seed(hparams.get("seed", 1234))
        trainer = Trainer(work_dir=hparams.get("work_dir") or "checkpoints/tmp",
                          val_check_interval=hparams.get("val_check_interval", 2000),
                          max_updates=hparams.get("max_updates", 2000000),
                          num_sanity_val_steps=hparams.get("num_sanity_val_steps", 0) if not hparams.get("validate") else 10000,
                          accumulate_grad_batches=hparams.get("accumulate_grad_batches", 1),
                          num_ckpt_keep=hparams.get("num_ckpt_keep", 3), seed=hparams.get("seed", 1234),
                          log_interval=hparams.get("tb_log_interval", 100))
        if not hparams.get("infer"):
            trainer.fit(cls)
        else:
            trainer.test(cls)
        return trainer

class SpeechDenoiserTask(SpeechEditingBaseTask):
    model_cls = GaussianDiffusion

    def build_tts_model(self):
        self.model = self.model_cls(
            phone_encoder=self.token_encoder, out_dims=hparams["audio_num_mel_bins"],
            denoise_fn=DIFF_DECODERS[hparams["diff_decoder_type"]](hparams),
            timesteps=hparams["timesteps"], time_scale=hparams["timescale"], loss_type=hparams["diff_loss_type"],
            spec_min=hparams["spec_min"], spec_max=hparams["spec_max"], hp=hparams)
        return self.model

    # ---- losses (tasks/tts/speech_base.py:219-257, tasks/speech_editing/speech_editing_base.py:58-108) ----------
    def word_ids(self, txt_tokens):
        """word_id = cumsum(is_sil) * (1 - is_sil)  (speech_editing_base.py:69-78); silence = the phone set's
        non-alphabetic tokens incl. the reserved ones (`self.sil_ids`, see __init__)."""
        # is_sil through a lookup table over the token ids (one gather instead of a compare + or per silence id: 11 -> 4 launches per step;
        # token ids are < len(token_encoder), the size of the embedding table they index)
        sil_ids = [int(i) for i in self.sil_ids]

        def build(_):
            lut = torch.zeros(max(len(self.token_encoder), max(sil_ids, default=0) + 1), dtype=torch.int64)
            lut[sil_ids] = 1
            return lut.to(txt_tokens.device)
        sil = self._sil_lut.get((txt_tokens.device, tuple(sil_ids), len(self.token_encoder)), build)[txt_tokens]
        word_id = (sil.cumsum(-1) * (1 - sil)).contiguous()
        # number of word slots: the reference sizes its scatter target with word_id.max() + 1, a device->host read in the
        # middle of every step; T_txt is an upper bound (a word has at least one token) and the empty slots have zero
        # ground-truth duration, i.e. weight 0 in the loss -- same sums, no synchronisation
        return word_id, int(txt_tokens.shape[1])

    def compute_losses(self, output, sample):
        """The loss dict of run_model(infer=False): l1_coarse, ssim_coarse, pdur, wdur, uv, f0 (all on the tape)."""
        if float(hparams.get("lambda_sent_dur", 0.0)) > 0:
            # speech_editing_base.py:86-89; every shipped config sets it to 0 -- refuse rather than silently drop a loss
            raise NotImplementedError("lambda_sent_dur > 0 (the `sdur` loss) is not implemented on this path")
        if not float(hparams.get("lambda_word_dur", 1.0)) > 0:
            raise NotImplementedError("lambda_word_dur <= 0: the reference then emits no `wdur` term; not implemented")
        A = autograd_ops
        target = sample["mels"].contiguous()
        B, T, M = target.shape
        tm = sample["time_mel_masks"].reshape(B, T).contiguous()
        pred = A.bct_to_btc(A.add_chan_mask(output["mel_out_bct"], None, tm))          # mel_out * mask
        target_m = ops.blend_mask(torch.zeros_like(target), target, tm, M)             # target * mask
        w = A.frame_weights(target_m)
        losses = {}
        for item in str(hparams["mel_losses"]).split("|"):
            name, lam = (item.split(":") + ["1.0"])[:2]
            if name == "l1":
                losses["l1_coarse"] = A.masked_l1(pred, target_m, w) * float(lam)
            elif name == "ssim":
                losses["ssim_coarse"] = A.ssim_loss(pred, target_m, w) * float(lam)
            else:
                raise NotImplementedError("mel loss %r" % name)
        word_id, n_words = self.word_ids(sample["txt_tokens"])
        losses["pdur"], losses["wdur"] = A.dur_losses(output["dur"], sample["mel2ph"], sample["txt_tokens"], word_id,
                                                       n_words, hparams["lambda_ph_dur"], hparams["lambda_word_dur"])
        if hparams["use_pitch_embed"]:
            losses["uv"], losses["f0"] = A.pitch_losses(output["pitch_pred_bct"], sample["f0"], sample["uv"],
                                                        sample["mel2ph"], hparams["lambda_uv"], hparams["lambda_f0"])
        return losses

    def run_model(self, sample, infer=False, tape=True, **kwargs):
        """tasks/speech_editing/spec_denoiser.py:39-62.  infer=False returns (losses, output) on an autograd tape
        whose every node is a kernel of libset_amd.so (tape=False: the same losses with no graph kept -- validation);
        infer=True returns the pasted output."""
        if not infer:
            target = sample["mels"]
            tmask = sample["time_mel_masks"][:, :, None]
            spk = sample.get("spk_embed") if not hparams["use_spk_id"] else sample.get("spk_ids")
            with (torch.enable_grad() if tape else torch.no_grad()):
                output = self.model(sample["txt_tokens"], tmask, mel2ph=sample["mel2ph"], spk_embed=spk,
                                    ref_mels=target, f0=sample["f0"], uv=sample["uv"], energy=None, infer=False, **kwargs)
                losses = self.compute_losses(output, sample)
            with torch.no_grad():
                B, T, M = target.shape
                output["mel_out"] = ops.blend_mask(target.contiguous(), output["mel_out"].detach().contiguous(),
                                                   tmask.reshape(B, T).contiguous(), M)
            return losses, output
        return self._run_model_infer(sample, **kwargs)

    @torch.no_grad()
    def _run_model_infer(self, sample, **kwargs):
        target = sample["mels"]
        tmask = sample["time_mel_masks"][:, :, None]
        spk = sample.get("spk_embed") if not hparams["use_spk_id"] else sample.get("spk_ids")
        output = self.model(sample["txt_tokens"], tmask, mel2ph=sample["mel2ph"], spk_embed=spk, ref_mels=target,
                            f0=sample["f0"], uv=sample["uv"], energy=None, infer=True, **kwargs)
        B, T, M = target.shape
        # mel_out*mask + target*(1-mask)   (spec_denoiser.py:53)
        output["mel_out"] = ops.blend_mask(target.contiguous(), output["mel_out"], tmask.reshape(B, T).contiguous(), M)
        return output

class SpeechDenoiserNormalTask(SpeechDenoiserTask):
    """tasks/speech_editing/spec_denoiser_normal.py:18-102 (egs/spec_denoiser_wo_masked_predictor.yaml:50): the same
    task over the GaussianDiffusion whose conditioner has no masked predictors."""
    model_cls = GaussianDiffusionNormal


class StutterSpeechTask(SpeechDenoiserTask):
    """tasks/speech_editing/stutter_speech.py:20-156 (egs/stutter_speech.yaml): the spec_denoiser task over GaussianDiffusionStutter,
    plus the stutter predictor's cross-entropy and focal losses, weighted by the global step in the optimised total (the logged losses
    stay unweighted), and the frame accuracies in validation."""
    model_cls = GaussianDiffusionStutter

    @staticmethod
    def remap_stutter_labels(m):
        """stutter_speech.py:75-76 without mutating the batch: > 0 -> 1 (stutter), < 0 -> 2 (pad: the collate fills with
        stutter_pad_idx = -1), 0 stays 0 (fluent).  int64 [B,T]."""
        return ((m > 0).long() + 2 * (m < 0).long()).contiguous()

    def loss_weights(self):
        """stutter_speech.py:101-104 at self.global_step; every other loss has weight 1."""
        g = self.global_step + 1
        return {"ce": 8e-3 + 5e-3 * g / 100000, "focal": 1 + 2 * g / 100000}

    def loss_terms(self, losses):
        w = self.loss_weights()
        with torch.enable_grad():
            return [v * w[k] if k in w else v for k, v in losses.items()]

    def run_model(self, sample, infer=False, tape=True, **kwargs):
        """stutter_speech.py:59-95.  infer=False: (losses, output), the loss dict in the reference's order (l1 / ssim, pdur, wdur, ce,
        focal, uv, f0); infer=True: the pasted output, `stutter_mel_masks` optional."""
        target = sample["mels"]
        labels = sample.get("stutter_mel_masks")
        if labels is not None:
            labels = self.remap_stutter_labels(labels)
            T = target.shape[1]
            if labels.shape[1] != T:  # masks collated narrower than the mels (an item's mask shorter than its mel): no label = pad
                labels = torch.nn.functional.pad(labels[:, :T], (0, max(0, T - labels.shape[1])), value=2).contiguous()
        tmask = sample["time_mel_masks"][:, :, None]
        spk = sample.get("spk_embed") if not hparams["use_spk_id"] else sample.get("spk_ids")
        if infer:
            with torch.no_grad():
                output = self.model(sample["txt_tokens"], tmask, labels, mel2ph=sample["mel2ph"], spk_embed=spk, ref_mels=target,
                                    f0=sample["f0"], uv=sample["uv"], energy=None, infer=True, **kwargs)
                B, T, M = target.shape
                output["mel_out"] = ops.blend_mask(target.contiguous(), output["mel_out"], tmask.reshape(B, T).contiguous(), M)
            return output
        if labels is None:
            raise KeyError("StutterSpeechTask: the batch has no 'stutter_mel_masks' (binarise with stutter masks)")
        with (torch.enable_grad() if tape else torch.no_grad()):
            output = self.model(sample["txt_tokens"], tmask, labels, mel2ph=sample["mel2ph"], spk_embed=spk, ref_mels=target,
                                f0=sample["f0"], uv=sample["uv"], energy=None, infer=False, **kwargs)
            base = self.compute_losses(output, sample)
        losses = {}
        for k in ("l1_coarse", "ssim_coarse", "pdur", "wdur"):
            if k in base:
                losses[k] = base.pop(k)
        losses["ce"], losses["focal"] = output.pop("stutter_ce"), output.pop("stutter_focal")
        losses.update(base)  # uv, f0
        output["stutter_mel_masks"] = labels
        with torch.no_grad():
            B, T, M = target.shape
            output["mel_out"] = ops.blend_mask(target.contiguous(), output["mel_out"].detach().contiguous(),
                                               tmask.reshape(B, T).contiguous(), M)
        return losses, output

    def _training_step(self, sample, batch_idx, optimizer_idx=-1, **kwargs):
        """stutter_speech.py:97-107: the step-weighted sum of the losses that carry a gradient."""
        losses, _ = self.run_model(sample, infer=False, **kwargs)
        w = self.loss_weights()
        with torch.enable_grad():
            total = sum(w.get(k, 1) * v for k, v in losses.items() if isinstance(v, torch.Tensor) and v.requires_grad)
        log = {k: v.detach() for k, v in losses.items()}
        log["batch_size"] = sample["txt_tokens"].shape[0]
        return total, log

    @staticmethod
    def frame_accuracy(logits, labels):
        """stutter_speech.py:131-140: acc = correctly predicted class-0 and class-1 frames / numel (pads in the denominator); acc_1 =
        class-1 recall, None without class-1 frames."""
        pred = logits.argmax(dim=-1)
        hit = pred == labels
        acc = ((hit & (pred == 0)).float().sum() + (hit & (pred == 1)).float().sum()) / labels.numel()
        ones = labels == 1
        acc_1 = (pred[ones] == 1).float().sum() / ones.sum().float() if bool(ones.any()) else None
        return acc, acc_1

    def validation_step(self, sample, batch_idx):
        """stutter_speech.py:109-156 without plots: the unweighted loss dict, `acc` / `acc_1`, and total_loss = the sum of the dict
        INCLUDING acc (the reference's quirk, kept)."""
        losses, output = self.run_model(sample, infer=False, tape=False, seed=batch_idx)
        acc, acc_1 = self.frame_accuracy(output["stutter_predictor_out"], output["stutter_mel_masks"])
        losses["acc"] = acc
        if acc_1 is not None:
            losses["acc_1"] = acc_1
        losses = {k: float(v) for k, v in losses.items()}
        return {"losses": losses, "total_loss": sum(losses.values()), "nsamples": sample.get("nsamples", 1)}

    @torch.no_grad()
    def predict_stutter(self, sample):
        """Detection: per-frame class ids int64 [B,T] (0 fluent, 1 stutter, 2 pad) from forward_stutter_predictor (all-zero time
        mask, ground-truth mel2ph and pitch, no diffusion)."""
        spk = sample.get("spk_embed") if not hparams["use_spk_id"] else sample.get("spk_ids")
        logits = self.model.forward_stutter_predictor(sample["txt_tokens"], sample["mel2ph"], spk, sample["mels"], sample["f0"],
                                                      sample["uv"])
        return logits.argmax(dim=-1)


class CampNetTask(SpeechEditingBaseTask):
    """tasks/speech_editing/campnet.py:19-138 (BASELINE configs[4]): `CampNetTask(SpeechEditingBaseTask)` -- the phone and
    word dictionaries of <binary_data_dir> size the model (`word_set.json`, campnet.py:22-23,28-31), `run_model` returns
    the coarse + fine masked mel losses and `mel_out` = the fine prediction pasted into the original (:49-82), one AdamW
    over all parameters with the warm-up schedule (:119-138), and the base class's `start()` / loaders over
    `StutterSpeechDataset` / validation / `--infer` test loop.  The attention-statistics logging (:101-117) and the
    tensorboard side of `save_valid_result` are not part of the build."""

    def __init__(self, ph_dict_size=None, word_dict_size=None, build_vocoder=True):
        super().__init__(build_vocoder=build_vocoder)
        bd = hparams.get("binary_data_dir", "") or ""
        word_path = os.path.join(bd, "word_set.json")
        self.word_encoder = build_token_encoder(word_path) if os.path.exists(word_path) else None
        if ph_dict_size is None:
            ph_dict_size = len(self.token_encoder)
        if word_dict_size is None:
            word_dict_size = len(self.word_encoder) if self.word_encoder is not None else hparams.get("word_dict_size", 100)
        self.ph_dict_size, self.word_dict_size = int(ph_dict_size), int(word_dict_size)

    def build_tts_model(self):
        from .campnet import CampNet
        self.model = CampNet(self.ph_dict_size, self.word_dict_size, hparams)
        return self.model

    def compute_losses(self, output, sample):
        """add_mel_loss on `mel_out_{coarse,fine} * mask` vs `mels * mask` (campnet.py:63-64; speech_base.py:219-257)."""
        A = autograd_ops
        target = sample["mels"].contiguous()
        B, T, M = target.shape
        tm = sample["time_mel_masks"].reshape(B, T).contiguous()
        target_m = ops.blend_mask(torch.zeros_like(target), target, tm, M)
        w = A.frame_weights(target_m)
        losses = {}
        for post in ("coarse", "fine"):
            pred = A.bct_to_btc(A.add_chan_mask(output["mel_out_%s_bct" % post], None, tm))
            pred_l1, pred_ssim = A.fanout(pred, 2)
            for item in str(hparams["mel_losses"]).split("|"):
                name, lam = (item.split(":") + ["1.0"])[:2]
                if name == "l1":
                    losses["l1_" + post] = A.masked_l1(pred_l1, target_m, w) * float(lam)
                elif name == "ssim":
                    losses["ssim_" + post] = A.ssim_loss(pred_ssim, target_m, w) * float(lam)
                else:
                    raise NotImplementedError("mel loss %r" % name)
        return losses

    def run_model(self, sample, infer=False, tape=True, **kwargs):
        """campnet.py:49-82.  `seed` / `t` (the Trainer passes every task the update's random streams) are not used: every
        dropout of egs/campnet.yaml is 0 and the model draws no noise.  tape=False: the losses without an autograd graph
        (validation)."""
        mels = sample["mels"]
        tmask = sample["time_mel_masks"][:, :, None]
        B, T, M = mels.shape
        if not infer:
            with (torch.enable_grad() if tape else torch.no_grad()):
                output = self.model(sample["txt_tokens"], spk_embed=sample.get("spk_embed"), spk_id=sample.get("spk_ids"),
                                    mels=mels, time_mel_masks=tmask, infer=False, global_step=self.global_step)
                losses = self.compute_losses(output, sample)
        else:
            with torch.no_grad():
                output = self.model(sample["txt_tokens"], spk_embed=sample.get("spk_embed"), spk_id=sample.get("spk_ids"),
                                    mels=mels, time_mel_masks=tmask, infer=True)
        with torch.no_grad():
            output["mel_out"] = ops.blend_mask(mels.contiguous(), output["mel_out_fine"].detach().contiguous(),
                                               tmask.reshape(B, T).contiguous(), M)
        return (losses, output) if not infer else output

    def training_step(self, sample, optimizer, **kwargs):
        out = _optimisation_step(self, sample, optimizer, **kwargs)
        self.global_step += 1
        return out


def _optimisation_step(task, sample, optimizer, **kwargs):
    """zero_grad -> run_model -> backward -> optimizer.step (base_task.py:101-137 for one optimizer).  A step that
    fails half way must not leave the zero arena open (later `_gzeros` calls would hand out stale, non-zero slices)."""
    optimizer.zero_grad()
    try:
        losses, _ = task.run_model(sample, infer=False, **kwargs)
        with torch.enable_grad():  # callers may run under a global no_grad
            total = autograd_ops.sum_losses(task.loss_terms(losses))
        total.backward()
    except BaseException:
        optimizer.abort_step()
        raise
    lr, _ = optimizer.step()
    return total.detach(), {k: v.detach() for k, v in losses.items()}, lr


def run_task():
    """tasks/run.py:9-14."""
    path = TASK_ALIASES.get(hparams["task_cls"], hparams["task_cls"])
    pkg, cls_name = path.rsplit(".", 1)
    return getattr(importlib.import_module(pkg), cls_name).start()


if __name__ == "__main__":
    set_hparams()
    run_task()
