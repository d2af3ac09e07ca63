"""StutterSpeech (FluentSpeech's stutter-oriented model) on the HIP kernels: the spec_denoiser diffusion model plus a stutter predictor
that labels every mel frame fluent / stutter / pad, and a stutter embedding added to the decoder input in training.

Module tree and state-dict keys equal modules/speech_editing/stutter_speech/spec_denoiser.py:18-30 (342 keys with egs/
stutter_speech.yaml), so reference checkpoints load with strict=True.  Conditioner order (:159-185):
  decoder_inp = fs(..., skip_decoder=True)
  stutter_predictor_out = predictor(decoder_inp, cond=MelEncoder(ref_mels) * nonpad)          (unmasked mels, before the additions)
  decoder_inp += stutter_embed[stutter_mel_masks] * nonpad                                      (training only)
  decoder_inp += MelEncoder(ref_mels * (1 - time_mel_masks)) * nonpad
then the unchanged diffusion part of GaussianDiffusion.
"""
import torch
from torch import nn

from . import autograd_ops, ops
from .fs import ConvBlocks, FastSpeech, _backend, _cw
from .spec_denoiser import GaussianDiffusion


class FastSpeechStutter(FastSpeech):
    """modules/speech_editing/stutter_speech/fs.py: the masked FastSpeech with `mel_out` and `decoder` deleted (:82-83)."""

    def __init__(self, dict_size, hp, out_dims=None):
        super().__init__(dict_size, hp, out_dims)
        del self.mel_out
        del self.decoder


class ConditionalConvBlocks(ConvBlocks):
    """modules/commons/conv.py:142-167 (is_BTC handled by the caller): x = (x + g_prenet(cond)) * nonpadding, then ConvBlocks with the
    mask recomputed from |x|.sum > 0."""

    def __init__(self, hidden_size, c_cond, c_out, dilations, kernel_size, layers_in_block=2, c_multiple=2, dropout=0.0, ln_eps=1e-5,
                 num_layers=None):
        if num_layers is not None:
            dilations = [1] * num_layers
        super().__init__(hidden_size, c_out, dilations, kernel_size, layers_in_block=layers_in_block, c_multiple=c_multiple,
                         ln_eps=ln_eps, dropout=dropout)
        self.g_prenet = nn.Conv1d(c_cond, hidden_size, 3, padding=1)
        nn.init.xavier_uniform_(self.g_prenet.weight)
        self._w_g = _cw(self.g_prenet)

    def run_cond(self, x, cond, nonpad, drop_seed=None, drop_site=0):
        x = _backend().conv1d(cond, self._w_g, self.g_prenet.bias, pad=1, res=x, mask=nonpad)
        return self.run(x, drop_seed, drop_site)


class StutterPredictor(nn.Module):
    """modules/speech_editing/stutter_speech/stutter_predictor.py:47-65: ConditionalConvBlocks (4 residual blocks of 2 pre-LN FFN units,
    k=5, dropout 0.3 on each branch) -> Linear(H, 3).  The linear layer and the losses are one kernel (ops.stutter_head /
    autograd_ops.stutter_losses)."""
    _site = 3  # Philox counter sites (seed, (3 * 16 + unit + 1) * 2^28): apart from the duration / pitch predictors' (fs._PredictorStack)

    def __init__(self, hidden_size, n_layers=4, odim=3, kernel_size=5, dropout_rate=0.3):
        super().__init__()
        self.conv = ConditionalConvBlocks(hidden_size, hidden_size, hidden_size, [1], kernel_size, num_layers=n_layers,
                                          dropout=dropout_rate)
        self.linear = nn.Linear(hidden_size, odim)

    def features(self, x, cond, nonpad, seed=0):
        """x, cond [B,H,T] -> post_net1 output [B,H,T] (the head's input)."""
        return self.conv.run_cond(x, cond, nonpad, seed, self._site * 16 + 1)

    def run(self, x, cond, nonpad, labels=None, seed=0):
        """(logits [B,T,3], ce, focal); ce / focal are None without labels (int64 [B,T] in {0, 1, 2})."""
        h = self.features(x, cond, nonpad, seed)
        if labels is None:
            return ops.stutter_head(h, self.linear.weight, self.linear.bias), None, None
        return autograd_ops.stutter_losses(h, self.linear.weight, self.linear.bias, labels)


class GaussianDiffusionStutter(GaussianDiffusion):
    """modules/speech_editing/stutter_speech/spec_denoiser.py:18-213.  Every parameter is reached by a loss (the reference deletes
    fs.decoder / fs.mel_out), so nothing is laid out as unused."""
    fs_cls = FastSpeechStutter
    unused_parameter_prefixes = ()

    def __init__(self, phone_encoder, out_dims, denoise_fn, timesteps=1000, time_scale=1, loss_type="l1", betas=None, spec_min=None,
                 spec_max=None, hp=None):
        super().__init__(phone_encoder, out_dims, denoise_fn, timesteps, time_scale, loss_type, betas, spec_min, spec_max, hp)
        H = self.fs.hidden_size
        self.stutter_embed = nn.Embedding(3, H)  # modules/commons/layers.py:45-50
        nn.init.normal_(self.stutter_embed.weight, mean=0, std=H ** -0.5)
        self.stutter_predictor = StutterPredictor(H)
        self._stutter_in = None

    def _stutter_head(self, dec_bct, ref_mels, tgt_nonpad, labels, seed):
        """predictor(decoder_inp, cond=MelEncoder(ref_mels) * nonpad, nonpad) on the unmasked mels."""
        scond = self.mel_encoder.run(ops.btc_to_bct(ref_mels.contiguous()), mask=tgt_nonpad)
        return self.stutter_predictor.run(dec_bct, scond, tgt_nonpad, labels, seed)

    def conditioner(self, txt_tokens, time_mel_masks, mel2ph, spk_embed, ref_mels, f0, uv, infer=False,
                    use_pred_mel2ph=False, use_pred_pitch=False, dropout_seed=0):
        F = autograd_ops if torch.is_grad_enabled() else ops
        labels = self._stutter_in
        ret = self.fs(txt_tokens, time_mel_masks, mel2ph, spk_embed, f0, uv, None, skip_decoder=True, infer=infer,
                      use_pred_mel2ph=use_pred_mel2ph, use_pred_pitch=use_pred_pitch, dropout_seed=dropout_seed)
        tgt_nonpad = ret["tgt_nonpad"]
        dec_p, dec = F.fanout(ret.pop("decoder_inp_bct"), 2)
        logits, ce, focal = self._stutter_head(dec_p, ref_mels, tgt_nonpad, None if infer else labels, dropout_seed)
        ret["stutter_predictor_out"] = logits
        if ce is not None:
            ret["stutter_ce"], ret["stutter_focal"] = ce, focal
        if not infer:
            # decoder_inp += stutter_embed(labels) * nonpad: the mask is the one of the mel encoder's conv epilogue below (decoder_inp is
            # already zero on padded frames), so (decoder_inp + embed + mel) * nonpad has the reference's values and gradients
            dec = F.embedding_bct(labels, self.stutter_embed.weight, out=dec, accumulate=True)
        B, T, M = ref_mels.shape
        tmask = time_mel_masks.reshape(B, T).contiguous()
        masked = ops.mul_one_minus_mask(ref_mels.contiguous(), tmask, M)  # ref_mels*(1-mask)
        cond = self.mel_encoder.run(ops.btc_to_bct(masked), res=dec, mask=tgt_nonpad)
        ret["decoder_inp"] = F.bct_to_btc(cond)
        return ret, cond

    def forward(self, txt_tokens, time_mel_masks, stutter_mel_masks, mel2ph, spk_embed, ref_mels, f0, uv, energy=None, infer=False,
                use_pred_mel2ph=False, use_pred_pitch=False, **kw):
        """The reference's signature (stutter_mel_masks: int64 [B,T] already remapped to {0: fluent, 1: stutter, 2: pad}; required
        with infer=False, unused with infer=True) and GaussianDiffusion's keyword-only parity extras.  ret also holds
        `stutter_predictor_out` [B,T,3] and, with labels, `stutter_ce` / `stutter_focal` (the head's losses, one kernel)."""
        if not infer:
            if stutter_mel_masks is None:
                raise ValueError("GaussianDiffusionStutter: stutter_mel_masks are required with infer=False")
            ops._i(stutter_mel_masks, "stutter_mel_masks")
        self._stutter_in = stutter_mel_masks
        try:
            return super().forward(txt_tokens, time_mel_masks, mel2ph, spk_embed, ref_mels, f0, uv, energy, infer, use_pred_mel2ph,
                                   use_pred_pitch, **kw)
        finally:
            self._stutter_in = None

    @torch.no_grad()
    def forward_stutter_predictor(self, txt_tokens, mel2ph, spk_embed, ref_mels, f0, uv, energy=None):
        """stutter_speech/spec_denoiser.py:187-199: detection only -- an all-zero time mask, ground-truth mel2ph and pitch, no
        diffusion.  Returns the logits [B,T,3]."""
        B, T = ref_mels.shape[0], ref_mels.shape[1]
        tmask = torch.zeros(B, T, 1, dtype=torch.float32, device=ref_mels.device)
        ret = self.fs(txt_tokens, tmask, mel2ph, spk_embed, f0, uv, None, skip_decoder=True)
        logits, _, _ = self._stutter_head(ret["decoder_inp_bct"], ref_mels, ret["tgt_nonpad"], None, 0)
        return logits
