"""Vocoder training losses on the GPU.  Built: the HiFi-GAN mel loss (tasks/vocoder/hifigan.py:35-38,
`F.l1_loss(mel_spectrogram(y_), mel_spectrogram(y))`) with its gradient with respect to the generated waveform (csrc/mel_loss.hip).

    loss_fn = MelSpectrogramLoss(hparams)
    loss_mel = loss_fn(y_, y) * hparams['lambda_mel']         # y_, y: [B, 1, N] or [B, N] fp32 on the GPU

The gradient is computed eagerly in the forward whenever y_hat asks for one, and the backward only scales it by the upstream scalar: the
spectral backward wants the waveform tile of y_hat the forward has just staged, the mel gradient is a by-product of the loss launch, and a
generator step always calls backward.  It also makes a second backward (retain_graph=True) the same bits by construction.  What it costs
is the three backward launches in a forward under autograd whose loss is never differentiated; torch.no_grad() skips them.

`y` is data: a `y` that requires grad raises instead of silently getting none.  There is no CPU fallback.
"""
import torch

from . import melspec, ops
from ._lib import check, lib as L

_HIFIGAN = melspec.FLAVOURS["hifigan"]


class _MelL1(torch.autograd.Function):
    """loss (0-dim) of the eager forward; g_wav is d loss / d y_hat, or None when nothing asked for it."""

    @staticmethod
    def forward(ctx, y_hat, loss, g_wav):
        ctx.g_wav = g_wav
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        g = ctx.g_wav
        if g is None:
            raise RuntimeError("mel loss: backward without a gradient computed in the forward")
        out = torch.empty_like(g)
        check(L().set_scale_bcast(ops._p(g), None, ops._p(out), g.numel(), 1, ops._p(gout.reshape(1).contiguous()), 1.0, ops._stream()),
              "set_scale_bcast")
        return out, None, None


class MelSpectrogramLoss(torch.nn.Module):
    """mean |ln mel(y_hat) - ln mel(y)| of mel_utils.mel_spectrogram's mel (input clamp, reflect pad of (fft_size - hop_size) / 2,
    sqrt(re^2 + im^2 + 1e-9), ln(max(mel, 1e-5))), differentiable in y_hat.

    Reads the hparams melspec.LogMel reads; `mel_basis` replaces the restated Slaney filterbank.  fft_size 1024, hop_size 256,
    n_mels <= 96, fp32 GPU tensors [B, N] or [B, 1, N] with N > 384; anything else raises.  `forward(..., return_mels=True)` also
    returns the two log-mels [B, T, n_mels] (detached; set_log_mel's bits); `sentinel` fills every output and scratch buffer before
    its kernel runs (the tests pass NaN: the kernels write every element)."""

    def __init__(self, hparams, mel_basis=None):
        super().__init__()
        fe = melspec.LogMel(hparams, "hifigan", mel_basis=mel_basis)
        if fe.n_fft != 1024 or fe.hop != 256 or fe.n_mels > 96:
            raise ValueError("the mel loss is built for fft_size 1024, hop_size 256, n_mels <= 96; got %d, %d, %d" % (fe.n_fft, fe.hop, fe.n_mels))
        self.fe = fe
        self._images = ops.CacheSlot()  # (DFT table, filterbank, transposed filterbank, inverse table) on the device last used

    def _build_images(self, device):
        fe = self.fe
        table = melspec.dft_table(fe.n_fft, fe.win_length, fe.bin_lo, fe.nbins)
        imgs = (melspec.pack_dft_table(table), melspec.pack_mel_basis(fe._basis, fe.bin_lo, fe.nbins),
                melspec.pack_mel_basis_t(fe._basis, fe.bin_lo, fe.nbins), melspec.pack_idft_table(table))
        return tuple(torch.from_numpy(i).to(device) for i in imgs)

    def _geometry(self):
        fe = self.fe
        return dict(n_fft=fe.n_fft, hop=fe.hop, n_mels=fe.n_mels, bin_lo=fe.bin_lo, nbins=fe.nbins, pad=fe.pad)

    def _check(self, y_hat, y):
        for t, name in ((y_hat, "y_hat"), (y, "y")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("%s must live on the GPU: the mel loss has no CPU fallback" % name)
            if t.dtype != torch.float32:
                raise TypeError("%s must be float32, got %s" % (name, t.dtype))
        if y.requires_grad:
            raise ValueError("y is data: the mel loss has no gradient with respect to it (pass y.detach())")
        if y_hat.shape != y.shape or y_hat.dim() not in (2, 3) or (y_hat.dim() == 3 and y_hat.shape[1] != 1):
            raise ValueError("y_hat and y must be equal [B, N] or [B, 1, N], got %s and %s" % (tuple(y_hat.shape), tuple(y.shape)))
        if y_hat.shape[-1] <= self.fe.pad:
            raise ValueError("reflect padding of %d needs more than %d samples, got %d" % (self.fe.pad, self.fe.pad, y_hat.shape[-1]))

    def forward(self, y_hat, y, return_mels=False, sentinel=None):
        self._check(y_hat, y)
        B, N = y_hat.shape[0], y_hat.shape[-1]
        # both waveforms in one buffer: one launch of 2 B rows for the two linear mels (a training segment is half a tile per row; two
        # launches of B tiles each leave most of the machine idle twice)
        both = torch.cat([y_hat.detach().reshape(B, N), y.reshape(B, N)])
        w_hat = both[:B]
        table, basis, basis_t, itable = self._images.get((w_hat.device,), lambda old: self._build_images(w_hat.device))
        geo = self._geometry()
        front = dict(geo, reflect=_HIFIGAN["reflect"], clamp_input=_HIFIGAN["clamp_input"], mag_eps=_HIFIGAN["mag_eps"], sentinel=sentinel)
        mel = ops.mel_linear(both, table, basis, **front)
        mel_hat, mel_y = mel[:B], mel[B:]
        loss, g_mel, log_hat, log_y = ops.mel_loss_fwd(mel_hat, mel_y, floor=_HIFIGAN["floor"], log_scale=_HIFIGAN["log_scale"],
                                                       return_logs=return_mels, sentinel=sentinel)
        g_wav = None
        if torch.is_grad_enabled() and y_hat.requires_grad:
            g_wav = ops.mel_loss_bwd(w_hat, g_mel, table, basis_t, itable, mag_eps=_HIFIGAN["mag_eps"], count=g_mel.numel(), sentinel=sentinel, **geo)
            g_wav = g_wav.reshape(y_hat.shape)
        out = _MelL1.apply(y_hat, loss, g_wav)
        return (out, log_hat, log_y) if return_mels else out


_CACHE = {}  # configuration -> MelSpectrogramLoss


def mel_l1_loss(y_hat, y, hparams):
    """The functional form: one MelSpectrogramLoss per configuration of the hparams it reads (as melspec.wav2spec keeps its LogMel)."""
    key = tuple(hparams.get(k) for k in melspec._HP_KEYS)
    fn = _CACHE.get(key)
    if fn is None:
        fn = _CACHE[key] = MelSpectrogramLoss({k: hparams[k] for k in melspec._HP_KEYS if k in hparams})
    return fn(y_hat, y)
