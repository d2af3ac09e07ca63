"""Vocoder training losses on the GPU.  Built: the HiFi-GAN mel loss (tasks/vocoder/hifigan.py:35-38,
`F.l1_loss(mel_spectrogram(y_), mel_spectrogram(y))`) with its gradient with respect to the generated waveform (csrc/mel_loss.hip).

    loss_fn = MelSpectrogramLoss(hparams)
    loss_mel = loss_fn(y_, y) * hparams['lambda_mel']         # y_, y: [B, 1, N] or [B, N] fp32 on the GPU

The gradient is computed eagerly in the forward whenever y_hat asks for one, and the backward only scales it by the upstream scalar: the
spectral backward wants the waveform tile of y_hat the forward has just staged, the mel gradient is a by-product of the loss launch, and a
generator step always calls backward.  It also makes a second backward (retain_graph=True) the same bits by construction.  What it costs
is the three backward launches in a forward under autograd whose loss is never differentiated; torch.no_grad() skips them.

`y` is data: a `y` that requires grad raises instead of silently getting none.  There is no CPU fallback.

Also built: the multi-resolution STFT loss (tasks/vocoder/hifigan.py:46-47 on modules/vocoder/hifigan/stft_loss.py; csrc/stft_loss.hip),
the other waveform-domain term of the generator step:

    stft_loss = MultiResolutionSTFTLoss()
    sc, mag = stft_loss(y.squeeze(1), y_.squeeze(1))          # the task's order: the REAL waveform first, the generated one second

differentiable in whichever one of the two arguments requires grad.  Its gradient is computed in backward(), once per resolution, from
the two upstream scalars combined on the device.
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


# ---- multi-resolution STFT loss -----------------------------------------------------------------------------------------------------------

class _StftLoss(torch.autograd.Function):
    """(sc, mag) of `mod`'s resolutions, averaged; backward runs the spectral backward once per resolution with both upstream scalars."""

    @staticmethod
    def forward(ctx, x, y, mod, sentinel):
        need = [bool(n) for n in ctx.needs_input_grad[:2]]
        which = 0 if need[0] else 1
        tables = mod._tables(x.device)
        keep = any(need) and not mod.recompute
        n = len(mod.geometries)
        res = [ops.stft_loss_fwd(x, y, tables[i][0], n_fft=g[0], hop=g[1], win=g[2], which=which, keep=keep, sentinel=sentinel)
               for i, g in enumerate(mod.geometries)]
        # the mean over the resolutions in the constructor's order: ((l0 + l1) + l2) / n, fp32 on the device
        tot = res[0][0]
        for r in res[1:]:
            tot = tot + r[0]
        if n > 1:
            tot = tot / n
        ctx.mod, ctx.which, ctx.sentinel = mod, which, sentinel
        ctx.stats, ctx.mags = [r[1] for r in res], [r[2] for r in res]
        ctx.save_for_backward(x, y)
        return tot[0].reshape(()), tot[1].reshape(())

    @staticmethod
    def backward(ctx, g_sc, g_mag):
        x, y = ctx.saved_tensors
        mod, which = ctx.mod, ctx.which
        u = [torch.zeros(1, dtype=torch.float32, device=x.device) if g is None else g.reshape(1).contiguous() for g in (g_sc, g_mag)]
        tables = mod._tables(x.device)
        g_wav = None
        for i, g in enumerate(mod.geometries):  # summed in the constructor's order: the first resolution writes, the others add
            g_wav = ops.stft_loss_bwd(x, y, tables[i][0], tables[i][1], n_fft=g[0], hop=g[1], win=g[2], which=which, stats=ctx.stats[i],
                                      u_sc=u[0], u_mag=u[1], scale=1.0 / len(mod.geometries), mag=ctx.mags[i], g_wav=g_wav,
                                      sentinel=ctx.sentinel)
        return (g_wav, None, None, None) if which == 0 else (None, g_wav, None, None)


class MultiResolutionSTFTLoss(torch.nn.Module):
    """The reference's MultiResolutionSTFTLoss: per resolution sc = ||y_mag - x_mag||_F / ||y_mag||_F and mag = mean |log y_mag - log
    x_mag| over the whole batch, with mag(s) = sqrt(clamp(re^2 + im^2, min=1e-7)) of torch.stft(center=True, reflect) under the periodic
    Hann window of win_length; the result is the two means over the resolutions.

    forward(x, y) -> (sc_loss, mag_loss), 0-dim.  x, y: equal fp32 GPU tensors [B, N] or [B, 1, N] with N > max(fft_size) / 2.  The task
    passes the real waveform as x and the generated one as y; the loss is differentiable in whichever ONE of them requires grad.
    `recompute=True` computes the other signal's spectrum again in backward instead of keeping its magnitudes from the forward.
    `sentinel` fills every output and scratch buffer before its kernel runs (the tests pass NaN)."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), window="hann_window",
                 recompute=False):
        super().__init__()
        if not len(fft_sizes) == len(hop_sizes) == len(win_lengths) or len(fft_sizes) == 0:
            raise ValueError("fft_sizes, hop_sizes and win_lengths must be equally long and not empty")
        if window != "hann_window":
            raise ValueError("the STFT loss is built for window='hann_window', got %r" % (window,))
        self.geometries = [tuple(int(v) for v in g) for g in zip(fft_sizes, hop_sizes, win_lengths)]
        built = ops.stft_geometries()
        for g in self.geometries:
            if g not in built:
                raise ValueError("the STFT loss has no kernels for (fft_size, hop, win_length) = %s; compiled geometries: %s" % (g, built))
        self.recompute = bool(recompute)
        self._images = ops.CacheSlot()  # per resolution (DFT table image, inverse table image) on the device last used

    def _build_images(self, device):
        out = []
        for n_fft, hop, win in self.geometries:
            table = melspec.dft_table(n_fft, win, 0, n_fft // 2 + 1)
            out.append((torch.from_numpy(melspec.pack_stft_table(table, win)).to(device),
                        torch.from_numpy(melspec.pack_stft_idft_table(table, hop, win)).to(device)))
        return out

    def _tables(self, device):
        return self._images.get((device,), lambda old: self._build_images(device))

    def _check(self, x, y):
        for t, name in ((x, "x"), (y, "y")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("%s must live on the GPU: the STFT loss has no CPU fallback" % name)
            if t.dtype != torch.float32:
                raise TypeError("%s must be float32, got %s" % (name, t.dtype))
        if x.shape != y.shape or x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
            raise ValueError("x and y must be equal [B, N] or [B, 1, N], got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        pad = max(g[0] for g in self.geometries) // 2
        if x.shape[-1] <= pad:
            raise ValueError("reflect padding of %d needs more than %d samples, got %d" % (pad, pad, x.shape[-1]))
        if torch.is_grad_enabled() and x.requires_grad and y.requires_grad:
            raise ValueError("the STFT loss is differentiable in one of its arguments; both require grad (detach the data)")

    def forward(self, x, y, sentinel=None):
        self._check(x, y)
        B, N = x.shape[0], x.shape[-1]
        return _StftLoss.apply(x.reshape(B, N).contiguous(), y.reshape(B, N).contiguous(), self, sentinel)


class STFTLoss(MultiResolutionSTFTLoss):
    """One resolution, the reference's signature: forward(x, y) -> (sc_loss, mag_loss)."""

    def __init__(self, fft_size=1024, shift_size=120, win_length=600, window="hann_window", recompute=False):
        super().__init__([fft_size], [shift_size], [win_length], window, recompute)


_STFT = {}  # (fft_size, hop_size, win_length) -> STFTLoss, for stft_magnitude's table images


def stft_magnitude(x, fft_size, hop_size, win_length, sentinel=None):
    """The reference's stft() on the GPU: x [B, N] fp32 -> sqrt(clamp(re^2 + im^2, min=1e-7)) [B, 1 + N // hop_size, fft_size/2 + 1]."""
    key = (int(fft_size), int(hop_size), int(win_length))
    fn = _STFT.get(key)
    if fn is None:
        fn = _STFT[key] = STFTLoss(*key)
    fn._check(x, x.detach())
    if x.dim() != 2:
        raise ValueError("stft_magnitude takes [B, N], got %s" % (tuple(x.shape),))
    return ops.stft_magnitude(x.detach().contiguous(), fn._tables(x.device)[0][0], n_fft=key[0], hop=key[1], win=key[2], sentinel=sentinel)
