"""tests/golden/msd_reference.npz: the reference's own MultiScaleDiscriminator, feature_loss and generator_loss
(modules/vocoder/hifigan/hifigan.py) in float64 on the seeded weights and waveforms of tests/msd_models.py at B = 2, T = 333, in eval()
and in train() (hparams['hop_size'] = 256) -- the scores, every map's mean, mean-abs and shape, the two generator-side losses, and the
spectral norm's u / v after the training forward.  Data only (no weights; 166 kB, nearly all of it the u / v vectors).  Also tests/golden/msd_bars.npz: the float32
mirror's errors of the end-to-end cases of tests/msd_models.py (mirror_errors), which the GPU test reads as its bars.

Run on a host with the reference checkout (oracle/ref_import.py names its place); never on a GPU box.
  python tools/make_msd_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import msd_models as MM  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED_W, SEED_Y, B, T = 61, 62, 2, 333


def record(ref_module):
    """What the golden file holds, from a module with the reference's MultiScaleDiscriminator and loss functions."""
    import importlib
    importlib.import_module("utils.commons.hparams").hparams["hop_size"] = 256
    out = {}
    y, y_hat = (torch.from_numpy(a).double().unsqueeze(1) for a in MM.waves(SEED_Y, B, T))
    for mode in ("eval", "train"):
        msd = ref_module.MultiScaleDiscriminator()
        msd.load_state_dict(MM.seeded_state(SEED_W), strict=True)
        msd = msd.double()
        msd.train(mode == "train")
        with torch.no_grad():
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = msd(y, y_hat)
            out[mode + ".feature_loss"] = np.float64(ref_module.feature_loss(fmap_rs, fmap_gs))
            out[mode + ".generator_loss"] = np.float64(ref_module.generator_loss(y_d_gs))
        for i in range(len(y_d_rs)):
            out["%s.score_r_%d" % (mode, i)] = y_d_rs[i].numpy()
            out["%s.score_g_%d" % (mode, i)] = y_d_gs[i].numpy()
            out["%s.map_stats_r_%d" % (mode, i)] = np.asarray([[m.mean().item(), m.abs().mean().item()] for m in fmap_rs[i]])
            out["%s.map_stats_g_%d" % (mode, i)] = np.asarray([[m.mean().item(), m.abs().mean().item()] for m in fmap_gs[i]])
            out["%s.map_shapes_%d" % (mode, i)] = np.asarray([list(m.shape) for m in fmap_gs[i]], np.int64)
        if mode == "train":
            for k, v in msd.state_dict().items():
                if k.endswith("weight_u") or (k.endswith("weight_v") and k.startswith("discriminators.0.")):
                    out["train.after." + k] = v.numpy()
    return out


if __name__ == "__main__":
    if not ref_import.available():
        sys.exit("the reference checkout is not present at %s" % ref_import.REF_ROOT)
    ref_import.install()
    import importlib
    rec = record(importlib.import_module("modules.vocoder.hifigan.hifigan"))
    path = os.path.join(ROOT, "tests", "golden", "msd_reference.npz")
    np.savez(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
    bars = {}
    for case in MM.E2E:
        for k, v in MM.mirror_errors(case).items():
            bars["%s.%s" % (case, k)] = v
    path = os.path.join(ROOT, "tests", "golden", "msd_bars.npz")
    np.savez(path, **bars)
    print("wrote", path, os.path.getsize(path), "bytes")
