"""tests/golden/mpd_reference.npz: the reference's own MultiPeriodDiscriminator, feature_loss, generator_loss and discriminator_loss
(modules/vocoder/hifigan/hifigan.py) in float64 on the seeded weights and waveforms of tests/mpd_models.py at B = 2, T = 200 -- the
scores, every map's mean and mean-abs, and the three losses.  Data only (a few kilobytes, no weights).  Also tests/golden/mpd_bars.npz: the
float32 mirror's errors of the end-to-end cases of tests/mpd_models.py (mirror_errors), which the GPU test reads as its bars.  The GPU machine has no reference:
this file is how the reference's numbers travel.

Run on a host with the reference checkout (oracle/ref_import.py names its place); never on a GPU box.
  python tools/make_mpd_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpd_models as MM  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED_W, SEED_Y, B, T = 11, 12, 2, 200


def record(ref_module):
    """What the golden file holds, from a module with the reference's MultiPeriodDiscriminator and loss functions."""
    mpd = ref_module.MultiPeriodDiscriminator()
    mpd.load_state_dict(MM.seeded_state(SEED_W), strict=True)
    mpd = mpd.double()
    y, y_hat = (torch.from_numpy(a).double().unsqueeze(1) for a in MM.waves(SEED_Y, B, T))
    with torch.no_grad():
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = mpd(y, y_hat)
        r_loss, g_loss = ref_module.discriminator_loss(y_d_rs, y_d_gs)
        out = dict(feature_loss=ref_module.feature_loss(fmap_rs, fmap_gs), generator_loss=ref_module.generator_loss(y_d_gs), disc_r_loss=r_loss,
                   disc_g_loss=g_loss)
    out = {k: np.float64(v) for k, v in out.items()}
    for i in range(len(y_d_rs)):
        out["score_r_%d" % i] = y_d_rs[i].numpy()
        out["score_g_%d" % i] = y_d_gs[i].numpy()
        out["map_stats_r_%d" % i] = np.asarray([[m.mean().item(), m.abs().mean().item()] for m in fmap_rs[i]])
        out["map_stats_g_%d" % i] = np.asarray([[m.mean().item(), m.abs().mean().item()] for m in fmap_gs[i]])
        out["map_shapes_%d" % i] = np.asarray([list(m.shape) for m in fmap_gs[i]], np.int64)
    return out


if __name__ == "__main__":
    if not ref_import.available():
        sys.exit("the reference checkout is not present at %s" % ref_import.REF_ROOT)
    ref_import.install()
    import importlib
    rec = record(importlib.import_module("modules.vocoder.hifigan.hifigan"))
    path = os.path.join(ROOT, "tests", "golden", "mpd_reference.npz")
    np.savez(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
    # the float32 mirror's errors of the end-to-end cases (no reference needed; recorded because the mirror is slow)
    bars = {}
    for case in MM.E2E:
        for k, v in MM.mirror_errors(case).items():
            bars["%s.%s" % (case, k)] = v
    path = os.path.join(ROOT, "tests", "golden", "mpd_bars.npz")
    np.savez(path, **bars)
    print("wrote", path, os.path.getsize(path), "bytes")
