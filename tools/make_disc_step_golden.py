"""tests/golden/disc_step_reference.npz: the reference's own MultiPeriodDiscriminator, MultiScaleDiscriminator (in eval() and in
train()) and discriminator_loss (modules/vocoder/hifigan/hifigan.py) in float64 on the seeded full-size states and waveforms of
tests/mpd_models.py / tests/msd_models.py at B = 2, T = 333, after `(r_loss + f_loss).backward()`: per parameter the gradient's sum,
L2 norm and 16 entries at seeded positions, and the two losses of each run.  Data only, no weights.  Also
tests/golden/disc_step_bars.npz: the float32 mirror's errors of the end-to-end cases of tests/disc_step_models.py (mirror_errors), which
the GPU test reads as its bars.

Run on a host with the reference checkout (oracle/ref_import.py names its place); never on a GPU box.  `--bars-only` skips the reference.
  python tools/make_disc_step_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import disc_step_models as DM  # noqa: E402
from oracle import ref_import  # noqa: E402


def record(ref_module, only=None):
    """What the golden file holds, from a module with the reference's discriminators and loss functions (`only`: one run's id)."""
    import importlib
    importlib.import_module("utils.commons.hparams").hparams["hop_size"] = 256
    out = {}
    for run in DM.GOLDEN_RUNS:
        name, kind, train, _sw, _sy = run
        if only not in (None, name):
            continue
        state, y, y_hat = DM.golden_inputs(run)
        net = ref_module.MultiPeriodDiscriminator() if kind == "mpd" else ref_module.MultiScaleDiscriminator()
        net.load_state_dict(state, strict=True)
        net = net.double()
        net.train(train)
        y_d_rs, y_d_gs, _fr, _fg = net(torch.from_numpy(y).double().unsqueeze(1), torch.from_numpy(y_hat).double().unsqueeze(1))
        r, f = ref_module.discriminator_loss(y_d_rs, y_d_gs)
        (r + f).backward()
        out[name + ".losses"] = np.asarray([r.item(), f.item()])
        for k, q in net.named_parameters():
            out["%s.grad.%s" % (name, k)] = DM.golden_stats(k, q.grad.numpy())
    return out


if __name__ == "__main__":
    if "--bars-only" not in sys.argv:
        if not ref_import.available():
            sys.exit("the reference checkout is not present at %s" % ref_import.REF_ROOT)
        ref_import.install()
        import importlib
        rec = record(importlib.import_module("modules.vocoder.hifigan.hifigan"))
        path = os.path.join(ROOT, "tests", "golden", "disc_step_reference.npz")
        np.savez(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
    bars = {}
    for case in DM.E2E:
        for k, v in DM.mirror_errors(case).items():
            bars["%s.%s" % (case, k)] = v
        print(case, "undecided (real, generated):", bars[case + ".undecided"])
    path = os.path.join(ROOT, "tests", "golden", "disc_step_bars.npz")
    np.savez(path, **bars)
    print("wrote", path, os.path.getsize(path), "bytes")
