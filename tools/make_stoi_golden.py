"""tests/golden/stoi_reference.json: the reference's own eval/stoi.py `stoi(x, y, 22050, extended=False)` on the seeded synthetic pairs of
tests/stoi_models.py -- case ids, lengths, seeds and the reference's d (null where it returns None).  The GPU machine has no reference:
this file is how the reference's numbers travel.

Run on a host with the reference checkout (oracle/ref_import.py names its place); never on a GPU box.
  python tools/make_stoi_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stoi_models as SM  # noqa: E402
from oracle import ref_import  # noqa: E402

if not ref_import.available():
    sys.exit("the reference checkout is not present at %s" % ref_import.REF_ROOT)
ref = SM.load_reference_stoi(ref_import.REF_ROOT)
cases = []
for name, c in SM.E2E.items():
    x, y = SM.pair(name)
    d = ref.stoi(x, y, SM.FS, extended=False)
    cases.append(dict(id=name, n=c["n"], seed=c["seed"], snr_db=c["snr_db"], d=None if d is None else float(d)))
    print(name, cases[-1]["d"], SM.stoi64(x, y)["d"])
out = os.path.join(ROOT, "tests", "golden", "stoi_reference.json")
with open(out, "w") as f:
    json.dump(dict(function="eval/stoi.py stoi(x, y, 22050, extended=False)", cases=cases), f, indent=1)
    f.write("\n")
print("wrote", out)
