"""bench.py --dump-outputs: the outputs of the last timed step as DIR/<name>.npy (float32 / float64), at most 64 MB in all, the
same from run to run with the same arguments.  Runs on CPU (the stubbed device of tests/test_dist_gloo.py, and the writer itself)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stub_bench(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SET_AMD_BENCH_STUB_DEVICE"] = "cpu"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_of_the_last_timed_step_repeat_from_run_to_run(tmp_path):
    runs = []
    for tag in ("a", "b"):
        d = _stub_bench(["--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / tag)])
        assert d["steps"] == 4 and d["ms_per_step"] > 0
        assert d["dump_outputs"]["arrays"] == {"mel_out": {"shape": [32, 800, 80], "dtype": "float32"}}
        runs.append(np.load(tmp_path / tag / "mel_out.npy"))
    assert runs[0].dtype == np.float32 and runs[0].shape == (32, 800, 80)
    assert np.array_equal(runs[0], runs[1])
    # the stub's output depends on the step's seed: the file holds the LAST timed step (seed = steps - 1), not another one
    d = _stub_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "c")])
    assert not np.array_equal(np.load(tmp_path / "c" / "mel_out.npy"), runs[0])


def test_dump_outputs_train_mode_writes_losses_and_parameters(tmp_path):
    d = _stub_bench(["--gpus", "1", "--mode", "train", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "loss_mse.npy", "params.npy"]
    assert float(np.load(tmp_path / "loss.npy")) == d["loss"]
    assert np.load(tmp_path / "params.npy").shape == ((d["grad_elems"] + 255) // 256 * 256,)  # the flat parameter buffer


def test_dump_writer_converts_types_and_samples_within_the_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    named = {"big": torch.randn(300, 1000, generator=g), "half": torch.randn(50, 100, generator=g).half(),
             "ids": torch.arange(1000), "f64": torch.randn(10, dtype=torch.float64, generator=g), "timing_ms": 1.5}
    arrs = bench.host_outputs(named)
    assert sorted(arrs) == ["big", "f64", "half", "ids"]  # plain values are not outputs
    assert arrs["big"].dtype == arrs["half"].dtype == np.float32 and arrs["ids"].dtype == arrs["f64"].dtype == np.float64
    budget = 400_000  # less than the 1.2 MB of "big" alone
    infos = [bench.dump_outputs(str(tmp_path / t), arrs, budget=budget) for t in ("a", "b")]
    assert infos[0] == infos[1]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    big = np.load(tmp_path / "a" / "big.npy")
    n = infos[0]["big"]["sampled_elements"]
    assert big.shape == (n,) and 0 < n < 300 * 1000
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))     # the same elements every run
    assert np.isin(big, arrs["big"].reshape(-1)).all()
    # under the budget nothing is sampled
    small = bench.dump_outputs(str(tmp_path / "c"), {"f64": arrs["f64"]}, budget=budget)
    assert small == {"f64": {"shape": [10], "dtype": "float64"}}
    assert np.array_equal(np.load(tmp_path / "c" / "f64.npy"), arrs["f64"])
