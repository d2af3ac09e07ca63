"""A plain `bench.py` run does only what its headline needs; `--full` adds the comparison lines, the CPU baseline, the other
configs (infer) and the dominant kernel's roofline over extra steps (train)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("mcd_vs_oracle", "max_abs_dmel_vs_oracle", "native_fp32_loop", "bf16x3_operand_loop", "bf16_operand_loop", "cpu_baseline",
             "speedup_vs_cpu_baseline", "e2e_b64_vocoder", "train_bf16", "campnet_train_bf16", "train_f32")


def _bench(argv, stub):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if stub:
        env["SET_AMD_BENCH_STUB_DEVICE"] = "cpu"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("mode", ["infer", "train"])
def test_full_is_an_option_of_both_modes(mode):
    plain = _bench(["--gpus", "1", "--mode", mode, "--steps", "2", "--warmup", "1"], stub=True)
    full = _bench(["--gpus", "1", "--mode", mode, "--steps", "2", "--warmup", "1", "--full"], stub=True)
    # the stub runs none of the extras: the two lines carry the same fields
    assert sorted(plain) == sorted(full)
    assert not set(FULL_ONLY) & set(plain)


@pytest.mark.gpu
def test_plain_infer_run_reports_the_headline_and_nothing_else():
    d = _bench(["--gpus", "1", "--steps", "1", "--warmup", "0"], stub=False)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d
    assert d["steps"] == 1 and d["warmup"] == 0 and d["value"] > 0
    assert d["roofline"]["launch_ms"] > 0
    assert not set(FULL_ONLY) & set(d)
