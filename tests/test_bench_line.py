"""What a bench.py line carries: a plain run the headline alone, --full the per-kernel durations and the roofline besides
(and, at full size, the CPU baseline and the other workloads — too slow for the suite)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernels_ms", "roofline", "cpu_baseline", "long_run", "generic", "run_time_specialisation", "rung4", "env_wrapper")


def _line(*argv) -> dict:
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "256", "--steps", "3",
                        "--warmup", "1", *argv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def plain() -> dict:
    return _line()


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(plain):
    assert all(plain.get(k) is not None for k in HEADLINE)
    assert plain["unit"] == "agent-steps/s" and plain["higher_is_better"] is True and plain["dtype"] == "u8"
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["rounds"]["n"] == 3
    assert not plain.keys() & set(FULL_ONLY)


@pytest.mark.gpu
def test_full_line_adds_the_kernel_figures(plain):
    full = _line("--full", "--no-cpu", "--no-extras")
    assert {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype")} == \
           {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype")}
    assert full["kernels_ms"]["mgx_obs_kernel"] > 0
    assert full["roofline"]["kernel"] in ("mgx_obs_kernel", "mgx_world_kernel_fast") and full["roofline"]["achieved"] > 0
    assert "cpu_baseline" not in full and "rung4" not in full
