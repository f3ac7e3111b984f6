"""bench.py's two kinds of run.  A plain run prints the headline line and none of the legs that take runs of their own; `--full`
adds them (the CPU baseline and the parity sample against the reference).  The tiny workloads keep every run to seconds."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_LEGS = ("cpu_baseline", "parity_sample", "boundary")


def _line(workload, *extra):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", workload, *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"bench.py failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_full_option_is_listed():
    """argparse answers --help before anything touches a GPU"""
    p = subprocess.run([sys.executable, BENCH, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["tiny", "tiny-d"])
def test_plain_and_full_lines(workload):
    plain = _line(workload)
    for k in HEADLINE:
        assert k in plain, k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["unit"] == "reads/s" and plain["higher_is_better"] is True and plain["dtype"] == "u32"
    assert not any(k in plain for k in FULL_LEGS), sorted(plain)

    full = _line(workload, "--full", "--cpu-sample-reads", "20000", "--cpu-threads", "4", "--no-cpu-t1", "--parity-sample-reads", "5000")
    for k in HEADLINE:
        assert k in full, k
    assert full["value"] > 0
    assert full["cpu_baseline"]["value"] is not None, full["cpu_baseline"]
    assert full["parity_sample"]["diff"] == 0, full["parity_sample"]
