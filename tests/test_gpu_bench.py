"""bench.py without --full: the headline line and the dump, none of what --full adds (CPU baselines, roofline,
checks, extras) -- also at two ranks, where the collectives --full adds must be left out on every rank alike."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _line(cmd, env=None):
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _plain(line):
    assert all(k in line for k in HEADLINE)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["full"] is False
    assert not {"roofline", "cpu_baseline", "extras"} & set(line)


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--windows", "4", "--dump-outputs", str(tmp_path)]
    line = _line(cmd)
    _plain(line)
    assert line["steps"] == 2 and line["warmup"] == 1
    rj = np.load(os.path.join(str(tmp_path), "residual_jacobian.npy"))
    assert rj.shape == (4, line["config"]["patches_per_window"], 3) and np.isfinite(rj).all() and np.any(rj != 0)


def test_plain_run_at_two_ranks():
    env = dict(os.environ, EBO_BENCH_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--c4-windows", "1"]
    line = _line(cmd, env)
    _plain(line)
    assert line["n_gpus"] == 2 and "patch rows sharded over 2" in line["config"]["workload"]
