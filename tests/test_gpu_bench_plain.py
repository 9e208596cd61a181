"""bench.py without --full: the headline line alone (K timed steps, no leg behind the region), and --dump-outputs -- what the last timed step
computed, the same bits from run to run with the same arguments, whatever the untimed clock warm-up did before the W warm-up steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
OUTPUTS = {"state": (16,), "eskf_state": (19,), "eskf_cov": (17, 17), "iterations": (), "num_residuals": ()}


def _bench(dump_dir, *extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(dump_dir), *extra]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in p.stdout.decode().split("\n") if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_same_last_step(tmp_path):
    a = _bench(tmp_path / "a")
    for k in CONTRACT:
        assert k in a, k
    assert a["steps"] == 7 and a["warmup"] == 2 and a["n_gpus"] == 1 and a["unit"] == "sweeps/s" and a["dtype"] == "f64"
    assert a["value"] > 0 and abs(a["value"] * a["ms_per_step"] / 1e3 - 1.0) < 1e-9
    for k in ("roofline", "cpu_baseline", "parity", "configs", "stream", "pcie_inclusive_sweeps_per_s", "detail"):
        assert k not in a, k                                               # legs of --full only
    b = _bench(tmp_path / "b", "--clock-warmup-ms", "0")                   # no clock warm-up: the same sweep in the last step
    for name, shape in OUTPUTS.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == shape and np.all(np.isfinite(x)), name
        assert np.array_equal(x, y), name
    assert np.load(tmp_path / "a" / "iterations.npy") == a["config"]["esikf_iterations_per_solve"]     # every sweep of the stream: same count
    assert np.load(tmp_path / "a" / "num_residuals.npy") == a["config"]["residuals_used"]
