"""bench.py end to end at a small size, each run a fresh child process: a plain run measures the headline and nothing
else; `--full` adds the measurements beside it (here the roofline's own runs, with the CPU baseline and the legs off)."""

import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SMALL = ["--gpus", "1", "--n", "20000", "--p", "500", "--alphas", "10", "--steps", "2", "--warmup", "1"]


def _run(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)  # (the group this test started, nothing else)
        out, err = proc.communicate()
        pytest.fail("bench.py did not finish within 300 s:\n" + err[-3000:])
    assert proc.returncode == 0, err[-3000:]
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0])


def _check_headline(line):
    assert line["metric"] == "fits/sec over 50-alpha Lasso path at n=100k p=5k"
    assert line["unit"] == "fits/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 10 / (2 * line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert line["roofline"]["launches_timed_with_hip_events"] > 0 and line["roofline"]["kernel_achieved"] > 0


def test_a_plain_run_measures_the_headline_alone(tmp_path):
    line = _run("--dump-outputs", str(tmp_path / "dump"))
    _check_headline(line)
    assert line["cpu_baseline"] is None
    assert not {"extra_legs", "strong_scaling", "value_mean_over_draws"} & set(line)
    assert set(line["summary"]) == {"path_level_roofline_frac"}
    roof = line["roofline"]
    assert roof["gradient_unit_ms"] is None and roof["read_stream_ceiling_gbs"] is None
    assert roof["frac"] == roof["kernel_frac"]
    betas = np.load(tmp_path / "dump" / "betas.npy")
    assert betas.dtype == np.float64 and betas.shape == (10, 500)


def test_full_adds_the_roofline_runs():
    line = _run("--full", "--cpu-budget", "0", "--no-extra")
    _check_headline(line)
    roof = line["roofline"]
    assert roof["read_stream_ceiling_gbs"] > 0
    if roof["gradient_unit_ms"]:
        assert roof["frac_is"] == "gradient unit (residuals + X^T R)" and roof["frac"] == roof["gradient_unit_frac"]
    assert "measured under --full" not in roof["frac_is"]
