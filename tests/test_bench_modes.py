"""bench.py without and with --full: a plain run prints the headline line from its timed steps alone, --full adds the
passes that take runs of their own; the timed steps and the dumped state are the same in both."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_is_off_by_default():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert a.full is False and (a.steps, a.warmup) == (3, 2)
    assert b.parse_args(["--full", "--no-cpu-baseline"]).full is True


def _run(tmp_path, tag, extra):
    out_dir = str(tmp_path / tag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c3", "--size", "24",
                        "--steps", "3", "--warmup", "2", "--dump-outputs", out_dir] + extra,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "concentration.npy"))


@pytest.mark.gpu
def test_plain_run_has_the_headline_and_full_adds_the_extra_passes(tmp_path):
    plain, c_plain = _run(tmp_path, "plain", [])
    full, c_full = _run(tmp_path, "full", ["--full", "--no-cpu-baseline"])
    for line in (plain, full):
        assert line["unit"] == "DoF-updates/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["steps"] == 3 and line["warmup"] == 2 and line["steps_completed"] == 3 and line["solver_status"] == 0
        assert line["value"] > 0 and line["ms_per_step"] > 0
        assert line["config"]["dofs"] == 25 ** 3
    assert plain["metric"] == full["metric"]
    # a plain run: nothing after the timed steps but the line
    assert "alt" not in plain and "cpu_baseline" not in plain
    roof = plain["roofline"]
    assert "stream_ceiling" not in roof and roof["isolated_spmv_launch_us"] is None and roof["traffic"] is None
    assert roof["achieved"] > 0 and roof["launches_timed"] > 0          # from the events inside the timed steps
    assert not any(k["name"].startswith("k_rd_") for k in roof["kernels"])
    # --full: the kernel pass, the isolated launches, the streaming ceiling and the fp32-Jacobian pass
    roof = full["roofline"]
    assert roof["stream_ceiling"] > 0 and roof["isolated_spmv_launch_us"] > 0
    assert any(k["name"].startswith("k_rd_assemble") for k in roof["kernels"])
    assert full["alt"]["fp32_jacobian_storage"]["solver_status"] == 0
    assert "cpu_baseline" not in full
    # the same timed steps: the same state after them
    assert np.linalg.norm(c_plain - c_full) <= 1e-12 * np.linalg.norm(c_full)
