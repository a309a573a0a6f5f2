"""bench.py without --full: the headline alone -- set up, warm up, time the steps, dump, print one JSON line.  The secondary figures (tiled32, frames/s
against frames in flight, config 3, latencies, PCIe-inclusive rate, natural and real-photograph frames, CPU baseline) are measured only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ["metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config", "matches_frame0", "roofline"]
FULL_ONLY = ["tiled32", "fps_vs_in_flight", "config3_as_specified", "single_frame_latency", "tracking_call_latency", "pcie_inclusive", "natural",
             "real_photos", "cpu_baseline", "extras"]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    from conftest import gpu_available
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "64", "--distinct", "64",
                        "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE) and not [k for k in FULL_ONLY if k in out]
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "u8/f64"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["config"]["frames_in_flight_per_gpu"] == 64
    assert out["value"] > 0 and out["value"] == pytest.approx(64 * 2 / (out["ms_per_step"] * 2e-3), rel=1e-3)
    assert out["dump_outputs"]["frames"] == 64 and sorted(f[:-4] for f in os.listdir(d)) == out["dump_outputs"]["arrays"]
    assert np.load(os.path.join(d, "keypoint_count.npy")).min() > 0
