"""A plain `bench.py --gpus 1` run does only what its headline needs: the JSON line carries the headline and the figures
taken from the timed steps' own events, and none of the legs that `--full` adds after the timed region (the CPU
baseline, the other configurations, the stream-population probes)."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_only():
    # a child process: nothing in THIS process has to touch the GPU first
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
    proc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, proc.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "layers/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert math.isfinite(out["value"]) and out["value"] > 0.0
    assert out["value"] == pytest.approx(54 * 1e3 / out["ms_per_step"])
    for key in ("update", "invert", "sample_and_replace"):
        assert math.isfinite(out["phases_ms"][key]) and out["phases_ms"][key] > 0.0
    assert 0.0 < out["roofline"]["frac"] < 1.0
    assert "cpu_baseline" not in out and "other_configs" not in out
