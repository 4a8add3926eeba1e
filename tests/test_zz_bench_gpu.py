"""bench.py's two kinds of run, each in a process of its own at a tiny size (2 scenes of 3 views, one warm-up and one timed step):
a plain run prints the headline line and nothing measured beside it; --full (narrowed to the step by --step-only) adds the per-kernel
figures to the same line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"value_single_scene", "value_r04_definition", "roofline", "roofline_attention", "roofline_gemm", "kernel_classes", "stages_ms",
             "single_scene", "alt", "scenes_in_flight_sweep", "configs", "postprocess_cam", "cpu_baseline", "torch_rocm_baseline",
             "parity_vs_cpu_oracle", "rccl", "view_sharded", "multi_gpu"}

pytestmark = pytest.mark.gpu


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--scenes", "2", "--views", "3", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_only():
    line = _bench()
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line), sorted(line)
    assert line["unit"] == "views/s" and line["higher_is_better"] is True
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(2 * 3, rel=1e-3)   # value = views per step / step time
    assert line["config"]["scenes_in_flight_per_gpu"] == 2 and line["config"]["views_per_scene"] == 3
    assert "parity" not in line["config"]


def test_full_run_adds_to_the_same_line():
    line = _bench("--full", "--step-only")
    assert HEADLINE <= set(line) and FULL_ONLY <= set(line), sorted(set(line) ^ FULL_ONLY)
    assert line["kernel_classes"] and line["stages_ms"] and line["roofline"]["launches"] > 0
    assert line["cpu_baseline"] is None and line["single_scene"] is None   # --step-only narrows --full to the step's own figures
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(2 * 3, rel=1e-3)
