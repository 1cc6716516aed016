"""bench.py's two kinds of run: a plain run prints the headline line and nothing it had to run extra work for; `--full` adds
the rooflines, the per-entry-point table, the MFMA figures and the 100-step figure (the CPU baseline, the evaluation and the
fixed-state MFMA passes are trimmed here with their --no-* options)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "ms_per_step_repeats"}
FULL_ONLY = {"roofline", "roofline_fwd", "roofline_mfma", "roofline_path", "kernels", "ms_per_step_100", "value_100", "eval",
             "cpu_baseline", "comm"}


def _line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rays", "256"]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_full_run():
    d = _line()
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d), sorted(d)
    assert d["steps"] == 3 and d["warmup"] == 1 and len(d["ms_per_step_repeats"]) == 3
    assert d["ms_per_step"] == sorted(d["ms_per_step_repeats"])[1]  # K < 100: the median of the three regions
    assert d["value"] > 0 and abs(d["value"] - 256 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    f = _line("--full", "--no-cpu-baseline", "--no-eval", "--no-mfma-states")
    assert HEADLINE <= set(f) and {"roofline", "roofline_fwd", "roofline_mfma", "roofline_path", "kernels",
                                   "ms_per_step_100", "value_100"} <= set(f), sorted(f)
    assert f["roofline"]["achieved"] > 0 and f["roofline_mfma"]["achieved"] > 0
    assert {k: f[k] for k in ("metric", "unit", "higher_is_better", "dtype")} == \
        {k: d[k] for k in ("metric", "unit", "higher_is_better", "dtype")}
