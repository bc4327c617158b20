"""bench.py on the GPU: a plain run times its steps and prints the headline line, nothing else; `--full` adds the measurements beside
it (live roofline probes, the fp8_mlp / fp8_all lines; the CPU baseline is skipped here for time)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--steps", "1", "--warmup", "0", "--batch", "1", "--size", "512"]
EXTRAS = ("roofline", "roofline_attention", "vae", "fp8_mlp", "fp8_all", "cpu_baseline")


def _line(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + FLAGS + args, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only():
    ln = _line([])
    assert ln["full"] is False and ln["value"] > 0 and ln["unit"] == "images/s" and ln["dtype"] == "bf16" and ln["steps"] == 1
    assert [k for k in EXTRAS if k in ln] == []


def test_full_run_adds_the_live_probes_and_the_fp8_lines():
    ln = _line(["--full", "--no-cpu-baseline"])
    assert ln["full"] is True and ln["value"] > 0 and ln["dtype"] == "bf16"
    assert ln["roofline"]["achieved"] > 0 and ln["roofline"]["matrix_pipe_alone"]["achieved"] > 0
    assert ln["fp8_mlp"]["images_s"] > 0 and ln["fp8_all"]["images_s"] > 0 and ln["fp8_mlp"]["roofline"]["achieved"] > 0
    assert "cpu_baseline" not in ln
