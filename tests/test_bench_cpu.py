"""bench.py --dump-outputs (CPU stand-in workload of --selftest-launcher): the dump is what the last timed step returned, it is the same
from run to run, and a larger output is cut to a fixed seeded sample under the size limit."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    return r, [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def test_dump_outputs_is_the_timed_result_and_repeats(tmp_path):
    import bench
    common = ["--selftest-launcher", "--steps", "3", "--warmup", "1", "--batch", "2", "--size", "128"]
    got = []
    for d in ("a", "b"):
        r, lines = _bench(common + ["--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
        assert lines[0]["steps"] == 3 and lines[0]["dump_outputs"]["arrays"]["latents"]["shape"] == [2, 64, 64]
        assert sorted(os.listdir(tmp_path / d)) == ["latents.npy"]
        got.append(np.load(tmp_path / d / "latents.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (2, 64, 64)
    assert np.array_equal(got[0], got[1])
    want = bench.stub_workload(argparse.Namespace(batch=2, size=128, denoise_steps=4), 0)()
    assert np.array_equal(got[0], want.numpy())


def test_dump_outputs_of_two_ranks_holds_every_rank(tmp_path):
    r, lines = _bench(["--gpus", "2", "--selftest-launcher", "--steps", "1", "--warmup", "0", "--batch", "1", "--size", "128",
                       "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
    a = np.load(tmp_path / "latents.npy")
    assert a.shape == (2, 1, 64, 64) and not np.array_equal(a[0], a[1])   # rank r draws its own noise (seed 100 + r)


def test_dump_outputs_samples_beyond_the_limit(tmp_path):
    import bench
    x = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    y = torch.arange(3000, dtype=torch.float64)
    limit = 8000
    rec = bench.dump_outputs({"x": x.bfloat16(), "y": y}, str(tmp_path / "a"), limit=limit)
    bench.dump_outputs({"x": x.bfloat16(), "y": y}, str(tmp_path / "b"), limit=limit)
    xa, ya = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert xa.dtype == np.float32 and ya.dtype == np.float64 and xa.nbytes + ya.nbytes <= limit
    assert rec["arrays"]["x"]["shape"] == [100, 100] and rec["arrays"]["x"]["elements"] == xa.size
    assert np.array_equal(xa, np.load(tmp_path / "b" / "x.npy")) and np.array_equal(ya, np.load(tmp_path / "b" / "y.npy"))
    # the sample is values at sorted, distinct flat indices (x.bfloat16() is exact below 256 only, so check y and x's order)
    assert np.all(np.diff(ya) > 0) and np.all(ya == np.round(ya)) and np.all(np.diff(xa) >= 0)
    small = bench.dump_outputs({"y": y}, str(tmp_path / "c"))
    assert small["arrays"]["y"]["sample"] is None and np.array_equal(np.load(tmp_path / "c" / "y.npy"), y.numpy())


def test_steps_below_one_is_refused():
    r, lines = _bench(["--selftest-launcher", "--steps", "0", "--warmup", "0", "--batch", "1", "--size", "128"])
    assert r.returncode != 0 and not lines and "--steps" in r.stderr


def test_full_is_off_by_default_and_the_line_says_which_run_it_was():
    common = ["--selftest-launcher", "--steps", "1", "--warmup", "0", "--batch", "1", "--size", "128"]
    for extra, want in (([], False), (["--full"], True)):
        r, lines = _bench(common + extra)
        assert r.returncode == 0 and len(lines) == 1 and lines[0]["full"] is want, r.stderr[-2000:]
