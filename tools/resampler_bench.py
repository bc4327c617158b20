#!/usr/bin/env python3
"""Time the MiniCPM-o Resampler on the HIP path (x2i_amd.resampler.Resampler) against the same module composed from torch.nn's own
LayerNorm and MultiheadAttention (tests/resampler_ref.py: LibraryResampler, which takes nn.MultiheadAttention's need_weights=True branch
as the model's module does), both in bf16 on the same GPU with the same random weights, at full width: embed 3584, 28 heads of 128,
kv_dim 1152, 64 queries, frames of 32 x 32 patches (L = 1024).  One case per process, so that each runs under a time limit of its own:
  --case 1 | 16 | 64   that many frames in ONE call (the model calls its Resampler once on all frames of a video); the HIP side walks
                       them in chunks of 16
  --case launches      the time of every launch inside one HIP forward of 16 frames (device events around each call of the binding)
  --case pair          the k and the v projection of 16 frames as two x2i_gemm_bf16 launches against one x2i_gemm_pair_bf16
The HIP side runs a planned forward.  Device events around each call, --warmup warm-ups per side, --reps interleaved repetitions (HIP,
torch, HIP, ...), median and min .. max per side.  --log appends to a file:
  for c in 1 16 64 launches pair; do timeout -k 10 300 python tools/resampler_bench.py --case $c --log profiles/resampler_bench.log || break; done"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import resampler_ref as RR  # noqa: E402
from x2i_amd import ops, resampler_ops  # noqa: E402
from x2i_amd.resampler import Resampler  # noqa: E402

FULL = dict(num_queries=64, embed_dim=3584, kv_dim=1152)
GRID = (32, 32)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    host = (time.perf_counter() - w0) * 1e3
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), host, out


def compare(say, label, sides, reps, warmup):
    """sides: [(name, fn)]; interleaved repetitions -> {name: median ms}"""
    with torch.no_grad():
        for _ in range(warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        ms, host = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}
        for _ in range(reps):
            for k, fn in sides:
                t, h, _ = timed(fn)
                ms[k].append(t)
                host[k].append(h)
    for k, _ in sides:
        say("%-12s %-6s: median %.3f ms (min %.3f .. max %.3f, %d reps), host enqueue %.3f ms"
            % (label, k, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k]), statistics.median(host[k])))
    return {k: statistics.median(v) for k, v in ms.items()}


def frames_case(say, hip, B, a):
    L = GRID[0] * GRID[1]
    lib = RR.LibraryResampler(hip.num_queries, hip.embed_dim, hip.num_heads, hip.kv_dim)
    lib.load_state_dict({k: v.float().cpu() for k, v in hip.state_dict().items()}, strict=True)
    lib = lib.to(device="cuda", dtype=torch.bfloat16)
    x = torch.randn((B, L, hip.kv_dim), generator=torch.Generator().manual_seed(B)).bfloat16().cuda()
    grids = [GRID] * B
    plan = hip.plan(grids, L)
    chunks = (B + 15) // 16
    label = "%d frame%s" % (B, "" if B == 1 else "s")
    med = compare(say, label, [("hip", lambda: hip(x, plan=plan)), ("torch", lambda: lib(x, grids))], a.reps, a.warmup)
    say("%-12s       : torch / HIP time %.2f x; the HIP forward enqueues %d launches (9 per chunk of 16 frames)" % (label, med["torch"] / med["hip"], 9 * chunks))


def launches_case(say, hip, a):
    """One forward of 16 frames with device events around every call of the binding"""
    B, L = 16, GRID[0] * GRID[1]
    x = torch.randn((B, L, hip.kv_dim), generator=torch.Generator().manual_seed(1)).bfloat16().cuda()
    plan = hip.plan([GRID] * B, L)
    names = ["gemm kv_proj", "ln_pos", "gemm k", "gemm v", "kv_split", "attention", "gemm out_proj", "ln_affine ln_post", "gemm proj"]
    marks = []

    def wrap(fn):
        def inner(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            marks.append((e0, e1))
            return out
        return inner
    saved = (ops.gemm, ops.ln_affine, resampler_ops.ln_pos, resampler_ops.kv_split, resampler_ops.attention)
    for _ in range(a.warmup):
        hip(x, plan=plan)
    ops.gemm, ops.ln_affine = wrap(saved[0]), wrap(saved[1])
    resampler_ops.ln_pos, resampler_ops.kv_split, resampler_ops.attention = wrap(saved[2]), wrap(saved[3]), wrap(saved[4])
    per = [[] for _ in names]
    try:
        for _ in range(a.reps):
            del marks[:]
            hip(x, plan=plan)
            torch.cuda.synchronize()
            assert len(marks) == len(names), "the forward of one chunk is %d launches, not %d" % (len(marks), len(names))
            for i, (e0, e1) in enumerate(marks):
                per[i].append(e0.elapsed_time(e1))
    finally:
        ops.gemm, ops.ln_affine, resampler_ops.ln_pos, resampler_ops.kv_split, resampler_ops.attention = saved
    total = sum(statistics.median(p) for p in per)
    for n, p in zip(names, per):
        say("16 frames, launch %-18s: median %.3f ms (min %.3f .. max %.3f), %4.1f %% of the sum" % (n, statistics.median(p), min(p), max(p), 100 * statistics.median(p) / total))
    say("16 frames, sum of the launches  : %.3f ms" % total)


def pair_case(say, hip, a):
    B, L, D = 16, GRID[0] * GRID[1], hip.embed_dim
    M = B * L
    g = torch.Generator().manual_seed(2)
    XK, XV = (torch.randn((M, D), generator=g).bfloat16().cuda() for _ in range(2))
    KV, KV2 = (torch.empty((M, 2 * D), device="cuda", dtype=torch.bfloat16) for _ in range(2))
    w, b = hip.attn.in_proj_weight, hip.attn.in_proj_bias
    gk = lambda out: dict(A=XK, W=w[D:2 * D], bias=b[D:2 * D], out=out, M=M, ldc=2 * D)           # noqa: E731
    gv = lambda out: dict(A=XV, W=w[2 * D:], bias=b[2 * D:], out=out, M=M, ldc=2 * D, c_offset=D)   # noqa: E731

    def plain():
        ops.gemm(**gk(KV))
        ops.gemm(**gv(KV))

    med = compare(say, "k | v GEMMs", [("plain", plain), ("paired", lambda: ops.gemm_pair(gk(KV2), gv(KV2)))], a.reps, a.warmup)
    torch.cuda.synchronize()
    say("k | v GEMMs        : paired / plain time %.3f x; outputs bit-identical: %s" % (med["paired"] / med["plain"], torch.equal(KV, KV2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("1", "16", "64", "launches", "pair"), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None, help="append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resampler_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("resampler_bench --case %s: %s, torch %s, reps %d (interleaved), warm-up %d per side" % (
        a.case, torch.cuda.get_device_name(0), torch.__version__, a.reps, a.warmup))
    hip = Resampler(device="cuda", **FULL).init_random_(0)
    with torch.no_grad():
        if a.case == "launches":
            launches_case(say, hip, a)
        elif a.case == "pair":
            pair_case(say, hip, a)
        else:
            frames_case(say, hip, int(a.case), a)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
