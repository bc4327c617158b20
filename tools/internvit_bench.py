#!/usr/bin/env python3
"""Time InternVL2.5's extract_feature -- InternViT-300M (24 layers of 1024 / 16 heads of 64 / 4096), the class token dropped, pixel_shuffle
and mlp1 to an LLM width of 896 -- on the HIP path (x2i_amd.internvit.InternVLVision) against the same computation in bf16 torch on the
same GPU with the same random weights, at 1, 2 and 13 tiles of 448 x 448 (1025 tokens each; the sampling scripts feed one tile per image,
13 is a full dynamic-resolution image with its thumbnail):
  hip     the HIP path, a planned eager forward: about 200 launches per call
  graph   the HIP path replayed from the graph InternVLVision(graph=True) captures on the second call of a shape
  naive   the restatement of tests/internvit_ref.py under naive attention (the scores materialised): what the model runs without flash
          attention, the code this stage runs today
  sdpa    the same with torch's scaled_dot_product_attention
The position table of the grid is made once per side, outside the timed region.  Device events around each call, every shape warmed up on
every side (the graph side's warm-up holds its eager call and its capture), REPS interleaved repetitions (hip, graph, naive, sdpa, hip,
...), median and min .. max per side; beside each figure the host time of the call.  Run it under a time limit (timeout -k 10 600 python
tools/internvit_bench.py --log profiles/internvit_bench.log); --max_seconds stops it from starting further cases itself.  `--only hip`
runs the eager HIP side alone (for a kernel trace)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import internvit_ref as IR  # noqa: E402
from x2i_amd.internvit import InternVisionTower, InternVLVision  # noqa: E402

TOWER = dict(hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, intermediate_size=4096, image_size=448, patch_size=14,
             layer_norm_eps=1e-6, hidden_act="gelu", norm_type="layer_norm", qk_normalization=False, qkv_bias=True)
LLM = 896
CASES = [1, 2, 13]      # tiles


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    host = (time.perf_counter() - w0) * 1e3
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), host, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=TOWER["num_hidden_layers"])
    ap.add_argument("--only", choices=("all", "hip"), default="all", help="hip: the eager HIP side alone (for a kernel trace)")
    ap.add_argument("--max_seconds", type=float, default=420.0, help="start no further case after this many seconds")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("internvit_bench: no GPU visible; there is nothing to time on the CPU")
    lines, start = [], time.perf_counter()

    def say(s):
        print(s, flush=True)
        lines.append(s)

    c = dict(TOWER, num_hidden_layers=a.layers)
    say("internvit_bench: %s, torch %s, %d layers, LLM width %d, reps %d (interleaved), warm-up %d per case and side" % (
        torch.cuda.get_device_name(0), torch.__version__, a.layers, LLM, a.reps, a.warmup))
    eager = InternVLVision(InternVisionTower(device="cuda", **c), LLM).init_random_(0)
    graphed = InternVLVision(eager.vision_model, LLM, graph=True)      # the same tower; the same mlp1 below
    graphed.mlp1.load_state_dict(eager.mlp1.state_dict(), strict=True)
    sd = {k: v.detach() for k, v in eager.state_dict().items()}
    g = c["image_size"] // c["patch_size"]
    launches = 3 + (8 + (2 if c["qk_normalization"] else 0)) * a.layers + 3
    with torch.no_grad():
        pos = IR.position_table(sd["vision_model.embeddings.position_embedding"], g, g, g)
    for B in CASES:
        label = "%2d tile%s" % (B, " " if B == 1 else "s")
        if time.perf_counter() - start > a.max_seconds:
            say("%s: skipped, %.0f s have passed (--max_seconds %.0f)" % (label, time.perf_counter() - start, a.max_seconds))
            continue
        x = IR.random_pixels(B, c["image_size"], seed=B).bfloat16().cuda()
        plan = eager.plan(B, g)
        sides = [("hip", lambda: eager(x, plan=plan)), ("graph", lambda: graphed(x)),
                 ("naive", lambda: IR.extract_feature(sd, x, c, torch.bfloat16, pos=pos)),
                 ("sdpa", lambda: IR.extract_feature(sd, x, c, torch.bfloat16, attn="sdpa", pos=pos))]
        if a.only == "hip":
            sides = sides[:1]
        with torch.no_grad():
            for _ in range(a.warmup):
                for _, fn in sides:
                    fn()
            torch.cuda.synchronize()
            ms, host, out = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}, {}
            for _ in range(a.reps):
                for k, fn in sides:
                    t, h, out[k] = timed(fn)
                    ms[k].append(t)
                    host[k].append(h)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, _ in sides:
            extra = ", %d launches" % launches if k == "hip" else (", one replay" if k == "graph" else "")
            say("%s %-5s: median %.3f ms (min %.3f .. max %.3f, %d reps), host %.3f ms%s"
                % (label, k, med[k], min(ms[k]), max(ms[k]), len(ms[k]), statistics.median(host[k]), extra))
        if a.only == "hip":
            continue
        say("%s      : naive / hip %.2f x, naive / graph %.2f x, sdpa / hip %.2f x, sdpa / graph %.2f x, hip / graph %.2f x"
            % (label, med["naive"] / med["hip"], med["naive"] / med["graph"], med["sdpa"] / med["hip"], med["sdpa"] / med["graph"], med["hip"] / med["graph"]))
        d = (out["hip"].float() - out["naive"].float()).norm() / out["naive"].float().norm()
        say("%s      : HIP against naive rel-L2 %.3e; graph == eager bit for bit: %s" % (label, float(d), bool(torch.equal(out["hip"], out["graph"]))))
        del out, x, plan
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
