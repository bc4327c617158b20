#!/usr/bin/env python3
"""Time the MiniCPM-o SigLIP vision tower on the HIP path (x2i_amd.siglip.SiglipVisionTower) against transformers'
Idefics2VisionTransformer (the same module under another name), both in bf16 on the same GPU with the same random weights, at full width:
27 layers, hidden 1152, 16 heads of 72, d_ff 4304, frames of 32 x 32 patches of 14 x 14 (L = 1024):
  1 image     one strip
  16 frames   one call of 16 strips, the reference's vision_batch_size
  64 frames   the reference's MAX_NUM_FRAMES as it runs them: four calls of 16
The HIP side runs a planned forward (the host work of the sizes done once); the library runs on the same strips with the [B, 1, L] mask
the reference builds, under `sdpa` and under `eager`.  (The strips are unpadded here, so the mask is all ones and the library may drop
it: the padded batches of mixed sizes, where it materialises an additive mask, are not timed.)  The comparator is the library: the code
this stage runs today.  Device events around each call, every shape warmed up on every side, REPS interleaved repetitions (HIP, sdpa,
eager, HIP, ...), median and min .. max per side; beside each HIP figure the number of launches it enqueues and the host time of
enqueuing them.  Run it under a time limit (timeout -k 10 600 python tools/siglip_bench.py --log profiles/siglip_vision_bench.log);
--max_seconds stops it from starting further cases itself.  `--only hip` runs the HIP side alone (for a kernel trace)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd.siglip import SiglipVisionTower  # noqa: E402

TOWER = dict(hidden_size=1152, num_attention_heads=16, num_hidden_layers=27, intermediate_size=4304, image_size=980, patch_size=14)
GRID = (32, 32)
CASES = [("1 image", 1, 1), ("16 frames", 16, 1), ("64 frames (4 x 16)", 16, 4)]      # (label, strips per call, calls)


def library_tower(c, attn):
    from transformers.models.idefics2.configuration_idefics2 import Idefics2VisionConfig
    from transformers.models.idefics2.modeling_idefics2 import Idefics2VisionTransformer
    cfg = Idefics2VisionConfig(hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, **c)
    cfg._attn_implementation = attn
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            return Idefics2VisionTransformer(cfg).eval().requires_grad_(False)
    finally:
        torch.set_default_dtype(old)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    host = (time.perf_counter() - w0) * 1e3
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), host, out


def compare(say, label, sides, reps, warmup, launches):
    """sides: [(name, fn)]; interleaved repetitions -> the last outputs"""
    with torch.no_grad():
        for _ in range(warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        ms, host, out = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}, {}
        for _ in range(reps):
            for k, fn in sides:
                t, h, out[k] = timed(fn)
                ms[k].append(t)
                host[k].append(h)
    for k, _ in sides:
        extra = ", %d launches" % launches if k == "hip" else ""
        say("%-28s %-5s: median %.3f ms (min %.3f .. max %.3f, %d reps), host enqueue %.3f ms%s"
            % (label, k, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k]), statistics.median(host[k]), extra))
    for k in ("sdpa", "eager"):
        if k in ms:
            say("%-28s      : library (%s) / HIP time %.2f x" % (label, k, statistics.median(ms[k]) / statistics.median(ms["hip"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=TOWER["num_hidden_layers"])
    ap.add_argument("--only", choices=("all", "hip"), default="all")
    ap.add_argument("--max_seconds", type=float, default=480.0, help="start no further case after this many seconds")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("siglip_bench: no GPU visible; there is nothing to time on the CPU")
    lines, start = [], time.perf_counter()

    def say(s):
        print(s, flush=True)
        lines.append(s)

    c = dict(TOWER, num_hidden_layers=a.layers)
    say("siglip_bench: %s, torch %s, %d layers, reps %d (interleaved), warm-up %d per case and side" % (
        torch.cuda.get_device_name(0), torch.__version__, a.layers, a.reps, a.warmup))
    hip = SiglipVisionTower(device="cuda", **c).init_random_(0)
    libs = {}
    if a.only == "all":
        for attn in ("sdpa", "eager"):
            libs[attn] = library_tower(c, attn)
            libs[attn].load_state_dict(hip.state_dict(), strict=True)
    h, w = GRID
    L, P = h * w, c["patch_size"]
    for label, B, calls in CASES:
        if time.perf_counter() - start > a.max_seconds:
            say("%s: skipped, %.0f s have passed (--max_seconds %.0f)" % (label, time.perf_counter() - start, a.max_seconds))
            continue
        g = torch.Generator().manual_seed(B + calls)
        xs = [torch.randn((B, 3, P, P * L), generator=g).bfloat16().cuda() for _ in range(calls)]
        mask = torch.ones((B, 1, L), dtype=torch.bool, device="cuda")
        plan = hip.plan([GRID] * B, L)
        sides = [("hip", lambda: [hip(x, plan=plan).last_hidden_state for x in xs])]
        for attn, lib in libs.items():
            sides.append((attn, lambda lib=lib: [lib(x, patch_attention_mask=mask).last_hidden_state for x in xs]))
        out = compare(say, label, sides, a.reps, a.warmup, calls * (3 + 8 * a.layers + 1))
        # (the library reads a 1 x L grid off the strip's mask and the HIP plan holds 32 x 32: other position ids, the same work)
        del out, xs
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
