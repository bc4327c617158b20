#!/usr/bin/env python3
"""Time the Qwen2.5-VL vision tower on the HIP path (x2i_amd.qwen_vision.Qwen2_5VisionTower) against transformers'
Qwen2_5_VisionTransformerPretrainedModel, both in bf16 on the same GPU with the same random weights:
  tower   the whole tower (32 layers, hidden 1280, 16 heads of 80, d_ff 3420, merger to 3584) at the shapes of the reference's calls, whose
          images are resized to 128 x 128: one image (grid (1, 10, 10), 100 patches), four images, one video of four frame pairs ((4, 10, 10)).
          The HIP side runs a planned forward (the host work of the grid done once); the library runs as it does today, host work included
  layer   one block at S = 1024 (grid (1, 32, 32)), a window layer (windows of 64) and a full-attention layer
  attn    the attention launch of such a layer alone (16 heads of 80), against torch's scaled_dot_product_attention called once per segment
          as the library's non-flash path calls it
The comparator is the library: the code this stage runs today.  Device events around each call, every shape warmed up on both sides, REPS
alternating repetitions (HIP, library, HIP, ...), median and min .. max per side; beside each HIP figure the number of launches it enqueues
and the host time of enqueuing them (the call's wall time without a synchronisation).  The tower is launch-bound at these shapes: read the
device time against launches x enqueue cost before reading it against FLOPs.  Run it under a time limit (timeout -k 10 600 python
tools/qwen_vision_bench.py --log profiles/qwen_vision_bench.log); --max_seconds stops it from starting further sections itself.
`--only hip` runs the HIP side alone (for a kernel trace)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import vit_ops  # noqa: E402
from x2i_amd.qwen_vision import Qwen2_5VisionTower  # noqa: E402

TOWER = dict(depth=32, hidden_size=1280, num_heads=16, intermediate_size=3420, out_hidden_size=3584, fullatt_block_indexes=(7, 15, 23, 31))
TOWER_GRIDS = [("1 image", [(1, 10, 10)]), ("4 images", [(1, 10, 10)] * 4), ("1 video", [(4, 10, 10)])]
LAYER_GRID = [(1, 32, 32)]


def library_tower(c):
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLVisionConfig
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel
    cfg = Qwen2_5_VLVisionConfig(**dict(c, fullatt_block_indexes=list(c["fullatt_block_indexes"])))
    cfg._attn_implementation = "sdpa"
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            return Qwen2_5_VisionTransformerPretrainedModel(cfg).eval().requires_grad_(False)
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
    """sides: [(name, fn)]; alternating repetitions -> {name: median ms}, the last outputs"""
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
        extra = ", %d launches" % launches if k == "hip" and launches else ""
        say("%-34s %-3s: median %.3f ms (min %.3f .. max %.3f, %d reps), host enqueue %.3f ms%s"
            % (label, k, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k]), statistics.median(host[k]), extra))
    if "lib" in ms:
        say("%-34s    : library / HIP time %.2f x" % (label, statistics.median(ms["lib"]) / statistics.median(ms["hip"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="tower,layer,attn")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("both", "hip"), default="both")
    ap.add_argument("--max_seconds", type=float, default=480.0, help="start no further section after this many seconds")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qwen_vision_bench: no GPU visible; there is nothing to time on the CPU")
    lines, start = [], time.perf_counter()

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def section(name):
        if name not in a.sections.split(","):
            return False
        if time.perf_counter() - start > a.max_seconds:
            say("%s: skipped, %.0f s have passed (--max_seconds %.0f)" % (name, time.perf_counter() - start, a.max_seconds))
            return False
        return True

    both = a.only == "both"
    say("qwen_vision_bench: %s, torch %s, reps %d (alternating), warm-up %d per shape and side" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.warmup))
    if section("tower"):
        hip = Qwen2_5VisionTower(device="cuda", **TOWER).init_random_(0)
        lib = None
        if both:
            lib = library_tower(TOWER)
            lib.load_state_dict(hip.state_dict(), strict=True)
        L = TOWER["depth"]
        for label, grid in TOWER_GRIDS:
            g = torch.tensor(grid).cuda()
            S = sum(t * h * w for t, h, w in grid)
            px = torch.randn((S, hip.patch_dim), generator=torch.Generator().manual_seed(S)).bfloat16().cuda()
            plan = hip.plan(grid)
            sides = [("hip", lambda: hip(px, plan=plan).pooler_output)]
            if lib is not None:
                sides.append(("lib", lambda: lib(px, grid_thw=g).pooler_output))
            out = compare(say, "tower %s (S=%d)" % (label, S), sides, a.reps, a.warmup, 1 + 9 * L + 3)
            if lib is not None:
                d = (out["hip"].float() - out["lib"].float()).norm() / out["lib"].float().norm()
                say("%-34s    : merged rows differ by rel-L2 %.3e (two bf16 paths)" % ("", float(d)))
        del hip, lib
        torch.cuda.empty_cache()
    do_layer, do_attn = section("layer"), section("attn")
    for name, fullatt in (("window", ()), ("full", (0,))):
        if not (do_layer or do_attn):
            break
        c = dict(TOWER, depth=1, fullatt_block_indexes=fullatt)
        hip = Qwen2_5VisionTower(device="cuda", **c).init_random_(1)
        plan = hip.plan(LAYER_GRID)
        S, D, H, dk = plan.S, 1280, 16, 80
        x = torch.randn((S, D), generator=torch.Generator().manual_seed(2)).bfloat16().cuda()
        y = torch.empty_like(x)
        cu = plan.cu_seqlens if fullatt else plan.cu_window_seqlens
        if do_layer:
            sides = [("hip", lambda: hip._block(0, plan, x, y))]
            if both:
                lib = library_tower(c)
                lib.load_state_dict(hip.state_dict(), strict=True)
                pe = (torch.cat((plan.cos[0], plan.cos[0]), -1), torch.cat((plan.sin[0], plan.sin[0]), -1))   # the library's full tables
                sides.append(("lib", lambda: lib.blocks[0](x, cu_seqlens=cu, position_embeddings=pe)))
            out = compare(say, "layer %s S=%d (%d segments)" % (name, S, cu.numel() - 1), sides, a.reps, a.warmup, 9)
            if both:
                d = (y.float() - out["lib"].float()).norm() / out["lib"].float().norm()
                say("%-34s    : outputs differ by rel-L2 %.3e (two bf16 paths)" % ("", float(d)))
        if do_attn:
            ws = plan.ws
            g = torch.Generator().manual_seed(3)
            for k in ("Q", "K", "VT"):
                ws[k].zero_()
            ws["Q"][:, :, :S, :dk] = torch.randn((1, H, S, dk), generator=g).bfloat16().cuda()
            ws["K"][:, :, :S, :dk] = torch.randn((1, H, S, dk), generator=g).bfloat16().cuda()
            ws["VT"][:, :, :dk, :S] = torch.randn((1, H, dk, S), generator=g).bfloat16().cuda()
            lo, hi = (plan.full_lo, plan.full_hi) if fullatt else (plan.win_lo, plan.win_hi)
            sides = [("hip", lambda: vit_ops.attention(ws["Q"], ws["K"], ws["VT"], ws["ATT"], 1, H, S, plan.Spad, dk, dk ** -0.5, D, S * D, lo, hi))]
            if both:
                q, k = ws["Q"][:, :, :S, :dk].contiguous(), ws["K"][:, :, :S, :dk].contiguous()
                v = ws["VT"][:, :, :dk, :S].transpose(-1, -2).contiguous()
                lens = (cu[1:] - cu[:-1]).tolist()
                sdpa = torch.nn.functional.scaled_dot_product_attention
                sides.append(("lib", lambda: torch.cat([sdpa(a_, b_, c_) for a_, b_, c_ in zip(*(t.split(lens, dim=2) for t in (q, k, v)))], dim=2)))
            compare(say, "attention %s S=%d H=16 dk=80" % (name, S), sides, a.reps, a.warmup, 1)
        del hip
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
