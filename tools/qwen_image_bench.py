#!/usr/bin/env python3
"""Time the Qwen2.5-VL image front end on the HIP path (handoff.HipQwenImage over x2i_amd.qwen_image.QwenImageFrontEnd) against the
library's own Pillow backend: Qwen2VLImageProcessorPil()(images=..., return_tensors="pt") followed by .to(device) of pixel_values.
  1, 4 and 16 x 128x128   the reference's case: every image is resized to 128 x 128 on the host first, and becomes 100 rows
  1 x 640x480, 1 x 1920x1080, 1 x 4000x3000
Both sides get the same PIL images through the same call.  Per side, host clocks: `call` until the call returns (for hip the pinned copy
and the enqueueing, for the library the whole computation and the copy's enqueueing) and `total` until a device synchronise after it.
Every side is warmed up, then REPS interleaved repetitions; median and min .. max.  Beside them the kernel's device time from device events
around the launch alone, on frames already on the device, and whether the two sides' pixel_values are equal bit for bit.

Then the in-place route on 16 x 128x128 (S = 1600 rows): `in place` is the front end writing bf16 rows straight into a [S, 1216]
workspace, `f32 + copy` is the front end writing float32 rows and the tower's PX[:, :1176].copy_(rows) behind it; device events around
each, frames already on the device for the kernel-only lines.

Every case runs in a child process of its own under a time limit (--case NAME runs one case in this process); the parent does not touch
the GPU and stops at the first case that fails.  No speed target: the result is stated as it falls.
  python tools/qwen_image_bench.py --log profiles/qwen_image_bench.log"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("1 x 128x128", 1, 128, 128), ("4 x 128x128", 4, 128, 128), ("16 x 128x128", 16, 128, 128), ("1 x 640x480", 1, 640, 480),
         ("1 x 1920x1080", 1, 1920, 1080), ("1 x 4000x3000", 1, 4000, 3000)]
IN_PLACE = "in place, 16 x 128x128"
LIMIT = 240                              # seconds per case: the first import of torch on a fresh machine is most of it


def clocks(torch, fn):
    """(ms until fn returns, ms until the device has finished too, fn's result)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, out


def device_ms(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def fmt(xs):
    return "%9.3f ms  (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


class Processor:
    def __init__(self, image_processor):
        self.image_processor = image_processor


def run_case(label, reps, warmup, say, banner=False):
    import numpy as np
    import torch
    from PIL import Image
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil

    from x2i_amd import handoff, image_binding as ib, image_rows_binding as irb
    if not torch.cuda.is_available():
        sys.exit("qwen_image_bench: needs a GPU")
    lib_ip = Qwen2VLImageProcessorPil()
    proc = Processor(lib_ip)
    hip = handoff.HipQwenImage(proc, "cuda").install()
    hip_ip, front = proc.image_processor, hip.front
    if banner:
        import PIL
        say("%s, torch %s, Pillow %s, transformers %s, %d CPU threads"
            % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__, __import__("transformers").__version__, torch.get_num_threads()))
    if label == IN_PLACE:
        return run_in_place(front, reps, warmup, say)
    _, n, w, h = next(c for c in CASES if c[0] == label)
    rng = np.random.default_rng(w + n)
    images = [Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for _ in range(n)]
    oh, ow = front.smart_resize(h, w)
    S = n * (oh // 14) * (ow // 14)
    sides = [("hip", lambda: hip_ip(images=images, return_tensors="pt")["pixel_values"]),
             ("lib", lambda: lib_ip(images=images, return_tensors="pt")["pixel_values"].to("cuda", non_blocking=True))]
    call, total, outs = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}, {}
    for _ in range(warmup):
        for k, fn in sides:
            clocks(torch, fn)
    for _ in range(reps):
        for k, fn in sides:
            c, t, outs[k] = clocks(torch, fn)
            call[k].append(c)
            total[k].append(t)
    assert hip.fallbacks == 0 and hip.calls == warmup + reps
    say()
    say("%s -> %dx%d, S = %d rows: %.3f MB of uint8 frames in, %.3f MB of float32 pixel_values out (the library uploads those), LDS plan "
        "(rows, patches, pitch) %s" % (label, ow, oh, S, 3e-6 * n * w * h, 4e-6 * S * 1176, ib.lds_plan(h, oh)))
    for k, _ in sides:
        say("  %-4s call  %s" % (k, fmt(call[k])))
        say("  %-4s total %s" % (k, fmt(total[k])))
    say("  lib / hip (medians): call %.2fx, total %.2fx" % (statistics.median(call["lib"]) / statistics.median(call["hip"]),
                                                            statistics.median(total["lib"]) / statistics.median(total["hip"])))
    say("  hip == lib bit for bit: %s" % bool(torch.equal(outs["hip"].view(torch.int32), outs["lib"].view(torch.int32))))
    # the kernel alone, device events around the launch, the frames already on the device
    frames = torch.from_numpy(np.stack([np.asarray(im) for im in images])).cuda().reshape(-1)
    out = torch.empty(S * 1176, dtype=torch.float32, device="cuda")
    hb, hc = front.tables(w, ow)
    vb, vc = front.tables(h, oh)
    launch = lambda: irb.rows(frames, w, h, 3 * w, 3 * w * h, n, 1, ow, oh, hb, hc, vb, vc, front.lut, out, S // n * 1176, 1176)   # noqa: E731
    for _ in range(max(warmup, 3)):
        launch()
    ks = [device_ms(torch, launch) for _ in range(max(reps, 20))]
    say("  image_rows_kernel %s   %.1f GB/s of frames read and values written" % (fmt(ks), (3 * n * w * h + 4 * S * 1176) / statistics.median(ks) * 1e-6))
    hip.remove()


def run_in_place(front, reps, warmup, say):
    import numpy as np
    import torch

    from x2i_amd import image_rows_binding as irb
    n, w, h, ow, oh, Kp = 16, 128, 128, 140, 140, 1216
    S = n * 100
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]
    PX = torch.zeros((S, Kp), dtype=torch.bfloat16, device="cuda")
    PX2 = torch.zeros((S, Kp), dtype=torch.bfloat16, device="cuda")
    in_place = lambda: front(arrays, out_dtype=torch.bfloat16, out=PX, row_stride=Kp)             # noqa: E731
    two_step = lambda: PX2[:, :1176].copy_(front(arrays)[0])                                       # noqa: E731
    sides = [("in place", in_place), ("f32 + copy", two_step)]
    call, total = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}
    for _ in range(warmup):
        for k, fn in sides:
            clocks(torch, fn)
    for _ in range(reps):
        for k, fn in sides:
            c, t, _ = clocks(torch, fn)
            call[k].append(c)
            total[k].append(t)
    say()
    say("%s -> %dx%d, S = %d rows into a bf16 [S, %d] workspace, from host arrays (pinned copy, transfer, launch)" % (IN_PLACE, ow, oh, S, Kp))
    for k, _ in sides:
        say("  %-10s call  %s" % (k, fmt(call[k])))
        say("  %-10s total %s" % (k, fmt(total[k])))
    say("  equal bits in the workspace: %s" % bool(torch.equal(PX.view(torch.int16), PX2.view(torch.int16))))
    frames = torch.from_numpy(np.stack(arrays)).cuda().reshape(-1)
    rows32 = torch.empty(S * 1176, dtype=torch.float32, device="cuda")
    hb, hc = front.tables(w, ow)
    vb, vc = front.tables(h, oh)
    flat = PX.view(-1)
    k_in = lambda: irb.rows(frames, w, h, 3 * w, 3 * w * h, n, 1, ow, oh, hb, hc, vb, vc, front.lut, flat, 100 * Kp, Kp)                    # noqa: E731

    def k_two():
        irb.rows(frames, w, h, 3 * w, 3 * w * h, n, 1, ow, oh, hb, hc, vb, vc, front.lut, rows32, 100 * 1176, 1176)
        PX2[:, :1176].copy_(rows32.view(S, 1176))

    for _ in range(3):
        k_in(), k_two()
    a, b = [], []
    for _ in range(max(reps, 20)):
        a.append(device_ms(torch, k_in))
        b.append(device_ms(torch, k_two))
    say("  device only, frames on the device: bf16 in place %s" % fmt(a))
    say("  device only, frames on the device: f32 + copy    %s" % fmt(b))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts per case)")
    ap.add_argument("--banner", action="store_true", help="with --case: print the device and library versions first")
    args = ap.parse_args()
    if args.case is not None:
        return run_case(args.case, args.reps, args.warmup, lambda s="": print(s, flush=True), args.banner)
    lines = ["qwen_image_bench: reps %d, warm-up %d, one child process per case, %d s limit each" % (args.reps, args.warmup, LIMIT)]
    print(lines[0], flush=True)
    status = 0
    for label in [c[0] for c in CASES] + [IN_PLACE]:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--case", label, "--reps", str(args.reps),
               "--warmup", str(args.warmup)] + (["--banner"] if label == CASES[0][0] else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.rstrip("\n").split("\n")
        if r.returncode != 0:                                   # nothing more is started on the GPU after a failure
            tail = "\n".join(r.stderr.strip().split("\n")[-15:])
            lines.append("%s: exit status %d, stopping\n%s" % (label, r.returncode, tail))
            print(lines[-1], flush=True)
            status = 1
            break
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
