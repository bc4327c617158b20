#!/usr/bin/env python3
"""Time the image back end (x2i_amd/image_out.py, abi/backend/x2i_image_out.h) against the tail it replaces, at 1024 x 1024 and 512 x 512,
B = 1 and 4.  Per case, in a child process of its own:
  (a) the parent's tail around an already decoded y (bf16 NHWC [B, H, W, 4], random values in the image's range):
        head   FluxPipeline._unpack_latents, / scaling_factor + shift_factor, decode's zeros + permuted copy      (device events)
        tail   y[..., :3].permute(0, 3, 1, 2).contiguous(), VaeImageProcessor.postprocess(image, "pil")           (host clock, synchronous)
  (b) the new one:
        x2i_latents_to_vae, x2i_image_to_u8    each by itself                                                    (device events)
      Device figures are per call over a train of 50 calls between two events; beside each stands the host's enqueue time per call, and a
      device figure no larger than it is a launch rate, not a kernel time.  The GB/s printed for x2i_image_to_u8 divide the bytes of one call
      by that figure; the calls of a train re-read one y, which fits the Infinity Cache, so they are no HBM bandwidth either.
        host   one asynchronous copy of the uint8 pixels into pinned memory, the event wait, Image.fromarray       (host clock)
      and what both sides then do alike, Image.save as .jpg into memory, for scale.
  (c) N consecutive Harness.generate calls under --synthetic --decode (full-size random FLUX, 4 steps, the FLUX VAE), files written to a
      temporary directory, until the last file is complete: without and with --hip_image_out, interleaved, one Harness.
Host clocks start behind a device synchronise; every side is warmed up; medians of REPS with min .. max.  The pixels of (a) and (b), and
the files of (c), are compared byte for byte.  The parent does not touch the GPU and stops at the first case that fails.  No speed target:
the result is stated as it falls.
  python tools/image_out_bench.py --log profiles/image_out_bench.log"""
import argparse
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("%dx%d B=%d" % (s, s, b), s, b) for s in (1024, 512) for b in (1, 4)]
LIMIT = 420                              # seconds per case


BATCH = 50                               # launches between two events: a kernel of microseconds is timed as a train of them


def device_ms(torch, fn, n=BATCH):
    """ms per call of fn on the device: n calls enqueued back to back between two events (one call would time the events and the launch
    latency as much as the kernel); where the calls are shorter than their enqueueing, this is the enqueue rate, and the line says so"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    h0 = time.perf_counter()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    h1 = time.perf_counter()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, (h1 - h0) * 1e3 / n


def host_ms(torch, fn):
    """ms from a synchronised device until fn has returned and the device is idle again; fn's result"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(xs):
    return "%9.3f ms  (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def run_case(label, reps, warmup, calls, runs, say, banner=False):
    import numpy as np
    import torch
    from PIL import Image

    from x2i_amd import image_out_binding as iob
    from x2i_amd.pipeline import FluxPipeline, VaeImageProcessor
    if not torch.cuda.is_available():
        sys.exit("image_out_bench: needs a GPU")
    _, size, B = next(c for c in CASES if c[0] == label)
    if banner:
        import PIL
        say("%s, torch %s, Pillow %s, %d CPU threads" % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__, torch.get_num_threads()))
    H = W = size
    h = w = size // 8
    sf, shift = 0.3611, 0.1159
    g = torch.Generator().manual_seed(size + B)
    lat = torch.randn((B, (h // 2) * (w // 2), 64), generator=g).to(torch.bfloat16).cuda()
    y = (torch.randn((B, H, W, 4), generator=g) * 0.7).to(torch.bfloat16).cuda()
    say()
    say("%s: %.2f MB of latents in; %.1f MB of float32 pixels leave the device in (a), %.1f MB of uint8 in (b)"
        % (label, 2e-6 * lat.numel(), 12e-6 * B * H * W, 3e-6 * B * H * W))

    # (a) the parent's two ends
    def head():
        x = FluxPipeline._unpack_latents(lat, size, size, 16)
        x = (x / sf) + shift
        z = torch.zeros((B, h, w, 64), device="cuda", dtype=torch.bfloat16)
        z[..., :16] = x.to(torch.bfloat16).permute(0, 2, 3, 1)
        return z

    proc = VaeImageProcessor(vae_scale_factor=16)
    tail = lambda: proc.postprocess(y[..., :3].permute(0, 3, 1, 2).contiguous(), output_type="pil")   # noqa: E731
    # (b) the new ones
    xo = torch.empty((B, h, w, 64), device="cuda", dtype=torch.bfloat16)
    n = B * H * W * 3
    dev, pinned, ev = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()
    k1 = lambda: iob.latents_to_vae(lat, h, w, 16, sf, shift, out=xo)      # noqa: E731
    k2 = lambda: iob.image_to_u8(y, out=dev)                               # noqa: E731

    def host():
        iob.image_to_u8(y, out=dev)
        pinned.copy_(dev, non_blocking=True)
        ev.record()
        ev.synchronize()
        a = pinned.numpy().reshape(B, H, W, 3)
        return [Image.fromarray(a[i]) for i in range(B)]

    for _ in range(max(warmup, 2)):
        head(), tail(), k1(), k2(), host()
    t = {k: [] for k in ("head", "tail", "k1", "k2", "host", "jpg", "head_enq", "k1_enq", "k2_enq")}
    for _ in range(reps):
        for k, fn in (("head", head), ("k1", k1), ("k2", k2)):
            d, e = device_ms(torch, fn)
            t[k].append(d)
            t[k + "_enq"].append(e)
        ms, old = host_ms(torch, tail)
        t["tail"].append(ms)
        ms, new = host_ms(torch, host)
        t["host"].append(ms)
        t0 = time.perf_counter()
        for im in new:
            im.save(io.BytesIO(), format="JPEG")
        t["jpg"].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(old, new)) and torch.equal(head(), xo)
    enq = lambda k: "   enqueue %.3f ms%s" % (statistics.median(t[k + "_enq"]),                     # noqa: E731
                                              " (launch-bound)" if statistics.median(t[k + "_enq"]) >= 0.9 * statistics.median(t[k]) else "")
    say("  (a) head: unpack, divide, add, zeros, copy (device)     %s%s" % (fmt(t["head"]), enq("head")))
    say("  (a) tail: NCHW copy + postprocess(..., 'pil') (host)     %s" % fmt(t["tail"]))
    say("  (b) x2i_latents_to_vae (device)                         %s%s" % (fmt(t["k1"]), enq("k1")))
    say("  (b) x2i_image_to_u8 (device)                            %s%s   %.0f GB/s read and written"
        % (fmt(t["k2"]), enq("k2"), (8 + 3) * B * H * W / statistics.median(t["k2"]) * 1e-6))
    say("  (b) host: kernel, pinned uint8 copy, wait, fromarray     %s" % fmt(t["host"]))
    say("  (a) / (b): head %.1fx, tail against host %.1fx; equal decoder inputs and equal pixels: %s"
        % (statistics.median(t["head"]) / statistics.median(t["k1"]), statistics.median(t["tail"]) / statistics.median(t["host"]), same))
    say("  both: Image.save as JPEG, %d image(s) (host)              %s" % (B, fmt(t["jpg"])))
    if not same:
        sys.exit("image_out_bench: the two sides differ")
    run_generate(size, B, calls, runs, say)


def run_generate(size, B, calls, runs, say):
    """(c): `calls` consecutive generate calls, wall clock from the first call until the last file is complete"""
    import torch

    from x2i_amd.image_out import ImageBackEnd, ImageWriter
    from x2i_amd.infer import harness as H
    with tempfile.TemporaryDirectory() as tmp:
        args = H.build_parser("qwenvl").parse_args(["--synthetic", "--decode", "--height", str(size), "--width", str(size), "--batch", str(B),
                                                     "--outputs", tmp, "--seed", "5"])
        hs = H.Harness(args, "qwen3b", H.SyntheticConditioner("qwen3b", "cuda"), "cuda")
        back, writer = ImageBackEnd(hs.vae, hs.device), ImageWriter()
        conds = [hs.embeds(batch=B, text_prompt="p%d" % i) for i in range(2)]

        def run(flag, tag):
            hs.image_out, hs.writer = (back, writer) if flag else (None, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(calls):
                pooled, embeds = conds[i % 2]
                hs.generate(pooled, embeds, tag, "img_%d" % i, seed=5 + i)
            hs.flush_outputs()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for tag in ("warm_plain", "warm_hip"):     # the eager pass, the capture and the first replay of the sampling graph; the ring
            run(tag.endswith("hip"), tag)
        plain, hip = [], []
        for r in range(runs):
            plain.append(run(False, "plain_%d" % r))
            hip.append(run(True, "hip_%d" % r))
        names = sorted(os.listdir(os.path.join(tmp, "plain_0")))
        same = names == sorted(os.listdir(os.path.join(tmp, "hip_0"))) and len(names) == calls * B and all(
            open(os.path.join(tmp, "plain_0", f), "rb").read() == open(os.path.join(tmp, "hip_0", f), "rb").read() for f in names)
        writer.close()
    say("  (c) %d generate calls (4 steps, decode, %d .jpg files), per call: without the flag %s" % (calls, calls * B, fmt([x / calls for x in plain])))
    say("  (c) %s                                  with --hip_image_out %s" % (" " * len(str(calls * B) + str(calls)), fmt([x / calls for x in hip])))
    say("  (c) without / with: %.3fx; the same files byte for byte: %s" % (statistics.median(plain) / statistics.median(hip), same))
    if not same:
        sys.exit("image_out_bench: the files differ")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=4, help="N of (c): consecutive generate calls per timed run")
    ap.add_argument("--runs", type=int, default=3, help="timed runs of (c) per side")
    ap.add_argument("--log", default=None)
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts per case)")
    ap.add_argument("--banner", action="store_true", help="with --case: print the device and library versions first")
    args = ap.parse_args()
    if args.case is not None:
        return run_case(args.case, args.reps, args.warmup, args.calls, args.runs, lambda s="": print(s, flush=True), args.banner)
    lines = ["image_out_bench: reps %d, warm-up %d, %d runs of %d generate calls per side of (c), one child process per case, %d s limit each"
             % (args.reps, args.warmup, args.runs, args.calls, LIMIT)]
    print(lines[0], flush=True)
    status = 0
    for label in [c[0] for c in CASES]:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--case", label, "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--calls", str(args.calls), "--runs", str(args.runs)] + (["--banner"] if label == CASES[0][0] else [])
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
