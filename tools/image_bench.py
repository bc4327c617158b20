#!/usr/bin/env python3
"""Time the MiniCPM-o image front end on the HIP path (handoff.HipImage over x2i_amd.image.ImageFrontEnd) against the same computation on
the host: what MiniCPMVImageProcessor.preprocess does for an image that is not sliced, composed here from Pillow + numpy + torch --
Image.resize(best_size, BICUBIC), astype(float32) / 255, (x - mean) / std, channel first, the strip layout [3, 14, 14 L], one float32 tensor
per frame -- followed by .to(device) of every tensor.
  64 x 1280x720    a video's 64 frames
  16 x 1920x1080
  1 x 4000x3000    one photograph (max_slice_nums = 1)
  1 x 128x128
Both sides get the same PIL images and are called the way the MiniCPM-o processor calls its image processor (do_pad, max_slice_nums=1,
return_tensors).  Per side, host clocks: `call` until the call returns (the host's own time: for hip the pinned copy and the enqueueing,
for the host side the whole computation and the copies' enqueueing) and `total` until a device synchronise after it.  Every side is
warmed up, then REPS interleaved repetitions; median and min .. max.  Beside them the kernel's device time from device events around the
launch alone, on frames already on the device, and whether the two sides' pixel_values are equal bit for bit.
No speed target: the result is stated as it falls.  Run it under a time limit (timeout -k 10 600 python tools/image_bench.py --log
profiles/image_frontend_bench.log)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import handoff, image_binding as ib  # noqa: E402

CASES = [("64 x 1280x720", 64, 1280, 720), ("16 x 1920x1080", 16, 1920, 1080), ("1 x 4000x3000", 1, 4000, 3000), ("1 x 128x128", 1, 128, 128)]


class Feature(dict):
    """pixel_values / image_sizes / tgt_sizes as they come (no tensor conversion is asked for here)"""

    def __init__(self, data=None, tensor_type=None):
        dict.__init__(self, data or {})

    @property
    def data(self):
        return self

    @data.setter
    def data(self, value):
        items = dict(value)
        self.clear()
        self.update(items)


class HostImageProcessor:
    """The host side: the fields a hand-off reads, and preprocess composed from Pillow + numpy + torch for images that are not sliced"""
    max_slice_nums, scale_resolution, patch_size, slice_mode = 9, 448, 14, True
    mean, std = np.array([0.5, 0.5, 0.5]), np.array([0.5, 0.5, 0.5])

    def get_sliced_grid(self, image_size, max_slice_nums, never_split=False):
        w, h = image_size
        multiple = min(math.ceil(w * h / self.scale_resolution ** 2), max_slice_nums)
        return None if multiple <= 1 or never_split else [1, multiple]

    def best_size(self, w, h):
        r = w / h
        height = int(self.scale_resolution / math.sqrt(r))
        width = int(height * r)
        fit = lambda v: max(round(v / 14) * 14, 14)   # noqa: E731
        return fit(width), fit(height)

    def one(self, image):
        assert self.get_sliced_grid(image.size, 1) is None
        small = image.resize(self.best_size(*image.size), resample=Image.Resampling.BICUBIC)
        x = np.asarray(small).astype(np.float32) / 255
        x = (x - self.mean.astype(x.dtype)) / self.std.astype(x.dtype)
        x = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))
        gh, gw = x.shape[1] // 14, x.shape[2] // 14
        return x.reshape(3, gh, 14, gw, 14).permute(0, 2, 1, 3, 4).reshape(3, 14, -1), np.array((gh, gw))

    def preprocess(self, images, do_pad=True, max_slice_nums=None, return_tensors=None):
        pv, sizes, tgt = [], [], []
        for group in images:
            done = [self.one(im) for im in group]
            pv.append([d[0] for d in done])
            sizes.append([im.size for im in group])
            tgt.append(np.vstack([d[1] for d in done]) if done else [])
        return Feature({"pixel_values": pv, "image_sizes": sizes, "tgt_sizes": tgt})

    __call__ = preprocess


class Processor:
    def __init__(self):
        self.image_processor = HostImageProcessor()


def clocks(fn):
    """(ms until fn returns, ms until the device has finished too, fn's result)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, out


def device_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def fmt(xs):
    return "%9.3f ms  (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_bench: needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import PIL
    proc = Processor()
    host_ip = proc.image_processor
    hip = handoff.HipImage(proc, "cuda").install()
    hip_ip = proc.image_processor
    say("image_bench: %s, torch %s, Pillow %s, %d CPU threads, reps %d, warm-up %d"
        % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__, torch.get_num_threads(), args.reps, args.warmup))
    for label, n, w, h in CASES:
        rng = np.random.default_rng(w + n)
        images = [[Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for _ in range(n)]]
        ow, oh = hip.front.best_size(w, h)
        sides = [
            ("hip", lambda: hip_ip(images, do_pad=True, max_slice_nums=1, return_tensors=None)["pixel_values"][0]),
            ("host", lambda: [t.to("cuda", non_blocking=True) for t in host_ip(images, do_pad=True, max_slice_nums=1, return_tensors=None)["pixel_values"][0]]),
        ]
        call, total, outs = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}, {}
        for _ in range(args.warmup):
            for k, fn in sides:
                clocks(fn)
        for _ in range(args.reps):
            for k, fn in sides:
                c, t, outs[k] = clocks(fn)
                call[k].append(c)
                total[k].append(t)
        assert hip.fallbacks == 0
        say()
        say("%s -> %dx%d: %.1f MB of uint8 frames in, %.1f MB of float32 pixel_values out, LDS plan (rows, patches, pitch) %s"
            % (label, ow, oh, 3e-6 * n * w * h, 12e-6 * n * ow * oh, ib.lds_plan(h, oh)))
        for k, _ in sides:
            say("  %-5s call  %s" % (k, fmt(call[k])))
            say("  %-5s total %s" % (k, fmt(total[k])))
        say("  host / hip (medians): call %.1fx, total %.1fx" % (statistics.median(call["host"]) / statistics.median(call["hip"]),
                                                                 statistics.median(total["host"]) / statistics.median(total["hip"])))
        say("  hip == host bit for bit: %s" % all(torch.equal(a, b) for a, b in zip(outs["hip"], outs["host"])))
        # the kernel alone, device events around the launch, the frames already on the device
        front = hip.front
        frames = torch.from_numpy(np.stack([np.asarray(im) for im in images[0]])).cuda().reshape(-1)
        out = torch.empty(n * 3 * ow * oh, dtype=torch.float32, device="cuda")
        hb, hc = front.tables(w, ow)
        vb, vc = front.tables(h, oh)
        launch = lambda: ib.frontend(frames, w, h, 3 * w, 3 * w * h, n, ow, oh, hb, hc, vb, vc, front.lut, out, 3 * ow * oh, oh // 14 * ow)   # noqa: E731
        for _ in range(args.warmup):
            launch()
        ks = [device_ms(launch) for _ in range(args.reps)]
        say("  image_frontend_kernel %s   %.1f GB/s of frames read and values written" % (fmt(ks), (3 * n * w * h + 12 * n * ow * oh) / statistics.median(ks) * 1e-6))
    hip.remove()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
