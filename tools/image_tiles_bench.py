#!/usr/bin/env python3
"""Time the tiled image front ends on the HIP path against the same computations on the host, composed here from Pillow + numpy + torch
and followed by .to(device), in the same run (the method of tools/image_bench.py):
  MiniCPM-o, max_slice_nums = 9   handoff.HipImage(slices=True) over x2i_amd.image.ImageFrontEnd  against  get_sliced_images -- the source
                                  image and the refine-size image by Image.resize(BICUBIC), the crops by Image.crop -- astype(float32) / 255,
                                  (x - mean) / std, channel first, the strip layout [3, 14, 14 L], one float32 tensor per slice
  InternVL2.5, max_num = 12       x2i_amd.internvl_image.InternVLImageFrontEnd.tiles  against  load_image -- Image.resize((448 gx, 448 gy)),
                                  the 448 x 448 crops, the thumbnail, per tile float().div(255), sub(mean).div(std), torch.stack
each on one 4000x3000, one 1920x1080 and one 640x480 image.  Per side, host clocks: `call` until the call returns and `total` until a
device synchronise after it.  Every side is warmed up, then REPS interleaved repetitions; median and min .. max.  Beside them the tiles
kernel's device time from device events around the launch alone, on a frame already on the device, and whether the two sides' values are
equal bit for bit.  No speed target: the result is stated as it falls.  Run it under a time limit (timeout -k 10 600 python
tools/image_tiles_bench.py --log profiles/image_tiles_bench.log)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import handoff, image_binding as ib, image_tiles_binding as itb  # noqa: E402
from x2i_amd.image import ImageFrontEnd  # noqa: E402
from x2i_amd.internvl_image import IMAGENET_MEAN, IMAGENET_STD, InternVLImageFrontEnd  # noqa: E402

SIZES = [(4000, 3000), (1920, 1080), (640, 480)]


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
    """The host side of MiniCPM-o: the fields a hand-off reads, and the sliced preprocess composed from Pillow + numpy + torch.  The sizes
    come from the front end's own arithmetic (equal to the processor's on the recorded fixture, tests/test_image_tiles_ref_cpu.py)."""
    max_slice_nums, scale_resolution, patch_size, slice_mode = 9, 448, 14, True
    mean, std = np.array([0.5, 0.5, 0.5]), np.array([0.5, 0.5, 0.5])
    sizes = ImageFrontEnd(device="cpu")

    def get_sliced_grid(self, image_size, max_slice_nums, never_split=False):
        grid = None if never_split else self.sizes.sliced_grid(image_size[0], image_size[1], max_slice_nums)
        return None if grid is None else list(grid)

    def one(self, image):
        x = np.asarray(image).astype(np.float32) / 255
        x = (x - self.mean.astype(x.dtype)) / self.std.astype(x.dtype)
        x = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))
        gh, gw = x.shape[1] // 14, x.shape[2] // 14
        return x.reshape(3, gh, 14, gw, 14).permute(0, 2, 1, 3, 4).reshape(3, 14, -1), np.array((gh, gw))

    def slices(self, image, max_slice_nums):
        source, grid, crop = self.sizes.slice_plan(image.size[0], image.size[1], max_slice_nums)
        out = [image.resize(source, resample=Image.Resampling.BICUBIC)]
        if grid is not None:
            (cw, ch), (gx, gy) = crop, grid
            refine = image.resize((cw * gx, ch * gy), resample=Image.Resampling.BICUBIC)
            out += [refine.crop((j * cw, i * ch, (j + 1) * cw, (i + 1) * ch)) for i in range(gy) for j in range(gx)]
        return out

    def preprocess(self, images, do_pad=True, max_slice_nums=None, return_tensors=None):
        m = self.max_slice_nums if max_slice_nums is None else int(max_slice_nums)
        pv, sizes, tgt = [], [], []
        for group in images:
            done = [self.one(s) for im in group for s in self.slices(im, m)]
            pv.append([d[0] for d in done])
            sizes.append([im.size for im in group])
            tgt.append(np.vstack([d[1] for d in done]) if done else [])
        return Feature({"pixel_values": pv, "image_sizes": sizes, "tgt_sizes": tgt})

    __call__ = preprocess


class Processor:
    def __init__(self):
        self.image_processor = HostImageProcessor()


def host_load_image(front, image, max_num=12):
    """load_image composed from Pillow + torch: float32 [tiles, 3, 448, 448] on the host"""
    gx, gy = front.grid(image.size[0], image.size[1], max_num)
    res = image.resize((448 * gx, 448 * gy))
    tiles = [res.crop(((i % gx) * 448, (i // gx) * 448, (i % gx + 1) * 448, (i // gx + 1) * 448)) for i in range(gx * gy)]
    if len(tiles) != 1:
        tiles.append(image.resize((448, 448)))
    mean, std = torch.tensor(IMAGENET_MEAN)[:, None, None], torch.tensor(IMAGENET_STD)[:, None, None]
    return torch.stack([torch.from_numpy(np.asarray(t)).permute(2, 0, 1).float().div(255).sub(mean).div(std) for t in tiles])


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


def compare(say, args, sides, equal):
    call, total, outs = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}, {}
    for _ in range(args.warmup):
        for k, fn in sides:
            clocks(fn)
    for _ in range(args.reps):
        for k, fn in sides:
            c, t, outs[k] = clocks(fn)
            call[k].append(c)
            total[k].append(t)
    for k, _ in sides:
        say("  %-5s call  %s" % (k, fmt(call[k])))
        say("  %-5s total %s" % (k, fmt(total[k])))
    say("  host / hip (medians): call %.1fx, total %.1fx" % (statistics.median(call["host"]) / statistics.median(call["hip"]),
                                                             statistics.median(total["host"]) / statistics.median(total["hip"])))
    say("  hip == host bit for bit: %s" % equal(outs["hip"], outs["host"]))


def kernel_alone(say, args, front, lut, image, ow, oh, tw, th, layout):
    w, h = image.size
    frame = torch.from_numpy(np.asarray(image)).cuda().reshape(-1)
    tile = 3 * tw * th
    n = (ow // tw) * (oh // th)
    out = torch.empty(n * tile, dtype=torch.float32, device="cuda")
    rs = tw if layout else th // 14 * tw
    launch = lambda: itb.tiles(frame, w, h, 3 * w, 3 * w * h, 1, ow, oh, tw, th, *front.tables(w, ow), *front.tables(h, oh), lut, out,   # noqa: E731
                               n * tile, tile, rs, layout)
    for _ in range(args.warmup):
        launch()
    ks = [device_ms(launch) for _ in range(args.reps)]
    say("  image_passes_kernel (x2i_image_tiles, %d crops of %dx%d, LDS plan %s) %s   %.1f GB/s of frame read and values written"
        % (n, tw, th, ib.lds_plan(h, oh), fmt(ks), (3 * w * h + 4 * n * tile) / statistics.median(ks) * 1e-6))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_tiles_bench: needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import PIL
    say("image_tiles_bench: %s, torch %s, Pillow %s, %d CPU threads, reps %d, warm-up %d"
        % (torch.cuda.get_device_name(0), torch.__version__, PIL.__version__, torch.get_num_threads(), args.reps, args.warmup))
    images = {}
    for w, h in SIZES:
        images[(w, h)] = Image.fromarray(np.random.default_rng(w).integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    # ---- MiniCPM-o, max_slice_nums = 9
    proc = Processor()
    host_ip = proc.image_processor
    hip = handoff.HipImage(proc, "cuda", slices=True).install()
    hip_ip = proc.image_processor
    for (w, h), image in images.items():
        source, grid, crop = hip.front.slice_plan(w, h, 9)
        say()
        say("MiniCPM-o 1 x %dx%d, max_slice_nums 9 -> source %dx%d + %d x %d crops of %dx%d: %.1f MB of uint8 in, %.1f MB of float32 pixel_values out"
            % (w, h, source[0], source[1], grid[0], grid[1], crop[0], crop[1], 3e-6 * w * h,
               12e-6 * (source[0] * source[1] + grid[0] * grid[1] * crop[0] * crop[1])))
        batch = [[image]]
        sides = [
            ("hip", lambda: hip_ip(batch, do_pad=True, max_slice_nums=9, return_tensors=None)["pixel_values"][0]),
            ("host", lambda: [t.to("cuda", non_blocking=True) for t in host_ip(batch, do_pad=True, max_slice_nums=9, return_tensors=None)["pixel_values"][0]]),
        ]
        compare(say, args, sides, lambda a, b: len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)))
        assert hip.fallbacks == 0
        kernel_alone(say, args, hip.front, hip.front.lut, image, crop[0] * grid[0], crop[1] * grid[1], crop[0], crop[1], itb.STRIP)
    hip.remove()
    # ---- InternVL2.5, max_num = 12
    front = InternVLImageFrontEnd(device="cuda")
    for (w, h), image in images.items():
        gx, gy = front.grid(w, h, 12)
        say()
        say("InternVL2.5 1 x %dx%d, max_num 12 -> %d x %d tiles of 448x448 + thumbnail: %.1f MB of uint8 in, %.1f MB of float32 pixel_values out"
            % (w, h, gx, gy, 3e-6 * w * h, 12e-6 * 448 * 448 * (gx * gy + 1)))
        sides = [
            ("hip", lambda: front.tiles([image], max_num=12)[0]),
            ("host", lambda: host_load_image(front, image, 12).to("cuda", non_blocking=True)),
        ]
        compare(say, args, sides, lambda a, b: torch.equal(a, b))
        kernel_alone(say, args, front, front.lut, image, 448 * gx, 448 * gy, 448, 448, itb.PLANAR)
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
