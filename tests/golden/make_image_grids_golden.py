#!/usr/bin/env python3
"""Records tests/golden/image_grids.json: what the reference's own grid functions give for about 200 image sizes.

  python tests/golden/make_image_grids_golden.py --reference DIR      (DIR: a checkout of the reference project)

The functions are pure arithmetic on sizes, and they are loaded from the reference as they stand; only what their modules import around
them is stubbed (transformers' image-processor base classes for minicpm/image_processing_minicpmv.py, torchvision.transforms for
utils/internvl_util.py), so that neither package version matters.  Recorded per size (w, h):
  minicpm[str(max_slice_nums)], max_slice_nums in 2, 6, 9:  [grid or null, source size, refine size or null]
      grid = get_sliced_grid, source = the size slice_image resizes the source image to, refine = get_refine_size(allow_upscale=True)
  internvl[str(max_num)], max_num in 1, 6, 12:  [gx, gy] of dynamic_preprocess (read off a stand-in image's resize call)
Nothing of the reference's text is copied; the file holds sizes and results only."""
import argparse
import importlib.util
import json
import os
import random
import sys
import types

SLICES, MAX_NUMS = (2, 6, 9), (1, 6, 12)


class _Anything:
    def __init__(self, *a, **k):
        pass

    @classmethod
    def register(cls, *a, **k):
        pass


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


def _load(path, name, stubs):
    saved = {k: sys.modules.get(k) for k in stubs}
    for k in stubs:
        sys.modules[k] = _Stub(k)
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                del sys.modules[k]
            else:
                sys.modules[k] = v
    return mod


def sizes():
    out = [(640, 480), (1280, 720), (97, 61), (4000, 3000), (1920, 1080), (128, 128), (448, 448), (449, 448), (448, 449), (449, 449),
           (450, 447), (500, 402), (402, 500), (224, 897), (897, 224)]
    out += [(9 * k, k) for k in (50, 100, 149, 150, 151, 300, 448)] + [(k, 9 * k) for k in (50, 100, 149, 150, 151, 300, 448)]   # 9:1, 1:9 strips
    out += [(w, h) for w in (641, 643, 1281, 1283, 903, 917, 1337) for h in (480, 481, 721)]           # halves in ensure_divide: round's ties
    out += [(2 * 448 + d, 448 + e) for d in (-1, 0, 1) for e in (-1, 0, 1)] + [(448 + e, 3 * 448 + d) for d in (-1, 0, 1) for e in (-1, 0, 1)]
    rng = random.Random(20260)
    while len(out) < 200:
        out.append((rng.randint(20, 4200), rng.randint(20, 4200)))
    assert len(set(out)) == len(out)
    return out


class _SizeOnly:
    """An image of which dynamic_preprocess reads the size; the first resize call carries the tiled size"""

    def __init__(self, size, log):
        self.size, self.log = size, log

    def resize(self, size, *a, **k):
        self.log.append(tuple(size))
        return self

    def crop(self, box):
        return self


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_grids.json"))
    args = ap.parse_args()
    mc = _load(os.path.join(args.reference, "minicpm", "image_processing_minicpmv.py"), "ref_minicpm_image",
               ["transformers", "transformers.image_processing_utils", "transformers.image_transforms", "transformers.image_utils", "transformers.utils"])
    iv = _load(os.path.join(args.reference, "utils", "internvl_util.py"), "ref_internvl_util", ["torchvision", "torchvision.transforms"])
    ip = mc.MiniCPMVImageProcessor()
    assert (ip.max_slice_nums, ip.scale_resolution, ip.patch_size) == (9, 448, 14)
    szs = sizes()
    rec = {"sizes": [list(s) for s in szs], "minicpm": {}, "internvl": {}}
    for m in SLICES:
        rows = []
        for wh in szs:
            grid = ip.get_sliced_grid(wh, m)
            if grid is None:
                rows.append([None, list(ip.find_best_resize(wh, 448, 14, allow_upscale=True)), None])
            else:
                rows.append([list(grid), list(ip.find_best_resize(wh, 448, 14)), list(ip.get_refine_size(wh, grid, 448, 14, allow_upscale=True))])
        rec["minicpm"][str(m)] = rows
    for m in MAX_NUMS:
        rows = []
        for wh in szs:
            log = []
            tiles = iv.dynamic_preprocess(_SizeOnly(wh, log), image_size=448, use_thumbnail=True, max_num=m)
            gx, gy = log[0][0] // 448, log[0][1] // 448
            assert log[0] == (448 * gx, 448 * gy) and len(tiles) == gx * gy + (gx * gy > 1) and (len(log) == 2) == (gx * gy > 1)
            rows.append([gx, gy])
        rec["internvl"][str(m)] = rows
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, separators=(",", ":")).replace("],[", "],\n[") + "\n")
    print("wrote %s: %d sizes" % (args.out, len(szs)))


if __name__ == "__main__":
    main()
