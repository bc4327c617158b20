"""The tiled image front ends restated in numpy on tests/image_ref.py (a helper of tests/test_image_tiles_*; it holds no tests): the
sliced form of MiniCPMVImageProcessor.preprocess (grid, source image, refine size, crops in row-major order, strip layout) and InternVL2.5's
load_image (the closest aspect ratio with its tie rule, the 448 x 448 crops of the resized whole, the thumbnail, ToTensor + Normalize).
A crop is a window of image_ref.resize of the WHOLE image, so everything stays integer arithmetic and a table lookup.

The `fault` arguments plant one deviation each; tests/test_image_tiles_ref_cpu.py asserts that every one of FAULTS differs from Pillow on
the inputs the GPU test uses.  "source_upscale" (the sliced source image sized with allow_upscale=True) is accepted as well but is NO
fault: an image is sliced only where w h > scale_resolution^2, and find_best_resize rescales every such image whatever allow_upscale
says; the CPU test proves that equality on every size of the fixture instead."""
import json
import math
import os

import numpy as np

from tests import image_ref as IR

PATCH = IR.PATCH
FAULTS = ("crop_own_box", "column_major", "refine_no_upscale", "source_last", "thumbnail_first", "thumbnail_single")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_grids.json")


def golden():
    """{"sizes": [(w, h)], "minicpm": {max_slice_nums: [(grid, source, refine)]}, "internvl": {max_num: [(gx, gy)]}} as recorded"""
    with open(GOLDEN) as f:
        rec = json.load(f)
    tup = lambda v: None if v is None else tuple(v)   # noqa: E731
    return {"sizes": [tuple(s) for s in rec["sizes"]],
            "minicpm": {int(m): [tuple(tup(v) for v in row) for row in rows] for m, rows in rec["minicpm"].items()},
            "internvl": {int(m): [tuple(r) for r in rows] for m, rows in rec["internvl"].items()}}


# ---------------------------------------------------------------------------------------------------------------- MiniCPM-o sizes
def find_best_resize(size, scale_resolution=448, patch=PATCH, allow_upscale=False):
    w, h = size
    if w * h > scale_resolution * scale_resolution or allow_upscale:
        r = w / h
        h = int(scale_resolution / math.sqrt(r))
        w = int(h * r)
    return IR.ensure_divide(w, patch), IR.ensure_divide(h, patch)


def sliced_grid(size, max_slice_nums, scale_resolution=448):
    """(gx, gy) or None: among the factorisations of multiple - 1, multiple, multiple + 1 slices (1 and more than max_slice_nums left
    out) the first whose log aspect ratio is nearest the image's"""
    w, h = size
    multiple = min(math.ceil(w * h / (scale_resolution * scale_resolution)), max_slice_nums)
    if multiple <= 1:
        return None
    best, err = (1, 1), float("inf")
    for n in (multiple - 1, multiple, multiple + 1):
        if n == 1 or n > max_slice_nums:
            continue
        for m in range(1, n + 1):
            if n % m == 0:
                e = abs(math.log(w / h) - math.log(m / (n // m)))
                if e < err:
                    best, err = (m, n // m), e
    return best


def refine_size(size, grid, scale_resolution=448, patch=PATCH, allow_upscale=True):
    """The size of the image the crops are cut from: the grid's cell (a FLOAT size) fitted as an image of its own, times the grid"""
    (w, h), (gx, gy) = size, grid
    cell = (IR.ensure_divide(w, gx) / gx, IR.ensure_divide(h, gy) / gy)
    bw, bh = find_best_resize(cell, scale_resolution, patch, allow_upscale)
    return bw * gx, bh * gy


def minicpm_sizes(size, max_slice_nums, scale_resolution=448, fault=None):
    """(grid or None, source size, refine size or None)"""
    grid = sliced_grid(size, max_slice_nums, scale_resolution)
    if grid is None:
        return None, find_best_resize(size, scale_resolution, PATCH, True), None
    return (grid, find_best_resize(size, scale_resolution, PATCH, fault == "source_upscale"),
            refine_size(size, grid, scale_resolution, PATCH, fault != "refine_no_upscale"))


# ---------------------------------------------------------------------------------------------------------------- crops
def crops_of(res, tile_w, tile_h):
    """The crops [tile_h, tile_w, 3] of a resized image, row-major"""
    return [res[i:i + tile_h, j:j + tile_w] for i in range(0, res.shape[0], tile_h) for j in range(0, res.shape[1], tile_w)]


def grid_crops(img, out_w, out_h, tile_w, tile_h, fault=None):
    """uint8 [H, W, 3] -> the gy gx crops [tile_h, tile_w, 3] of resize(img, out_w, out_h), row-major"""
    gx, gy = out_w // tile_w, out_h // tile_h
    assert gx * tile_w == out_w and gy * tile_h == out_h
    h, w = img.shape[:2]
    if fault == "crop_own_box":      # each crop resized from its own box of the input: no taps across the crops' edges
        crops = [IR.resize(img[i * h // gy:(i + 1) * h // gy, j * w // gx:(j + 1) * w // gx], tile_w, tile_h) for i in range(gy) for j in range(gx)]
    else:
        crops = crops_of(IR.resize(img, out_w, out_h), tile_w, tile_h)
    if fault == "column_major":
        crops = [crops[i * gx + j] for j in range(gx) for i in range(gy)]
    return crops


def strip_of(u8, table):
    return IR.strip(np.stack([table[c][u8[:, :, c]] for c in range(3)], axis=-1))


def planar_of(u8, table):
    return np.stack([table[c][u8[:, :, c]] for c in range(3)])


def tiles_expected(img, out_w, out_h, tile_w, tile_h, layout, table):
    """What x2i_image_tiles stores for one frame: a list of float32 crops, [3, 14, 14 L] (layout 0) or [3, tile_h, tile_w] (layout 1)"""
    return [(planar_of if layout else strip_of)(c, table) for c in grid_crops(img, out_w, out_h, tile_w, tile_h)]


def minicpm_slices(img, max_slice_nums=9, scale_resolution=448, fault=None):
    """get_sliced_images as uint8 arrays: [source, crops ...]"""
    h, w = img.shape[:2]
    grid, source, refine = minicpm_sizes((w, h), max_slice_nums, scale_resolution, fault)
    out = [IR.resize(img, *source)]
    if grid is not None:
        crops = grid_crops(img, refine[0], refine[1], refine[0] // grid[0], refine[1] // grid[1], fault)
        out = crops + out if fault == "source_last" else out + crops
    return out


def minicpm_preprocess(images, max_slice_nums=9, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), scale_resolution=448):
    """What MiniCPMVImageProcessor.preprocess gives for a list of uint8 [H, W, 3] arrays: ([float32 [3, 14, 14 L]] with every image's
    source image and crops in a row, [(w, h)] per image, int [slices, 2] of (patch rows, patch columns))"""
    table = IR.lut(mean, std)
    pv, sizes, tgt = [], [], []
    for img in images:
        for s in minicpm_slices(img, max_slice_nums, scale_resolution):
            pv.append(strip_of(s, table))
            tgt.append((s.shape[0] // PATCH, s.shape[1] // PATCH))
        sizes.append((img.shape[1], img.shape[0]))
    return pv, sizes, np.array(tgt)


# ---------------------------------------------------------------------------------------------------------------- InternVL2.5
def target_ratios(min_num=1, max_num=12):
    """The candidate grids in the order dynamic_preprocess tries them: a SET of (i, j), then a stable sort by area.  Ties of
    closest_ratio fall by this order, so the list is built the way the original builds it"""
    ratios = set()
    for n in range(min_num, max_num + 1):                     # (the same pairs added in the same order: a set iterates by its history)
        for i in range(1, n + 1):
            for j in range(1, n + 1):
                if min_num <= i * j <= max_num:
                    ratios.add((i, j))
    return sorted(ratios, key=lambda r: r[0] * r[1])


def closest_ratio(w, h, max_num=12, image_size=448):
    """(gx, gy): the nearest aspect ratio; of equally near ones the later wins where the image's area exceeds half the grid's"""
    aspect, best, best_diff = w / h, (1, 1), float("inf")
    for r in target_ratios(1, max_num):
        diff = abs(aspect - r[0] / r[1])
        if diff < best_diff:
            best, best_diff = r, diff
        elif diff == best_diff and w * h > 0.5 * image_size * image_size * r[0] * r[1]:
            best = r
    return best


def internvl_tiles(img, max_num=12, image_size=448, use_thumbnail=True, fault=None):
    """dynamic_preprocess as uint8 arrays [448, 448, 3]: the crops of the resized whole in the order (i % gx, i // gx), then the thumbnail
    where there is more than one crop"""
    h, w = img.shape[:2]
    gx, gy = closest_ratio(w, h, max_num, image_size)
    out = grid_crops(img, image_size * gx, image_size * gy, image_size, image_size, fault)
    if use_thumbnail and (len(out) != 1 or fault == "thumbnail_single"):
        thumb = [IR.resize(img, image_size, image_size)]
        out = thumb + out if fault == "thumbnail_first" else out + thumb
    return out


def torch_lut(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """float32 [3, 256]: ToTensor (v.float().div(255)) and Normalize (sub mean, div std, both float32 tensors), torch's own expressions"""
    import torch
    v = torch.arange(256, dtype=torch.uint8).float().div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return torch.stack([v.sub(m[c]).div(s[c]) for c in range(3)]).numpy()


def load_image(img, max_num=12, image_size=448, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """load_image: float32 [tiles, 3, 448, 448]"""
    table = torch_lut(mean, std)
    return np.stack([planar_of(t, table) for t in internvl_tiles(img, max_num, image_size)])


# ---------------------------------------------------------------------------------------------------------------- the GPU test's cases
# (name, in_w, in_h, out_w, out_h, tile_w, tile_h, layout).  LDS plan (rows, patches per workgroup) beside the cases that choose it.
GPU_CASES = [
    ("minicpm-640x480-slices9", 640, 480, 728, 546, 364, 546, 0),      # the fixture's grid (2, 1) for max_slice_nums 9: crops 26 x 39 patches
    ("minicpm-640x480-slices2", 640, 480, 728, 546, 364, 546, 0),      # ... and for 2: the same grid and refine size, as recorded
    ("cell-5x3-patches", 100, 75, 140, 126, 70, 42, 0),                # 5 patches wide (4 + a partial tile of 1 at every crop's edge), 3 high
    ("cell-5x3-patches-planar", 100, 75, 140, 126, 70, 42, 1),
    ("strip-9x1", 300, 40, 378, 28, 42, 28, 0),
    ("strip-1x9", 40, 300, 42, 252, 42, 28, 0),
    ("strip-1x9-planar", 40, 300, 42, 252, 42, 28, 1),
    ("internvl-97x61", 97, 61, 1344, 896, 448, 448, 1),                # enlarged, 3 x 2 tiles (the 7th, the thumbnail, is a 1 x 1 grid)
    ("internvl-97x61-thumbnail", 97, 61, 448, 448, 448, 448, 1),
    ("reduce-4000x3000", 4000, 3000, 84, 42, 42, 14, 0),               # rows 1214 of at most 1489: one patch per workgroup
    ("reduce-two-patches", 61, 500, 140, 14, 70, 14, 0),               # rows 500: two patches per workgroup, 5 = 2 + 2 + 1 per crop
    ("width-unchanged", 84, 61, 84, 84, 42, 28, 0),
    ("height-unchanged", 61, 56, 140, 56, 70, 28, 1),
]

# the end-to-end inputs of the GPU test: (w, h) per image, in the order of the call
E2E_MINICPM = [(640, 480), (97, 61), (640, 480), (1280, 720)]           # max_slice_nums 9: grids (2, 1), none, (2, 1), (3, 2)
E2E_INTERNVL = [(97, 61), (128, 128), (97, 61), (640, 480)]             # max_num 12: 3 x 2 + 1, 1, 3 x 2 + 1, 4 x 3 + 1 tiles


def e2e_images(sizes, seed=11):
    return [IR.edge_frames(w, h, 1, seed=seed + i)[0] for i, (w, h) in enumerate(sizes)]


# ---------------------------------------------------------------------------------------------------------------- stand-in processor
class SlicingStubImageProcessor(IR.StubImageProcessor):
    """IR.StubImageProcessor with the processor's real grid and the sliced preprocess restated above: per image [source, crops ...]"""

    def get_sliced_grid(self, image_size, max_slice_nums, never_split=False):
        grid = None if never_split else sliced_grid(image_size, max_slice_nums, self.scale_resolution)
        return None if grid is None else list(grid)

    def preprocess(self, images, do_pad=True, max_slice_nums=None, return_tensors=None, **kwargs):
        if not isinstance(images, list):
            images = [[images]]
        elif len(images) and not isinstance(images[0], list):
            images = [images]
        slices = self.max_slice_nums if max_slice_nums is None else int(max_slice_nums)
        pv, sizes, tgt = [], [], []
        for group in images:
            arrays = [np.asarray(im.convert("RGB") if hasattr(im, "convert") else im) for im in group]
            self.sliced += sum(self.get_sliced_grid((a.shape[1], a.shape[0]), slices) is not None for a in arrays)
            p, s, t = minicpm_preprocess(arrays, slices, self.mean, self.std, self.scale_resolution) if arrays else ([], [], [])
            pv.append(p)
            sizes.append(s)
            tgt.append(t)
        return IR.StubBatchFeature(data={"pixel_values": pv, "image_sizes": sizes, "tgt_sizes": tgt}, tensor_type=return_tensors)
