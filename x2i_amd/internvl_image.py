"""The InternVL2.5 image front end on the HIP path: what `load_image` of the model's utilities computes on the host -- dynamic_preprocess
(the grid of 448 x 448 tiles whose aspect ratio is nearest the image's, cut from ONE Pillow resize of the whole image, and a 448 x 448
thumbnail where there is more than one tile), ToTensor and Normalize -- as launches of libx2i_hip.so
(include/frontend/tiles/x2i_image_tiles.h, csrc/image_tiles.hip, planar layout).  The tower behind it is x2i_amd/internvit.py.

`image.resize(size)` without a filter is BICUBIC for an RGB image, so the arithmetic is the one of include/frontend/x2i_image.h; the
transform's own Resize((448, 448)) meets a 448 x 448 tile and copies it.  ToTensor + Normalize are a [3][256] float32 table made with
torch's own float32 expressions.  The result equals the host's float32 values bit for bit; bf16 is one rounding of them.

A run of consecutive, equally sized images costs two launches: the crops of the grid, and the thumbnails (a 1 x 1 grid) behind them.
"""
import torch

from . import image_tiles_binding as itb
from .image import StagedFrontEnd

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def tensor_lut(mean, std):
    """float32 [3, 256]: ToTensor's v.float().div(255), then Normalize's sub(mean).div(std) with float32 mean and std"""
    v = torch.arange(256, dtype=torch.uint8).float().div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return torch.stack([v.sub(m[c]).div(s[c]) for c in range(3)])


def target_ratios(min_num, max_num):
    """dynamic_preprocess's candidate grids in the order it tries them.  The order decides ties, and it is the order of a stable sort by
    area over the iteration of a SET of (i, j), so the set is filled with the same pairs in the same order"""
    ratios = set()
    for n in range(min_num, max_num + 1):                     # (the same pairs added in the same order: a set iterates by its history)
        for i in range(1, n + 1):
            for j in range(1, n + 1):
                if min_num <= i * j <= max_num:
                    ratios.add((i, j))
    return sorted(ratios, key=lambda r: r[0] * r[1])


def closest_ratio(w, h, max_num=12, image_size=448, min_num=1):
    """find_closest_aspect_ratio: (gx, gy).  Of equally near ratios the first stays, unless a later one's grid has less than twice the
    image's area"""
    aspect, best, best_diff = w / h, (1, 1), float("inf")
    for r in target_ratios(min_num, max_num):
        diff = abs(aspect - r[0] / r[1])
        if diff < best_diff:
            best, best_diff = r, diff
        elif diff == best_diff and w * h > 0.5 * image_size * image_size * r[0] * r[1]:
            best = r
    return best


class InternVLImageFrontEnd(StagedFrontEnd):
    """images -> (pixel_values [sum of tiles, 3, image_size, image_size] on the device, num_patches_list)"""

    _noun = "images"

    def __init__(self, image_size=448, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda"):
        super().__init__(mean, std, device)
        image_size = int(image_size)
        if image_size < itb.PATCH or image_size % itb.PATCH or image_size > itb.PATCH * itb.MAX_PATCHES:
            raise ValueError("x2i_amd InternVLImageFrontEnd: image_size = %d must be a multiple of 14 in 14..980" % image_size)
        self.image_size = image_size
        self.lut = tensor_lut(self.mean, self.std).to(self.device)

    def grid(self, w, h, max_num=12):
        """(gx, gy) of a w x h image"""
        max_num = int(max_num)
        if not 1 <= max_num <= itb.MAX_GRID:
            raise ValueError("x2i_amd InternVLImageFrontEnd: max_num = %d must be in 1..12 (a grid side is at most 12 tiles)" % max_num)
        return closest_ratio(w, h, max_num, self.image_size)

    @torch.no_grad()
    def tiles(self, images, max_num=12, use_thumbnail=True, out_dtype=torch.float32, plan=None):
        """images: PIL RGB images or uint8 [H, W, 3] arrays.  -> (pixel_values of out_dtype (float32 or bfloat16), per image the crops in
        the order (i % gx, i // gx) and then the thumbnail where there is more than one crop; num_patches_list, the tiles per image)"""
        arrays = self._as_arrays(images)
        self._check_out_dtype(out_dtype)
        S = self.image_size
        grids = [self.grid(a.shape[1], a.shape[0], max_num) for a in arrays]
        counts = [gx * gy + int(bool(use_thumbnail) and gx * gy > 1) for gx, gy in grids]
        for a, (gx, gy) in zip(arrays, grids):
            itb.check_sizes(a.shape[1], a.shape[0], S * gx, S * gy, S, S)
            itb.check_sizes(a.shape[1], a.shape[0], S, S, S, S)
        plan = self._plan_of_call(plan, sum(a.size for a in arrays))
        tile = 3 * S * S
        out = torch.empty(sum(counts) * tile, dtype=out_dtype, device=self.device)
        runs = []                                               # (first image, images) of a run of equally sized images: one grid, one stride
        for i, a in enumerate(arrays):
            if runs and arrays[runs[-1][0]].shape == a.shape:
                runs[-1][1] += 1
            else:
                runs.append([i, 1])
        dst = 0
        for (i, n), dev in self._staged(plan, [((i, n), arrays[i:i + n]) for i, n in runs]):
            (h, w), (gx, gy), per = arrays[i].shape[:2], grids[i], counts[i]
            fb = 3 * w * h
            itb.tiles(dev, w, h, 3 * w, fb, n, S * gx, S * gy, S, S, *self.tables(w, S * gx), *self.tables(h, S * gy), self.lut,
                      out[dst:dst + n * per * tile], per * tile, tile, S, itb.PLANAR)
            if per > gx * gy:                                 # the thumbnails: the last tile of every image of the run
                itb.tiles(dev, w, h, 3 * w, fb, n, S, S, S, S, *self.tables(w, S), *self.tables(h, S), self.lut,
                          out[dst + gx * gy * tile:dst + n * per * tile], per * tile, tile, S, itb.PLANAR)
            dst += n * per * tile
        return out.view(sum(counts), 3, S, S), counts
