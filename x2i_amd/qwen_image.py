"""The Qwen2.5-VL image front end on the HIP path: what `Qwen2VLImageProcessor` computes on the host with its Pillow backend --
smart_resize, Pillow's BICUBIC resize, / 255, (x - mean) / std, the temporal duplicate and the flattening into patch rows [S, 1176] in
merge-unit order -- as one launch of libx2i_hip.so per run of equally sized images (include/frontend/rows/qwen/x2i_image_rows.h,
csrc/image_rows.hip).  The tower behind it is x2i_amd/qwen_vision.py, and the rows can be written straight into its padded bf16 workspace
(`out=tower.pixel_workspace(plan), row_stride=1216, out_dtype=bfloat16`, then `tower.forward_from_workspace(plan)`).

The arithmetic is that of x2i_amd/image.py (include/frontend/x2i_image.h), whose coefficient tables (`axis_tables`) and normalisation table
(`norm_lut`) are used as they are; the result equals the processor's float32 values bit for bit.

Host work of a call: the tables are made once per (in, out) pair and kept on the device.  A call copies the images into one pinned buffer,
starts one asynchronous transfer and one launch per run of adjacent, equally sized images (the rows of an image follow those of the image
before it, so only neighbours share a launch).  No device-to-host read; `image_grid_thw` is made on the host from the sizes.  The only wait is
for the previous call's transfers out of the same pinned buffer.

A clip (`clip`) is a list of equally sized frames: two frames per temporal step, the last frame of an odd clip repeated.  That is the
library's layout for a video; its video processor RESIZES with other arithmetic (torchvision), so a clip equals the library only for frames
that need no resize or were resized by Pillow.
"""
import math

import numpy as np
import torch

from . import image as im, image_binding as ib, image_rows_binding as irb
from .image import ImagePlan, StagedFrontEnd

PATCH, MERGE, TEMPORAL, ROW = irb.PATCH, 2, 2, irb.ROW
FACTOR = PATCH * MERGE
_BICUBIC = 3                                                     # PIL.Image.BICUBIC, PILImageResampling.BICUBIC


class QwenImageFrontEnd(StagedFrontEnd):
    """images -> (pixel_rows [S, 1176] on the device, image_grid_thw int64 [n, 3] on the host).  mean, std: three values each;
    min_pixels, max_pixels: the processor's size["shortest_edge"] and size["longest_edge"]."""

    def __init__(self, mean=(0.48145466, 0.4578275, 0.40821073), std=(0.26862954, 0.26130258, 0.27577711), min_pixels=56 * 56,
                 max_pixels=28 * 28 * 1280, device="cuda"):
        super().__init__(mean, std, device)
        if not 0 < int(min_pixels) <= int(max_pixels):
            raise ValueError("x2i_amd QwenImageFrontEnd: need 0 < min_pixels <= max_pixels (got %r, %r)" % (min_pixels, max_pixels))
        self.min_pixels, self.max_pixels = int(min_pixels), int(max_pixels)
        self.lut = torch.from_numpy(im.norm_lut(self.mean, self.std)).to(self.device)

    @classmethod
    def from_hf(cls, image_processor, device="cuda"):
        """The front end of a Qwen2VLImageProcessor (Pillow backend or the slow processor): its mean, std and pixel bounds.  ValueError,
        naming the field, for what the kernel does not serve."""
        ip = image_processor
        for name, want in (("patch_size", PATCH), ("merge_size", MERGE), ("temporal_patch_size", TEMPORAL)):
            if getattr(ip, name, want) != want:
                raise ValueError("x2i_amd QwenImageFrontEnd: %s = %r; the kernel is built for %s = %d" % (name, getattr(ip, name), name, want))
        if int(getattr(ip, "resample", _BICUBIC)) != _BICUBIC:
            raise ValueError("x2i_amd QwenImageFrontEnd: resample = %r; the kernel computes BICUBIC (3) only" % (ip.resample,))
        for name in ("do_resize", "do_rescale", "do_normalize"):
            if not getattr(ip, name, True):
                raise ValueError("x2i_amd QwenImageFrontEnd: %s is off; the kernel always resizes, rescales by 1 / 255 and normalises" % name)
        if getattr(ip, "rescale_factor", 1 / 255) != 1 / 255:
            raise ValueError("x2i_amd QwenImageFrontEnd: rescale_factor = %r; the table is made for 1 / 255" % (ip.rescale_factor,))
        size = getattr(ip, "size", None) or {}
        get = (lambda k: size.get(k)) if isinstance(size, dict) else (lambda k: getattr(size, k, None))     # noqa: E731
        lo, hi = get("shortest_edge"), get("longest_edge")
        lo = getattr(ip, "min_pixels", None) if lo is None else lo
        hi = getattr(ip, "max_pixels", None) if hi is None else hi
        if lo is None or hi is None:
            raise ValueError("x2i_amd QwenImageFrontEnd: size = %r holds no shortest_edge / longest_edge and the processor has no "
                             "min_pixels / max_pixels" % (size,))
        return cls(np.asarray(ip.image_mean, dtype=np.float64).reshape(-1), np.asarray(ip.image_std, dtype=np.float64).reshape(-1), lo, hi, device)

    def smart_resize(self, h, w):
        """The library's smart_resize(h, w, 28, min_pixels, max_pixels) -> (H, W), its ValueError for aspect ratios over 200 included"""
        if max(h, w) / min(h, w) > 200:
            raise ValueError("absolute aspect ratio must be smaller than 200, got %s" % (max(h, w) / min(h, w),))
        hb, wb = round(h / FACTOR) * FACTOR, round(w / FACTOR) * FACTOR
        if hb * wb > self.max_pixels:
            beta = math.sqrt((h * w) / self.max_pixels)
            hb, wb = max(FACTOR, math.floor(h / beta / FACTOR) * FACTOR), max(FACTOR, math.floor(w / beta / FACTOR) * FACTOR)
        elif hb * wb < self.min_pixels:
            beta = math.sqrt(self.min_pixels / (h * w))
            hb, wb = math.ceil(h * beta / FACTOR) * FACTOR, math.ceil(w * beta / FACTOR) * FACTOR
        return hb, wb

    def served(self, w, h):
        """None where images of w x h pixels are served, else the reason they are not (smart_resize's refusal or the kernel's own)"""
        try:
            oh, ow = self.smart_resize(h, w)
            irb.check_sizes(w, h, ow, oh)
        except (ValueError, ib.X2IError) as e:
            return str(e)
        return None

    # ------------------------------------------------------------------ call
    def _run(self, groups, out_dtype, plan, out, row_stride, resize):
        """groups: [(arrays of one size, n_items, t_in)] in the order of their rows -> (rows [S, 1176] view, [(grid_t, gh, gw)] per item)"""
        self._check_out_dtype(out_dtype)
        row_stride = int(row_stride)
        if row_stride < ROW:
            raise ValueError("x2i_amd QwenImageFrontEnd: row_stride = %d must be at least 1176" % row_stride)
        todo, grids, S = [], [], 0
        for arrays, n_items, t_in in groups:
            h, w = arrays[0].shape[:2]
            oh, ow = self.smart_resize(h, w) if resize else (h, w)
            grid_t, gh, gw = irb.check_sizes(w, h, ow, oh, n_items, t_in)
            todo.append((arrays, n_items, t_in, w, h, ow, oh, S, grid_t * gh * gw))
            grids += [(grid_t, gh, gw)] * n_items
            S += n_items * grid_t * gh * gw
        plan = self._plan_of_call(plan, sum(a.size for g in groups for a in g[0]))
        need = (S - 1) * row_stride + ROW
        if out is None:
            out = torch.empty(S * row_stride, dtype=out_dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != out_dtype or out.device.type != "cuda" or not out.is_contiguous()
              or out.device.index != (torch.cuda.current_device() if self.device.index is None else self.device.index) or out.numel() < need):
            raise ValueError("x2i_amd QwenImageFrontEnd: out must be a contiguous %s tensor on %s of at least %d elements (%d rows, row stride %d)"
                             % (out_dtype, self.device, need, S, row_stride))
        flat = out.view(-1)
        for _, _, _, w, h, ow, oh, _, _ in todo:                # every table is made, and its accumulator bound checked, before any launch
            self.tables(w, ow), self.tables(h, oh)
        for (_, n_items, t_in, w, h, ow, oh, row0, item_rows), dev in self._staged(plan, [(t, t[0]) for t in todo]):
            irb.rows(dev, w, h, 3 * w, 3 * w * h, n_items, t_in, ow, oh, *self.tables(w, ow), *self.tables(h, oh), self.lut,
                     flat[row0 * row_stride:], item_rows * row_stride, row_stride)
        return flat.as_strided((S, ROW), (row_stride, 1)), np.array(grids, dtype=np.int64).reshape(-1, 3)

    @torch.no_grad()
    def __call__(self, images, out_dtype=torch.float32, plan=None, out=None, row_stride=ROW):
        """images: PIL RGB images or uint8 [H, W, 3] arrays.  -> (pixel_rows [S, 1176] of out_dtype (float32 or bfloat16) on the device, rows
        row_stride elements apart, in the order of the images; image_grid_thw, a host int64 array [n, 3] of (1, gh, gw)).  out: a
        contiguous buffer of out_dtype on the device to write into (of at least (S - 1) * row_stride + 1176 elements; nothing but the
        rows' 1176 columns is written), else one is allocated."""
        arrays = self._as_arrays(images)
        runs = []
        for a in arrays:                                        # runs of adjacent images of one size
            if runs and runs[-1][0].shape == a.shape and len(runs[-1]) < irb.MAX_FRAMES:
                runs[-1].append(a)
            else:
                runs.append([a])
        return self._run([(g, len(g), 1) for g in runs], out_dtype, plan, out, row_stride, True)

    @torch.no_grad()
    def clip(self, frames, out_dtype=torch.float32, plan=None, out=None, row_stride=ROW, resize=True):
        """frames: one list of equally sized uint8 frames (PIL RGB images or [H, W, 3] arrays), T of them.  -> (rows [ceil(T / 2) gh gw, 1176],
        the host int64 array [[ceil(T / 2), gh, gw]]): temporal slot tp of step t holds frame min(2 t + tp, T - 1).  resize=False takes the
        frames at their own size (a multiple of 28 on both sides)."""
        arrays = self._as_arrays(frames)
        if any(a.shape != arrays[0].shape for a in arrays):
            raise ValueError("x2i_amd QwenImageFrontEnd: the frames of a clip must have one size (got %r)" % (sorted({a.shape[:2] for a in arrays}),))
        return self._run([(arrays, 1, len(arrays))], out_dtype, plan, out, row_stride, resize)


__all__ = ["QwenImageFrontEnd", "ImagePlan"]
