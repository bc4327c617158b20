"""The MiniCPM-o image front end on the HIP path: what `MiniCPMVImageProcessor.preprocess` computes on the host for an image that is
not sliced (max_slice_nums = 1, a video's frames) -- Pillow's BICUBIC resize to the processor's best size, / 255, (x - mean) / std, the strip
layout [3, 14, 14 L] -- as one launch of libx2i_hip.so per group of equally sized frames (include/frontend/x2i_image.h, csrc/image.hip).
The tower behind it is x2i_amd/siglip.py.

An image that the processor slices (more than scale_resolution^2 pixels under max_slice_nums > 1) goes through `sliced`: the source image
by the same launch, and the crops of the refine-size image by one launch of include/frontend/tiles/x2i_image_tiles.h (csrc/image_tiles.hip)
per group, in the processor's order [source, crops row by row].

The arithmetic (Pillow's integer resample with its 22-bit coefficients and the uint8 image between the two passes, a 256-entry table per
channel for the normalisation) stands in the header; the result equals the processor's float32 values bit for bit.

Host work of a call: the coefficient tables are made once per (in, out) pair, in float64, and kept on the device; the normalisation table is
made once (from_hf).  A call copies each group of equally sized frames into one pinned buffer, starts one asynchronous transfer and one
launch per group.  No device-to-host read.  The only wait is for the previous call's transfers out of the same pinned buffer, before it is
overwritten.
"""
import math

import numpy as np
import torch

from . import image_binding as ib, image_tiles_binding as itb

PATCH = ib.PATCH


def cubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def axis_tables(n_in, n_out):
    """(bound int32 [n_out, 2], coef int32 [n_out, ksize]) of include/frontend/x2i_image.h for one axis, in float64 with the sums in
    Pillow's order.  ValueError where sum |K| 255 + 2^21 would not fit the int32 accumulator."""
    k = ib.ksize(n_in, n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    bound = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, k), dtype=np.int32)
    one = float(1 << ib.PRECISION_BITS)
    for xx in range(n_out):
        xmin, xmax = ib.window(n_in, n_out, xx)
        center = (xx + 0.5) * scale
        w = [cubic((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        bound[xx] = (xmin, xmax)
        for x in range(xmax):
            kx = w[x] / ww
            coef[xx, x] = int(kx * one + 0.5) if kx >= 0 else int(kx * one - 0.5)
    worst = int(np.abs(coef.astype(np.int64)).sum(axis=1).max())
    if worst * 255 + (1 << (ib.PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError("x2i_amd ImageFrontEnd: the coefficients of %d -> %d sum to %d in absolute value; the int32 accumulator holds "
                         "sums below %d" % (n_in, n_out, worst, ((1 << 31) - (1 << (ib.PRECISION_BITS - 1))) // 255))
    return bound, coef


def norm_lut(mean, std):
    """float32 [3, 256]: the processor's own numpy expressions, astype(float32) / 255 and then (x - mean) / std with mean and std cast to
    float32 (transformers' normalize casts them to the image's dtype)"""
    v = np.arange(256, dtype=np.uint8).astype(np.float32) / 255
    return np.stack([(v - np.float32(mean[c])) / np.float32(std[c]) for c in range(3)]).astype(np.float32)


class ImagePlan:
    """The buffers of calls on at most `nbytes` bytes of frames (ImageFrontEnd.plan)"""


class StagedFrontEnd:
    """What the three image front ends (ImageFrontEnd, qwen_image.QwenImageFrontEnd, internvl_image.InternVLImageFrontEnd) share: the
    device, the check of mean and std, the coefficient tables, the staging plan and the staging sequence of a call.  A front end adds its
    normalisation table `lut`, its size rules, its grouping rule and its launches.  Refusals name the class that raised them."""

    _noun = "frames"                                            # what the "plan holds" refusal calls the input of a call

    def __init__(self, mean, std, device):
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3 or not all(std):
            raise ValueError("x2i_amd %s: mean and std must hold three values, std none of them zero (got %r, %r)" % (type(self).__name__, mean, std))
        self.mean, self.std, self.device = mean, std, torch.device(device)
        self._tables = {}
        self._plan = None

    def tables(self, n_in, n_out):
        """(bound, coef) of one axis on the device, made once per (n_in, n_out); (None, None) where the axis does not resize"""
        if n_in == n_out:
            return None, None
        t = self._tables.get((n_in, n_out))
        if t is None:
            t = self._tables[(n_in, n_out)] = tuple(torch.from_numpy(a).to(self.device) for a in axis_tables(n_in, n_out))
        return t

    def plan(self, nbytes):
        """The pinned staging buffer and the device frame buffer of calls on at most nbytes bytes of frames"""
        nbytes = int(nbytes)
        if nbytes < 1:
            raise ValueError("x2i_amd %s: a plan needs at least one byte of frames (got %d)" % (type(self).__name__, nbytes))
        p = ImagePlan()
        cuda = self.device.type == "cuda"
        p.nbytes, p.device = nbytes, self.device
        p.stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=cuda)
        p.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        p.sent = torch.cuda.Event() if cuda else None
        p.busy = False
        return p

    @staticmethod
    def _as_arrays(frames):
        """A list of uint8 [H, W, 3] arrays of PIL RGB images, arrays, or one [n, H, W, 3] array.  (A static function, whose refusals name
        ImageFrontEnd for all three front ends.)"""
        if isinstance(frames, np.ndarray) and frames.ndim == 4:
            frames = list(frames)
        out = []
        for f in frames:
            if not isinstance(f, np.ndarray):
                if getattr(f, "mode", None) != "RGB":
                    raise ValueError("x2i_amd ImageFrontEnd: a frame must be a PIL image of mode RGB or a uint8 [H, W, 3] array (got %r)"
                                     % (getattr(f, "mode", type(f).__name__),))
                f = np.asarray(f)
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or not f.shape[0] or not f.shape[1]:
                raise ValueError("x2i_amd ImageFrontEnd: a frame must be a uint8 [H, W, 3] array (got %s %s)" % (f.dtype, f.shape))
            out.append(f)
        if not out:
            raise ValueError("x2i_amd ImageFrontEnd: frames must be a non-empty list")
        return out

    def _check_out_dtype(self, out_dtype):
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("x2i_amd %s: out_dtype must be float32 or bfloat16 (got %r)" % (type(self).__name__, out_dtype))

    def _plan_of_call(self, plan, nbytes):
        """The plan a call on nbytes bytes runs with: the caller's, else the kept one, made anew where it is too small or on another device.
        ValueError for a plan that does not hold the call, X2IError on a device that is not a GPU."""
        if plan is None:
            plan = self._plan
            if plan is None or plan.nbytes < nbytes or plan.device != self.device:
                plan = self._plan = self.plan(nbytes)
        if plan.nbytes < nbytes or plan.device != self.device:
            raise ValueError("x2i_amd %s: the plan holds %d bytes on %s; the call holds %d bytes of %s on %s"
                             % (type(self).__name__, plan.nbytes, plan.device, nbytes, self._noun, self.device))
        if self.device.type != "cuda":
            raise ib.X2IError("x2i_amd: %s runs on the GPU only (the module is on %s); there is no CPU fallback" % (type(self).__name__, self.device))
        return plan

    def _staged(self, plan, groups):
        """groups: [(the front end's own record of a group, its equally sized arrays)].  A generator over the groups: each is copied into
        the pinned buffer behind the groups before it, its asynchronous transfer is started and (the record, the frames on the device) is
        yielded for the caller to launch on; behind the last group the event of the call is recorded.  Run it to its end, as a for loop
        over it alone does."""
        if plan.busy:
            plan.sent.synchronize()                            # the previous call's transfers out of the staging buffer (long done, as a rule)
        stage, src = plan.stage.numpy(), 0
        for record, arrays in groups:
            (h, w), n = arrays[0].shape[:2], len(arrays)
            end = src + n * 3 * w * h
            pinned = stage[src:end].reshape(n, h, w, 3)
            for j, a in enumerate(arrays):
                pinned[j] = a
            dev = plan.dev[src:end]
            dev.copy_(plan.stage[src:end], non_blocking=True)
            yield record, dev
            src = end
        plan.sent.record()
        plan.busy = True


class ImageFrontEnd(StagedFrontEnd):
    """frames -> ([float32 [3, 14, 14 L] on the device], tgt_sizes).  mean, std: three values each; scale_resolution: the processor's."""

    def __init__(self, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), scale_resolution=448, device="cuda"):
        super().__init__(mean, std, device)
        if int(scale_resolution) < PATCH:
            raise ValueError("x2i_amd ImageFrontEnd: scale_resolution = %r must be at least the patch size 14" % (scale_resolution,))
        self.scale_resolution = int(scale_resolution)
        self.lut = torch.from_numpy(norm_lut(self.mean, self.std)).to(self.device)

    @classmethod
    def from_hf(cls, image_processor, device="cuda"):
        """The front end of a MiniCPMVImageProcessor: its scale_resolution, mean and std.  ValueError, naming the field, for what the kernel
        does not serve."""
        ip = image_processor
        if ip.patch_size != PATCH:
            raise ValueError("x2i_amd ImageFrontEnd: patch_size = %r; the kernel is built for patch_size = 14" % (ip.patch_size,))
        if not getattr(ip, "slice_mode", True):
            raise ValueError("x2i_amd ImageFrontEnd: slice_mode is off; without it the processor does not resize and the front end does not apply")
        return cls(np.asarray(ip.mean).reshape(-1), np.asarray(ip.std).reshape(-1), ip.scale_resolution, device)

    def best_size(self, w, h):
        """The processor's find_best_resize((w, h), scale_resolution, 14, allow_upscale=True)"""
        r = w / h
        height = int(self.scale_resolution / math.sqrt(r))
        width = int(height * r)
        fit = lambda v: max(round(v / PATCH) * PATCH, PATCH)   # noqa: E731
        return fit(width), fit(height)

    def sliced_grid(self, w, h, max_slice_nums):
        """The processor's get_sliced_grid((w, h), max_slice_nums): (gx, gy), or None for an image that is not sliced"""
        sr = self.scale_resolution
        multiple = min(math.ceil(w * h / (sr * sr)), int(max_slice_nums))
        if multiple <= 1:
            return None
        best, err = (1, 1), float("inf")
        for n in (multiple - 1, multiple, multiple + 1):
            if n == 1 or n > max_slice_nums:
                continue
            for m in range(1, n + 1):                          # the first of equally near grids stays, as in the processor
                if n % m == 0:
                    e = abs(math.log(w / h) - math.log(m / (n // m)))
                    if e < err:
                        best, err = (m, n // m), e
        return best

    def refine_size(self, w, h, grid):
        """The processor's get_refine_size((w, h), grid, allow_upscale=True): the grid's cell -- a float size, sides rounded to the grid
        with Python's round (ties to even) -- fitted like an image of its own, times the grid"""
        gx, gy = grid
        fit = lambda v, g: max(round(v / g) * g, g)   # noqa: E731
        cw, ch = self.best_size(fit(w, gx) / gx, fit(h, gy) / gy)
        return cw * gx, ch * gy

    def slice_plan(self, w, h, max_slice_nums=1):
        """(source size, grid or None, crop size or None) of a w x h image.  The source image of a sliced image is
        find_best_resize(allow_upscale=False); an image is sliced only where w h > scale_resolution^2, where that is best_size."""
        grid = self.sliced_grid(w, h, max_slice_nums)
        if grid is None:
            return self.best_size(w, h), None, None
        rw, rh = self.refine_size(w, h, grid)
        return self.best_size(w, h), grid, (rw // grid[0], rh // grid[1])

    def served(self, w, h, max_slice_nums=1):
        """None where frames of w x h pixels are served, else the reason they are not (the kernel's own refusal)"""
        try:
            (ow, oh), grid, crop = self.slice_plan(w, h, max_slice_nums)
            ib.check_sizes(w, h, ow, oh)
            if grid is not None:
                itb.check_sizes(w, h, crop[0] * grid[0], crop[1] * grid[1], crop[0], crop[1])
        except ib.X2IError as e:
            return str(e)
        return None

    # ------------------------------------------------------------------ call
    @torch.no_grad()
    def __call__(self, frames, out_dtype=torch.float32, plan=None):
        """frames: PIL RGB images, uint8 [H, W, 3] arrays, or one uint8 [n, H, W, 3] array.  -> (a list of [3, 14, 14 L] tensors of
        out_dtype (float32 or bfloat16) on the device, views of one buffer, in the order of the frames; tgt_sizes, a host int array [n, 2]
        of (patch rows, patch columns)).  No frame is sliced (max_slice_nums = 1)."""
        values, tgt = self.sliced(frames, 1, out_dtype, plan)
        return [v[0] for v in values], np.vstack(tgt)

    @torch.no_grad()
    def sliced(self, frames, max_slice_nums=9, out_dtype=torch.float32, plan=None):
        """The processor's get_sliced_images per frame.  -> (per frame the list [source image, crops row by row] of [3, 14, 14 L] tensors
        of out_dtype on the device, views of one buffer -- the source image alone for a frame that is not sliced; per frame a host int
        array [slices, 2] of (patch rows, patch columns)).  A group of equally sized frames costs one launch for the source images and,
        where they are sliced, one for the crops."""
        arrays = self._as_arrays(frames)
        self._check_out_dtype(out_dtype)
        if int(max_slice_nums) < 1:
            raise ValueError("x2i_amd ImageFrontEnd: max_slice_nums = %r must be at least 1" % (max_slice_nums,))
        groups = {}                                             # (w, h) -> frame indices, in the order of first appearance
        for i, a in enumerate(arrays):
            groups.setdefault((a.shape[1], a.shape[0]), []).append(i)
        plans = {wh: self.slice_plan(wh[0], wh[1], int(max_slice_nums)) for wh in groups}
        for (w, h), ((ow, oh), grid, crop) in plans.items():
            ib.check_sizes(w, h, ow, oh)
            if grid is not None:
                itb.check_sizes(w, h, crop[0] * grid[0], crop[1] * grid[1], crop[0], crop[1])
        plan = self._plan_of_call(plan, sum(a.size for a in arrays))
        elems = {}                                              # (w, h) -> elements of a frame's source image, of one crop, crops per frame
        for wh, ((ow, oh), grid, crop) in plans.items():
            elems[wh] = (3 * ow * oh, 0, 0) if grid is None else (3 * ow * oh, 3 * crop[0] * crop[1], grid[0] * grid[1])
            for n_in, n_out in ((wh[0], ow), (wh[1], oh)) + (() if grid is None else ((wh[0], crop[0] * grid[0]), (wh[1], crop[1] * grid[1]))):
                self.tables(n_in, n_out)                        # every table is made, and its accumulator bound checked, before any launch
        out = torch.empty(sum((e + c * k) * len(groups[wh]) for wh, (e, c, k) in elems.items()), dtype=out_dtype, device=self.device)
        views, tgt, dst = [None] * len(arrays), [None] * len(arrays), 0
        for ((w, h), idx), dev in self._staged(plan, [(item, [arrays[i] for i in item[1]]) for item in groups.items()]):
            ((ow, oh), grid, crop), n, fb = plans[(w, h)], len(idx), 3 * w * h
            e, c, k = elems[(w, h)]
            L14 = oh // PATCH * ow
            ib.frontend(dev, w, h, 3 * w, fb, n, ow, oh, *self.tables(w, ow), *self.tables(h, oh), self.lut, out[dst:dst + n * e], e, L14)
            for j, i in enumerate(idx):
                views[i] = [out[dst + j * e:dst + (j + 1) * e].view(3, PATCH, L14)]
                tgt[i] = [(oh // PATCH, ow // PATCH)]
            dst += n * e
            if grid is not None:
                (cw, ch), (gx, gy) = crop, grid
                C14 = ch // PATCH * cw
                itb.tiles(dev, w, h, 3 * w, fb, n, cw * gx, ch * gy, cw, ch, *self.tables(w, cw * gx), *self.tables(h, ch * gy), self.lut,
                          out[dst:dst + n * k * c], k * c, c, C14, itb.STRIP)
                for j, i in enumerate(idx):
                    views[i] += [out[dst + (j * k + t) * c:dst + (j * k + t + 1) * c].view(3, PATCH, C14) for t in range(k)]
                    tgt[i] += [(ch // PATCH, cw // PATCH)] * k
                dst += n * k * c
        return views, [np.array(t) for t in tgt]
