"""The MiniCPM-o image front end restated in numpy (a helper of tests/test_image_*; it holds no tests): Pillow's ImagingResample for 8 bits
per channel with the BICUBIC filter, the processor's normalisation as a 256-entry table per channel, and the strip layout of
reshape_by_patch.  Everything here is integer arithmetic or a table lookup, so a kernel can equal it bit for bit.

The `fault` argument of coefficients / resize plants one deviation each; tests/test_image_ref_cpu.py asserts that every one of them differs
from Pillow on the inputs the GPU test uses."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
PATCH = 14
FAULTS = ("no_u8_between", "a_075", "sign_blind_round", "vertical_first", "unnormalised")
# "round_coef" (Python's round() in place of the signed truncation) is accepted too; it is no fault unless a coefficient is an exact tie


def cubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def coefficients(n_in, n_out, fault=None):
    """(bounds int32 [n_out, 2] = (xmin, xmax), K int32 [n_out, ksize]) of one axis; the sums run in Pillow's order, in float64"""
    a = -0.75 if fault == "a_075" else -0.5
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    K = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [cubic((x + xmin - center + 0.5) / fs, a) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx] = (xmin, xmax)
        for x in range(xmax):
            k = w[x] if fault == "unnormalised" else w[x] / ww
            v = k * (1 << PRECISION_BITS)
            if fault == "round_coef":
                K[xx, x] = int(round(v))
            elif fault == "sign_blind_round":
                K[xx, x] = int(v + 0.5)
            else:
                K[xx, x] = int(v + 0.5) if k >= 0 else int(v - 0.5)
    return bounds, K


def _raw_sums(img, bounds, K, axis):
    """sum_x pixel[xmin + x] K_x along `axis` (0: vertical, 1: horizontal) of img [H, W, C] (integers), int64, nothing shifted"""
    img = np.moveaxis(np.asarray(img).astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + img.shape[1:], dtype=np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        k = K[xx, :xmax].astype(np.int64).reshape((-1,) + (1,) * (img.ndim - 1))
        out[xx] = (img[xmin:xmin + xmax] * k).sum(axis=0)
    return np.moveaxis(out, 0, axis)


def resize_sums(img, out_w, out_h, fault=None):
    """([(axis, pre-clip values (2^21 + sum) >> 22 of that pass, int64)] for the passes that run, the uint8 result [out_h, out_w, C])
    of img uint8 [H, W, C]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    in_h, in_w = img.shape[:2]
    order = [(1, in_w, out_w), (0, in_h, out_h)]
    if fault == "vertical_first":
        order.reverse()
    passes, cur, frac = [], img, 0
    for axis, n_in, n_out in order:
        if n_in == n_out:
            continue
        b, K = coefficients(n_in, n_out, fault)
        raw = _raw_sums(cur, b, K, axis)
        frac += PRECISION_BITS
        pre = ((1 << (frac - 1)) + raw) >> frac
        passes.append((axis, pre))
        if fault == "no_u8_between":
            cur = raw                                          # a wider intermediate: neither rounded to 8 bits nor clipped
        else:
            cur, frac = np.clip(pre, 0, 255).astype(np.uint8), 0
    if frac:
        cur = np.clip(passes[-1][1], 0, 255).astype(np.uint8)
    return passes, cur


def resize(img, out_w, out_h, fault=None):
    """PIL.Image.fromarray(img).resize((out_w, out_h), BICUBIC) as a uint8 array [out_h, out_w, C]: horizontal pass first, a uint8 image
    between the passes, a pass left out where the size does not change"""
    return resize_sums(img, out_w, out_h, fault)[1]


def lut(mean, std):
    """float32 [3, 256] with the processor's own numpy expressions: astype(float32) / 255, then (x - mean) / std with mean and std cast to
    the image's dtype (transformers' normalize)"""
    v = np.arange(256, dtype=np.uint8).astype(np.float32) / 255
    mean = np.asarray(mean, dtype=np.float64).astype(np.float32)
    std = np.asarray(std, dtype=np.float64).astype(np.float32)
    return np.stack([(v - mean[c]) / std[c] for c in range(3)]).astype(np.float32)


def strip(norm):
    """float [H, W, 3] -> [3, 14, 14 L]: out[c][r][(ph gw + pw) 14 + q] = norm[14 ph + r][14 pw + q][c]"""
    H, W, _ = norm.shape
    gh, gw = H // PATCH, W // PATCH
    x = norm.reshape(gh, PATCH, gw, PATCH, 3)                   # ph r pw q c
    return np.ascontiguousarray(x.transpose(4, 1, 0, 2, 3)).reshape(3, PATCH, gh * gw * PATCH)


def ensure_divide(length, patch=PATCH):
    return max(round(length / patch) * patch, patch)


def best_size(w, h, scale_resolution=448, patch=PATCH):
    """find_best_resize((w, h), scale_resolution, patch, allow_upscale=True)"""
    r = w / h
    height = int(scale_resolution / math.sqrt(r))
    width = int(height * r)
    return ensure_divide(width, patch), ensure_divide(height, patch)


def to_bf16_bits(x):
    """float32 array -> uint16 bf16 bits, one rounding to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def front_end(img, out_w, out_h, table):
    """uint8 [H, W, 3] -> float32 [3, 14, 14 L]: resize, table lookup, strip layout"""
    res = resize(img, out_w, out_h)
    norm = np.stack([table[c][res[:, :, c]] for c in range(3)], axis=-1)
    return strip(norm)


def preprocess(images, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), scale_resolution=448):
    """What MiniCPMVImageProcessor.preprocess gives for a list of uint8 [H, W, 3] arrays under max_slice_nums = 1 with no image sliced:
    ([float32 [3, 14, 14 L]], [(w, h)], int [n, 2] of (patch rows, patch columns))"""
    table = lut(mean, std)
    pv, sizes, tgt = [], [], []
    for img in images:
        h, w = img.shape[:2]
        ow, oh = best_size(w, h, scale_resolution)
        pv.append(front_end(img, ow, oh, table))
        sizes.append((w, h))
        tgt.append((oh // PATCH, ow // PATCH))
    return pv, sizes, np.array(tgt)


def edge_frames(w, h, n=3, seed=0):
    """n uint8 frames [h, w, 3] of different content: random bytes, with hard 0 | 255 steps along both axes (rows and columns of blocks
    that reach every border), so that the cubic's negative lobes drive a pass's sum below 0 and above 255"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    out = []
    for i in range(n):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        bw, bh = max(w // 3, 2), max(h // 3, 2)
        # two quadrant-like blocks of 0 and 255 that meet in vertical and horizontal steps, shifted per frame
        x0, y0 = (i * 3) % max(w - 2 * bw, 1), (i * 5) % max(h - 2 * bh, 1)
        img[y0:y0 + bh, x0:x0 + bw] = 0
        img[y0:y0 + bh, x0 + bw:x0 + 2 * bw] = 255
        img[y0 + bh:y0 + 2 * bh, x0:x0 + bw] = 255
        img[y0 + bh:y0 + 2 * bh, x0 + bw:x0 + 2 * bw] = 0
        out.append(img)
    return out


GPU_CASES = [  # (in_w, in_h, out_w, out_h)
    (97, 61, 42, 28), (20, 33, 56, 84), (97, 33, 42, 84), (42, 61, 42, 28), (97, 28, 42, 28), (42, 28, 42, 28), (231, 120, 28, 14),
    (61, 97, 70, 14),
]


def window_is_cut(n_in, n_out):
    """(some output's tap window is cut at the low border, some output's at the high border) of one axis"""
    scale = n_in / n_out
    support = 2.0 * max(scale, 1.0)
    centers = [(xx + 0.5) * scale for xx in range(n_out)]
    return any(int(c - support + 0.5) < 0 for c in centers), any(int(c + support + 0.5) > n_in for c in centers)


# ---------------------------------------------------------------------------------------------------------------- stand-in processor
class StubBatchFeature(dict):
    """The behaviour of the MiniCPM-o processor's batch-feature type that matters to a hand-off: with tensor_type "pt" every leaf of the
    nested lists that is not a tensor becomes one, and a leaf that already IS a tensor is replaced by None (the type's converter returns
    nothing for it)"""

    def __init__(self, data=None, tensor_type=None):
        import torch
        dict.__init__(self)

        def convert(v):
            if isinstance(v, list):
                return [convert(x) for x in v]
            return None if isinstance(v, torch.Tensor) else torch.as_tensor(v)
        for k, v in (data or {}).items():
            self[k] = convert(v) if tensor_type == "pt" else v

    @property
    def data(self):
        return self

    @data.setter
    def data(self, value):
        if value is not self:
            items = dict(value)
            self.clear()
            self.update(items)


class StubImageProcessor:
    """What a hand-off reads of MiniCPMVImageProcessor, with preprocess restated on image_ref (the source image only; a sliced image is
    counted in `sliced`): the fields, get_sliced_grid's None / not None, the nesting of the three result lists"""
    model_input_names = ["pixel_values"]

    def __init__(self, max_slice_nums=9, scale_resolution=448, patch_size=14, slice_mode=True, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        self.max_slice_nums, self.scale_resolution, self.patch_size, self.slice_mode = max_slice_nums, scale_resolution, patch_size, slice_mode
        self.mean, self.std = np.array(mean), np.array(std)
        self.version, self.image_feature_size, self.use_image_id = 2.6, 64, False
        self.calls = self.sliced = 0

    def get_sliced_grid(self, image_size, max_slice_nums, never_split=False):
        w, h = image_size
        multiple = min(math.ceil(w * h / (self.scale_resolution * self.scale_resolution)), max_slice_nums)
        return None if multiple <= 1 or never_split else [1, multiple]

    def get_slice_image_placeholder(self, image_size, image_idx=0, max_slice_nums=None, use_image_id=None):
        return "<image>%s</image>" % ("<unk>" * self.image_feature_size)

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
            p, s, t = preprocess(arrays, self.mean, self.std, self.scale_resolution) if arrays else ([], [], [])
            pv.append(p)
            sizes.append(s)
            tgt.append(t)
        return StubBatchFeature(data={"pixel_values": pv, "image_sizes": sizes, "tgt_sizes": tgt}, tensor_type=return_tensors)

    def __call__(self, images, **kwargs):
        self.calls += 1
        return self.preprocess(images, **kwargs)


class StubProcessor:
    """The image part of the MiniCPM-o processor's call: the image processor's call as the processor makes it"""

    def __init__(self, image_processor):
        self.image_processor = image_processor

    def image_inputs(self, images, max_slice_nums=1, return_tensors="pt"):
        return self.image_processor(images, do_pad=True, max_slice_nums=max_slice_nums, return_tensors=return_tensors)
