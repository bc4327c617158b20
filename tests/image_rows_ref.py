"""The Qwen2.5-VL image front end restated in numpy (a helper of tests/test_image_rows_*; it holds no tests): the library's smart_resize,
Pillow's 8-bit BICUBIC resize and the normalisation table of tests/image_ref.py, and the patch rows [S, 1176] of Qwen2VLImageProcessor with
the temporal axis.  Integer arithmetic, a table lookup and a permutation, so a kernel can equal it bit for bit.

The `fault` argument of rows_of / rows_expected plants one deviation of the layout or of the temporal rule each;
tests/test_image_rows_ref_cpu.py asserts that every one of them changes the output on the cases the GPU test uses."""
import math

import numpy as np

from tests import image_ref as IR
from tests.image_ref import to_bf16_bits  # noqa: F401  (reused by the GPU test)

PATCH, MERGE, FACTOR, ROW = 14, 2, 28, 1176
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # OPENAI_CLIP_MEAN / _STD, the processor's defaults
MIN_PIXELS, MAX_PIXELS = 56 * 56, 28 * 28 * 1280
FAULTS = ("row_major", "unit_hw_swapped", "tp_outside_channel", "odd_clip_zero_padded", "per_slot_resize_of_wrong_frame")


def smart_resize(h, w, min_pixels=MIN_PIXELS, max_pixels=MAX_PIXELS, factor=FACTOR):
    """The library's smart_resize -> (H, W); ValueError for aspect ratios over 200"""
    if max(h, w) / min(h, w) > 200:
        raise ValueError("absolute aspect ratio must be smaller than 200, got %s" % (max(h, w) / min(h, w),))
    hb, wb = round(h / factor) * factor, round(w / factor) * factor
    if hb * wb > max_pixels:
        beta = math.sqrt((h * w) / max_pixels)
        hb, wb = max(factor, math.floor(h / beta / factor) * factor), max(factor, math.floor(w / beta / factor) * factor)
    elif hb * wb < min_pixels:
        beta = math.sqrt(min_pixels / (h * w))
        hb, wb = math.ceil(h * beta / factor) * factor, math.ceil(w * beta / factor) * factor
    return hb, wb


def rows_of(resized, table, fault=None):
    """resized: the t_in uint8 [H, W, 3] frames of ONE item after the resize -> float32 [grid_t gh gw, 1176]:
    out[row][c 392 + tp 196 + r 14 + q] = table[c][frame min(2 t + tp, t_in - 1)][14 ph + r][14 pw + q][c],
    row = t gh gw + ((ph / 2)(gw / 2) + pw / 2) 4 + (ph % 2) 2 + pw % 2"""
    t_in = len(resized)
    H, W = resized[0].shape[:2]
    gh, gw, gt = H // PATCH, W // PATCH, (t_in + 1) // 2
    norm = [np.stack([table[c][f[:, :, c]] for c in range(3)], axis=-1) for f in resized]       # [H, W, 3] float32 per frame
    x = np.zeros((gt, 2, H, W, 3), dtype=np.float32)
    for t in range(gt):
        for tp in range(2):
            f = 2 * t + (1 - tp if fault == "per_slot_resize_of_wrong_frame" else tp)
            if f > t_in - 1 and fault == "odd_clip_zero_padded":
                continue
            x[t, tp] = norm[min(f, t_in - 1)]
    x = x.reshape(gt, 2, gh // 2, 2, PATCH, gw // 2, 2, PATCH, 3)        # t tp hb hm r wb wm q c
    order = {None: (0, 2, 5, 3, 6, 8, 1, 4, 7),                          # t hb wb hm wm c tp r q
             "row_major": (0, 2, 3, 5, 6, 8, 1, 4, 7), "unit_hw_swapped": (0, 2, 5, 6, 3, 8, 1, 4, 7),
             "tp_outside_channel": (0, 2, 5, 3, 6, 1, 8, 4, 7)}.get(fault, (0, 2, 5, 3, 6, 8, 1, 4, 7))
    return np.ascontiguousarray(x.transpose(order)).reshape(gt * gh * gw, ROW)


def rows_expected(frames, out_w, out_h, table, fault=None):
    """frames: the t_in uint8 [h, w, 3] frames of ONE item -> float32 [grid_t gh gw, 1176], the resize restated in numpy (image_ref.resize)"""
    return rows_of([IR.resize(f, out_w, out_h) for f in frames], table, fault)


def rows_by_the_formula(resized, table):
    """rows_of, element by element from the issue's formula (slow: for small cases, as a check of the permutation above)"""
    t_in = len(resized)
    H, W = resized[0].shape[:2]
    gh, gw, gt = H // PATCH, W // PATCH, (t_in + 1) // 2
    out = np.full((gt * gh * gw, ROW), np.nan, dtype=np.float32)
    for t in range(gt):
        for tp in range(2):
            f = resized[min(2 * t + tp, t_in - 1)]
            for ph in range(gh):
                for pw in range(gw):
                    row = t * gh * gw + ((ph // 2) * (gw // 2) + pw // 2) * 4 + (ph % 2) * 2 + (pw % 2)
                    for c in range(3):
                        for r in range(PATCH):
                            for q in range(PATCH):
                                out[row, c * 392 + tp * 196 + r * 14 + q] = table[c][f[14 * ph + r, 14 * pw + q, c]]
    return out


def pil_resize(img, out_w, out_h):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((out_w, out_h), Image.BICUBIC))


def preprocess(images, mean=MEAN, std=STD, min_pixels=MIN_PIXELS, max_pixels=MAX_PIXELS, resize=IR.resize):
    """What Qwen2VLImageProcessor gives for a list of uint8 [H, W, 3] arrays: (pixel_values float32 [S, 1176], image_grid_thw int64 [n, 3]).
    resize: image_ref.resize (numpy) or pil_resize (Pillow itself; the two are equal, tests/test_image_ref_cpu.py)"""
    table = IR.lut(mean, std)
    rows, grid = [], []
    for img in images:
        H, W = smart_resize(img.shape[0], img.shape[1], min_pixels, max_pixels)
        rows.append(rows_of([resize(img, W, H)], table))
        grid.append((1, H // PATCH, W // PATCH))
    return np.concatenate(rows), np.array(grid, dtype=np.int64)


def item_frames(in_w, in_h, t_in, n_items):
    """n_items lists of t_in frames of different content (image_ref.edge_frames)"""
    frames = IR.edge_frames(in_w, in_h, n_items * t_in)
    return [frames[i * t_in:(i + 1) * t_in] for i in range(n_items)]


GPU_CASES = [  # (name, in_w, in_h, out_w, out_h, t_in, n_items): the smallest shapes at which each part of the kernel can still go wrong
    ("copy_one_unit", 28, 28, 28, 28, 1, 1),             # no resize; one merge unit
    ("copy_tiles_4_4_2_pair", 140, 56, 140, 56, 2, 1),   # no resize; gw = 10: column tiles of 4, 4, 2 and 5 units per row (odd)
    ("reference_128_to_140", 128, 128, 140, 140, 1, 3),  # the reference's own case; upscale on both axes
    ("cut_windows", 20, 10, 56, 28, 1, 2),               # tap windows cut at every edge; gw = 4
    ("odd_clip_down", 37, 61, 28, 56, 3, 1),             # odd clip; downscale on both axes; a single partial tile
    ("many_rows_lds", 400, 300, 112, 84, 1, 1),          # scale 3.57: the many-row LDS plan; gw = 8 and gh = 6
    ("wide_up_down", 1000, 30, 1008, 28, 1, 1),          # one axis up and the other down; 72 patches of columns
    ("two_steps_items", 200, 90, 196, 84, 4, 2),         # two temporal steps per item and several items
]

LIBRARY_SIZES = [(128, 128), (200, 90), (37, 61), (640, 480), (28, 28), (1000, 30), (140, 140), (4000, 3000)]     # (w, h)
