"""tests/image_tiles_ref.py and the host arithmetic of x2i_amd/image.py and x2i_amd/internvl_image.py against what they restate (no GPU):
the recorded results of the reference's own grid functions (tests/golden/image_grids.json, written by
tests/golden/make_image_grids_golden.py) on every entry; Pillow's `resize(size).crop(box)` byte for byte on every crop; F.unfold's strip
layout and torch's ToTensor / Normalize expressions; and the planted faults, each of which must differ from the Pillow composition on the
inputs tests/test_image_tiles_gpu.py uses."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from tests import image_ref as IR
from tests import image_tiles_ref as TR


# ---------------------------------------------------------------------------------------------------------------- the recorded grids
def test_the_fixture_covers_what_it_should():
    g = TR.golden()
    sizes = g["sizes"]
    assert 190 <= len(sizes) <= 260 and len(set(sizes)) == len(sizes)
    assert set(g["minicpm"]) == {2, 6, 9} and set(g["internvl"]) == {1, 6, 12}
    assert all(len(rows) == len(sizes) for rows in list(g["minicpm"].values()) + list(g["internvl"].values()))
    assert any(w == 9 * h for w, h in sizes) and any(h == 9 * w for w, h in sizes)                       # 9:1 and 1:9 strips
    assert any(448 * 448 < w * h <= 448 * 448 + 900 for w, h in sizes)                                   # areas just over 448^2
    # sizes on round's ties: a side that is an odd multiple of half the grid, so that ensure_divide rounds a half (to even)
    ties = [(wh, row[0]) for wh, row in zip(sizes, g["minicpm"][9]) if row[0] and ((2 * wh[0]) % row[0][0] == 0 and wh[0] % row[0][0]
                                                                                   or (2 * wh[1]) % row[0][1] == 0 and wh[1] % row[0][1])]
    assert len(ties) >= 5, ties
    grids = {row[0] for row in g["minicpm"][9]}
    assert None in grids and {(1, 9), (9, 1), (3, 3), (2, 1), (1, 2)} <= grids
    assert {(1, 1), (12, 1), (1, 12), (4, 3), (3, 2)} <= set(g["internvl"][12]) and set(g["internvl"][1]) == {(1, 1)}
    i = sizes.index((640, 480))
    assert g["minicpm"][9][i] == g["minicpm"][2][i] == ((2, 1), (518, 392), (728, 546)) and g["internvl"][12][i] == (4, 3)
    assert g["internvl"][12][sizes.index((1280, 720))] == (4, 2) and g["internvl"][12][sizes.index((97, 61))] == (3, 2)
    # the GPU test's named cases are the fixture's: 640 x 480 under max_slice_nums 9 and 2, 97 x 61 under max_num 12
    cases = {c[0]: c[1:] for c in TR.GPU_CASES}
    for m in (9, 2):
        (gx, gy), _, (rw, rh) = g["minicpm"][m][i]
        assert cases["minicpm-640x480-slices%d" % m] == (640, 480, rw, rh, rw // gx, rh // gy, 0)
    gx, gy = g["internvl"][12][sizes.index((97, 61))]
    assert cases["internvl-97x61"] == (97, 61, 448 * gx, 448 * gy, 448, 448, 1) and gx * gy + 1 == 7


def test_the_restated_grids_equal_the_fixture_on_every_entry():
    from x2i_amd import internvl_image as IV
    from x2i_amd.image import ImageFrontEnd
    g = TR.golden()
    fe = ImageFrontEnd(device="cpu")
    for m in (2, 6, 9):
        for (w, h), (grid, source, refine) in zip(g["sizes"], g["minicpm"][m]):
            assert TR.minicpm_sizes((w, h), m) == (grid, source, refine), (w, h, m)
            # "source_upscale" is no fault: a sliced image has more than 448^2 pixels and is rescaled whatever allow_upscale says
            assert TR.minicpm_sizes((w, h), m, fault="source_upscale") == (grid, source, refine), (w, h, m)
            src, fgrid, crop = fe.slice_plan(w, h, m)
            assert (fgrid, src) == (grid, source), (w, h, m)
            assert (crop is None) == (refine is None) and (crop is None or (crop[0] * grid[0], crop[1] * grid[1]) == refine), (w, h, m)
    assert [TR.target_ratios(1, m) for m in (1, 6, 12)] == [IV.target_ratios(1, m) for m in (1, 6, 12)]
    for m in (1, 6, 12):
        for (w, h), want in zip(g["sizes"], g["internvl"][m]):
            assert TR.closest_ratio(w, h, m) == want == IV.closest_ratio(w, h, m), (w, h, m)


def test_the_tie_rule_of_the_aspect_ratio_is_exercised_and_depends_on_the_order():
    """Some recorded size has several candidates at the same distance; taking the first or the last of them instead gives another grid
    somewhere in the fixture"""
    g = TR.golden()
    ratios = TR.target_ratios(1, 12)
    tied = first_differs = last_differs = 0
    for (w, h), want in zip(g["sizes"], g["internvl"][12]):
        diffs = [abs(w / h - r[0] / r[1]) for r in ratios]
        near = [r for r, d in zip(ratios, diffs) if d == min(diffs)]
        tied += len(near) > 1
        first_differs += near[0] != want
        last_differs += near[-1] != want
    assert tied >= 5 and first_differs >= 1 and last_differs >= 1


# ---------------------------------------------------------------------------------------------------------------- Pillow, byte for byte
def _pillow_crops(img, ow, oh, tw, th, order="row"):
    res = Image.fromarray(img).resize((ow, oh), resample=Image.Resampling.BICUBIC)
    gx, gy = ow // tw, oh // th
    cells = [(i, j) for i in range(gy) for j in range(gx)] if order == "row" else [(i, j) for j in range(gx) for i in range(gy)]
    return [np.asarray(res.crop((j * tw, i * th, (j + 1) * tw, (i + 1) * th))) for i, j in cells]


KERNEL_SHAPES = sorted({c[1:7] for c in TR.GPU_CASES})          # (in_w, in_h, out_w, out_h, tile_w, tile_h): ten size pairs


@functools.lru_cache(maxsize=None)
def _frame(iw, ih):
    return IR.edge_frames(iw, ih, 2)[1]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d-%dx%d-%dx%d" % s for s in KERNEL_SHAPES])
def test_crops_equal_pillows_resize_and_crop_byte_for_byte(shape):
    iw, ih, ow, oh, tw, th = shape
    img = _frame(iw, ih)
    got, want = TR.grid_crops(img, ow, oh, tw, th), _pillow_crops(img, ow, oh, tw, th)
    assert len(got) == len(want) == (ow // tw) * (oh // th)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (th, tw, 3) and np.array_equal(a, b), "crop %d differs from Pillow" % k
    if len(got) > 1:
        assert any(not np.array_equal(a, b) for a, b in zip(TR.grid_crops(img, ow, oh, tw, th, "crop_own_box"), want))
        assert any(not np.array_equal(got[0], c) for c in got[1:])
    if ow // tw > 1 and oh // th > 1:
        assert any(not np.array_equal(a, b) for a, b in zip(TR.grid_crops(img, ow, oh, tw, th, "column_major"), want))
        assert all(np.array_equal(a, b) for a, b in zip(TR.grid_crops(img, ow, oh, tw, th, "column_major"), _pillow_crops(img, ow, oh, tw, th, "column")))


def test_default_filter_of_resize_is_bicubic_for_rgb_and_a_448_tile_resizes_to_itself():
    img = Image.fromarray(_frame(97, 61))
    assert np.array_equal(np.asarray(img.resize((1344, 896))), np.asarray(img.resize((1344, 896), resample=Image.Resampling.BICUBIC)))
    tile = img.resize((448, 448))
    assert np.array_equal(np.asarray(tile.resize((448, 448), resample=Image.Resampling.BICUBIC)), np.asarray(tile))


def test_both_layouts_equal_unfold_and_totensor_normalize():
    from x2i_amd import internvl_image as IV
    u8 = TR.grid_crops(_frame(100, 75), 140, 126, 70, 42)[3]
    # strip: the processor's numpy normalisation, channel first, then reshape_by_patch's unfold
    table = IR.lut((0.5, 0.4, 0.3), (0.5, 0.25, 0.2))
    x = u8.astype(np.float32) / 255
    x = (x - np.array((0.5, 0.4, 0.3)).astype(np.float32)) / np.array((0.5, 0.25, 0.2)).astype(np.float32)
    image = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))
    patches = torch.nn.functional.unfold(image, (14, 14), stride=(14, 14)).reshape(3, 14, 14, -1)
    want = patches.permute(0, 1, 3, 2).reshape(3, 14, -1).numpy()
    got = TR.strip_of(u8, table)
    assert got.shape == (3, 14, 14 * 15) and np.array_equal(got.view(np.int32), want.view(np.int32))
    # planar: ToTensor (HWC uint8 -> CHW float / 255) and Normalize (sub mean, div std) in torch's float32
    t = torch.from_numpy(u8).permute(2, 0, 1).float().div(255)
    mean, std = torch.tensor(TR.IMAGENET_MEAN)[:, None, None], torch.tensor(TR.IMAGENET_STD)[:, None, None]
    want = t.sub(mean).div(std).numpy()
    got = TR.planar_of(u8, TR.torch_lut())
    assert got.shape == (3, 42, 70) and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(IV.tensor_lut(TR.IMAGENET_MEAN, TR.IMAGENET_STD).numpy().view(np.int32), TR.torch_lut().view(np.int32))
    # every one of the 768 entries, against the expressions on a whole image of that value
    for v in range(256):
        t = torch.full((3, 1, 1), v, dtype=torch.uint8).float().div(255)
        assert np.array_equal(t.sub(mean).div(std).numpy().reshape(3).view(np.int32), TR.torch_lut()[:, v].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- the two host pipelines
def _pillow_minicpm(img, max_slice_nums):
    """get_sliced_images composed from Pillow calls and the recorded sizes' arithmetic: [source, crops row by row]"""
    h, w = img.shape[:2]
    grid, source, refine = TR.minicpm_sizes((w, h), max_slice_nums)
    pil = Image.fromarray(img)
    out = [np.asarray(pil.resize(source, resample=Image.Resampling.BICUBIC))]
    if grid is not None:
        out += _pillow_crops(img, refine[0], refine[1], refine[0] // grid[0], refine[1] // grid[1])
    return out


def _pillow_internvl(img, max_num=12):
    h, w = img.shape[:2]
    gx, gy = TR.closest_ratio(w, h, max_num)
    pil = Image.fromarray(img)
    res = pil.resize((448 * gx, 448 * gy))
    out = [np.asarray(res.crop(((i % gx) * 448, (i // gx) * 448, (i % gx + 1) * 448, (i // gx + 1) * 448))) for i in range(gx * gy)]
    if len(out) != 1:
        out.append(np.asarray(pil.resize((448, 448))))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _e2e():
    return TR.e2e_images(TR.E2E_MINICPM), TR.e2e_images(TR.E2E_INTERNVL)


def test_the_restated_pipelines_equal_the_pillow_compositions_on_the_gpu_tests_inputs():
    mc, iv = _e2e()
    assert [len(TR.minicpm_slices(a, 9)) for a in mc] == [3, 1, 3, 7] and [len(TR.internvl_tiles(a)) for a in iv] == [7, 1, 7, 13]
    for k, a in enumerate(mc):
        for m in (9, 2, 1) if k == 0 else (9,):
            assert _same(TR.minicpm_slices(a, m), _pillow_minicpm(a, m))
    for a in iv:
        assert _same(TR.internvl_tiles(a), _pillow_internvl(a))
    pv, sizes, tgt = TR.minicpm_preprocess(mc, 9)
    assert len(pv) == 14 and sizes == TR.E2E_MINICPM and tgt.shape == (14, 2)
    assert tgt[:4].tolist() == [[28, 37], [39, 26], [39, 26], [25, 40]] and all(p.shape == (3, 14, 14 * r * c) for p, (r, c) in zip(pv, tgt))
    lv = TR.load_image(iv[0])
    assert lv.shape == (7, 3, 448, 448) and lv.dtype == np.float32
    # under max_slice_nums = 1 the sliced restatement is image_ref's preprocess
    one, want = TR.minicpm_preprocess(mc, 1), IR.preprocess(mc)
    assert all(np.array_equal(a, b) for a, b in zip(one[0], want[0])) and np.array_equal(one[2], want[2])


@pytest.mark.parametrize("fault", TR.FAULTS)
def test_planted_faults_differ_from_pillow_on_the_gpu_tests_inputs(fault):
    mc, iv = _e2e()
    if fault in ("crop_own_box", "column_major"):
        hit_mc = [not _same(TR.minicpm_slices(a, 9, fault=fault), _pillow_minicpm(a, 9)) for a in mc]
        hit_iv = [not _same(TR.internvl_tiles(a, fault=fault), _pillow_internvl(a)) for a in iv]
        # every multi-crop image for the box; every image with more than one row AND column of crops for the order
        assert hit_mc == ([True, False, True, True] if fault == "crop_own_box" else [False, False, False, True])
        assert hit_iv == [True, False, True, True]
    elif fault in ("refine_no_upscale", "source_last"):
        hit = [not _same(TR.minicpm_slices(a, 9, fault=fault), _pillow_minicpm(a, 9)) for a in mc]
        assert hit == [True, False, True, True]          # (every cell here has fewer than 448^2 pixels and is enlarged)
    else:
        hit = [not _same(TR.internvl_tiles(a, fault=fault), _pillow_internvl(a)) for a in iv]
        assert hit == ([False, True, False, False] if fault == "thumbnail_single" else [True, False, True, True])
