"""The tiled image front end's kernel (csrc/image_tiles.hip) on the GPU against tests/image_tiles_ref.py, the numpy restatement of
Pillow's `resize(size).crop(box)`, the normalisation tables and the two layouts (itself equal to Pillow byte for byte:
tests/test_image_tiles_ref_cpu.py).  Equality is exact, float32 bit for bit and bf16 as one rounding of that float32.

Every case runs two frames of different content (image_ref.edge_frames, whose 0 | 255 steps drive both passes' pre-clip sums out of range)
through one launch, from a buffer whose row pitch exceeds 3 w and is no multiple of 4, into a sentinel-filled buffer whose row, tile and
frame strides are all padded: everything outside the crops' elements and the guards on either side stay untouched, and a relaunch gives
the same bits.  Then the two front ends end to end: ImageFrontEnd.sliced and handoff.HipImage(slices=True) against the restated sliced
preprocess, InternVLImageFrontEnd.tiles against the restated load_image, and the conditioner's tile with and without --hip_image."""
import functools

import numpy as np
import pytest
import torch

from tests import image_ref as IR
from tests import image_tiles_ref as TR

pytestmark = pytest.mark.gpu

G = 256                                  # guard elements on either side of every buffer
SENTINEL = 777.0
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # three different channels
PAD_BYTE = 0xAB
N = 2


@functools.lru_cache(maxsize=None)
def _case(iw, ih, ow, oh, tw, th, layout):
    """(frames, the expected float32 crops per frame, the reference's passes per frame); computed once, never written to"""
    frames = IR.edge_frames(iw, ih, N)
    table = IR.lut(MEAN, STD)
    sums = [IR.resize_sums(f, ow, oh) for f in frames]       # (passes, the resized image): one resize per frame serves both
    layout_of = TR.planar_of if layout else TR.strip_of
    return frames, [[layout_of(c, table) for c in TR.crops_of(res, tw, th)] for _, res in sums], [p for p, _ in sums]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _expected_bits(x, dtype):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.float32:
        return torch.from_numpy(x.view(np.int32))
    return torch.from_numpy(IR.to_bf16_bits(x).view(np.int16))


def _differing(t, want, dtype):
    return int((_bits(t.cpu().contiguous()) != _expected_bits(want, dtype)).sum())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", TR.GPU_CASES, ids=[c[0] for c in TR.GPU_CASES])
def test_kernel_equals_the_reference_bit_for_bit(case, dtype):
    from x2i_amd import image as IM, image_binding as ib, image_tiles_binding as itb
    name, iw, ih, ow, oh, tw, th, layout = case
    frames, expected, passes = _case(iw, ih, ow, oh, tw, th, layout)
    gx, gy = ow // tw, oh // th
    # ---- coverage of the case, asserted on the reference before anything is launched
    ran = [axis for axis, _ in passes[0]]
    assert ran == [a for a, differs in ((1, iw != ow), (0, ih != oh)) if differs]
    for j, axis in enumerate(ran):
        lo, hi = min(int(p[j][1].min()) for p in passes), max(int(p[j][1].max()) for p in passes)
        print("%s: %dx%d -> %dx%d as %d x %d crops, pass along axis %d: pre-clip sums in [%d, %d], LDS plan %s"
              % (name, iw, ih, ow, oh, gx, gy, axis, lo, hi, ib.lds_plan(ih, oh)))
        assert lo < 0 and hi > 255
    assert any(not np.array_equal(frames[0], f) for f in frames[1:]) and len(expected[0]) == gx * gy
    # ---- buffers
    pitch = 3 * iw + 5
    pitch += pitch % 4 == 0
    assert pitch > 3 * iw and pitch % 4
    fpitch = ih * pitch + 7
    host = np.full(2 * G + N * fpitch, PAD_BYTE, dtype=np.uint8)
    for f, img in enumerate(frames):
        rows = host[G + f * fpitch:G + f * fpitch + ih * pitch].reshape(ih, pitch)
        rows[:, :3 * iw] = img.reshape(ih, 3 * iw)
    src_all = torch.from_numpy(host).cuda()
    src = src_all[G:G + N * fpitch]
    row_len, rows_per_tile, _ = itb.tile_extent(tw, th, layout, 0)
    rs = row_len + 42 if layout == 0 else row_len + 3         # padded rows (three patches' worth, or an odd three elements)
    ts = rows_per_tile * rs + 13                             # ... tiles
    fs = gx * gy * ts + 11                                   # ... and frames
    out_all = torch.full((2 * G + N * fs,), SENTINEL, dtype=dtype, device="cuda")
    out = out_all[G:G + N * fs]
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    hb, hc = (dev(a) for a in IM.axis_tables(iw, ow)) if iw != ow else (None, None)
    vb, vc = (dev(a) for a in IM.axis_tables(ih, oh)) if ih != oh else (None, None)
    lut = torch.from_numpy(IM.norm_lut(MEAN, STD)).cuda()
    launch = lambda: itb.tiles(src, iw, ih, pitch, fpitch, N, ow, oh, tw, th, hb, hc, vb, vc, lut, out, fs, ts, rs, layout)      # noqa: E731
    launch()
    first = _bits(out_all).cpu().clone()
    # ---- the values, and everything outside the crops' elements
    got = out.cpu()
    sent = _bits(torch.full((1,), SENTINEL, dtype=dtype))[0]
    mask = torch.zeros(N * fs, dtype=torch.bool)             # what the launch may write
    shape = (3, th, tw) if layout else (3, 14, row_len)
    for f in range(N):
        for t in range(gx * gy):
            at = f * fs + t * ts
            tile = got[at:at + rows_per_tile * rs].view(rows_per_tile, rs)[:, :row_len].reshape(shape)
            want = _expected_bits(expected[f][t], dtype)
            assert tuple(want.shape) == shape
            diff = int((_bits(tile.contiguous()) != want).sum())
            assert diff == 0, "frame %d crop %d: %d of %d elements differ from the reference" % (f, t, diff, want.numel())
            mask[at:at + rows_per_tile * rs].view(rows_per_tile, rs)[:, :row_len] = True
    assert bool((_bits(got)[~mask] == sent).all()), "an element outside the crops was written"
    whole = _bits(out_all).cpu()
    assert bool((whole[:G] == sent).all()) and bool((whole[-G:] == sent).all())
    assert bool((src_all.cpu() == torch.from_numpy(host)).all())
    # ---- a relaunch is bit-identical
    launch()
    assert torch.equal(_bits(out_all).cpu(), first)


def test_a_whole_image_as_one_crop_equals_the_unsliced_entry_point():
    """x2i_image_tiles with a 1 x 1 grid and the strip layout writes what x2i_image_frontend writes"""
    from x2i_amd import image as IM, image_binding as ib, image_tiles_binding as itb
    iw, ih, ow, oh = 97, 61, 70, 42
    frames = torch.from_numpy(np.stack(IR.edge_frames(iw, ih, N))).cuda().reshape(-1)
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    hb, hc = (dev(a) for a in IM.axis_tables(iw, ow))
    vb, vc = (dev(a) for a in IM.axis_tables(ih, oh))
    lut = torch.from_numpy(IM.norm_lut(MEAN, STD)).cuda()
    e = 3 * ow * oh
    a, b = torch.zeros(N * e, device="cuda"), torch.ones(N * e, device="cuda")
    ib.frontend(frames, iw, ih, 3 * iw, 3 * iw * ih, N, ow, oh, hb, hc, vb, vc, lut, a, e, oh // 14 * ow)
    itb.tiles(frames, iw, ih, 3 * iw, 3 * iw * ih, N, ow, oh, ow, oh, hb, hc, vb, vc, lut, b, e, e, oh // 14 * ow, itb.STRIP)
    assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _minicpm():
    arrays = TR.e2e_images(TR.E2E_MINICPM)
    return arrays, TR.minicpm_preprocess(arrays, 9)


def test_image_front_end_sliced_equals_the_restated_preprocess():
    from PIL import Image

    from x2i_amd.image import ImageFrontEnd
    arrays, (want, _, want_tgt) = _minicpm()
    fe = ImageFrontEnd(device="cuda")
    for given in (arrays, [Image.fromarray(a) for a in arrays]):
        values, tgt = fe.sliced(given, 9)
        assert [len(v) for v in values] == [3, 1, 3, 7] and np.vstack(tgt).tolist() == want_tgt.tolist()
        flat = [v for vs in values for v in vs]
        for v, w in zip(flat, want):
            assert v.device.type == "cuda" and v.dtype == torch.float32 and tuple(v.shape) == w.shape
            assert _differing(v, w, torch.float32) == 0
    half, _ = fe.sliced(arrays[:1], 9, out_dtype=torch.bfloat16)
    assert [_differing(v, w, torch.bfloat16) for v, w in zip(half[0], want[:3])] == [0, 0, 0]
    # max_slice_nums = 2 gives 640 x 480 the same grid; 1 slices nothing and is the existing call
    two, _ = fe.sliced(arrays[:1], 2)
    assert [_differing(v, w, torch.float32) for v, w in zip(two[0], want[:3])] == [0, 0, 0]
    one, tgt1 = fe(arrays[:2])
    assert len(one) == 2 and tgt1.tolist() == [[28, 37], [25, 40]] and _differing(one[0], want[0], torch.float32) == 0


def test_hip_image_with_slices_on_a_mixed_list_equals_the_restated_preprocess():
    from PIL import Image

    from x2i_amd import handoff
    arrays, (want, want_sizes, want_tgt) = _minicpm()
    images = [Image.fromarray(a) for a in arrays]
    ip = TR.SlicingStubImageProcessor()
    proc = IR.StubProcessor(ip)
    with handoff.HipImage(proc, device="cuda", slices=True) as hi:
        feat = proc.image_inputs([images[:2], images[2:]], max_slice_nums=9, return_tensors="pt")
        assert (hi.calls, hi.fallbacks, ip.calls) == (1, 0, 0) and type(feat) is IR.StubBatchFeature
        assert list(feat.keys()) == ["pixel_values", "image_sizes", "tgt_sizes"]
        pv = feat["pixel_values"]
        assert [len(g) for g in pv] == [4, 10]
        for v, w in zip(pv[0] + pv[1], want):
            assert v.device.type == "cuda" and v.dtype == torch.float32 and tuple(v.shape) == w.shape and _differing(v, w, torch.float32) == 0
        assert [tuple(t.tolist()) for g in feat["image_sizes"] for t in g] == want_sizes
        assert all(t.device.type == "cpu" for t in feat["tgt_sizes"]) and torch.cat(list(feat["tgt_sizes"])).tolist() == want_tgt.tolist()
    assert proc.image_processor is ip
    ref = proc.image_inputs([images[:2], images[2:]], max_slice_nums=9, return_tensors="pt")            # the original, after remove()
    assert ip.calls == 1 and all(torch.equal(a, b.cpu()) for a, b in zip(ref["pixel_values"][0] + ref["pixel_values"][1], pv[0] + pv[1]))
    assert all(torch.equal(a, b) for a, b in zip(ref["tgt_sizes"], feat["tgt_sizes"]))


def test_internvl_tiles_equal_the_restated_load_image():
    from PIL import Image

    from x2i_amd.internvl_image import InternVLImageFrontEnd
    arrays = TR.e2e_images(TR.E2E_INTERNVL) + TR.e2e_images(TR.E2E_INTERNVL[:1], seed=40)
    arrays = arrays[:3] + [arrays[4], arrays[3]]          # 97x61, 128x128, 97x61, 97x61, 640x480: a run of two equally sized images inside
    want = np.concatenate([TR.load_image(a) for a in arrays])
    fe = InternVLImageFrontEnd(device="cuda")
    pv, counts = fe.tiles([Image.fromarray(a) for a in arrays])
    assert counts == [7, 1, 7, 7, 13] and tuple(pv.shape) == (35, 3, 448, 448) and pv.dtype == torch.float32 and pv.device.type == "cuda"
    bad = [_differing(pv[k], want[k], torch.float32) for k in range(35)]
    assert bad == [0] * 35, bad
    half, _ = fe.tiles(arrays[:2], out_dtype=torch.bfloat16)
    assert tuple(half.shape) == (8, 3, 448, 448) and _differing(half, want[:8], torch.bfloat16) == 0
    # without the thumbnail, and with max_num = 1 (one tile: the thumbnail's own resize)
    bare, counts = fe.tiles(arrays[:2], use_thumbnail=False)
    assert counts == [6, 1] and _differing(bare, np.concatenate([want[:6], want[7:8]]), torch.float32) == 0
    single, counts = fe.tiles(arrays[:1], max_num=1)
    assert counts == [1] and _differing(single, want[6:7], torch.float32) == 0


def test_the_conditioners_tile_is_the_same_with_and_without_hip_image(tmp_path):
    from PIL import Image

    from x2i_amd.infer.inference_internvl import InternVLConditioner
    paths = []
    for i, (w, h) in enumerate(((640, 480), (97, 61))):
        paths.append(str(tmp_path / ("%d.png" % i)))
        Image.fromarray(IR.edge_frames(w, h, 1, seed=i)[0]).save(paths[-1])
    bare = torch.nn.Linear(2, 2)
    plain = InternVLConditioner(None, "cuda", prefill_only=False, model=bare, tokenizer=object())
    hip = InternVLConditioner(None, "cuda", prefill_only=False, model=bare, tokenizer=object(), hip_image=True)
    a, b = plain.image_tiles(paths), hip.image_tiles(paths)
    assert a.dtype == b.dtype == torch.bfloat16 and tuple(a.shape) == tuple(b.shape) == (2, 3, 448, 448) and b.device.type == "cuda"
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a[0], a[1])
