"""The Qwen2.5-VL image front end's kernel (csrc/image_rows.hip) on the GPU against tests/image_rows_ref.py, the numpy restatement of
Qwen2VLImageProcessor's Pillow backend (itself equal to the library bit for bit: tests/test_image_rows_ref_cpu.py).  Equality is exact,
float32 bit for bit and bf16 as one rounding of that float32.

Every case runs with the tight row stride 1176, and with rows 1216 apart and a padded item stride in a buffer pre-filled with a sentinel bit
pattern: every element outside the formula keeps it, the guards on either side included.  Then the front end, the hand-off and the in-place
route into the vision tower's padded workspace end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import image_ref as IR
from tests import image_rows_ref as RR

pytestmark = pytest.mark.gpu

G = 256                                  # guard elements on either side of every buffer
SENTINEL = 777.0
ROW = 1176


@functools.lru_cache(maxsize=None)
def _case(name):
    """(the case, its items' frames, the expected float32 rows per item); computed once, never written to"""
    case = next(c for c in RR.GPU_CASES if c[0] == name)
    _, iw, ih, ow, oh, t_in, n_items = case
    items = RR.item_frames(iw, ih, t_in, n_items)
    table = IR.lut(RR.MEAN, RR.STD)
    return case, items, [RR.rows_expected(fr, ow, oh, table) for fr in items]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _expected_bits(x, dtype):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.float32:
        return torch.from_numpy(x.view(np.int32))
    return torch.from_numpy(RR.to_bf16_bits(x).view(np.int16))


def _differing(t, want, dtype):
    return int((_bits(t.cpu().contiguous()) != _expected_bits(want, dtype)).sum())


def _launcher(case, items, dtype, rs, item_pad):
    """(launch, the whole output buffer with its guards, the item stride) of one case: the frames in one flat device buffer"""
    from x2i_amd import image as IM, image_rows_binding as irb
    _, iw, ih, ow, oh, t_in, n_items = case
    src = torch.from_numpy(np.stack([f for fr in items for f in fr])).cuda().reshape(-1)
    rows = (t_in + 1) // 2 * (oh // 14) * (ow // 14)
    ois = rows * rs + item_pad
    out_all = torch.full((2 * G + n_items * ois,), SENTINEL, dtype=dtype, device="cuda")
    out = out_all[G:G + n_items * ois]
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    hb, hc = (dev(a) for a in IM.axis_tables(iw, ow)) if iw != ow else (None, None)
    vb, vc = (dev(a) for a in IM.axis_tables(ih, oh)) if ih != oh else (None, None)
    lut = torch.from_numpy(IM.norm_lut(RR.MEAN, RR.STD)).cuda()
    launch = lambda: irb.rows(src, iw, ih, 3 * iw, 3 * iw * ih, n_items, t_in, ow, oh, hb, hc, vb, vc, lut, out, ois, rs)      # noqa: E731
    return launch, out_all, ois, rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in RR.GPU_CASES])
def test_kernel_equals_the_reference_bit_for_bit(name, dtype):
    from x2i_amd import image_binding as ib
    case, items, expected = _case(name)
    _, iw, ih, ow, oh, t_in, n_items = case
    print("%s: %d item(s) of %d frame(s) %dx%d -> %dx%d, LDS plan %s" % (name, n_items, t_in, iw, ih, ow, oh, ib.lds_plan(ih, oh)))
    assert all(len(fr) == t_in for fr in items) and len(items) == n_items
    flat = [f for fr in items for f in fr]
    assert all(not np.array_equal(flat[0], f) for f in flat[1:])            # every frame has content of its own
    sent = _bits(torch.full((1,), SENTINEL, dtype=dtype))[0]
    for rs, item_pad in ((ROW, 0), (1216, 53)):
        launch, out_all, ois, rows = _launcher(case, items, dtype, rs, item_pad)
        assert expected[0].shape == (rows, ROW)
        launch()
        whole = _bits(out_all).cpu()
        got = whole[G:G + n_items * ois]
        mask = torch.zeros(n_items * ois, dtype=torch.bool)          # what the launch may write
        for i in range(n_items):
            view = got[i * ois:i * ois + rows * rs].view(rows, rs)[:, :ROW]
            want = _expected_bits(expected[i], dtype)
            diff = int((view != want).sum())
            assert diff == 0, "row stride %d, item %d: %d of %d elements differ from the reference" % (rs, i, diff, want.numel())
            mask[i * ois:i * ois + rows * rs].view(rows, rs)[:, :ROW] = True
        assert int(mask.sum()) == n_items * rows * ROW
        assert bool((got[~mask] == sent).all()), "an element outside the rows' 1176 columns was written (row stride %d)" % rs
        assert bool((whole[:G] == sent).all()) and bool((whole[-G:] == sent).all())


def test_a_relaunch_gives_the_same_bits():
    case, items, _ = _case("two_steps_items")
    launch, out_all, _, _ = _launcher(case, items, torch.float32, 1216, 53)
    launch()
    first = _bits(out_all).cpu().clone()
    launch()
    assert torch.equal(_bits(out_all).cpu(), first)


# ---------------------------------------------------------------------------------------------------------------- end to end
MIXED = ((128, 128), (128, 128), (200, 90), (128, 128))      # (w, h): a run of two, then two runs of one


@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(11)
    arrays = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for w, h in MIXED]
    return arrays, RR.preprocess(arrays)


def test_the_front_end_on_a_mixed_list_equals_the_restated_processor():
    from PIL import Image

    from x2i_amd.qwen_image import QwenImageFrontEnd
    arrays, (want, want_grid) = _mixed()
    fe = QwenImageFrontEnd(device="cuda")
    assert want_grid.tolist() == [[1, 10, 10], [1, 10, 10], [1, 6, 14], [1, 10, 10]]
    for given in (arrays, [Image.fromarray(a) for a in arrays]):
        rows, grid = fe(given)
        assert rows.device.type == "cuda" and rows.dtype == torch.float32 and tuple(rows.shape) == want.shape == (384, ROW)
        assert grid.dtype == np.int64 and grid.tolist() == want_grid.tolist()
        assert _differing(rows, want, torch.float32) == 0
    half, _ = fe(arrays, out_dtype=torch.bfloat16)
    assert _differing(half, want, torch.bfloat16) == 0
    # a clip of the three equal images: two steps, the second one the third image twice
    clip, g = fe.clip([arrays[0], arrays[1], arrays[3]])
    assert g.tolist() == [[2, 10, 10]]
    table = IR.lut(RR.MEAN, RR.STD)
    assert _differing(clip, RR.rows_expected([arrays[0], arrays[1], arrays[3]], 140, 140, table), torch.float32) == 0
    with pytest.raises(ValueError, match="one size"):
        fe.clip(arrays[1:3])


class _Processor:
    """A stand-in for the Qwen2.5-VL processor: what a hand-off touches is its `image_processor`"""

    def __init__(self, image_processor):
        self.image_processor = image_processor


def test_hip_qwen_image_through_a_stand_in_processor_equals_the_library():
    from PIL import Image
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    from transformers.feature_extraction_utils import BatchFeature

    from x2i_amd import handoff
    arrays, _ = _mixed()
    images = [Image.fromarray(a) for a in arrays]
    ip = mod.Qwen2VLImageProcessorPil()
    proc = _Processor(ip)
    want = ip(images=images, return_tensors="pt")
    with handoff.HipQwenImage(proc, device="cuda") as hi:
        assert proc.image_processor is not ip and proc.image_processor.merge_size == 2 and proc.image_processor.size == ip.size
        got = proc.image_processor(images=images, return_tensors="pt")
        assert isinstance(got, BatchFeature) and type(got) is type(want) and list(got.keys()) == list(want.keys())
        pv = got["pixel_values"]
        assert pv.device.type == "cuda" and pv.dtype == torch.float32 and tuple(pv.shape) == tuple(want["pixel_values"].shape)
        assert torch.equal(_bits(pv), _bits(want["pixel_values"].cuda()))
        assert got["image_grid_thw"].dtype == want["image_grid_thw"].dtype and torch.equal(got["image_grid_thw"], want["image_grid_thw"])
        assert (hi.calls, hi.fallbacks, hi.last_reason) == (1, 0, None)
        # overrides that change nothing are served; one image alone too
        one = proc.image_processor(images=images[2], return_tensors="pt", do_resize=True, patch_size=14, size=dict(ip.size))
        assert hi.calls == 2 and torch.equal(_bits(one["pixel_values"]), _bits(ip(images=images[2], return_tensors="pt")["pixel_values"].cuda()))
        # the whole call goes to the original: a grey-scale image, do_resize=False, videos=
        grey = [images[0], Image.fromarray(arrays[1][:, :, 0])]
        out = proc.image_processor(images=grey, return_tensors="pt")
        assert (hi.calls, hi.fallbacks) == (2, 1) and "not an RGB image" in hi.last_reason and out["pixel_values"].device.type == "cpu"
        assert torch.equal(out["pixel_values"], ip(images=grey, return_tensors="pt")["pixel_values"])
        square = [Image.fromarray(arrays[0][:112, :112])]
        out = proc.image_processor(images=square, return_tensors="pt", do_resize=False)
        assert (hi.calls, hi.fallbacks) == (2, 2) and "do_resize" in hi.last_reason and out["pixel_values"].device.type == "cpu"
        with pytest.raises(Exception):
            proc.image_processor(images=images[:1], videos=[images[:2]], return_tensors="pt")       # the original takes no videos=
        assert (hi.calls, hi.fallbacks) == (2, 3) and "videos" in hi.last_reason
        out = proc.image_processor(images=images[:1], return_tensors="pt", size={"shortest_edge": 28 * 28, "longest_edge": 56 * 56})
        assert (hi.calls, hi.fallbacks) == (2, 4) and "size" in hi.last_reason and tuple(out["pixel_values"].shape) == (16, ROW)
    assert proc.image_processor is ip and "image_processor" in proc.__dict__


def test_rows_written_in_place_into_the_towers_workspace_give_the_towers_bits():
    from tests import qwen_vision_ref as VR
    from x2i_amd import handoff
    from x2i_amd.qwen_image import QwenImageFrontEnd
    from x2i_amd.qwen_vision import Qwen2_5VisionTower
    cfg = VR.library_config(2, 160, 2, 172, 256, (1,))
    tower = Qwen2_5VisionTower(cfg, device="cuda").init_random_(seed=3)
    arrays, (want, _) = _mixed()
    fe = QwenImageFrontEnd(device="cuda")
    rows32, grid = fe(arrays[:1])
    assert grid.tolist() == [[1, 10, 10]] and _differing(rows32, want[:100], torch.float32) == 0
    plan = tower.plan(grid.tolist())
    ref = tower(rows32, plan=plan)
    ref = (ref.pooler_output.clone(), ref.last_hidden_state.clone())
    assert tuple(ref[0].shape) == (25, 256) and tuple(ref[1].shape) == (100, 160)
    PX = tower.pixel_workspace(plan)
    assert PX.dtype == torch.bfloat16 and tuple(PX.shape) == (100, 1216) and PX.data_ptr() == plan.ws["PX"].data_ptr()
    PX[:, :ROW].fill_(SENTINEL)                                  # what forward's copy left there must not be what is read next
    view, _ = fe(arrays[:1], out_dtype=torch.bfloat16, out=PX, row_stride=1216)
    assert view.data_ptr() == PX.data_ptr() and view.stride() == (1216, 1) and tuple(view.shape) == (100, ROW)
    assert _differing(PX[:, :ROW], want[:100], torch.bfloat16) == 0 and int((PX[:, ROW:] != 0).sum()) == 0
    out = tower.forward_from_workspace(plan)
    assert torch.equal(_bits16(out.pooler_output), _bits16(ref[0])) and torch.equal(_bits16(out.last_hidden_state), _bits16(ref[1]))
    assert int((PX[:, ROW:] != 0).sum()) == 0
    # the hand-offs: HipQwenImage(tower=...) hands out that view, and HipVision's forward recognises it and does not copy
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    from PIL import Image
    proc = _Processor(mod.Qwen2VLImageProcessorPil())
    hv = handoff.HipVision.__new__(handoff.HipVision)
    hv.tower, hv.calls, hv.in_place = tower, 0, 0
    with handoff.HipQwenImage(proc, device="cuda", tower=tower) as hi:
        PX = tower.pixel_workspace(tower._plan_for(((1, 10, 10),)))          # the plan the tower keeps for this grid
        PX[:, :ROW].fill_(SENTINEL)
        feat = proc.image_processor(images=[Image.fromarray(arrays[0])], return_tensors="pt")
        pv = feat["pixel_values"]
        assert hi.calls == 1 and pv.dtype == torch.bfloat16 and pv.data_ptr() == PX.data_ptr() and pv.stride() == (1216, 1)
        got = hv._forward(pv, grid_thw=feat["image_grid_thw"])
        assert (hv.calls, hv.in_place) == (1, 1) and torch.equal(_bits16(got.pooler_output), _bits16(ref[0]))
        other = hv._forward(rows32, grid_thw=feat["image_grid_thw"])          # any other input takes the copying forward
        assert (hv.calls, hv.in_place) == (2, 1) and torch.equal(_bits16(other.pooler_output), _bits16(ref[0]))
        copy = hv._forward(pv.clone(), grid_thw=feat["image_grid_thw"])
        assert (hv.calls, hv.in_place) == (3, 1) and torch.equal(_bits16(copy.last_hidden_state), _bits16(ref[1]))


def _bits16(t):
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16)
