"""The numpy restatement of the Qwen2.5-VL image processor (tests/image_rows_ref.py) against the installed library's Pillow backend, bit
for bit; smart_resize (the restatement and QwenImageFrontEnd's) against rows recorded from the library; the planted faults; the temporal
rule.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import image_ref as IR
from tests import image_rows_ref as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen_smart_resize.json")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def test_the_restatement_equals_the_librarys_pillow_backend_bit_for_bit():
    pytest.importorskip("PIL")
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    from PIL import Image
    ip = mod.Qwen2VLImageProcessorPil()
    assert tuple(ip.image_mean) == RR.MEAN and tuple(ip.image_std) == RR.STD
    assert (ip.size["shortest_edge"], ip.size["longest_edge"]) == (RR.MIN_PIXELS, RR.MAX_PIXELS)
    rng = np.random.default_rng(7)
    sizes = list(RR.LIBRARY_SIZES) + [(int(rng.integers(20, 700)), int(rng.integers(20, 700))) for _ in range(20)]
    assert len(sizes) == 28
    for w, h in sizes:
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        got = ip([Image.fromarray(img)], return_tensors="pt")
        want, grid = RR.preprocess([img], resize=RR.pil_resize)
        assert got["image_grid_thw"].tolist() == grid.tolist(), (w, h)
        pv = got["pixel_values"].numpy()
        assert pv.dtype == np.float32 and pv.shape == want.shape, (w, h)
        assert np.array_equal(_bits(pv), _bits(want)), "%d x %d: %d elements differ" % (w, h, int((_bits(pv) != _bits(want)).sum()))
    # a batch of several sizes is the concatenation, and the numpy resize stands for Pillow's
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for w, h in ((128, 128), (200, 90), (37, 61))]
    got = ip([Image.fromarray(a) for a in imgs], return_tensors="pt")
    want, grid = RR.preprocess(imgs)
    assert got["image_grid_thw"].tolist() == grid.tolist() and np.array_equal(_bits(got["pixel_values"].numpy()), _bits(want))


def test_the_tables_of_the_host_module_are_the_restatements():
    from x2i_amd import image as IM
    assert np.array_equal(_bits(IM.norm_lut(RR.MEAN, RR.STD)), _bits(IR.lut(RR.MEAN, RR.STD)))
    other = np.arange(256, dtype=np.float32) * np.float32(1 / 255)           # a multiplication is NOT the processor's division
    assert not np.array_equal(_bits(other), _bits(np.arange(256, dtype=np.uint8).astype(np.float32) / 255))


def test_smart_resize_equals_the_rows_recorded_from_the_library():
    from x2i_amd.qwen_image import QwenImageFrontEnd
    rows = json.load(open(GOLDEN))
    assert 180 <= len(rows) <= 260
    branches = {"round": 0, "over": 0, "under": 0, "refused": 0, "odd_units": 0}
    for h, w, lo, hi, H, W in rows:
        fe = QwenImageFrontEnd(min_pixels=lo, max_pixels=hi, device="cpu")
        if H is None:
            branches["refused"] += 1
            for fn in (lambda: RR.smart_resize(h, w, lo, hi), lambda: fe.smart_resize(h, w)):
                with pytest.raises(ValueError, match="aspect ratio"):
                    fn()
            assert "aspect ratio" in fe.served(w, h)
            continue
        assert RR.smart_resize(h, w, lo, hi) == (H, W) == fe.smart_resize(h, w), (h, w, lo, hi)
        hb, wb = round(h / 28) * 28, round(w / 28) * 28
        branches["over" if hb * wb > hi else "under" if hb * wb < lo else "round"] += 1
        branches["odd_units"] += (H // 28) % 2 == 1 or (W // 28) % 2 == 1
    assert all(v >= 10 for v in branches.values()), branches


def _case_rows(case, fault=None):
    _, iw, ih, ow, oh, t_in, n_items = case
    table = IR.lut(RR.MEAN, RR.STD)
    return [RR.rows_expected(fr, ow, oh, table, fault) for fr in RR.item_frames(iw, ih, t_in, n_items)]


SMALL = [c for c in RR.GPU_CASES if c[3] * c[4] * c[5] * c[6] <= 140 * 140 * 3]      # every case but the pair of 4-frame clips


def test_the_cases_are_the_issues_and_the_permutation_is_the_formula():
    assert [c[1:] for c in RR.GPU_CASES] == [(28, 28, 28, 28, 1, 1), (140, 56, 140, 56, 2, 1), (128, 128, 140, 140, 1, 3), (20, 10, 56, 28, 1, 2),
                                             (37, 61, 28, 56, 3, 1), (400, 300, 112, 84, 1, 1), (1000, 30, 1008, 28, 1, 1), (200, 90, 196, 84, 4, 2)]
    table = IR.lut(RR.MEAN, RR.STD)
    for case in (RR.GPU_CASES[0], RR.GPU_CASES[1], RR.GPU_CASES[4]):
        _, iw, ih, ow, oh, t_in, _ = case
        frames = RR.item_frames(iw, ih, t_in, 1)[0]
        resized = [IR.resize(f, ow, oh) for f in frames]
        slow = RR.rows_by_the_formula(resized, table)
        assert not np.isnan(slow).any()
        assert np.array_equal(_bits(slow), _bits(RR.rows_of(resized, table)))
    assert RR.smart_resize(128, 128) == (140, 140)                       # the reference's 128 x 128 image becomes 100 rows
    # the library's layout of an image, from its own reshape: (gh / 2, gw / 2, 2, 2, C, tp, 14, 14)
    res = IR.resize(RR.item_frames(128, 128, 1, 1)[0][0], 140, 140)
    norm = np.stack([table[c][res[:, :, c]] for c in range(3)])          # [C, H, W]
    p = norm.reshape(3, 5, 2, 14, 5, 2, 14).transpose(1, 4, 2, 5, 0, 3, 6)
    p = np.broadcast_to(p[:, :, :, :, :, None], p.shape[:5] + (2,) + p.shape[5:]).reshape(100, 1176)
    assert np.array_equal(_bits(p), _bits(RR.rows_of([res], table)))


@pytest.mark.parametrize("fault", RR.FAULTS)
def test_every_planted_fault_changes_the_output_on_a_gpu_case(fault):
    changed = []
    for case in SMALL:
        good, bad = _case_rows(case), _case_rows(case, fault)
        if any(not np.array_equal(_bits(g), _bits(b)) for g, b in zip(good, bad)):
            changed.append(case[0])
    print(fault, "changes", changed)
    assert changed, fault
    if fault in ("odd_clip_zero_padded",):
        assert "odd_clip_down" in changed
    if fault == "per_slot_resize_of_wrong_frame":
        assert "copy_tiles_4_4_2_pair" in changed and "copy_one_unit" not in changed      # an image's two slots are the same frame


def test_an_images_slots_are_equal_and_an_odd_clip_repeats_its_last_frame():
    table = IR.lut(RR.MEAN, RR.STD)
    rows = _case_rows(RR.GPU_CASES[2])[0].reshape(100, 3, 2, 196)
    assert np.array_equal(_bits(rows[:, :, 0]), _bits(rows[:, :, 1]))
    _, iw, ih, ow, oh, t_in, _ = RR.GPU_CASES[4]
    assert t_in == 3
    frames = RR.item_frames(iw, ih, 3, 1)[0]
    clip = RR.rows_expected(frames, ow, oh, table)
    n = (oh // 14) * (ow // 14)
    assert clip.shape == (2 * n, 1176)
    step1 = clip[n:].reshape(n, 3, 2, 196)
    last = RR.rows_expected(frames[2:], ow, oh, table).reshape(n, 3, 2, 196)
    assert np.array_equal(_bits(step1[:, :, 0]), _bits(step1[:, :, 1])) and np.array_equal(_bits(step1), _bits(last))
    step0 = clip[:n].reshape(n, 3, 2, 196)
    assert not np.array_equal(_bits(step0[:, :, 0]), _bits(step0[:, :, 1]))
    assert np.array_equal(_bits(step0[:, :, 1]), _bits(RR.rows_expected(frames[1:2], ow, oh, table).reshape(n, 3, 2, 196)[:, :, 0]))


def test_from_hf_reads_the_processor_and_refuses_by_field():
    from x2i_amd.qwen_image import QwenImageFrontEnd

    class IP:
        image_mean, image_std = list(RR.MEAN), list(RR.STD)
        size = {"shortest_edge": 3136, "longest_edge": 12845056}
        patch_size, merge_size, temporal_patch_size, resample = 14, 2, 2, 3
        do_resize = do_rescale = do_normalize = True

    fe = QwenImageFrontEnd.from_hf(IP(), device="cpu")
    assert (fe.min_pixels, fe.max_pixels) == (3136, 12845056) and np.array_equal(_bits(fe.lut.numpy()), _bits(IR.lut(RR.MEAN, RR.STD)))
    for field, value in (("patch_size", 16), ("merge_size", 1), ("temporal_patch_size", 1), ("resample", 2), ("do_resize", False),
                         ("do_rescale", False), ("do_normalize", False)):
        ip = IP()
        setattr(ip, field, value)
        with pytest.raises(ValueError, match=field):
            QwenImageFrontEnd.from_hf(ip, device="cpu")
    old = IP()
    old.size, old.min_pixels, old.max_pixels = {}, 784, 16384
    fe = QwenImageFrontEnd.from_hf(old, device="cpu")
    assert (fe.min_pixels, fe.max_pixels) == (784, 16384) and fe.smart_resize(128, 128) == (112, 112)
    assert fe.served(128, 128) is None and "in_w=70000" in fe.served(70000, 4000)
    with pytest.raises(Exception, match="GPU only"):
        fe([np.zeros((28, 28, 3), dtype=np.uint8)])
