"""tests/image_ref.py against what it restates (no GPU): Pillow's BICUBIC resize byte for byte, the processor's numpy normalisation, F.unfold
and the reference's reshape / permute for the strip layout, find_best_resize's known answers.  And the planted faults: each deviation a port
could make must show on the inputs tests/test_image_gpu.py uses, or that test could not tell the port from the real thing.

The planted faults, counted on the GPU test's frames against Pillow (differing bytes, summed over the three frames of a case):
no uint8 rounding between the passes, the vertical pass first (both only where two passes run), a = -0.75, unnormalised coefficients,
and coefficients rounded without regard to their sign (int(v + 0.5) for negative v too).  One more was asked for and CANNOT differ:
rounding the coefficients with Python's round() in place of the signed +-0.5 truncation.  round() and the truncation agree on every value
that is not an exact tie (a fraction of exactly one half), and no coefficient of any GPU case is a tie, so that variant yields the very
same tables (0 differing coefficients, 0 differing bytes on every case).  test_round_is_not_a_fault_on_these_tables asserts exactly that,
so the day a case with a tie is added it says so; the sign-blind rounding stands in as the rounding fault that does show."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from tests import image_ref as IR

PAIRS = [(1280, 720, 602, 336), (97, 61, 574, 350), (640, 480, 518, 392), (33, 500, 112, 1722), (448, 300, 546, 364), (450, 448, 448, 448),
         (448, 448, 448, 448)]


@functools.lru_cache(maxsize=None)
def _frames(iw, ih):
    return IR.edge_frames(iw, ih, 3 if iw * ih < 100000 else 1)


def _pillow(img, ow, oh):
    return np.asarray(Image.fromarray(img).resize((ow, oh), resample=Image.Resampling.BICUBIC))


@pytest.mark.parametrize("iw,ih,ow,oh", PAIRS + IR.GPU_CASES, ids=["%dx%d-%dx%d" % c for c in PAIRS + IR.GPU_CASES])
def test_resize_equals_pillow_byte_for_byte(iw, ih, ow, oh):
    for img in _frames(iw, ih):
        assert (img == 0).any() and (img == 255).any() and len(np.unique(img)) > 100       # hard edges beside random bytes
        got, want = IR.resize(img, ow, oh), _pillow(img, ow, oh)
        assert got.shape == want.shape == (oh, ow, 3) and got.dtype == np.uint8
        assert int((got != want).sum()) == 0


@functools.lru_cache(maxsize=None)
def _fault_counts():
    """{(case, fault): differing bytes against Pillow, summed over the case's three frames}"""
    out = {}
    for case in IR.GPU_CASES:
        iw, ih, ow, oh = case
        want = [_pillow(img, ow, oh) for img in _frames(iw, ih)]
        for fault in IR.FAULTS:
            out[(case, fault)] = sum(int((IR.resize(img, ow, oh, fault) != w).sum()) for img, w in zip(_frames(iw, ih), want))
    return out


@pytest.mark.parametrize("fault", IR.FAULTS)
def test_planted_faults_differ_from_pillow_on_the_gpu_tests_inputs(fault):
    """Each fault shows on the GPU test's inputs.  The four that change a pass's arithmetic wholesale show on EVERY case in which their code
    runs; the sign-blind rounding moves a negative coefficient by one unit of 2^-22 and so moves few bytes: it must show on the inputs
    taken together and on every case with two passes."""
    counts = _fault_counts()
    total = 0
    for case in IR.GPU_CASES:
        iw, ih, ow, oh = case
        passes = int(iw != ow) + int(ih != oh)
        diff = counts[(case, fault)]
        total += diff
        print("%dx%d -> %dx%d  %-16s %d differing bytes" % (case + (fault, diff)))
        runs = passes == 2 if fault in ("no_u8_between", "vertical_first") else passes >= 1
        if not runs:
            assert diff == 0                   # nothing to plant: the fault's code does not run
        elif fault != "sign_blind_round" or passes == 2:
            assert diff > 0, case
    assert total > 0


def test_every_fault_is_planted_somewhere_and_the_cases_run_every_combination_of_passes():
    combos = {(iw != ow, ih != oh) for iw, ih, ow, oh in IR.GPU_CASES}
    assert combos == {(True, True), (True, False), (False, True), (False, False)}
    assert set(IR.FAULTS) == {"no_u8_between", "a_075", "sign_blind_round", "vertical_first", "unnormalised"}


def test_round_is_not_a_fault_on_these_tables():
    """See the module's docstring: Python's round() gives the same coefficients as the signed truncation unless a value is an exact tie"""
    for iw, ih, ow, oh in IR.GPU_CASES + PAIRS:
        for n_in, n_out in ((iw, ow), (ih, oh)):
            if n_in == n_out:
                continue
            b, K = IR.coefficients(n_in, n_out)
            b2, K2 = IR.coefficients(n_in, n_out, "round_coef")
            assert np.array_equal(b, b2) and int((K != K2).sum()) == 0
            b3, K3 = IR.coefficients(n_in, n_out, "sign_blind_round")
            assert int((K != K3).sum()) > 0 and int(np.abs(K.astype(np.int64) - K3).max()) == 1


def test_accumulator_bound_over_the_supported_scales():
    """sum |K| 255 + 2^21 must stay below 2^31: the largest sum |K| over a sweep of scales from 70-fold enlargement to 80-fold reduction,
    cut windows included, is 1.2686 * 2^22, against the 2.0059 * 2^22 the int32 accumulator holds"""
    worst = 0
    sweep = [(n_in, n_out) for n_in in list(range(1, 64)) + [97, 231, 500, 720, 1280, 1489, 3000, 4000] for n_out in (14, 28, 42, 70, 336, 602, 980)]
    for n_in, n_out in sweep:
        if n_in != n_out and n_in * n_out <= 4000 * 980:
            K = IR.coefficients(n_in, n_out)[1].astype(np.int64)
            worst = max(worst, int(np.abs(K).sum(axis=1).max()))
    print("largest sum |K| = %d = %.4f * 2^22; sum |K| * 255 + 2^21 = %d of %d" % (worst, worst / 2 ** 22, worst * 255 + 2 ** 21, 2 ** 31))
    assert worst * 255 + 2 ** 21 < 2 ** 31 and worst <= 1.27 * 2 ** 22


def test_lut_equals_the_processors_numpy_expressions_for_all_768_entries():
    from x2i_amd.image import norm_lut
    for mean, std in (((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))):
        # the processor: to_numpy_array(image).astype(np.float32) / 255, then transformers' normalize, which casts mean and std to the image's dtype
        v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
        x = v.astype(np.float32) / 255
        want = (x - np.array(mean).astype(x.dtype)) / np.array(std).astype(x.dtype)
        assert want.dtype == np.float32
        want = want[0].T                                          # [3, 256]
        for table in (IR.lut(mean, std), norm_lut(mean, std)):
            assert table.dtype == np.float32 and table.shape == (3, 256)
            assert np.array_equal(table.view(np.int32), np.ascontiguousarray(want).view(np.int32))
    try:
        from transformers.image_transforms import normalize
    except Exception:                                             # the library's own function, where it imports
        return
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2).astype(np.float32) / 255
    lib = normalize(img, mean=np.array([0.5, 0.4, 0.3]), std=np.array([0.5, 0.25, 0.2]), input_data_format="channels_last")
    table = IR.lut((0.5, 0.4, 0.3), (0.5, 0.25, 0.2))
    assert np.array_equal(np.asarray(lib, dtype=np.float32).reshape(256, 3).T.copy().view(np.int32), table.view(np.int32))


def test_strip_layout_equals_unfold_and_the_references_reshape():
    rng = np.random.default_rng(3)
    for H, W in ((28, 42), (14, 70), (84, 56)):
        norm = rng.standard_normal((H, W, 3)).astype(np.float32)
        image = torch.from_numpy(np.ascontiguousarray(norm.transpose(2, 0, 1)))          # channel first, as the processor holds it
        patches = torch.nn.functional.unfold(image, (14, 14), stride=(14, 14))
        patches = patches.reshape(image.size(0), 14, 14, -1)
        want = patches.permute(0, 1, 3, 2).reshape(image.size(0), 14, -1).numpy()
        got = IR.strip(norm)
        assert got.shape == want.shape == (3, 14, H * W // 14) and np.array_equal(got, want)
        gw = W // 14
        for c, r, ph, pw, q in ((0, 0, 0, 0, 0), (2, 13, H // 14 - 1, gw - 1, 13), (1, 5, H // 14 - 1, 1, 7)):
            assert got[c, r, (ph * gw + pw) * 14 + q] == norm[14 * ph + r, 14 * pw + q, c]


def test_best_size_gives_the_known_answers():
    from x2i_amd.image import ImageFrontEnd
    known = {(1280, 720): (602, 336), (1920, 1080): (602, 336), (640, 480): (518, 392), (97, 61): (560, 350), (448, 448): (448, 448)}
    fe = ImageFrontEnd(device="cpu")
    for (w, h), want in known.items():
        assert IR.best_size(w, h) == want and fe.best_size(w, h) == want
    assert IR.best_size(4000, 3000) == (518, 392) and IR.best_size(128, 128) == (448, 448)


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -0.4980392, 3.1415927, 0.0], dtype=np.float32)     # two exact ties among them
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(IR.to_bf16_bits(x).view(np.int16), want)
    table = IR.lut((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    assert np.array_equal(IR.to_bf16_bits(table).view(np.int16), torch.from_numpy(table).to(torch.bfloat16).view(torch.int16).numpy())
