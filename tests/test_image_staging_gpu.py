"""The staging path of the three image front ends (x2i_amd/image.py, qwen_image.py, internvl_image.py) on the GPU: the pinned buffer, the
asynchronous transfer per group, the cached plan and its regrowth, through ImageFrontEnd.__call__, ImageFrontEnd.sliced,
QwenImageFrontEnd.__call__ and InternVLImageFrontEnd.tiles.  Every output is compared bit for bit with the numpy restatements of
tests/image_ref.py, tests/image_tiles_ref.py and tests/image_rows_ref.py.

The shapes are the smallest at which staging can go wrong: three images of two sizes in the order A, B, A, so that the second group lies
at a non-zero offset of the pinned buffer, MiniCPM-o's grouping (equal sizes anywhere in the list) reorders the frames and the neighbour
grouping of the other two does not.  The kernels themselves are tested in tests/test_image_gpu.py, test_image_tiles_gpu.py and
test_image_rows_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import image_ref as IR
from tests import image_rows_ref as RR
from tests import image_tiles_ref as TR

pytestmark = pytest.mark.gpu

SIZES = ((37, 61), (128, 96), (37, 61))          # (w, h): A, B, A
SCALE, SLICES = 56, 4                            # MiniCPM-o: B (128 x 96 > 56 x 56) is sliced into a 2 x 2 grid, A (37 x 61) is not
TILE, MAX_NUM = 28, 4                            # InternVL2.5: tiles of 28 x 28, at most 4 of them and the thumbnail
PATHS = ("call", "sliced", "qwen", "internvl")


def _front_end(path):
    from x2i_amd.image import ImageFrontEnd
    from x2i_amd.internvl_image import InternVLImageFrontEnd
    from x2i_amd.qwen_image import QwenImageFrontEnd
    if path == "qwen":
        return QwenImageFrontEnd(device="cuda")
    if path == "internvl":
        return InternVLImageFrontEnd(image_size=TILE, device="cuda")
    return ImageFrontEnd(scale_resolution=SCALE, device="cuda")


def _run(path, fe, arrays, plan=None):
    """The call's device tensors as a flat list, in the order of the images"""
    if path == "call":
        return list(fe(arrays, plan=plan)[0])
    if path == "sliced":
        return [v for vs in fe.sliced(arrays, SLICES, plan=plan)[0] for v in vs]
    if path == "qwen":
        return [fe(arrays, plan=plan)[0]]
    return [fe.tiles(arrays, max_num=MAX_NUM, plan=plan)[0]]


def _reference(path, arrays):
    if path == "call":
        return IR.preprocess(arrays, scale_resolution=SCALE)[0]
    if path == "sliced":
        return TR.minicpm_preprocess(arrays, SLICES, scale_resolution=SCALE)[0]
    if path == "qwen":
        return [RR.preprocess(arrays)[0]]
    return [np.concatenate([TR.load_image(a, MAX_NUM, TILE) for a in arrays])]


@functools.lru_cache(maxsize=None)
def _images(seed, sizes=SIZES):
    """uint8 [h, w, 3] arrays of the sizes, content of their own per seed and position; computed once, never written to"""
    return tuple(IR.edge_frames(w, h, 1, seed=seed + i)[0] for i, (w, h) in enumerate(sizes))


@functools.lru_cache(maxsize=None)
def _expected(path, seed, sizes=SIZES):
    return _reference(path, list(_images(seed, sizes)))


def _differing(got, want):
    """Elements of the device tensors that differ from the float32 references in their bits, per tensor"""
    assert len(got) == len(want)
    out = []
    for t, w in zip(got, want):
        assert t.device.type == "cuda" and t.dtype == torch.float32 and tuple(t.shape) == w.shape
        bits = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32).view(np.int32))
        out.append(int((t.cpu().contiguous().view(torch.int32) != bits).sum()))
    return out


def test_one_size_is_sliced_and_the_other_is_not():
    from x2i_amd.image import ImageFrontEnd
    fe = ImageFrontEnd(scale_resolution=SCALE, device="cpu")
    (a, b) = SIZES[:2]
    assert fe.slice_plan(a[0], a[1], SLICES)[1] is None and fe.slice_plan(b[0], b[1], SLICES)[1] == (2, 2)
    assert TR.sliced_grid(a, SLICES, SCALE) is None and TR.sliced_grid(b, SLICES, SCALE) == (2, 2)
    assert SIZES[0] == SIZES[2] != SIZES[1]


@pytest.mark.parametrize("path", PATHS)
def test_mixed_sizes_and_a_second_call_through_the_cached_plan(path):
    fe = _front_end(path)
    nbytes = sum(a.size for a in _images(1))
    first = _run(path, fe, list(_images(1)))
    plan = fe._plan
    assert plan is not None and plan.nbytes == nbytes and plan.busy
    assert not any(np.array_equal(x, y) for x, y in zip(_images(1), _images(2)))          # other content, the same sizes
    second = _run(path, fe, list(_images(2)))
    assert fe._plan is plan                                      # the cached plan, its pinned buffer overwritten after the wait
    assert _differing(second, _expected(path, 2)) == [0] * len(second)
    assert _differing(first, _expected(path, 1)) == [0] * len(first)       # what the first call's transfers carried, read after the second


@pytest.mark.parametrize("path", PATHS)
def test_a_plan_regrows_and_an_explicit_plan_holds_exactly_the_call(path):
    fe = _front_end(path)
    one = _run(path, fe, list(_images(1, SIZES[:1])))
    small = fe._plan
    assert small.nbytes == _images(1)[0].size
    assert _differing(one, _expected(path, 1, SIZES[:1])) == [0] * len(one)
    nbytes = sum(a.size for a in _images(1))
    grown = _run(path, fe, list(_images(1)))                     # more bytes than the cached plan holds: a new one
    assert fe._plan is not small and fe._plan.nbytes == nbytes
    assert _differing(grown, _expected(path, 1)) == [0] * len(grown)
    kept = fe._plan
    exact = fe.plan(nbytes)
    given = _run(path, fe, list(_images(2)), plan=exact)
    assert fe._plan is kept and exact.busy                       # an explicit plan is used and not kept
    assert _differing(given, _expected(path, 2)) == [0] * len(given)
    with pytest.raises(ValueError, match="plan holds"):
        _run(path, fe, list(_images(2)), plan=fe.plan(nbytes - 1))
