"""The image front end's kernel (csrc/image.hip) on the GPU against tests/image_ref.py, the numpy restatement of Pillow's 8-bit BICUBIC
resample, the processor's normalisation and the strip layout (itself equal to Pillow byte for byte: tests/test_image_ref_cpu.py).  Equality
is exact, float32 bit for bit and bf16 as one rounding of that float32.

Every case runs three frames of different content through one launch, from a buffer whose row pitch exceeds 3 w and is no multiple of 4,
into a padded batch [n, 3, 14, 14 Lmax] with Lmax > L that is filled with a sentinel: columns at and beyond 14 L, the gaps between the
frames and the guards on either side stay untouched, and a relaunch gives the same bits.  Before it launches, a case asserts that its input
drives the reference's pre-clip sum below 0 and above 255 in each pass that runs, and that each resizing axis has an output whose tap window
is cut at either border."""
import functools

import numpy as np
import pytest
import torch

from tests import image_ref as IR

pytestmark = pytest.mark.gpu

G = 256                                  # guard elements on either side of every buffer
SENTINEL = 777.0
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # three different channels
PAD_BYTE = 0xAB


@functools.lru_cache(maxsize=None)
def _case(iw, ih, ow, oh):
    """(frames, expected float32 [3, 14, 14 L] per frame, the reference's passes per frame); computed once, never written to"""
    frames = IR.edge_frames(iw, ih, 3)
    table = IR.lut(MEAN, STD)
    return frames, [IR.front_end(f, ow, oh, table) for f in frames], [IR.resize_sums(f, ow, oh)[0] for f in frames]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _expected_bits(x, dtype):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.float32:
        return torch.from_numpy(x.view(np.int32))
    return torch.from_numpy(IR.to_bf16_bits(x).view(np.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("iw,ih,ow,oh", IR.GPU_CASES, ids=["%dx%d-%dx%d" % c for c in IR.GPU_CASES])
def test_kernel_equals_the_reference_bit_for_bit(iw, ih, ow, oh, dtype):
    from x2i_amd import image as IM, image_binding as ib
    frames, expected, passes = _case(iw, ih, ow, oh)
    n = len(frames)
    # ---- coverage of the case, asserted on the reference before anything is launched
    ran = [axis for axis, _ in passes[0]]
    assert ran == [a for a, differs in ((1, iw != ow), (0, ih != oh)) if differs]
    for j, axis in enumerate(ran):
        lo, hi = min(int(p[j][1].min()) for p in passes), max(int(p[j][1].max()) for p in passes)
        print("%dx%d -> %dx%d  pass along axis %d: pre-clip sums in [%d, %d]" % (iw, ih, ow, oh, axis, lo, hi))
        assert lo < 0 and hi > 255
    for n_in, n_out in ((iw, ow), (ih, oh)):
        if n_in != n_out:
            assert IR.window_is_cut(n_in, n_out) == (True, True)
    assert any(not np.array_equal(frames[0], f) for f in frames[1:])
    # ---- buffers
    pitch = 3 * iw + 5
    pitch += pitch % 4 == 0
    assert pitch > 3 * iw and pitch % 4
    fpitch = ih * pitch + 7
    host = np.full(2 * G + n * fpitch, PAD_BYTE, dtype=np.uint8)
    for f, img in enumerate(frames):
        rows = host[G + f * fpitch:G + f * fpitch + ih * pitch].reshape(ih, pitch)
        rows[:, :3 * iw] = img.reshape(ih, 3 * iw)
    src_all = torch.from_numpy(host).cuda()
    src = src_all[G:G + n * fpitch]
    L = (oh // 14) * (ow // 14)
    rs = 14 * (L + 3)                                        # Lmax = L + 3
    fs = 42 * rs + 11
    out_all = torch.full((2 * G + n * fs,), SENTINEL, dtype=dtype, device="cuda")
    out = out_all[G:G + n * fs]
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()      # noqa: E731
    hb, hc = (dev(a) for a in IM.axis_tables(iw, ow)) if iw != ow else (None, None)
    vb, vc = (dev(a) for a in IM.axis_tables(ih, oh)) if ih != oh else (None, None)
    if iw != ow:
        rb, rk = IR.coefficients(iw, ow)
        assert np.array_equal(hb.cpu().numpy(), rb) and np.array_equal(hc.cpu().numpy(), rk)
    lut = torch.from_numpy(IM.norm_lut(MEAN, STD)).cuda()
    assert np.array_equal(lut.cpu().numpy().view(np.int32), IR.lut(MEAN, STD).view(np.int32))
    launch = lambda: ib.frontend(src, iw, ih, pitch, fpitch, n, ow, oh, hb, hc, vb, vc, lut, out, fs, rs)      # noqa: E731
    launch()
    first = _bits(out_all).cpu().clone()
    # ---- the values, the untouched columns, gaps and guards
    got = out.cpu()
    sent = _bits(torch.full((1,), SENTINEL, dtype=dtype))[0]
    mask = torch.zeros(n * fs, dtype=torch.bool)             # what the launch may write
    for f in range(n):
        frame = got[f * fs:f * fs + 42 * rs].view(3, 14, rs)
        want = _expected_bits(expected[f], dtype)
        assert want.shape == (3, 14, 14 * L)
        diff = int((_bits(frame[:, :, :14 * L].contiguous()) != want).sum())
        assert diff == 0, "frame %d: %d of %d elements differ from the reference" % (f, diff, want.numel())
        mask[f * fs:f * fs + 42 * rs].view(3, 14, rs)[:, :, :14 * L] = True
    assert bool((_bits(got)[~mask] == sent).all()), "a column beyond 14 L or a gap between the frames was written"
    whole = _bits(out_all).cpu()
    assert bool((whole[:G] == sent).all()) and bool((whole[-G:] == sent).all())
    assert bool((src_all.cpu() == torch.from_numpy(host)).all())
    # ---- a relaunch is bit-identical
    launch()
    assert torch.equal(_bits(out_all).cpu(), first)


@functools.lru_cache(maxsize=None)
def _video_frames():
    return np.stack(IR.edge_frames(1280, 720, 2, seed=7))


def test_front_end_at_1280x720_equals_the_reference_end_to_end():
    from PIL import Image

    from x2i_amd.image import ImageFrontEnd
    frames = _video_frames()
    fe = ImageFrontEnd(device="cuda")
    assert fe.best_size(1280, 720) == (602, 336)
    table = IR.lut((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    want = [IR.front_end(f, 602, 336, table) for f in frames]
    for given in (frames, [Image.fromarray(f) for f in frames]):
        values, tgt = fe(given)
        assert tgt.tolist() == [[24, 43], [24, 43]] and len(values) == 2
        for v, w in zip(values, want):
            assert v.device.type == "cuda" and v.dtype == torch.float32 and tuple(v.shape) == (3, 14, 14 * 24 * 43)
            assert int((_bits(v.cpu().contiguous()) != _expected_bits(w, torch.float32)).sum()) == 0
    half, _ = fe(frames[:1], out_dtype=torch.bfloat16)
    assert int((_bits(half[0].cpu().contiguous()) != _expected_bits(want[0], torch.bfloat16)).sum()) == 0


def test_hip_image_through_a_stand_in_processor_equals_the_restated_preprocess():
    from PIL import Image

    from x2i_amd import handoff
    sizes = [(97, 61), (64, 48), (97, 61), (64, 48), (97, 61)]              # five frames of two sizes, interleaved
    arrays = [IR.edge_frames(w, h, 1, seed=i)[0] for i, (w, h) in enumerate(sizes)]
    images = [Image.fromarray(a) for a in arrays]
    want, want_sizes, want_tgt = IR.preprocess(arrays)
    ip = IR.StubImageProcessor()
    proc = IR.StubProcessor(ip)
    with handoff.HipImage(proc, device="cuda") as hi:
        feat = proc.image_inputs([images], max_slice_nums=1, return_tensors="pt")
        assert (hi.calls, hi.fallbacks, ip.calls) == (1, 0, 0) and type(feat) is IR.StubBatchFeature
        assert list(feat.keys()) == ["pixel_values", "image_sizes", "tgt_sizes"]
        pv = feat["pixel_values"]
        assert len(pv) == 1 and len(pv[0]) == 5
        for v, w in zip(pv[0], want):
            assert v.device.type == "cuda" and v.dtype == torch.float32 and tuple(v.shape) == w.shape
            assert int((_bits(v.cpu().contiguous()) != _expected_bits(w, torch.float32)).sum()) == 0
        assert [t.tolist() for t in feat["image_sizes"][0]] == [list(s) for s in want_sizes]
        assert feat["tgt_sizes"][0].device.type == "cpu" and feat["tgt_sizes"][0].tolist() == want_tgt.tolist()
    assert proc.image_processor is ip
    ref = proc.image_inputs([images], max_slice_nums=1, return_tensors="pt")            # the original, after remove()
    assert ip.calls == 1 and all(torch.equal(a, b.cpu()) for a, b in zip(ref["pixel_values"][0], pv[0]))
    assert torch.equal(ref["tgt_sizes"][0], feat["tgt_sizes"][0]) and all(torch.equal(a, b) for a, b in zip(ref["image_sizes"][0], feat["image_sizes"][0]))
