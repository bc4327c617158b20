"""The image front end without a GPU: ImageFrontEnd's tables, refusals and plan (x2i_amd/image.py), and the wiring of handoff.HipImage,
MiniCPMConditioner(hip_image=True) and --hip_image around a stand-in processor that calls its image processor the way the MiniCPM-o
processor does (tests/image_ref.py: StubProcessor, StubImageProcessor, StubBatchFeature).  ImageFrontEnd.__call__ is replaced by the numpy
reference here; the kernel is tested in tests/test_image_gpu.py."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import image_ref as IR


def _reference_call(self, frames, out_dtype=torch.float32, plan=None):
    """What ImageFrontEnd.__call__ returns, from the numpy reference (on the CPU)"""
    arrays = self._as_arrays(frames)
    table = self.lut.numpy()
    values, tgt = [], []
    for a in arrays:
        ow, oh = self.best_size(a.shape[1], a.shape[0])
        values.append(torch.from_numpy(IR.front_end(a, ow, oh, table)).to(out_dtype))
        tgt.append((oh // 14, ow // 14))
    return values, np.array(tgt)


def _image(w, h, seed=0, mode="RGB"):
    return Image.fromarray(IR.edge_frames(w, h, 1, seed=seed)[0]).convert(mode)


# ---------------------------------------------------------------------------------------------------------------- ImageFrontEnd on the host
def test_tables_lut_and_from_hf():
    from x2i_amd import image as IM
    fe = IM.ImageFrontEnd.from_hf(IR.StubImageProcessor(mean=(0.5, 0.4, 0.3), std=(0.5, 0.25, 0.2), scale_resolution=448), "cpu")
    assert fe.device.type == "cpu" and fe.scale_resolution == 448 and fe.lut.dtype == torch.float32 and tuple(fe.lut.shape) == (3, 256)
    assert np.array_equal(fe.lut.numpy().view(np.int32), IR.lut((0.5, 0.4, 0.3), (0.5, 0.25, 0.2)).view(np.int32))
    for n_in, n_out in ((1280, 602), (61, 28), (20, 56), (231, 28), (120, 14)):
        b, k = IM.axis_tables(n_in, n_out)
        rb, rk = IR.coefficients(n_in, n_out)
        assert b.dtype == k.dtype == np.int32 and np.array_equal(b, rb) and np.array_equal(k, rk)
        tb, tk = fe.tables(n_in, n_out)
        assert tb.dtype == tk.dtype == torch.int32 and fe.tables(n_in, n_out)[0] is tb              # made once
    assert fe.tables(448, 448) == (None, None)
    assert fe.best_size(1280, 720) == (602, 336) and IM.ImageFrontEnd(scale_resolution=224, device="cpu").best_size(448, 448) == (224, 224)
    assert fe.served(1280, 720) is None and fe.served(4000, 3000) is None
    assert "multiple of 14 in 14..980" in fe.served(3000, 100) and "LDS plan does not fit" in fe.served(40000, 40000)


def test_from_hf_and_constructor_refusals_name_the_field():
    from x2i_amd.image import ImageFrontEnd
    with pytest.raises(ValueError, match="patch_size"):
        ImageFrontEnd.from_hf(IR.StubImageProcessor(patch_size=16), "cpu")
    with pytest.raises(ValueError, match="slice_mode"):
        ImageFrontEnd.from_hf(IR.StubImageProcessor(slice_mode=False), "cpu")
    with pytest.raises(ValueError, match="mean and std"):
        ImageFrontEnd(mean=(0.5, 0.5), device="cpu")
    with pytest.raises(ValueError, match="mean and std"):
        ImageFrontEnd(std=(0.5, 0.0, 0.5), device="cpu")
    with pytest.raises(ValueError, match="scale_resolution"):
        ImageFrontEnd(scale_resolution=7, device="cpu")


def test_plan_and_call_refusals():
    from x2i_amd import image_binding as ib
    from x2i_amd.image import ImageFrontEnd
    fe = ImageFrontEnd(device="cpu")
    p = fe.plan(1000)
    assert p.nbytes == p.stage.numel() == p.dev.numel() == 1000 and p.stage.dtype == torch.uint8 and not p.busy
    with pytest.raises(ValueError, match="plan needs"):
        fe.plan(0)
    ok = np.zeros((20, 30, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="non-empty"):
        fe([])
    with pytest.raises(ValueError, match=r"uint8 \[H, W, 3\]"):
        fe([ok.astype(np.float32)])
    with pytest.raises(ValueError, match=r"uint8 \[H, W, 3\]"):
        fe([np.zeros((20, 30, 4), dtype=np.uint8)])
    with pytest.raises(ValueError, match="mode RGB"):
        fe([Image.fromarray(ok).convert("L")])
    with pytest.raises(ValueError, match="out_dtype"):
        fe([ok], out_dtype=torch.float16)
    with pytest.raises(ValueError, match="plan holds"):
        fe([ok], plan=p)
    with pytest.raises(ib.X2IError, match="multiple of 14 in 14..980"):
        fe([np.zeros((10, 900, 3), dtype=np.uint8)])
    with pytest.raises(ib.X2IError, match="GPU only"):       # no fallback
        fe([ok])
    with pytest.raises(ib.X2IError, match="GPU only"):
        fe(np.zeros((2, 20, 30, 3), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_hip_image_serves_the_processors_call_and_forwards_attributes(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.image import ImageFrontEnd
    monkeypatch.setattr(ImageFrontEnd, "__call__", _reference_call)
    ip = IR.StubImageProcessor()
    proc = IR.StubProcessor(ip)
    hi = handoff.HipImage(proc, device="cpu")
    assert (hi.calls, hi.fallbacks) == (0, 0) and proc.image_processor is ip and ip.calls == 0
    a, b, c = _image(97, 61, 1), _image(64, 48, 2), _image(97, 61, 3)
    want = proc.image_inputs([[a, b], [c]], max_slice_nums=1)
    assert ip.calls == 1
    with hi:
        sub = proc.image_processor
        assert sub is not ip and sub.version == 2.6 and sub.max_slice_nums == 9 and sub.patch_size == 14 and sub.image_feature_size == 64
        assert sub.model_input_names == ["pixel_values"] and sub.mean is ip.mean
        assert sub.get_slice_image_placeholder((97, 61), 0, 1, False) == ip.get_slice_image_placeholder((97, 61), 0, 1, False)
        assert sub.get_sliced_grid((1280, 720), 9) == ip.get_sliced_grid((1280, 720), 9) is not None
        with pytest.raises(AttributeError):
            sub.no_such_field
        got = proc.image_inputs([[a, b], [c]], max_slice_nums=1)
        assert (hi.calls, hi.fallbacks, ip.calls) == (1, 0, 1) and type(got) is type(want) is IR.StubBatchFeature
        assert list(got.keys()) == list(want.keys()) == ["pixel_values", "image_sizes", "tgt_sizes"]
        assert [len(g) for g in got["pixel_values"]] == [2, 1]
        for g, w in zip(got["pixel_values"], want["pixel_values"]):
            assert all(x is not None and torch.equal(x, y) and x.dtype == torch.float32 for x, y in zip(g, w))
        for key in ("image_sizes", "tgt_sizes"):
            for g, w in zip(got[key], want[key]):
                if isinstance(w, list):
                    assert len(g) == len(w) and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(g, w))
                else:
                    assert torch.equal(g, w) and g.dtype == w.dtype
        # the other forms of images the processor accepts: one image, one flat list
        one = sub(a, do_pad=True, max_slice_nums=1, return_tensors="pt")
        assert len(one["pixel_values"]) == 1 and torch.equal(one["pixel_values"][0][0], want["pixel_values"][0][0]) and hi.calls == 2
        flat = sub([a, b], max_slice_nums=1)                       # no return_tensors: host values stay what they are
        assert hi.calls == 3 and flat["image_sizes"] == [[(97, 61), (64, 48)]] and isinstance(flat["tgt_sizes"][0], np.ndarray)
        assert flat["tgt_sizes"][0].tolist() == [[25, 40], [28, 37]] and ip.calls == 1
    assert proc.image_processor is ip


def test_hip_image_sends_the_whole_call_to_the_original_for_each_reason(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.image import ImageFrontEnd
    monkeypatch.setattr(ImageFrontEnd, "__call__", _reference_call)
    ip = IR.StubImageProcessor()
    proc = IR.StubProcessor(ip)
    small, big = _image(97, 61, 1), _image(640, 480, 2)
    with handoff.HipImage(proc, device="cpu") as hi:
        sub = proc.image_processor
        reasons = []

        def falls(images, **kw):
            before = (hi.calls, hi.fallbacks, ip.calls)
            out = sub(images, **kw)
            assert (hi.calls, hi.fallbacks, ip.calls) == (before[0], before[1] + 1, before[2] + 1) and "pixel_values" in out
            reasons.append(hi.last_reason)
            return out
        # slicing under the call's max_slice_nums: 640 x 480 exceeds 448 x 448, so it is sliced unless max_slice_nums is 1
        assert proc.image_inputs([[small, big]], max_slice_nums=1) is not None and (hi.calls, hi.fallbacks) == (1, 0)
        falls([[small, big]], do_pad=True, max_slice_nums=9, return_tensors="pt")
        falls([[small, big]], do_pad=True, max_slice_nums=None, return_tensors="pt")            # the processor's own default, 9
        falls([[small, big]], return_tensors="pt")
        assert reasons == ["an image that is sliced"] * 3 and ip.sliced == 3
        # not an RGB image of 8 bits per channel
        falls([[small, _image(97, 61, mode="L")]], max_slice_nums=1)
        falls([[small.convert("RGBA")]], max_slice_nums=1)
        falls([[np.asarray(small)]], max_slice_nums=1)
        falls([[Image.fromarray(np.zeros((20, 30), dtype=np.uint16))]], max_slice_nums=1)
        assert reasons[3:] == ["an input that is not an RGB image of 8 bits per channel"] * 4
        # a side over 70 patches, and a scale the kernel refuses
        falls([[_image(900, 10)]], max_slice_nums=1)
        assert "out_w=4228 must be a multiple of 14 in 14..980" in reasons[-1]            # 302 patches wide
        monkeypatch.setattr(hi.front, "served", lambda w, h: "x2i_amd: the image front end's LDS plan does not fit: a stand-in")
        falls([[small]], max_slice_nums=1)
        assert "LDS plan does not fit" in reasons[-1]
        monkeypatch.undo()
        monkeypatch.setattr(ImageFrontEnd, "__call__", _reference_call)
        # another form of call, an empty batch
        falls([[small]], max_slice_nums=1, data_format="channels_first")
        falls([[small], []], max_slice_nums=1)
        assert reasons[-2:] == ["another form of call", "an empty or unknown batch"]
        assert hi.calls == 1 and hi.fallbacks == len(reasons) == 11
        proc.image_inputs([[small]], max_slice_nums=1)
        assert hi.calls == 2


def test_remove_restores_the_original_also_on_exceptions():
    from x2i_amd import handoff
    ip = IR.StubImageProcessor()
    proc = IR.StubProcessor(ip)
    hi = handoff.HipImage(proc, device="cpu")
    with pytest.raises(KeyError):
        with hi:
            assert proc.image_processor is not ip
            raise KeyError("inside")
    assert proc.image_processor is ip
    hi.install().install()
    assert proc.image_processor is not ip
    hi.remove()
    hi.remove()
    assert proc.image_processor is ip and proc.__dict__["image_processor"] is ip
    with pytest.raises(RuntimeError, match="image_processor"):
        handoff.HipImage(object())
    with pytest.raises(ValueError, match="patch_size"):
        handoff.HipImage(IR.StubProcessor(IR.StubImageProcessor(patch_size=16)), device="cpu")
    with pytest.raises(ValueError, match="slice_mode"):
        handoff.HipImage(IR.StubProcessor(IR.StubImageProcessor(slice_mode=False)), device="cpu")


def test_hip_image_flag_parses_and_reaches_the_conditioner(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_minicpm as im
    from x2i_amd.infer.harness import build_parser
    p = build_parser("minicpm")
    assert p.parse_args(["--synthetic"]).hip_image is False
    a = p.parse_args(["--synthetic", "--task", "video2image", "--hip_image"])
    assert a.hip_image is True and not (a.hip_vision or a.hip_resampler or a.hip_decoder or a.hip_mel or a.hip_audio)
    text = " ".join(p.format_help().split())
    assert "--hip_image" in text and "MiniCPMVImageProcessor" in text and "x2i_amd/image.py" in text
    seen = {}

    class Cond:
        def __init__(self, path, device, **kw):
            seen.update(kw)

    class Stop(Exception):
        pass

    def harness(*a, **k):
        raise Stop()
    monkeypatch.setattr(im, "MiniCPMConditioner", Cond)
    monkeypatch.setattr(im, "Harness", harness)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    with pytest.raises(Stop):
        im.main(["--hip_image"])
    assert seen["hip_image"] is True and seen["hip_mel"] is False and seen["hip_vision"] is False
    with pytest.raises(Stop):
        im.main(["--hip_vision"])
    assert seen["hip_image"] is False and seen["hip_vision"] is True
    monkeypatch.undo()
    # the conditioner installs the patch on its processor
    ip = IR.StubImageProcessor()
    proc = IR.StubProcessor(ip)
    bare = torch.nn.Linear(2, 2)
    cond = im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc, hip_image=True)
    assert isinstance(cond.image, handoff.HipImage) and proc.image_processor is not ip and cond.mel is None and cond.vision is None
    cond.image.remove()
    assert proc.image_processor is ip
    assert im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc).image is None and proc.image_processor is ip
