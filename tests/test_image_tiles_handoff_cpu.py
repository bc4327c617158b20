"""The tiled image front ends without a GPU: the routing and counters of handoff.HipImage(slices=...) around stand-in processors
(tests/image_tiles_ref.py: SlicingStubImageProcessor, whose grid is the processor's real one), --max_slice_nums and the conditioners'
wiring, and the refusals of InternVLImageFrontEnd.  ImageFrontEnd.__call__ and .sliced are replaced by the numpy reference here; the
kernels are tested in tests/test_image_tiles_gpu.py."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import image_ref as IR
from tests import image_tiles_ref as TR


def _reference_sliced(self, frames, max_slice_nums=9, out_dtype=torch.float32, plan=None):
    """What ImageFrontEnd.sliced returns, from the numpy reference (on the CPU)"""
    values, tgt = [], []
    for a in self._as_arrays(frames):
        pv, _, t = TR.minicpm_preprocess([a], max_slice_nums, scale_resolution=self.scale_resolution)
        values.append([torch.from_numpy(p).to(out_dtype) for p in pv])
        tgt.append(t)
    return values, tgt


def _reference_call(self, frames, out_dtype=torch.float32, plan=None):
    values, tgt = _reference_sliced(self, frames, 1, out_dtype)
    return [v[0] for v in values], np.vstack(tgt)


def _image(w, h, seed=0, mode="RGB"):
    return Image.fromarray(IR.edge_frames(w, h, 1, seed=seed)[0]).convert(mode)


@pytest.fixture
def patched(monkeypatch):
    from x2i_amd.image import ImageFrontEnd
    monkeypatch.setattr(ImageFrontEnd, "__call__", _reference_call)
    monkeypatch.setattr(ImageFrontEnd, "sliced", _reference_sliced)


def _equal_features(got, want):
    assert type(got) is type(want) is IR.StubBatchFeature and list(got.keys()) == list(want.keys()) == ["pixel_values", "image_sizes", "tgt_sizes"]
    assert [len(g) for g in got["pixel_values"]] == [len(g) for g in want["pixel_values"]]
    for g, w in zip(got["pixel_values"], want["pixel_values"]):
        assert all(x is not None and x.dtype == torch.float32 and torch.equal(x, y) for x, y in zip(g, w))
    for key in ("image_sizes", "tgt_sizes"):
        for g, w in zip(got[key], want[key]):
            if isinstance(w, list):
                assert len(g) == len(w) and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(g, w))
            else:
                assert torch.equal(g, w) and g.dtype == w.dtype


def test_the_default_still_sends_a_sliced_call_to_the_original(patched):
    from x2i_amd import handoff
    ip = TR.SlicingStubImageProcessor()
    proc = IR.StubProcessor(ip)
    small, big = _image(97, 61, 1), _image(640, 480, 2)
    for hi in (handoff.HipImage(proc, device="cpu"), handoff.HipImage(proc, device="cpu", slices=False)):
        assert hi.slices is False
        with hi:
            before = ip.calls
            out = proc.image_inputs([[small, big]], max_slice_nums=9)
            assert (hi.calls, hi.fallbacks, hi.last_reason, ip.calls) == (0, 1, "an image that is sliced", before + 1)
            assert len(out["pixel_values"][0]) == 4                      # the original's own slices: 1 + (1 + 2)
            proc.image_inputs([[small, big]], max_slice_nums=1)
            assert (hi.calls, hi.fallbacks, ip.calls) == (1, 1, before + 1)


def test_slices_true_serves_sliced_images_in_the_originals_form(patched):
    from x2i_amd import handoff
    ip = TR.SlicingStubImageProcessor()
    proc = IR.StubProcessor(ip)
    a, b, c = _image(97, 61, 1), _image(640, 480, 2), _image(500, 402, 3)
    want9 = proc.image_inputs([[a, b], [c]], max_slice_nums=9)
    want2 = proc.image_inputs([[b, a]], max_slice_nums=2)
    want1 = proc.image_inputs([[a, b]], max_slice_nums=1)
    assert ip.calls == 3 and [len(g) for g in want9["pixel_values"]] == [4, 3]
    with handoff.HipImage(proc, device="cpu", slices=True) as hi:
        assert hi.slices is True and proc.image_processor.get_sliced_grid((640, 480), 9) == [2, 1]
        got = proc.image_inputs([[a, b], [c]], max_slice_nums=9)
        assert (hi.calls, hi.fallbacks, ip.calls) == (1, 0, 3)
        _equal_features(got, want9)
        assert got["tgt_sizes"][0].tolist() == [[25, 40], [28, 37], [39, 26], [39, 26]] and [tuple(t.tolist()) for t in got["image_sizes"][0]] == [(97, 61), (640, 480)]
        _equal_features(proc.image_inputs([[b, a]], max_slice_nums=2), want2)
        _equal_features(proc.image_inputs([[a, b]], max_slice_nums=1), want1)                    # nothing sliced: the existing path
        assert (hi.calls, hi.fallbacks, ip.calls) == (3, 0, 3)
        # max_slice_nums left out or None: the processor's own default, 9
        sub = proc.image_processor
        _equal_features(sub([[a, b], [c]], do_pad=True, return_tensors="pt"), want9)
        _equal_features(sub([[a, b], [c]], max_slice_nums=None, return_tensors="pt"), want9)
        assert (hi.calls, hi.fallbacks, ip.calls) == (5, 0, 3)
    assert proc.image_processor is ip


def test_slices_true_keeps_every_other_refusal(patched, monkeypatch):
    from x2i_amd import handoff
    ip = TR.SlicingStubImageProcessor()
    proc = IR.StubProcessor(ip)
    small, big = _image(97, 61, 1), _image(640, 480, 2)
    with handoff.HipImage(proc, device="cpu", slices=True) as hi:
        sub = proc.image_processor
        reasons = []

        def falls(images, **kw):
            before = (hi.calls, hi.fallbacks, ip.calls)
            out = sub(images, **kw)
            assert (hi.calls, hi.fallbacks, ip.calls) == (before[0], before[1] + 1, before[2] + 1) and "pixel_values" in out
            reasons.append(hi.last_reason)

        # mixed lists: one refused image sends the WHOLE call, sliced images included, to the original
        falls([[big, _image(97, 61, mode="L")]], max_slice_nums=9)
        falls([[big, small.convert("RGBA")]], max_slice_nums=9)
        falls([[np.asarray(big), small]], max_slice_nums=9)
        assert reasons == ["an input that is not an RGB image of 8 bits per channel"] * 3
        falls([[big, _image(900, 10)]], max_slice_nums=1)                     # a source image 302 patches wide
        assert "out_w=4228 must be a multiple of 14 in 14..980" in reasons[-1]
        falls([[big, _image(9000, 100)]], max_slice_nums=9)                   # sliced 9 x 1, and the source image is still too wide
        assert "must be a multiple of 14 in 14..980" in reasons[-1]
        monkeypatch.setattr(hi.front, "served", lambda w, h, m=1: "x2i_amd: the image front end's LDS plan does not fit: a stand-in")
        falls([[big]], max_slice_nums=9)
        assert "LDS plan does not fit" in reasons[-1]
        monkeypatch.undo()
        from x2i_amd.image import ImageFrontEnd
        monkeypatch.setattr(ImageFrontEnd, "__call__", _reference_call)
        monkeypatch.setattr(ImageFrontEnd, "sliced", _reference_sliced)
        falls([[big]], max_slice_nums=9, data_format="channels_first")
        falls([[big], []], max_slice_nums=9)
        assert reasons[-2:] == ["another form of call", "an empty or unknown batch"]
        # a processor whose grid is not the front end's (IR.StubImageProcessor's is [1, multiple]) is not served either
        monkeypatch.setattr(ip, "get_sliced_grid", lambda size, m, never_split=False: IR.StubImageProcessor.get_sliced_grid(ip, size, m))
        falls([[big]], max_slice_nums=9)
        assert reasons[-1] == "a slicing grid other than the front end's"
        monkeypatch.undo()
        monkeypatch.setattr(ImageFrontEnd, "__call__", _reference_call)
        monkeypatch.setattr(ImageFrontEnd, "sliced", _reference_sliced)
        assert hi.calls == 0 and hi.fallbacks == len(reasons) == 9
        proc.image_inputs([[big]], max_slice_nums=9)
        assert hi.calls == 1


def test_front_end_served_and_slice_plan_on_the_host():
    from x2i_amd import image_binding as ib
    from x2i_amd.image import ImageFrontEnd
    fe = ImageFrontEnd(device="cpu")
    assert fe.slice_plan(640, 480, 9) == ((518, 392), (2, 1), (364, 546)) and fe.slice_plan(640, 480, 1) == ((518, 392), None, None)
    assert fe.slice_plan(4000, 3000, 9) == ((518, 392), (3, 3), (518, 392)) and fe.slice_plan(97, 61, 9) == ((560, 350), None, None)
    assert fe.served(640, 480, 9) is None and fe.served(4000, 3000, 9) is None and fe.served(4000, 3000) is None
    assert "multiple of 14 in 14..980" in fe.served(9000, 100, 9) and "LDS plan does not fit" in fe.served(40000, 40000, 9)
    with pytest.raises(ValueError, match="max_slice_nums"):
        fe.sliced([np.zeros((20, 30, 3), dtype=np.uint8)], 0)
    with pytest.raises(ib.X2IError, match="GPU only"):       # no fallback
        fe.sliced([np.zeros((480, 640, 3), dtype=np.uint8)], 9)


def test_max_slice_nums_flag_reaches_the_conditioner_and_the_processor(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_minicpm as im
    from x2i_amd.infer.harness import build_parser
    p = build_parser("minicpm")
    assert p.parse_args(["--synthetic"]).max_slice_nums == 1 and p.parse_args(["--max_slice_nums", "9"]).max_slice_nums == 9
    text = " ".join(p.format_help().split())
    assert "--max_slice_nums" in text and "HipImage(slices=True)" in text and "x2i_image_tiles.h" in text
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
        im.main(["--hip_image", "--max_slice_nums", "9"])
    assert seen["hip_image"] is True and seen["max_slice_nums"] == 9
    with pytest.raises(Stop):
        im.main(["--hip_image"])
    assert seen["max_slice_nums"] == 1
    monkeypatch.undo()
    bare = torch.nn.Linear(2, 2)
    for n, slices in ((1, False), (9, True)):
        ip = TR.SlicingStubImageProcessor()
        proc = IR.StubProcessor(ip)
        cond = im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc, hip_image=True, max_slice_nums=n)
        assert isinstance(cond.image, handoff.HipImage) and cond.image.slices is slices and cond.max_slice_nums == n
        cond.image.remove()
    cond = im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc, max_slice_nums=9)
    assert cond.image is None and cond.max_slice_nums == 9 and proc.image_processor is ip
    with pytest.raises(ValueError, match="max_slice_nums"):
        im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc, max_slice_nums=0)
    # the processor is called with the conditioner's value
    import inspect
    assert "max_slice_nums=self.max_slice_nums" in inspect.getsource(im.MiniCPMConditioner.__call__)


def test_internvl_front_end_on_the_host():
    from x2i_amd import image_tiles_binding as itb
    from x2i_amd.internvl_image import InternVLImageFrontEnd
    fe = InternVLImageFrontEnd(device="cpu")
    assert fe.image_size == 448 and tuple(fe.lut.shape) == (3, 256) and fe.lut.dtype == torch.float32
    assert np.array_equal(fe.lut.numpy().view(np.int32), TR.torch_lut().view(np.int32))
    assert fe.grid(640, 480) == (4, 3) and fe.grid(1280, 720) == (4, 2) and fe.grid(97, 61) == (3, 2) and fe.grid(128, 128) == (1, 1)
    assert fe.grid(640, 480, 1) == (1, 1)
    with pytest.raises(ValueError, match="max_num"):
        fe.grid(640, 480, 13)
    with pytest.raises(ValueError, match="image_size"):
        InternVLImageFrontEnd(image_size=450, device="cpu")
    with pytest.raises(ValueError, match="mean and std"):
        InternVLImageFrontEnd(std=(1, 0, 1), device="cpu")
    ok = np.zeros((20, 30, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="non-empty"):
        fe.tiles([])
    with pytest.raises(ValueError, match="mode RGB"):
        fe.tiles([Image.fromarray(ok).convert("L")])
    with pytest.raises(ValueError, match="out_dtype"):
        fe.tiles([ok], out_dtype=torch.float16)
    with pytest.raises(itb.X2IError, match="LDS plan does not fit"):
        fe.tiles([np.zeros((60000, 4, 3), dtype=np.uint8)])
    with pytest.raises(itb.X2IError, match="GPU only"):       # no fallback
        fe.tiles([ok])


def test_internvl_conditioner_takes_the_flag_and_is_unchanged_without_it(monkeypatch, tmp_path):
    from x2i_amd import internvl_image
    from x2i_amd.infer import inference_internvl as ii
    from x2i_amd.infer.harness import build_parser
    a = build_parser("internvl").parse_args(["--synthetic", "--hip_image"])
    assert a.hip_image is True and build_parser("internvl").parse_args(["--synthetic"]).hip_image is False
    assert "x2i_amd/internvl_image.py" in " ".join(build_parser("internvl").format_help().split())
    made = []

    class Front:
        def __init__(self, image_size, device):
            made.append((image_size, device))

        def tiles(self, images, max_num, out_dtype):
            made.append(([im.size for im in images], max_num, out_dtype))
            return torch.zeros(len(images), 3, 448, 448, dtype=out_dtype), [1] * len(images)

    monkeypatch.setattr(internvl_image, "InternVLImageFrontEnd", Front)
    bare = torch.nn.Linear(2, 2)
    path = str(tmp_path / "a.png")
    arr = IR.edge_frames(97, 61, 1)[0]
    Image.fromarray(arr).save(path)
    plain = ii.InternVLConditioner(None, "cpu", prefill_only=False, model=bare, tokenizer=object())
    assert plain.image is None and not made
    got = plain.image_tiles([path])
    # what the conditioner computed before the flag existed, written out
    im = Image.open(path).convert("RGB").resize((128, 128)).resize((448, 448))
    t = torch.from_numpy(np.asarray(im)).float().div(255).permute(2, 0, 1)
    mean, std = torch.tensor([0.485, 0.456, 0.406])[:, None, None], torch.tensor([0.229, 0.224, 0.225])[:, None, None]
    want = torch.stack([(t - mean) / std]).to("cpu", torch.bfloat16)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (1, 3, 448, 448) and torch.equal(got, want)
    cond = ii.InternVLConditioner(None, "cpu", prefill_only=False, model=bare, tokenizer=object(), hip_image=True)
    assert isinstance(cond.image, Front) and made == [(448, "cpu")]
    out = cond.image_tiles([path, path])
    assert made[-1] == ([(128, 128), (128, 128)], 1, torch.bfloat16) and tuple(out.shape) == (2, 3, 448, 448)
