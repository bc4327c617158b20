"""The Qwen2.5-VL image front end without a GPU: the routing and counters of handoff.HipQwenImage around the library's Pillow image
processor (every route that ends at the original runs here), and the wiring of QwenVLConditioner(hip_image=True),
MultiTurnConditioner(hip_image=True) and --hip_image."""
import numpy as np
import pytest
import torch

PIL_Image = pytest.importorskip("PIL.Image")
MOD = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")


class _Processor:
    def __init__(self, image_processor):
        self.image_processor = image_processor


def _image(w, h, seed=0):
    return PIL_Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8))


def test_hip_qwen_image_installs_forwards_attributes_and_restores():
    from x2i_amd import handoff
    ip = MOD.Qwen2VLImageProcessorPil()
    proc = _Processor(ip)
    hi = handoff.HipQwenImage(proc, device="cpu")
    assert proc.image_processor is ip and (hi.calls, hi.fallbacks, hi.last_reason) == (0, 0, None) and hi.tower is None
    assert (hi.front.min_pixels, hi.front.max_pixels) == (56 * 56, 28 * 28 * 1280)
    assert hi.install() is hi and hi.install() is hi and proc.image_processor is not ip
    assert proc.image_processor.patch_size == 14 and proc.image_processor.image_mean == ip.image_mean
    assert proc.image_processor.get_number_of_image_patches(128, 128) == 100
    hi.remove()
    hi.remove()
    assert proc.image_processor is ip
    with pytest.raises(RuntimeError, match="no Qwen2.5-VL image processor"):
        handoff.HipQwenImage(object())
    with pytest.raises(ValueError, match="merge_size"):
        handoff.HipQwenImage(_Processor(MOD.Qwen2VLImageProcessorPil(merge_size=1)), device="cpu")
    with pytest.raises(ValueError, match="resample"):
        handoff.HipQwenImage(_Processor(MOD.Qwen2VLImageProcessorPil(resample=2)), device="cpu")


def test_every_refused_call_goes_whole_to_the_original_with_its_reason():
    from x2i_amd import handoff
    ip = MOD.Qwen2VLImageProcessorPil()
    proc = _Processor(ip)
    rgb, grey = _image(112, 112), _image(64, 64).convert("L")      # 112 = 4 x 28: do_resize=False is valid
    with handoff.HipQwenImage(proc, device="cpu") as hi:
        call = proc.image_processor
        for n, (kw, reason) in enumerate([
                (dict(images=[rgb, grey]), "not an RGB image"), (dict(images=[rgb], do_resize=False), "do_resize"),
                (dict(images=[rgb], size={"shortest_edge": 784, "longest_edge": 3136}), "size"), (dict(images=[rgb], resample=2), "resample"),
                (dict(images=[rgb], patch_size=16), "patch_size"), (dict(images=[rgb], image_mean=[0.5, 0.5, 0.5]), "image_mean"),
                (dict(images=[np.zeros((64, 64, 3), dtype=np.float32)]), "not an RGB image"), (dict(images=[]), "empty")], 1):
            try:
                got = call(return_tensors="pt", **kw)
                want = ip(return_tensors="pt", **kw)
                assert torch.equal(got["pixel_values"], want["pixel_values"]) and torch.equal(got["image_grid_thw"], want["image_grid_thw"])
            except (ValueError, TypeError, IndexError):         # what the original itself makes of such a call
                assert "empty" in reason
            assert (hi.calls, hi.fallbacks) == (0, n) and reason in hi.last_reason, (kw.keys(), hi.last_reason)
        with pytest.raises(TypeError):
            call(images=[rgb], videos=[[rgb, rgb]], return_tensors="pt")
        assert "videos" in hi.last_reason
        with pytest.raises(ValueError, match="aspect ratio"):
            call(images=[_image(2100, 10)], return_tensors="pt")
        assert "aspect ratio" in hi.last_reason and hi.calls == 0
        # a call that IS served reaches the front end, which has no CPU path: an error, never a quiet fallback
        with pytest.raises(Exception, match="GPU only"):
            call(images=[rgb, rgb], return_tensors="pt", do_resize=True, size=dict(ip.size), videos=None)
        assert hi.calls == 1
    assert proc.image_processor is ip


def test_hip_image_flag_parses_and_reaches_the_qwen_conditioners(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_multi_turn as mt, inference_qwenvl as iq
    from x2i_amd.infer.harness import build_parser
    p = build_parser("qwenvl")
    assert p.parse_args(["--synthetic"]).hip_image is False and p.parse_args(["--synthetic", "--hip_image", "--hip_vision"]).hip_image is True
    text = " ".join(p.format_help().split())
    assert "Qwen2VLImageProcessor" in text and "x2i_amd/qwen_image.py" in text and "x2i_image_rows.h" in text
    seen = {}

    class Cond:
        def __init__(self, path, device, *a, **kw):
            seen.update(kw)

    class Stop(Exception):
        pass

    def harness(*a, **kw):
        raise Stop

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for mod, name in ((iq, "QwenVLConditioner"), (mt, "MultiTurnConditioner")):
        monkeypatch.setattr(mod, name, Cond)
        monkeypatch.setattr(mod, "Harness", harness)
        for flags, want in ((["--hip_image"], True), ([], False)):
            seen.clear()
            with pytest.raises(Stop):
                mod.main(flags + ["--qwen_path", "nowhere"])
            assert seen["hip_image"] is want
    monkeypatch.undo()
    ip = MOD.Qwen2VLImageProcessorPil()
    proc = _Processor(ip)
    cond = iq.QwenVLConditioner(None, "cpu", prefill_only=False, model=torch.nn.Linear(2, 2), processor=proc, hip_image=True)
    assert isinstance(cond.image, handoff.HipQwenImage) and cond.image.tower is None and cond.vision is None and proc.image_processor is not ip
    cond.image.remove()
    assert iq.QwenVLConditioner(None, "cpu", prefill_only=False, model=torch.nn.Linear(2, 2), processor=proc).image is None
    cond = mt.MultiTurnConditioner(None, "cpu", model=torch.nn.Linear(2, 2), processor=proc, hip_image=True)
    assert isinstance(cond.image, handoff.HipQwenImage) and proc.image_processor is not ip
    cond.image.remove()
    assert proc.image_processor is ip and mt.MultiTurnConditioner(None, "cpu", model=object(), processor=proc).image is None
