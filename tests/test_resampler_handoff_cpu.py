"""The wiring of the MiniCPM-o Resampler's hand-off without a GPU: --hip_resampler, MiniCPMConditioner(hip_resampler=True) and
handoff.HipResampler's install / remove on a stub model."""
import pytest
import torch

from tests import resampler_ref as RR


def _stub():
    model = torch.nn.Module()
    model.vpm = torch.nn.Linear(2, 2)
    model.resampler = RR.LibraryResampler(8, 256, 2, 64)
    model.resampler.load_state_dict(RR.random_state_dict(8, 256, 64, 3), strict=True)
    return model


def test_flag_parses_and_defaults_to_off():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("minicpm")
    assert p.parse_args(["--synthetic"]).hip_resampler is False
    a = p.parse_args(["--synthetic", "--hip_resampler"])
    assert a.hip_resampler is True and a.hip_vision is False and a.hip_decoder is False and a.hip_generate is False
    b = p.parse_args(["--synthetic", "--hip_vision"])
    assert b.hip_vision is True and b.hip_resampler is False
    text = " ".join(p.format_help().split())
    assert "--hip_resampler" in text and "model.resampler" in text


def test_find_resampler():
    from x2i_amd import handoff
    model = _stub()
    assert handoff.find_resampler(model) is model.resampler
    bare = torch.nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="resampler"):
        handoff.find_resampler(bare)
    with pytest.raises(RuntimeError, match="resampler"):
        handoff.HipResampler(bare)


def test_flag_reaches_the_conditioner_and_install(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_minicpm as im
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
        im.main(["--hip_resampler"])
    assert seen["hip_resampler"] is True and seen["hip_vision"] is False
    with pytest.raises(Stop):
        im.main(["--hip_vision"])
    assert seen["hip_resampler"] is False and seen["hip_vision"] is True
    monkeypatch.undo()
    # the conditioner reaches HipResampler.install() on a stub model
    model = _stub()
    res = model.resampler
    cond = im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=model, hip_resampler=True)
    assert isinstance(cond.resampler, handoff.HipResampler) and res.__dict__["forward"] == cond.resampler._forward and cond.vision is None
    assert "forward" not in model.vpm.__dict__
    cond.resampler.remove()
    assert "forward" not in res.__dict__
    with pytest.raises(RuntimeError, match="resampler"):
        im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=torch.nn.Linear(2, 2), hip_resampler=True)


def test_hip_vision_alone_installs_no_resampler(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_minicpm as im

    class FakeSiglip:
        def __init__(self, model):
            self.model = model

        def install(self):
            self.installed = True
            return self
    monkeypatch.setattr(handoff, "HipSiglip", FakeSiglip)
    model = _stub()
    cond = im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=model, hip_vision=True)
    assert cond.vision.installed and cond.resampler is None and "forward" not in model.resampler.__dict__
    assert im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=model).resampler is None


def test_install_remove_restore_what_was_there():
    from x2i_amd import handoff
    model = _stub()
    res = model.resampler
    hr = handoff.HipResampler(model)
    assert hr.calls == 0 and "forward" not in res.__dict__ and hr.resampler.num_queries == 8
    with hr:
        assert res.__dict__["forward"] == hr._forward
    assert "forward" not in res.__dict__
    with pytest.raises(KeyError):
        with hr:
            raise KeyError("inside")
    assert "forward" not in res.__dict__
    mine = lambda *a, **k: None
    res.forward = mine
    hr.install().install()
    hr.remove()
    assert res.__dict__["forward"] is mine
