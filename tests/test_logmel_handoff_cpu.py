"""The log-mel front end without a GPU: LogMel's tables, plan arithmetic and refusals (x2i_amd/logmel.py), and the wiring of
handoff.HipLogMel, MiniCPMConditioner(hip_mel=True) and --hip_mel around a stub processor that consumes the feature extractor the way the
MiniCPM-o processor does.  LogMel.__call__ is replaced by the float64 reference here; the kernels are tested in tests/test_logmel_gpu.py."""
import numpy as np
import pytest
import torch

from tests import logmel_ref as LR


class StubProcessor:
    """The audio part of the MiniCPM-o processor: the extractor's call, the slice by the mask's sums, transpose, pad_sequence"""

    def __init__(self, feature_extractor):
        self.feature_extractor = feature_extractor

    def audio_features(self, waves, **kwargs):
        inputs = self.feature_extractor(waves, sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt", **kwargs)
        feats, lens = inputs["input_features"], inputs["attention_mask"].sum(dim=1)
        assert lens.device.type == "cpu"
        kept = [f[:, :n].permute(1, 0) for f, n in zip(feats, lens)]
        return torch.nn.utils.rnn.pad_sequence(kept, batch_first=True, padding_value=0.0).permute(0, 2, 1), torch.hstack(list(lens))


def _extractor(**kw):
    from transformers import WhisperFeatureExtractor
    return WhisperFeatureExtractor(**kw)


def _reference_call(self, waves, out_dtype=torch.float32, T_out=None, plan=None):
    """What LogMel.__call__ returns, from the float64 reference (on the CPU)"""
    f = self.fbank[:201, :self.n_mels].double().numpy()
    Ls = [LR.kept_frames(len(w), self.n_samples) for w in waves]
    T_out = max(Ls) if T_out is None else T_out
    out = torch.zeros((len(waves), self.n_mels, T_out), dtype=out_dtype)
    for b, w in enumerate(waves):
        out[b, :, :Ls[b]] = torch.from_numpy(LR.ref64(np.asarray(w), self.n_samples, f)[1][:, :Ls[b]]).to(out_dtype)
    return out, Ls


# ---------------------------------------------------------------------------------------------------------------- LogMel on the host
def test_tables_and_from_hf():
    from x2i_amd import logmel as LM, logmel_binding as lb
    fe = _extractor()
    lm = LM.LogMel.from_hf(fe, "cpu")
    assert (lm.n_mels, lm.n_samples, lm.T) == (80, 480000, 3000) and lm.device.type == "cpu"
    assert tuple(lm.dft.shape) == lb.DFT_SHAPE and tuple(lm.fbank.shape) == lb.FBANK_SHAPE and lm.dft.dtype == lm.fbank.dtype == torch.float32
    assert torch.equal(lm.fbank[:201, :80], torch.from_numpy(LR.mel_filters(80))) and not bool(lm.fbank[201:].any()) and not bool(lm.fbank[:, 80:].any())
    cos, sin = LR.tables32()
    tab = lm.dft.reshape(400, 7, 2, 32)
    assert torch.equal(tab[:, :, 0].reshape(400, 224)[:, :201], cos) and torch.equal(tab[:, :, 1].reshape(400, 224)[:, :201], sin)
    assert not bool(tab[:, :, :, :].reshape(400, 7, 2, 32)[:, 6, :, 9:].any())           # bins 201 .. 223
    w = LM.hann_window()
    assert w[0] == 0.0 and w[200] == 1.0 and np.allclose(w, torch.hann_window(400, dtype=torch.float64).numpy(), atol=1e-15)
    assert LM.LogMel.from_hf(_extractor(feature_size=128), "cpu").n_mels == 128
    assert LM.LogMel.from_hf(_extractor(chunk_length=1), "cpu").T == 100


def test_from_hf_refusals_name_the_field():
    from x2i_amd.logmel import LogMel
    for kw, field in ((dict(n_fft=512), "n_fft"), (dict(hop_length=128), "hop_length"), (dict(sampling_rate=16050, chunk_length=1), "n_samples"),
                      (dict(feature_size=160), "feature_size"), (dict(dither=1e-4), "dither"), (dict(do_normalize=True), "do_normalize")):
        with pytest.raises(ValueError, match=field):
            LogMel.from_hf(_extractor(**kw), "cpu")
    with pytest.raises(ValueError, match="mel_filters"):
        LogMel(np.zeros((200, 80)), device="cpu")
    with pytest.raises(ValueError, match="n_samples"):
        LogMel(np.zeros((201, 80)), n_samples=1000, device="cpu")


def test_plan_and_call_refusals():
    from x2i_amd import logmel_binding as lb
    from x2i_amd.logmel import LogMel
    lm = LogMel.from_hf(_extractor(), "cpu")
    p = lm.plan(3, 1001)
    assert (p.B, p.ldw, p.head) == (3, 1004, 16) and p.stage.numel() == p.dev.numel() == 16 + 4 * 3 * 1004
    assert p.stage_n.dtype == torch.int32 and p.stage_n.shape == (3,) and p.stage_w.shape == p.wave.shape == (3, 1004)
    assert p.stage_w.data_ptr() == p.stage.data_ptr() + 16 and p.lg.numel() == 3 * 80 * 3000 and p.part.numel() == 3 * 94
    assert lm.lengths([1, 160, 161, 480000]) == [1, 1, 2, 3000]
    for bad in ((0, 10), (1, 0), (1, 480001)):
        with pytest.raises(ValueError, match="plan"):
            lm.plan(*bad)
    with pytest.raises(ValueError, match="n_samples = 480000"):
        lm([np.zeros(480001, dtype=np.float32)])
    with pytest.raises(ValueError, match="1-D float"):
        lm([np.zeros((2, 5), dtype=np.float32)])
    with pytest.raises(ValueError, match="1-D float"):
        lm([])
    with pytest.raises(ValueError, match="n_samples"):
        lm([np.zeros(0, dtype=np.float32)])
    with pytest.raises(ValueError, match="out_dtype"):
        lm([np.zeros(5, dtype=np.float32)], out_dtype=torch.float16)
    with pytest.raises(ValueError, match="plan is for"):
        lm([np.zeros(5, dtype=np.float32)], plan=p)
    with pytest.raises(lb.X2IError, match="GPU only"):       # no fallback
        lm([np.zeros(5, dtype=np.float32)])


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_hip_logmel_install_remove_and_forwarding(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.logmel import LogMel
    monkeypatch.setattr(LogMel, "__call__", _reference_call)
    fe = _extractor()
    proc = StubProcessor(fe)
    hm = handoff.HipLogMel(proc, device="cpu")
    assert hm.calls == 0 and proc.feature_extractor is fe and hm.logmel.n_mels == 80
    waves = [LR.six_signals()["clip"], LR.dropped_frame_case(1e-3), np.zeros(161, dtype=np.float32)]
    want, want_lens = proc.audio_features(waves)
    with hm:
        sub = proc.feature_extractor
        assert sub is not fe and sub.hop_length == 160 and sub.n_samples == 480000 and sub.model_input_names == ["input_features"]
        assert sub.mel_filters is fe.mel_filters and sub.nb_max_frames == 3000
        with pytest.raises(AttributeError):
            sub.no_such_field
        got, got_lens = proc.audio_features(waves)
        assert hm.calls == 1 and got.shape == want.shape == (3, 80, 7) and got.dtype == torch.float32
        assert got_lens.tolist() == want_lens.tolist() == [7, 6, 2]
        assert float((got - want).abs().max()) <= 1e-4 and bool((got[2, :, :2] == -1.5).all()) and not bool(got[2, :, 2:].any())
        full = sub(waves, sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt")
        assert full["input_features"].shape == (3, 80, 3000) and full["attention_mask"].shape == (3, 3000)
        assert full["attention_mask"].sum(dim=1).tolist() == [7, 6, 2] and hm.calls == 2
        # every other form of call is the original's
        ref = fe(waves, sampling_rate=16000, return_tensors="pt")
        for kw in (dict(sampling_rate=16000, return_tensors="pt"),
                   dict(sampling_rate=16000, return_attention_mask=True, padding="longest", return_tensors="pt"),
                   dict(sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="np"),
                   dict(sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt", truncation=False),
                   dict(return_attention_mask=True, padding="max_length", return_tensors="pt")):
            other = sub(waves, **kw)
            assert hm.calls == 2 and "input_features" in other
        assert torch.equal(sub(waves, sampling_rate=16000, return_tensors="pt")["input_features"], ref["input_features"])
        long = [np.zeros(480001, dtype=np.float32)]                  # the original truncates; LogMel would refuse
        assert sub(long, sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt")["input_features"].shape == (1, 80, 3000)
        assert sub([[0.0, 0.1]], sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt")["input_features"].shape[0] == 1
        assert hm.calls == 2
        with pytest.raises(ValueError, match="sampling rate"):
            sub(waves, sampling_rate=8000)
    assert proc.feature_extractor is fe
    with pytest.raises(KeyError):
        with hm:
            raise KeyError("inside")
    assert proc.feature_extractor is fe
    hm.install().install()
    assert proc.feature_extractor is not fe
    hm.remove()
    hm.remove()
    assert proc.feature_extractor is fe and proc.__dict__["feature_extractor"] is fe
    with pytest.raises(RuntimeError, match="feature_extractor"):
        handoff.HipLogMel(object())
    with pytest.raises(ValueError, match="n_fft"):
        handoff.HipLogMel(StubProcessor(_extractor(n_fft=512)), device="cpu")


def test_hip_mel_flag_parses_and_reaches_the_conditioner(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_minicpm as im
    from x2i_amd.infer.harness import build_parser
    p = build_parser("minicpm")
    assert p.parse_args(["--synthetic"]).hip_mel is False
    a = p.parse_args(["--synthetic", "--task", "audio2image", "--hip_mel"])
    assert a.hip_mel is True and a.hip_audio is False
    b = p.parse_args(["--synthetic", "--hip_mel", "--hip_audio"])
    assert b.hip_mel and b.hip_audio
    text = " ".join(p.format_help().split())
    assert "--hip_mel" in text and "WhisperFeatureExtractor" in text and "x2i_amd/logmel.py" in text
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
        im.main(["--hip_mel"])
    assert seen["hip_mel"] is True and seen["hip_audio"] is False
    with pytest.raises(Stop):
        im.main(["--hip_audio"])
    assert seen["hip_mel"] is False and seen["hip_audio"] is True
    monkeypatch.undo()
    # the conditioner installs the patch on its processor
    proc = StubProcessor(_extractor())
    fe = proc.feature_extractor
    bare = torch.nn.Linear(2, 2)
    cond = im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc, hip_mel=True)
    assert isinstance(cond.mel, handoff.HipLogMel) and proc.feature_extractor is not fe and cond.audio is None
    cond.mel.remove()
    assert proc.feature_extractor is fe
    assert im.MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, processor=proc).mel is None and proc.feature_extractor is fe
