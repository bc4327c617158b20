"""The MiniCPM-o Whisper audio tower without a GPU: the parameter names and the packed storage of x2i_amd/whisper.py, the plan's arithmetic,
every refusal, the extension header include/x2i_whisper.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and the wiring of handoff.HipAudio,
MiniCPMConditioner(hip_audio=True) and --hip_audio."""
import ctypes as C

import pytest
import torch

from tests import whisper_ref as WR

TINY = dict(d_model=128, encoder_attention_heads=2, encoder_ffn_dim=256, encoder_layers=2, max_source_positions=150, embed_dim=96, pool_step=2)


def _tiny(**kw):
    from x2i_amd.whisper import WhisperAudioTower
    f = dict(TINY, device="cpu")
    f.update(kw)
    return WhisperAudioTower(**f)


def _lib_and_sd(seed):
    cfg, apm, proj = WR.library_tower(128, 2, 256, 2, 150, 96)
    sd = WR.random_state_dict(apm, proj, seed)
    WR.load_state_dict_into(apm, proj, sd)
    return cfg, apm, proj, sd


# ---------------------------------------------------------------------------------------------------------------- names and packed storage
def test_state_dict_names_are_the_checkpoints_and_load_strictly():
    cfg, apm, proj, want = _lib_and_sd(seed=2)
    tower = _tiny()
    sd = tower.state_dict()
    assert set(sd) == set(want) and all(sd[k].shape == want[k].shape for k in sd)
    for name in ("apm.conv1.weight", "apm.conv2.bias", "apm.embed_positions.weight", "apm.layers.1.self_attn.q_proj.bias",
                 "apm.layers.1.self_attn.k_proj.weight", "apm.layers.0.self_attn.v_proj.bias", "apm.layers.0.self_attn.out_proj.weight",
                 "apm.layers.0.self_attn_layer_norm.bias", "apm.layers.1.fc1.weight", "apm.layers.1.fc2.bias", "apm.layers.1.final_layer_norm.weight",
                 "apm.layer_norm.weight", "audio_projection_layer.linear1.weight", "audio_projection_layer.linear2.bias"):
        assert name in sd, name
    assert "apm.layers.0.self_attn.k_proj.bias" not in sd and sd["apm.embed_positions.weight"].shape == (150, 128)
    tower.load_state_dict({k: v.bfloat16() for k, v in want.items()}, strict=True)
    assert all(torch.equal(v.float(), want[k]) for k, v in tower.state_dict().items())
    with pytest.raises(RuntimeError):
        tower.load_state_dict({k: v for k, v in want.items() if k != "apm.layers.1.self_attn.v_proj.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        tower.load_state_dict(dict(want, **{"apm.layers.1.self_attn.k_proj.bias": torch.zeros(128)}), strict=True)
    with pytest.raises(ValueError, match="assign"):
        tower.load_state_dict(want, assign=True)
    # from_hf copies instantiated modules
    from x2i_amd.whisper import WhisperAudioTower
    copy = WhisperAudioTower.from_hf(apm, proj, 5)
    assert copy.device.type == "cpu" and copy.config.pool_step == 5 and copy.config.embed_dim == 96 and copy.config.encoder_layers == 2
    assert copy.config.max_source_positions == 150 and not copy.training
    assert all(torch.equal(v.float(), want[k]) for k, v in copy.state_dict().items()) and torch.equal(copy._conv2, tower._conv2)


def test_conv2_permutation_zero_k_bias_and_padded_conv1_are_pinned():
    cfg, apm, proj, want = _lib_and_sd(seed=3)
    tower = _tiny()
    tower.load_state_dict({k: v.bfloat16() for k, v in want.items()}, strict=True)
    D = 128
    # conv2: column k * D + ci of the packed matrix is weight[:, ci, k] -- the order of three consecutive token-major rows
    w2 = want["apm.conv2.weight"].bfloat16()
    assert tower._conv2.shape == (D, 3 * D) and tower._conv2.is_contiguous()
    for k in range(3):
        assert torch.equal(tower._conv2[:, k * D:(k + 1) * D], w2[:, :, k])
    # q | k | v: views of one weight and one bias whose k slice is zero
    for i in range(2):
        w, b = tower._fused["%d.qkv.w" % i], tower._fused["%d.qkv.b" % i]
        att = tower.apm.layers[i].self_attn
        assert w.shape == (3 * D, D) and b.shape == (3 * D,) and not bool(b[D:2 * D].any()) and not hasattr(att.k_proj, "bias")
        for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
            assert getattr(att, nm).weight.data_ptr() == w[j * D:].data_ptr()
            assert torch.equal(w[j * D:(j + 1) * D].float(), want["apm.layers.%d.self_attn.%s.weight" % (i, nm)])
        assert torch.equal(b[:D].float(), want["apm.layers.%d.self_attn.q_proj.bias" % i]) and att.v_proj.bias.data_ptr() == b[2 * D:].data_ptr()
    # conv1: the first 240 columns of a [D, 256] matrix, (ci, k) order, zero tail
    c1 = tower._fused["c1"]
    assert tower.Kp == 256 and c1.shape == (D, 256) and not bool(c1[:, 240:].any()) and tower.apm.conv1.weight.data_ptr() == c1.data_ptr()
    assert torch.equal(c1[:, :240].float(), want["apm.conv1.weight"].reshape(D, 240))
    # _apply re-points the views and makes the permuted copy again; a parameter written in place needs pack_()
    before = tower._conv2
    t2 = tower.to(torch.bfloat16)
    assert t2.apm.layers[1].self_attn.v_proj.weight.data_ptr() == t2._fused["1.qkv.w"][2 * D:].data_ptr()
    assert t2._conv2 is not before and torch.equal(t2._conv2, before)
    with torch.no_grad():
        tower.apm.conv2.weight.zero_()
    assert not bool(tower.pack_()._conv2.any())


# ---------------------------------------------------------------------------------------------------------------- plan
def test_plan_arithmetic():
    tower = _tiny()
    p = tower.plan([260, 90], 260, 50)
    assert (p.B, p.T, p.S, p.Spad, p.n_max, p.counts, p.chunk_frames) == (2, 260, 130, 192, 65, [65, 22], 50) and not hasattr(p, "ws")
    assert p.ids.tolist() == list(range(130)) * 2 and p.ids.dtype == torch.int32 and not bool(p.row_lo.any())
    # the mel length 90 meets post-conv indices: sample 1 sees 90 of its 45 real rows' worth of keys, as in the model
    assert p.key_hi[0].tolist() == [50] * 50 + [100] * 50 + [130] * 30 and p.key_hi[1].tolist() == [50] * 50 + [90] * 80
    assert torch.equal(p.row_hi, p.key_hi) and p.row_hi.dtype == torch.int32 and p.row_hi.is_contiguous()
    q = tower.plan(torch.tensor([7]), 7, 0)
    assert (q.S, q.Spad, q.n_max, q.counts) == (4, 64, 2, [2]) and q.key_hi.tolist() == [[4] * 4]
    assert tower.plan([1], 1).S == 1 and tower.plan([1], 1).counts == [0] and tower.plan([1], 1).n_max == 0
    assert tower.plan([299], 299).S == 150
    odd = _tiny(pool_step=5).plan([11, 23], 23, 3)
    assert (odd.S, odd.n_max, odd.counts) == (12, 2, [1, 2]) and odd.key_hi[0].tolist() == [3, 3, 3, 6, 6, 6, 9, 9, 9, 11, 11, 11]


def test_refusals():
    tower = _tiny()
    with pytest.raises(ValueError, match="beyond the 150 rows of embed_positions"):
        tower.plan([301], 301)
    with pytest.raises(ValueError, match="at least one"):
        tower.plan([1], 0)
    for lens in ([], [0], [8], [7, -1]):
        with pytest.raises(ValueError, match="feature_lens"):
            tower.plan(lens, 7)
    for bad, msg in ((dict(dtype=torch.float16), "bf16"), (dict(d_model=192), "64 wide"), (dict(encoder_attention_heads=4), "64 wide"),
                     (dict(encoder_layers=0), "layer"), (dict(activation_function="relu"), "gelu"), (dict(pool_step=0), "pool_step"),
                     (dict(pool_step=9), "pool_step"), (dict(embed_dim=100), "multiples of 8")):
        with pytest.raises(ValueError, match=msg):
            _tiny(**bad)
    with pytest.raises(TypeError, match="unknown"):
        _tiny(depth=2)
    with pytest.raises(ValueError, match="bf16"):
        _tiny().float()
    with pytest.raises(ValueError, match="eval-only"):
        tower.train()
    assert tower.eval() is tower and not tower.training
    mel = torch.zeros((2, 80, 7))
    with pytest.raises(ValueError, match="plan is for"):
        tower(mel, plan=tower.plan([7], 7))
    with pytest.raises(ValueError, match="plan is for"):
        tower(mel, plan=tower.plan([9, 9], 9))
    with pytest.raises(ValueError, match="GPU only"):
        tower(mel, plan=tower.plan([7, 7], 7))
    with pytest.raises(ValueError, match="mel must be"):
        tower(torch.zeros((2, 81, 7)))
    with pytest.raises(ValueError, match="at least one"):
        tower(torch.zeros((2, 80, 0)))
    with pytest.raises(ValueError, match="feature_lens for"):
        tower(mel, feature_lens=[7])


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import whisper_ops
    lib = whisper_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    rows = lambda **kw: lib.x2i_whisper_mel_rows_bf16(*[kw.get(k, d) for k, d in (
        ("mel", fake), ("mbs", 80 * 260), ("mld", 260), ("Xr", fake), ("ldx", 256), ("B", 2), ("Cin", 80), ("T", 260), ("Kp", 256), ("st", None))])
    assert rows(B=0) < 0 and rows(Cin=0) < 0 and rows(T=0) < 0 and b"T=0" in err()
    assert rows(B=70000) < 0 and b"B=70000" in err()
    assert rows(Kp=232, ldx=232) < 0 and b"Kp=232" in err()      # < 3 * Cin
    assert rows(Kp=244) < 0 and b"Kp=244" in err()              # not a multiple of 8
    assert rows(ldx=248) < 0 and b"ldx" in err()                # < Kp
    assert rows(ldx=260) < 0 and b"ldx" in err()
    assert rows(mld=259) < 0 and b"mel_ld" in err()             # < T
    assert rows(mbs=80 * 260 - 1) < 0 and b"mel_batch_stride" in err()
    assert rows(Xr=C.c_void_p(0x1008)) < 0 and b"aligned" in err()
    assert rows(mel=C.c_void_p(0x1001)) < 0 and b"aligned" in err()
    for k in ("mel", "Xr"):
        assert rows(**{k: None}) < 0 and b"null" in err()
    pool = lambda **kw: lib.x2i_whisper_pool_rows_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("xbs", 131 * 96), ("ldx", 96), ("Y", fake), ("ybs", 65 * 96), ("ldy", 96), ("B", 2), ("S", 131), ("D", 96), ("k", 2), ("st", None))])
    assert pool(k=0) < 0 and b"k=0" in err()
    assert pool(k=9) < 0 and b"k=9" in err()
    assert pool(S=1) < 0 and b"S=1" in err()                    # S < k
    assert pool(D=100, ldx=104, ldy=104, xbs=131 * 104, ybs=65 * 104) < 0 and b"D=100" in err()
    assert pool(B=0) < 0 and pool(D=0) < 0
    assert pool(ldx=88) < 0 and b"ldx" in err()
    assert pool(ldy=100) < 0 and pool(ldy=88) < 0
    assert pool(xbs=131 * 96 - 8) < 0 and pool(ybs=65 * 96 - 8) < 0 and pool(xbs=131 * 96 + 4) < 0 and pool(ybs=65 * 96 + 4) < 0
    assert pool(X=C.c_void_p(0x1008)) < 0 and b"aligned" in err() and pool(Y=C.c_void_p(0x1008)) < 0
    for k in ("X", "Y"):
        assert pool(**{k: None}) < 0 and b"null" in err()


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_hip_audio_flag_parses_and_reaches_the_conditioner(monkeypatch):
    from x2i_amd.infer import inference_minicpm as im
    from x2i_amd.infer.harness import build_parser
    p = build_parser("minicpm")
    assert p.parse_args(["--synthetic"]).hip_audio is False
    a = p.parse_args(["--synthetic", "--task", "audio2image", "--hip_audio"])
    assert a.hip_audio is True and a.hip_vision is False and a.hip_resampler is False and a.hip_decoder is False
    b = p.parse_args(["--synthetic", "--hip_vision", "--hip_resampler", "--hip_audio", "--full_generate"])
    assert b.hip_audio and b.hip_vision and b.hip_resampler and b.full_generate
    text = " ".join(p.format_help().split())
    assert "--hip_audio" in text and "model.apm" in text and "get_audio_embedding" in text
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
        im.main(["--hip_audio"])
    assert seen["hip_audio"] is True and seen["hip_vision"] is False and seen["hip_resampler"] is False
    with pytest.raises(Stop):
        im.main(["--hip_vision"])
    assert seen["hip_audio"] is False


def _stand_in(k=2):
    cfg, apm, proj, sd = _lib_and_sd(seed=4)
    return WR.StandInModel(apm, proj, k)


def test_find_apm_and_hip_audio_install_remove_without_a_gpu():
    """install / remove swap `get_audio_embedding` on the instance and restore what was there (nothing, or an earlier instance attribute);
    what the HIP tower does not serve goes to the original"""
    from x2i_amd import handoff
    from x2i_amd.infer.inference_minicpm import MiniCPMConditioner
    model = _stand_in()
    assert handoff.find_apm(model) is model.apm
    bare = torch.nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="apm"):
        handoff.find_apm(bare)
    with pytest.raises(RuntimeError, match="apm"):
        handoff.HipAudio(bare)
    with pytest.raises(RuntimeError, match="apm"):
        MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, hip_audio=True)
    assert MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare).audio is None
    half = torch.nn.Module()
    half.apm = model.apm
    with pytest.raises(RuntimeError, match="audio_projection_layer"):
        handoff.HipAudio(half)
    ha = handoff.HipAudio(model)
    assert ha.calls == 0 and ha.tower.config.pool_step == 2 and ha.tower.config.embed_dim == 96 and "get_audio_embedding" not in model.__dict__
    with ha:
        assert model.__dict__["get_audio_embedding"] == ha._get_audio_embedding
        assert model.get_audio_embedding({"audio_features": [], "audio_feature_lens": []}) == [] and model.get_audio_embedding({}, chunk_length=1.0) == []
        assert ha.calls == 0 and model.original_calls == 0            # no audio: served here, and no tower call
        # not served: another hidden state, or training -- the original runs
        model.audio_encoder_layer = -2
        assert model.get_audio_embedding({}) == [] and model.original_calls == 1
        model.audio_encoder_layer = -1
        model.training = True
        assert len(model.get_audio_embedding({}, dummy=True)) == 1 and model.original_calls == 2 and ha.calls == 0
        model.training = False
    assert "get_audio_embedding" not in model.__dict__
    with pytest.raises(KeyError):
        with ha:
            raise KeyError("inside")
    assert "get_audio_embedding" not in model.__dict__
    cond = MiniCPMConditioner(None, "cpu", prefill_only=False, model=model, hip_audio=True)      # reaches HipAudio.install()
    assert isinstance(cond.audio, handoff.HipAudio) and model.__dict__["get_audio_embedding"] == cond.audio._get_audio_embedding
    assert cond.vision is None and cond.resampler is None
    cond.audio.remove()
    mine = lambda *a, **k: None
    model.get_audio_embedding = mine
    ha.install().install()
    ha.remove()
    assert model.__dict__["get_audio_embedding"] is mine
    # the pooling step is read off the pooler when the config has none
    del model.get_audio_embedding
    model.config = None
    model.audio_avg_pooler = torch.nn.AvgPool1d(5, stride=5)
    assert handoff.HipAudio(model).tower.config.pool_step == 5
