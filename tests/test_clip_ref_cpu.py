"""CPU-side checks of the CLIP text encoder work (no GPU): the float64 restatement of the model against the library in float64, the checkers
of tests/clip_ref.py against the mistakes they are there to catch, pooling known answers, the extension header include/x2i_clip.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and the host module's refusals and key spellings."""
import ctypes as C
import os

import pytest
import torch

from tests import clip_ref as CR


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
@pytest.mark.parametrize("eos_token_id", [2, 63])
def test_float64_restatement_equals_the_library_in_float64(eos_token_id):
    """hidden 128, 2 heads, 2 layers, ids [3, 77]; the largest id (eos_token_id 2) or the first eos (63) at positions 0, 40 and 76 of the
    three samples, so that a wrong gather index shows.  Bound 1e-9 (measured: a few 1e-15)."""
    cfg, lib = CR.library_model(128, 2, 2, 512, vocab=64, eos_token_id=eos_token_id)
    sd = CR.random_model_state_dict(lib, seed=3)
    lib = lib.double()
    lib.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ids = CR.ids_with_eos_at(3, 77, 64, (0, 40, 76), eos_token_id, seed=4)
    assert CR.pool_index(ids, eos_token_id).tolist() == [0, 40, 76]
    out = lib(ids, output_hidden_states=False)
    prefix = "text_model." if any(k.startswith("text_model.") for k in sd) else ""
    last, pooled = CR.model_reference(sd, ids, num_heads=2, eps=cfg.layer_norm_eps, eos_token_id=eos_token_id, prefix=prefix)
    e_last, e_pool = CR.rel_l2(last, out.last_hidden_state), CR.rel_l2(pooled, out.pooler_output)
    print("restatement vs library (eos %d): last_hidden_state %.3e, pooler_output %.3e" % (eos_token_id, e_last, e_pool))
    assert last.shape == out.last_hidden_state.shape == (3, 77, 128) and pooled.shape == out.pooler_output.shape == (3, 128)
    assert e_last <= 1e-9 and e_pool <= 1e-9
    assert float((last - out.last_hidden_state).abs().max()) <= 1e-9 * max(1.0, float(out.last_hidden_state.abs().max()))
    assert float(out.last_hidden_state.std()) > 0.1      # a live output, not a collapsed one
    # the three pooled rows are three different rows of the hidden state
    assert torch.equal(pooled, last[torch.arange(3), torch.tensor([0, 40, 76])])
    assert not torch.equal(pooled[1], last[1, 39]) and not torch.equal(pooled[1], last[1, 41])


# ---------------------------------------------------------------------------------------------------------------- the checkers reject
def _wrong_attention(Q, K, V, S, scale, kind):
    """float64 attention with one deliberate mistake in the mask"""
    f = torch.float64
    pos = torch.arange(S)
    rel = pos[None, :] - pos[:, None]           # key - query
    masked = {"none": rel > 0, "unmasked": rel > S, "strict": rel >= 0, "shifted": rel > 1}[kind]
    q, k, v = (t[:, :, :S].to(f) for t in (Q, K, V))
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(masked, float("-inf"))
    if kind == "strict":
        s[:, :, 0, 0] = 0.0                      # (row 0 would be empty: let it keep its one key)
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("kind", ["unmasked", "strict", "shifted"])
@pytest.mark.parametrize("S", [77, 300])
def test_attention_checker_rejects(kind, S):
    B, H, dk = 1, 2, 64
    Q, K, V = CR.attention_inputs(B, H, S, dk, seed=11)
    ref = CR.attention_reference(Q, K, V, S, dk ** -0.5)
    CR.check_attention("exact", _wrong_attention(Q, K, V, S, dk ** -0.5, "none"), ref)          # the restatement without a mistake passes
    CR.check_attention("bf16 output", ref.bfloat16(), ref)                                        # ... and so does one rounding of it
    with pytest.raises(AssertionError):
        CR.check_attention(kind, _wrong_attention(Q, K, V, S, dk ** -0.5, kind), ref)


def test_quick_gelu_checker_accepts_one_rounding_and_rejects_other_gelus_and_two_roundings():
    x = (2.0 * torch.randn((7, 256), generator=torch.Generator().manual_seed(6))).bfloat16()
    f32 = x.float() * torch.sigmoid(1.702 * x.float())
    assert CR.check_quick_gelu("one rounding", f32.bfloat16(), x) <= CR.TOL_ROW + 2.0 ** -19
    with pytest.raises(AssertionError):
        CR.check_quick_gelu("erf form", torch.nn.functional.gelu(x.double()).bfloat16(), x)
    with pytest.raises(AssertionError):
        CR.check_quick_gelu("tanh form", torch.nn.functional.gelu(x.double(), approximate="tanh").bfloat16(), x)
    with pytest.raises(AssertionError):     # the library's bf16 path: the sigmoid rounded to bf16, then the product
        CR.check_quick_gelu("two roundings", (x.float() * torch.sigmoid(1.702 * x.float()).bfloat16().float()).bfloat16(), x)


# ---------------------------------------------------------------------------------------------------------------- pooling
def test_pooling_known_answers():
    ids = torch.tensor([[5, 9, 9, 3], [9, 1, 9, 9], [0, 0, 0, 0], [1, 2, 7, 7]])
    assert CR.pool_index(ids, 2).tolist() == [1, 0, 0, 2]                    # ties go to the first maximum
    assert torch.equal(CR.pool_index(ids, 2), ids.to(torch.int).argmax(-1))  # ... as the library's argmax does
    ids = torch.tensor([[4, 6, 7, 7, 7], [7, 7, 7, 7, 7], [4, 5, 6, 8, 9], [9, 9, 9, 9, 7]])
    assert CR.pool_index(ids, 7).tolist() == [2, 0, 0, 4]                    # an eos followed by pad equal to eos; no eos gives 0
    assert torch.equal(CR.pool_index(ids, 7), (ids.to(torch.int) == 7).int().argmax(-1))


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import clip_ops
    lib = clip_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    att = lambda **kw: lib.x2i_clip_attention_bf16(*[kw.get(k, d) for k, d in (("Q", fake), ("K", fake), ("VT", fake), ("O", fake), ("B", 1), ("H", 2),
                                                   ("S", 77), ("Spad", 128), ("dk", 64), ("scale", 0.125), ("ldo", 128), ("obs", 77 * 128), ("st", None))])
    assert att(dk=32) < 0 and b"dk=32" in err()
    assert att(dk=128) < 0 and b"dk=128" in err()
    assert att(Spad=100) < 0 and b"Spad" in err()
    assert att(Spad=64) < 0 and b"Spad" in err()              # Spad < S
    assert att(ldo=64, obs=77 * 64) < 0 and b"H*dk" in err()  # ldo < H * dk
    assert att(ldo=130) < 0 and b"aligned" in err()
    for k in ("Q", "K", "VT", "O"):
        assert att(**{k: None}) < 0 and b"null" in err()
    assert att(scale=0.0) < 0 and b"scale" in err()
    assert lib.x2i_clip_embed_bf16(fake, fake, fake, fake, 2, 77, 100, 64, None) < 0 and b"D=100" in err()
    assert lib.x2i_clip_embed_bf16(None, fake, fake, fake, 2, 77, 128, 64, None) < 0 and b"null" in err()
    assert lib.x2i_clip_embed_bf16(fake, fake, fake, fake, 2, 77, 128, 0, None) < 0
    assert lib.x2i_clip_quick_gelu_bf16(fake, 12, fake, 12, 4, 12, None) < 0 and b"F=12" in err()
    assert lib.x2i_clip_quick_gelu_bf16(fake, 64, None, 64, 4, 64, None) < 0 and b"null" in err()
    assert lib.x2i_clip_quick_gelu_bf16(fake, 60, fake, 64, 4, 64, None) < 0 and b"strides" in err()
    assert lib.x2i_clip_pool_bf16(fake, fake, 100, fake, 100, 2, 77, 100, 2, None) < 0 and b"D=100" in err()
    assert lib.x2i_clip_pool_bf16(fake, None, 128, fake, 128, 2, 77, 128, 2, None) < 0 and b"null" in err()
    assert lib.x2i_clip_pool_bf16(fake, fake, 64, fake, 128, 2, 77, 128, 2, None) < 0 and b"strides" in err()


# ---------------------------------------------------------------------------------------------------------------- host module
OK = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=1, vocab_size=16, max_position_embeddings=77, device="cpu")


def test_unsupported_configurations_and_arguments_raise():
    from x2i_amd._lib import X2IError
    from x2i_amd.clip import CLIPTextModel
    for bad in (dict(hidden_act="gelu"), dict(num_attention_heads=4), dict(hidden_size=256), dict(intermediate_size=100)):   # head widths 32, 128
        with pytest.raises(ValueError):
            CLIPTextModel(**dict(OK, **bad))
    with pytest.raises(ValueError):
        CLIPTextModel(dtype=torch.float32, **OK)
    with pytest.raises(TypeError):
        CLIPTextModel(projection_dim=64, **OK)
    m = CLIPTextModel(**OK)
    with pytest.raises(ValueError):
        m(torch.zeros((1, 78), dtype=torch.long))                     # S = 78 with 77 positions
    ids = torch.zeros((1, 6), dtype=torch.long)
    mask = torch.ones((1, 6), dtype=torch.long)
    mask[0, 5] = 0
    with pytest.raises(ValueError):
        m(ids, attention_mask=mask)
    with pytest.raises(ValueError):
        m(ids, position_ids=torch.arange(6)[None])
    with pytest.raises(ValueError):
        m(ids, output_hidden_states=True)
    with pytest.raises(ValueError):
        m()
    with pytest.raises(X2IError):      # an all-ones mask is accepted; on the CPU the first launch then refuses: no fallback
        m(ids, attention_mask=torch.ones((1, 6), dtype=torch.long), output_hidden_states=False)


def test_both_key_spellings_load_and_an_unknown_key_is_refused():
    from x2i_amd.clip import CLIPTextModel
    cfg, lib = CR.library_model(128, 2, 2, 256, vocab=16)
    m = CLIPTextModel(cfg, device="cpu")
    sd = {k: v.bfloat16() for k, v in CR.random_model_state_dict(lib, seed=1).items()}
    want = {k: tuple(v.shape) for k, v in CR.with_prefix(sd).items()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want          # the module's own names are the prefixed ones
    assert "text_model.encoder.layers.1.self_attn.q_proj.bias" in want and "text_model.final_layer_norm.weight" in want
    for spell in (CR.with_prefix, CR.strip_prefix):
        m2 = CLIPTextModel(cfg, device="cpu")
        m2.load_state_dict(spell(sd), strict=True)
        for k, v in m2.state_dict().items():
            assert torch.equal(v, CR.with_prefix(sd)[k]), k
        # the q|k|v views share stacked storage
        assert torch.equal(m2._fused["1.qkv.w"][128:256], CR.with_prefix(sd)["text_model.encoder.layers.1.self_attn.k_proj.weight"])
        assert torch.equal(m2._fused["0.qkv.b"][256:], CR.with_prefix(sd)["text_model.encoder.layers.0.self_attn.v_proj.bias"])
        with pytest.raises(RuntimeError):
            m2.load_state_dict(dict(spell(sd), **{"text_projection.weight": torch.zeros((8, 128))}), strict=True)
        short = dict(spell(sd))
        short.pop(next(k for k in short if k.endswith("final_layer_norm.bias")))
        with pytest.raises(RuntimeError):
            m2.load_state_dict(short, strict=True)
    with pytest.raises(ValueError):
        m.load_state_dict(dict(CR.with_prefix(sd), **CR.strip_prefix(sd)))


def test_from_pretrained_reads_both_spellings_of_a_library_checkpoint(tmp_path):
    """from_pretrained on what the library's save_pretrained writes (config.json + model.safetensors), and on the same file re-keyed to the
    `text_model.` prefix of the 4.x checkpoints"""
    from safetensors.torch import load_file, save_file
    from x2i_amd.clip import CLIPTextModel
    cfg, lib = CR.library_model(128, 2, 2, 256, vocab=16, eos_token_id=9)
    lib.save_pretrained(str(tmp_path / "a"))
    sd = load_file(str(tmp_path / "a" / "model.safetensors"))
    os.makedirs(tmp_path / "b")
    save_file(CR.with_prefix(sd) if not any(k.startswith("text_model.") for k in sd) else CR.strip_prefix(sd), str(tmp_path / "b" / "model.safetensors"))
    with open(tmp_path / "a" / "config.json") as src, open(tmp_path / "b" / "config.json", "w") as dst:
        dst.write(src.read())
    for d in ("a", "b"):
        m = CLIPTextModel.from_pretrained(str(tmp_path), subfolder=d, device="cpu")
        got = m.state_dict()
        assert set(got) == set(CR.with_prefix(sd))
        for k, v in got.items():
            assert v.dtype == torch.bfloat16 and torch.equal(v, CR.with_prefix(sd)[k].bfloat16()), k
        c = m.config
        assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers, c.vocab_size, c.eos_token_id) == (128, 2, 256, 2, 16, 9)


def test_harness_loader_reads_both_subfolders_of_a_pipeline_directory(tmp_path):
    from transformers import T5EncoderModel as LibraryT5
    from tests import t5_ref as TR
    from x2i_amd.clip import CLIPTextModel
    from x2i_amd.infer.harness import load_text_encoders
    from x2i_amd.t5 import T5EncoderModel
    from x2i_amd.text_encoders import TextEncoders
    CR.library_model(128, 2, 1, 256, vocab=16)[1].save_pretrained(str(tmp_path / "text_encoder"))
    LibraryT5(TR.library_config(64, 2, 32, 128, 1, vocab=16)).save_pretrained(str(tmp_path / "text_encoder_2"))
    te = load_text_encoders(str(tmp_path), "cpu")
    assert isinstance(te, TextEncoders) and isinstance(te.clip, CLIPTextModel) and isinstance(te.t5, T5EncoderModel)
    assert te.clip.config.hidden_size == 128 and te.t5.config.d_model == 64 and te.device.type == "cpu"


def test_text_encoders_need_ids_or_tokenizers():
    from x2i_amd.text_encoders import TextEncoders
    te = TextEncoders(clip=None, t5=None)
    with pytest.raises(ValueError):
        te.tokenize("a photo of a cat")
    with pytest.raises(ValueError):
        te.get_t5_input_embeds(clip_ids=torch.zeros((1, 77), dtype=torch.long))
