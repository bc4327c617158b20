"""CPU-side checks of Qwen2 decoding with a key/value cache (no GPU): the extension header include/x2i_qwen_decode.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), every refusal of its three entry points, the float64 restatement of cached decoding (tests/qwen_decode_ref.py) against
the library's own cached `generate` and against Qwen2_5_VLTextModel under three position axes, the next-position rule, the cache's shapes
and refusals, and the harness flag."""
import ctypes as C
import os

import pytest
import torch

from tests import qwen_decode_ref as DR
from tests import qwen_ref as QR
from tests.test_qwen_ref_cpu import _keep_norm_arithmetic_in_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Worst rel-L2 of the restatement of cached decoding against the library in float64 (its norms kept in float64), measured here over the
# cases below: 7.5e-16 (generate, both paddings), 4.3e-16 (three position axes).  Three times the larger.
RESTATEMENT_BOUND = 2.3e-15


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_the_headers_constants_are_the_bindings():
    from x2i_amd import qwen_decode_ops
    text = open(os.path.join(ROOT, "include", "x2i_qwen_decode.h")).read()
    assert "#define X2I_QWEN_DECODE_CHUNK %d\n" % qwen_decode_ops.CHUNK in text
    assert qwen_decode_ops.workspace_floats(2, 28, 640, 128) == 2 * 28 * 3 * 130


def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import qwen_decode_ops
    lib = qwen_decode_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    odd8, odd4, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1004), C.c_void_p(0x1002)
    err = lambda: lib.x2i_last_error()
    ws_ok = qwen_decode_ops.workspace_floats(1, 4, 128, 128)
    att = lambda **kw: lib.x2i_qwen_decode_attention_bf16(*[kw.get(k, d) for k, d in (
        ("Q", fake), ("K", fake), ("VT", fake), ("lo", fake), ("hi", fake), ("O", fake), ("ws", fake), ("wsn", ws_ok), ("B", 1), ("Hq", 4), ("Hkv", 2),
        ("cap", 128), ("dk", 128), ("scale", 0.088), ("ldo", 512), ("st", None))])
    assert att(dk=32) < 0 and b"dk=32" in err()
    assert att(dk=96) < 0 and b"dk=96" in err()
    assert att(Hq=3) < 0 and b"Hkv" in err()
    assert att(Hkv=0) < 0 and att(B=0) < 0
    assert att(Hq=34, ldo=34 * 128, wsn=10 ** 9) < 0 and b"group of 17" in err()
    assert att(Hq=32, ldo=32 * 128, wsn=ws_ok * 8 - 1) < 0 and b"workspace" in err()       # a group of 16 is taken: the next check refuses
    assert att(cap=100) < 0 and b"cap=100" in err()
    assert att(cap=0) < 0 and b"cap=0" in err()
    assert att(lo=None) < 0 and b"required" in err()
    assert att(hi=None) < 0 and b"required" in err()
    assert att(lo=odd2) < 0 and b"aligned" in err()
    assert att(wsn=ws_ok - 1) < 0 and b"workspace too small" in err()
    assert att(cap=320, wsn=ws_ok) < 0 and b"workspace too small" in err()                 # two chunks need twice as much
    assert att(ldo=256) < 0 and b"Hq*dk" in err()
    assert att(ldo=514) < 0 and b"aligned" in err()
    assert att(Q=odd8) < 0 and b"aligned" in err()
    assert att(O=odd4) < 0 and b"aligned" in err()
    for k in ("Q", "K", "VT", "O", "ws"):
        assert att(**{k: None}) < 0 and b"null" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert att(scale=bad) < 0 and b"scale" in err()
    rope = lambda **kw: lib.x2i_qwen_decode_rope_append_bf16(*[kw.get(k, d) for k, d in (
        ("qkv", fake), ("ld", 1024), ("cos", fake), ("sin", fake), ("slot", fake), ("Q", fake), ("K", fake), ("VT", fake), ("B", 1), ("Hq", 4),
        ("Hkv", 2), ("cap", 128), ("dk", 128), ("st", None))])
    assert rope(dk=32) < 0 and b"dk=32" in err()
    assert rope(dk=96) < 0 and b"dk=96" in err()
    assert rope(ld=1016) < 0 and b"ld" in err()               # < (Hq + 2 Hkv) * dk
    assert rope(ld=1028) < 0 and b"ld" in err()
    assert rope(cap=100) < 0 and b"cap" in err()
    assert rope(cap=0) < 0 and rope(Hkv=0) < 0 and rope(B=0) < 0
    for k in ("qkv", "cos", "sin", "slot", "Q", "K", "VT"):
        assert rope(**{k: None}) < 0 and b"null" in err()
    assert rope(cos=odd4) < 0 and b"aligned" in err()
    assert rope(slot=odd2) < 0 and b"aligned" in err()
    lin = lambda **kw: lib.x2i_qwen_decode_linear_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("ldx", 64), ("W", fake), ("ldw", 64), ("bias", fake), ("res", None), ("ldr", 0), ("Y", fake), ("ldy", 32), ("B", 2), ("N", 32),
        ("K", 64), ("mode", 0), ("st", None))])
    assert lin(B=0) < 0 and b"B=0" in err()
    assert lin(B=9) < 0 and b"B=9" in err()
    assert lin(K=60, ldx=64) < 0 and b"K=60" in err()
    assert lin(K=0) < 0 and lin(N=0) < 0
    assert lin(mode=2) < 0 and b"mode=2" in err()
    assert lin(mode=1, res=fake, ldr=32) < 0 and b"residual" in err()
    assert lin(ldx=56) < 0 and lin(ldw=68) < 0 and lin(ldy=24) < 0 and lin(res=fake, ldr=24) < 0 and b"aligned" in err()
    assert lin(X=odd8) < 0 and b"aligned" in err()
    assert lin(W=odd8) < 0 and b"aligned" in err()
    for k in ("X", "W", "Y"):
        assert lin(**{k: None}) < 0 and b"null" in err()


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_cached_decoding_restated_equals_the_librarys_cached_generate_in_float64():
    """A tiny Qwen2ForCausalLM (hidden 256, 2 heads of 128, 1 kv head, 2 layers) in float64, norms kept in float64; sample 0 left-padded,
    sample 1 right-padded; generate(use_cache=True, do_sample=False) for five tokens.  The hidden states of its four decode passes against
    the restatement over each sample's compacted sequence, the steps at the positions the next-position rule gives."""
    from transformers import Qwen2ForCausalLM
    cfg = QR.library_config(256, 2, 1, 512, 2)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    sd = QR.random_stack_state_dict(model.model, seed=5)
    model.model.load_state_dict(sd, strict=True)
    model = model.double()
    _keep_norm_arithmetic_in_float64(model.model)
    B, S, T = 2, 20, 5
    ids = torch.randint(2, 64, (B, S), generator=torch.Generator().manual_seed(6))
    k_lo, k_hi = [7, 0], [S, 13]
    mask = torch.zeros((B, S), dtype=torch.long)
    for b in range(B):
        mask[b, k_lo[b]:k_hi[b]] = 1
    # position_ids = cumsum(mask) - 1 as generate derives them, but handed over with the padding columns left at the running count: generate
    # continues from the LAST COLUMN's id + 1, which under right padding is only then the count of valid tokens (on its own it fills the
    # padding with 0 and goes on at 1, 2, .. -- the library's known right-padding defect, which it warns about and nothing here follows)
    pos = (mask.cumsum(-1) - 1).clamp_min(0)
    assert pos[1].tolist() == list(range(13)) + [12] * 7
    out = model.generate(input_ids=ids, attention_mask=mask, position_ids=pos, max_new_tokens=T, min_new_tokens=T, do_sample=False, use_cache=True,
                         pad_token_id=0, output_hidden_states=True, return_dict_in_generate=True)
    assert out.sequences.shape == (B, S + T) and len(out.hidden_states) == T
    want = torch.cat([torch.stack(tuple(h), 1) for h in out.hidden_states[1:]], 2)            # [B, C, T - 1, D]: the passes of tokens 0 .. T - 2
    table = sd["embed_tokens.weight"].double()
    x, steps = table[ids], table[out.sequences[:, S:S + T - 1]]
    assert DR.next_positions(pos, mask).tolist() == [13, 13]     # the count of valid tokens
    got = DR.decode_reference(sd, x, steps, pos, k_lo, k_hi, num_heads=2, num_kv_heads=1, eps=cfg.rms_norm_eps, dk=128, theta=1000000.0)
    e = QR.rel_l2(got, want)
    print("cached decoding restated vs Qwen2ForCausalLM.generate in float64: rel-L2 %.3e" % e)
    assert got.shape == want.shape == (B, 3, T - 1, 256) and float(want[:, -1].std()) > 0.1
    assert e <= RESTATEMENT_BOUND
    # a wrong next position is seen: the same steps one position later (the slot a right-padded sample's token lands in, say)
    late = DR.decode_reference(sd, x, steps, pos, k_lo, k_hi, num_heads=2, num_kv_heads=1, eps=cfg.rms_norm_eps, dk=128, theta=1000000.0,
                               step_offset=1)
    assert QR.rel_l2(late, want) > 1e-4


def test_cached_decoding_restated_equals_qwen2_5_vl_text_model_under_three_axes_in_float64():
    """Qwen2_5_VLTextModel, three position axes that differ, extended by the next-position rule (every axis continues at 1 + the largest id
    of the prompt over all axes): the library's full causal pass over prompt + steps, rows of the steps"""
    cfg, lib = QR.library_stack(256, 2, 1, 512, 2, vl=True)
    sd = QR.random_stack_state_dict(lib, seed=3)
    lib = lib.double()
    lib.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    _keep_norm_arithmetic_in_float64(lib)
    B, S, T = 2, 40, 4
    g = torch.Generator().manual_seed(4)
    x, steps = torch.randn((B, S, 256), generator=g).bfloat16().double(), torch.randn((B, T, 256), generator=g).bfloat16().double()
    pos = QR.mrope_positions(B, S, seed=5)
    nxt = DR.next_positions(pos, None)
    assert nxt.tolist() == [int(pos[:, b].max()) + 1 for b in range(B)] and int(nxt.min()) > S      # the width axis runs ahead of the text axis
    pcat = torch.cat((pos, DR.step_positions(nxt, T).expand(3, B, T)), -1)
    out = lib(inputs_embeds=torch.cat((x, steps), 1), position_ids=pcat, output_hidden_states=True, use_cache=False)
    want = torch.stack(tuple(out.hidden_states), 1)[:, :, S:]
    got = DR.decode_reference(sd, x, steps, pos, None, None, num_heads=2, num_kv_heads=1, eps=cfg.rms_norm_eps, dk=128, theta=1000000.0,
                              mrope_section=[16, 24, 24])
    e = QR.rel_l2(got, want)
    print("cached decoding restated vs Qwen2_5_VLTextModel in float64, three axes: rel-L2 %.3e" % e)
    assert e <= RESTATEMENT_BOUND


def test_references_of_the_kernels_on_known_values():
    """attention: uniform scores average V over the range, an empty or inverted range is 0, ranges are clamped; the gate's expectation is
    silu(a) b with a bound that a second rounding of silu(a) breaks"""
    B, Hq, Hkv, dk, cap = 2, 4, 2, 64, 128
    Qd = torch.zeros((B, Hq, dk))
    g = torch.Generator().manual_seed(1)
    K, V = torch.randn((B, Hkv, cap, dk), generator=g), torch.randn((B, Hkv, cap, dk), generator=g)
    ref = DR.attention_reference(Qd, K, V, [10, 90], [20, 80], 0.125)
    assert torch.allclose(ref[0, 3], V[0, 1, 10:20].double().mean(0), atol=1e-14) and bool((ref[1] == 0).all())
    assert torch.equal(DR.attention_reference(Qd, K, V, [-5, 0], [20, 4000], 0.125), DR.attention_reference(Qd, K, V, [0, 0], [20, cap], 0.125))
    X = torch.randn((3, 256), generator=g).bfloat16()
    W, bias = (torch.randn((128, 256), generator=g) / 16).bfloat16(), torch.randn((128,), generator=g).bfloat16()
    want, bound, delta = DR.gate_expect(X, W, bias)
    a, b = X.float() @ W[:64].float().T + bias[:64].float(), X.float() @ W[64:].float().T + bias[64:].float()
    one = (torch.nn.functional.silu(a) * b).bfloat16()
    assert bool(((one.double() - want).abs() <= bound).all()) and bool((delta < bound).all())
    two = (torch.nn.functional.silu(a).bfloat16().float() * b).bfloat16()
    assert not bool(((two.double() - want).abs() <= bound).all())
    swapped = (torch.nn.functional.silu(b) * a).bfloat16()
    assert not bool(((swapped.double() - want).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------------------------- host module
OK = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=256, num_hidden_layers=2, vocab_size=16, device="cpu")


def test_new_cache_shapes_refusals_and_the_next_position_rule():
    from x2i_amd._lib import X2IError
    from x2i_amd.qwen import Qwen2DecodeCache, Qwen2DecoderStack
    m = Qwen2DecoderStack(**OK)
    c = m.new_cache(2, 70)
    assert isinstance(c, Qwen2DecodeCache) and c.cap == 128 and c.B == 2 and c.steps is None
    assert c.K.shape == (2, 2, 1, 128, 64) and c.VT.shape == (2, 2, 1, 64, 128) and c.K.dtype == c.VT.dtype == torch.bfloat16
    assert not bool(c.K.any()) and not bool(c.VT.any())                                    # zeroed once: finite
    assert c.k_lo.shape == c.k_hi.shape == (2,) and c.k_lo.dtype == c.k_hi.dtype == torch.int32 and c.pos.shape == (2,)
    assert c.ws.dtype == torch.float32 and c.ws.numel() == 2 * 2 * 1 * 66
    assert m.new_cache(1, 64).cap == 64 and m.new_cache(1, 65).cap == 128 and m.new_cache(1, 257).ws.numel() == 2 * 2 * 66
    for bad in ((0, 64), (9, 64), (1, 0)):
        with pytest.raises(ValueError):
            m.new_cache(*bad)
    # the rule: ranges from the mask, next position 1 + the largest position id of the valid tokens
    mask = torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]])
    pos = (mask.cumsum(-1) - 1).clamp_min(0)
    c._set_prompt(6, None, None, mask, pos)
    assert c.k_lo.tolist() == [2, 0] and c.k_hi.tolist() == [6, 3] and c.pos.tolist() == [4, 3] and c.steps == 6
    assert c.pos.tolist() == DR.next_positions(pos, mask).tolist()
    c._set_prompt(6, None, None, None, torch.arange(6)[None].expand(2, 6))
    assert c.k_lo.tolist() == [0, 0] and c.k_hi.tolist() == [6, 6] and c.pos.tolist() == [6, 6]
    cos, sin = c._step_tables()
    assert c.slot.tolist() == [6, 6] and c.k_hi.tolist() == [7, 7] and c.pos.tolist() == [7, 7] and cos.shape == sin.shape == (2, 32)
    from x2i_amd.qwen import rope_tables
    want_c, want_s = rope_tables(torch.tensor([[6], [6]]), 64, m.config.rope_theta)
    assert torch.equal(cos, want_c[:, 0]) and torch.equal(sin, want_s[:, 0])              # rope_tables' own values
    # three axes: every axis continues at the same next position
    mv = Qwen2DecoderStack(**dict(OK, rope_type="mrope", mrope_section=[8, 12, 12]))
    cv = mv.new_cache(2, 70)
    p3 = QR.mrope_positions(2, 6, seed=1)
    cv._set_prompt(6, None, None, mask, p3)
    want = DR.next_positions(p3, mask)
    assert cv.pos.shape == (3, 2) and torch.equal(cv.pos, want.expand(3, 2)) and int(want[0]) == int(p3[:, 0, 2:].max()) + 1
    cos, sin = cv._step_tables()
    want_c, want_s = rope_tables(want.expand(3, 2)[..., None], 64, mv.config.rope_theta, [8, 12, 12])
    assert torch.equal(cos, want_c[:, 0]) and torch.equal(sin, want_s[:, 0])
    # refusals of the host calls
    x = torch.zeros((2, 6, 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="prefill"):
        m.decode_step(m.new_cache(2, 70), inputs_embeds=x[:, :1])
    with pytest.raises(ValueError, match="new_cache"):
        m.prefill(cv, inputs_embeds=x)
    with pytest.raises(ValueError, match="new_cache"):
        m.decode_step(object(), inputs_embeds=x[:, :1])
    with pytest.raises(ValueError, match="cap"):
        m.prefill(m.new_cache(2, 64), inputs_embeds=torch.zeros((2, 64, 128), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="cap"):
        m.prefill(m.new_cache(1, 64), inputs_embeds=x)                                     # another batch size
    with pytest.raises(ValueError):
        m.decode_step(c)
    with pytest.raises(X2IError):        # on the CPU the first launch refuses: no fallback
        m.prefill(m.new_cache(2, 70), inputs_embeds=x)
    with pytest.raises(X2IError):
        m.decode_step(c, inputs_embeds=x[:, :1])
    # forward is as it was
    with pytest.raises(ValueError, match="prefill only"):
        m(inputs_embeds=x, use_cache=True)


def test_harness_takes_the_hip_generate_flag_and_defaults_stay():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("qwenvl")
    a = p.parse_args(["--synthetic"])
    assert a.hip_generate is False and a.hip_decoder is False and a.hip_vision is False and a.full_generate is False and a.use_answer is False
    assert a.num_steps == 4 and a.num_gen_imgs == 1 and a.batch == 1 and a.no_graph is False and a.qwen_size == "7b"
    assert p.parse_args(["--synthetic", "--hip_generate"]).hip_generate is True


def test_hip_generate_refuses_a_sampling_generation_config_by_name():
    from transformers import GenerationConfig
    from x2i_amd.handoff import HipGenerate
    with pytest.raises(ValueError, match="--full_generate"):
        HipGenerate.refuse_sampling(GenerationConfig(do_sample=True, top_k=50))
    with pytest.raises(ValueError, match="--full_generate"):
        HipGenerate.refuse_sampling(GenerationConfig(do_sample=True, top_k=None))
    HipGenerate.refuse_sampling(GenerationConfig(do_sample=True, top_k=1))        # Qwen2.5-VL's own: sampling from one candidate is greedy
    HipGenerate.refuse_sampling(GenerationConfig(do_sample=False))
    HipGenerate.refuse_sampling(None)
