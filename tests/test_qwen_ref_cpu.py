"""CPU-side checks of the Qwen2 decoder prefill work (no GPU): the float64 restatement of the stack against the library in float64 under both
paddings and under M-RoPE, rope_tables bit for bit against the library's rotary embedding, the key ranges of a mask, the checkers of
tests/qwen_ref.py against the mistakes they are there to catch, the extension header include/x2i_qwen.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and the host module's refusals and parameter names."""
import ctypes as C

import pytest
import torch

from tests import qwen_ref as QR


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def _keep_norm_arithmetic_in_float64(stack):
    """The library's Qwen2RMSNorm casts its input to float32 for the whole normalisation whatever the model's dtype, so a `.double()` stack
    still carries float32 norms (about 1e-7 relative).  This replaces that one cast: the same formula in the input's dtype."""
    import types

    def forward(self, hidden_states):
        variance = hidden_states.pow(2).mean(-1, keepdim=True)
        return self.weight * (hidden_states * torch.rsqrt(variance + self.variance_epsilon))
    n = 0
    for m in stack.modules():
        if type(m).__name__.endswith("RMSNorm"):
            m.forward = types.MethodType(forward, m)
            n += 1
    assert n == 2 * len(stack.layers) + 1
    return stack


def _library_hidden_states(lib, x, mask, position_ids):
    out = lib(inputs_embeds=x, attention_mask=mask, position_ids=position_ids, output_hidden_states=True, use_cache=False)
    return torch.stack(tuple(out.hidden_states), 1)


def _restatement_vs_library(vl, padding, B=2, S=77, hidden=256, heads=2, kv=1, inter=512):
    cfg, lib = QR.library_stack(hidden, heads, kv, inter, 2, vl=vl)
    sd = QR.random_stack_state_dict(lib, seed=3)
    lib = lib.double()
    lib.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    x = torch.randn((B, S, hidden), generator=torch.Generator().manual_seed(4)).bfloat16().double()
    mask, k_lo, k_hi = None, None, None
    if padding == "right":
        k_lo, k_hi = [0, 0], [50, S]
    elif padding == "left":
        k_lo, k_hi = [0, 30], [S, S]
    if padding != "none":
        mask = torch.zeros((B, S), dtype=torch.long)
        for b in range(B):
            mask[b, k_lo[b]:k_hi[b]] = 1
    pos = QR.mrope_positions(B, S, seed=5) if vl else None
    as_is = _library_hidden_states(lib, x, mask, pos)
    want = _library_hidden_states(_keep_norm_arithmetic_in_float64(lib), x, mask, pos)
    # the library's own rotary table: float32 values, which its float64 model multiplies as they are
    ids = pos if vl else torch.arange(S)[None].expand(B, S)
    cos, sin = QR.half_tables(*lib.rotary_emb(x, ids), mrope_section=[16, 24, 24] if vl else None)
    assert cos.dtype == torch.float64 and torch.equal(cos, cos.float().double())           # (float32 values)
    got = QR.stack_reference(sd, x, cos, sin, num_heads=heads, num_kv_heads=kv, eps=cfg.rms_norm_eps, k_lo=k_lo, k_hi=k_hi)
    assert got.shape == want.shape == (B, 3, S, hidden)
    keep = torch.ones((B, S), dtype=torch.bool)
    if padding == "left":                                   # the library defines nothing on the rows before the first valid token
        for b in range(B):
            keep[b, :k_lo[b]] = False
    keep = keep[:, None, :, None].expand_as(want)
    e = float((got[keep] - want[keep]).norm() / want[keep].norm())
    e_as_is = float((got[keep] - as_is[keep]).norm() / as_is[keep].norm())
    worst = float((got[keep] - want[keep]).abs().max())
    print("restatement vs library (vl=%s, %s padding): float64 norms rel-L2 %.3e, worst element %.3e; as it is %.3e" % (vl, padding, e, worst, e_as_is))
    assert bool(torch.isfinite(got).all()) and float(want[:, -1].std()) > 0.1      # a live output, not a collapsed one
    # Every hidden state to 1e-12 against the library with its norms kept in float64, and to 1e-5 against the library as it is: Qwen2RMSNorm
    # normalises in float32 even in a float64 model (statistics within (log2 D + 2) 2^-24 < 6e-7, the normalised value rounded to 2^-24), which
    # no float64 restatement can follow to 1e-12; the five norms of a two-layer stack each pass that on -- 1.5e-6 before any amplification by
    # the layers; 1e-5 leaves room for that and is four orders below the bf16 errors the GPU tests compare (measured: 7.6e-8).
    assert e <= 1e-12 and worst <= 1e-12 * max(1.0, float(want[keep].abs().max())) and e_as_is <= 1e-5


@pytest.mark.parametrize("padding", ["none", "right", "left"])
def test_float64_restatement_equals_qwen2model_in_float64(padding):
    """Qwen2Model, 2 layers, hidden 256, 2 q heads / 1 kv head of 128, x [2, 77, 256]; all rows for right padding, the rows s >= k_lo for left
    padding.  The restatement has no float32 step (the rotary table is the library's own; the library's float32 norm is pinned separately in
    _restatement_vs_library), so the bound is 1e-12 (measured: a few 1e-15)."""
    _restatement_vs_library(False, padding)


def test_float64_restatement_equals_qwen2_5_vl_text_model_in_float64():
    """Qwen2_5_VLTextModel with three position axes that differ from each other and mrope_section [16, 24, 24]"""
    pos = QR.mrope_positions(2, 77, seed=5)
    assert not torch.equal(pos[0], pos[1]) and not torch.equal(pos[1], pos[2]) and not torch.equal(pos[0], pos[2])
    _restatement_vs_library(True, "none")


# ---------------------------------------------------------------------------------------------------------------- rope tables
@pytest.mark.parametrize("vl", [False, True])
@pytest.mark.parametrize("dk,hidden,heads", [(128, 256, 2), (64, 128, 2)])
def test_rope_tables_are_bit_equal_to_the_librarys_rotary_embedding(vl, dk, hidden, heads):
    """positions up to 4000; under M-RoPE after the library's selection of chunk i from axis i % 3"""
    from x2i_amd.qwen import rope_tables
    cfg, lib = QR.library_stack(hidden, heads, 1, 256, 1, vl=vl)
    B, S = 2, 130
    sec = cfg.rope_parameters.get("mrope_section") if vl else None
    if vl:
        pos = QR.mrope_positions(B, S, seed=1)
        pos[:, 1] += 3870          # up to 4000
    else:
        pos = torch.randint(0, 4001, (B, S), generator=torch.Generator().manual_seed(2))
        pos[0, :3] = torch.tensor([0, 1, 4000])
    want_c, want_s = QR.half_tables(*lib.rotary_emb(torch.zeros((B, S, hidden)), pos), mrope_section=sec)
    cos, sin = rope_tables(pos, dk, cfg.rope_parameters["rope_theta"], sec)
    assert cos.dtype == sin.dtype == torch.float32 and cos.shape == sin.shape == (B, S, dk // 2)
    assert torch.equal(cos, want_c) and torch.equal(sin, want_s)
    # with the stack's scratch buffers: the same values, and the buffers are reused
    scratch = {}
    c2, s2 = rope_tables(pos, dk, cfg.rope_parameters["rope_theta"], sec, _scratch=scratch)
    ang = scratch["ang"]
    c3, s3 = rope_tables(pos, dk, cfg.rope_parameters["rope_theta"], sec, _scratch=scratch)
    assert torch.equal(c2, cos) and torch.equal(s3, sin) and scratch["ang"] is ang
    if vl:
        with pytest.raises(ValueError):
            rope_tables(pos, dk, 1e6, None)
        with pytest.raises(ValueError):
            rope_tables(pos, dk, 1e6, [1, 2, 3])


# ---------------------------------------------------------------------------------------------------------------- masks
def test_key_ranges_and_the_mask_check():
    from x2i_amd.qwen import Qwen2DecoderStack, key_ranges, mask_state
    S = 9
    rows = {"right": ([1, 1, 1, 1, 1, 0, 0, 0, 0], (0, 5)), "left": ([0, 0, 0, 1, 1, 1, 1, 1, 1], (3, 9)),
            "both": ([0, 0, 1, 1, 1, 0, 0, 0, 0], (2, 5)), "ones": ([1] * 9, (0, 9)), "one key": ([0] * 8 + [1], (8, 9))}
    mask = torch.tensor([r for r, _ in rows.values()])
    lo, hi = key_ranges(mask)
    assert lo.dtype == hi.dtype == torch.int32
    assert lo.tolist() == [w[0] for _, w in rows.values()] and hi.tolist() == [w[1] for _, w in rows.values()]
    assert mask_state(mask) == (True, False) and mask_state(torch.ones((2, S), dtype=torch.long)) == (True, True)
    assert key_ranges(torch.ones((2, S), dtype=torch.bool))[1].tolist() == [S, S]
    hole = torch.tensor([[1, 1, 0, 1, 1, 0, 0, 0, 0], [1] * 9])
    empty = torch.tensor([[1] * 9, [0] * 9])
    assert mask_state(hole)[0] is False and mask_state(empty)[0] is False
    assert [t.tolist() for t in key_ranges(empty)] == [[0, 0], [9, 0]]           # an all-zero row is the empty range
    m = Qwen2DecoderStack(**OK)
    x = torch.zeros((2, S, 128), dtype=torch.bfloat16)
    for bad in (hole, empty):
        with pytest.raises(ValueError, match="contiguous"):
            m(inputs_embeds=x, attention_mask=bad)
    with pytest.raises(ValueError):
        m(inputs_embeds=x, attention_mask=torch.ones((2, S + 1), dtype=torch.long))


# ---------------------------------------------------------------------------------------------------------------- the checkers reject
def _wrong_attention(Q, K, V, S, scale, kind):
    """float64 attention with one deliberate mistake in the mask or in the head mapping"""
    f = torch.float64
    Hq, Hkv = Q.shape[1], K.shape[1]
    rep = Hq // Hkv
    pos = torch.arange(S)
    rel = pos[None, :] - pos[:, None]           # key - query
    masked = {"none": rel > 0, "modulo": rel > 0, "unmasked": rel > S, "strict": rel >= 0, "shifted": rel > 1}[kind]
    heads = torch.arange(Hq) % Hkv if kind == "modulo" else torch.arange(Hq) // rep
    q, k, v = Q[:, :, :S].to(f), K[:, heads, :S].to(f), V[:, heads, :S].to(f)
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(masked, float("-inf"))
    if kind == "strict":
        s[:, :, 0, 0] = 0.0                      # (row 0 would be empty: let it keep its one key)
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("kind", ["unmasked", "strict", "shifted", "modulo"])
@pytest.mark.parametrize("S", [77, 300])
def test_attention_checker_rejects(kind, S):
    """an unmasked, a strict (j < i) and a shifted causal mask; h % Hkv instead of h // rep"""
    B, Hq, Hkv, dk = 1, 4, 2, 128
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=11)
    ref = QR.attention_reference(Q, K, V, S, dk ** -0.5)
    QR.check_attention("exact", _wrong_attention(Q, K, V, S, dk ** -0.5, "none"), ref)            # the restatement without a mistake passes
    QR.check_attention("bf16 output", ref.bfloat16(), ref)                                          # ... and so does one rounding of it
    with pytest.raises(AssertionError):
        QR.check_attention(kind, _wrong_attention(Q, K, V, S, dk ** -0.5, kind), ref)


def test_attention_checker_rejects_the_uniform_average_on_rows_before_the_range():
    """The kernel's trap: a row with no counted key that comes out as the average of V instead of 0; and a range that is ignored"""
    B, Hq, Hkv, S, dk = 2, 4, 2, 130, 128
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=12)
    k_lo, k_hi = [70, 0], [S, S]
    ref = QR.attention_reference(Q, K, V, S, dk ** -0.5, k_lo, k_hi)
    assert bool((ref[0, :, :70] == 0).all()) and bool((ref[0, :, 70:] != 0).any(-1).all()) and bool((ref[1] != 0).any(-1).all())
    QR.check_attention("one rounding", ref.bfloat16(), ref, k_lo=k_lo)
    trap = ref.clone()
    trap[0, :, 64:70] = V[0, :, :64].double().mean(1).repeat_interleave(2, dim=0)[:, None]
    with pytest.raises(AssertionError, match="exactly 0"):
        QR.check_attention("average", trap.bfloat16(), ref, k_lo=k_lo)
    with pytest.raises(AssertionError):
        QR.check_attention("average", trap.bfloat16(), ref)
    with pytest.raises(AssertionError):
        QR.check_attention("no range", QR.attention_reference(Q, K, V, S, dk ** -0.5), ref)


def _rope_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, n, 1, 128), generator=g).bfloat16()
    ang = torch.rand((1, n, 64), generator=g) * 4000.0
    return x, torch.cos(ang), torch.sin(ang)


def _rope_f32(x, cos, sin, kind="one rounding"):
    """f32 forms of the rotation on x [B, S, H, dk] with half tables: the kernel's, and the mistakes the checker is there to catch"""
    x1, x2 = x.float()[..., :64], x.float()[..., 64:]
    c, s = cos[:, :, None], sin[:, :, None]
    if kind == "one rounding":
        return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), -1).bfloat16()
    if kind == "sign":
        return torch.cat((x1 * c + x2 * s, x2 * c - x1 * s), -1).bfloat16()
    if kind == "interleaved":                    # pairs (x[2k], x[2k+1]) instead of (x[k], x[k + dk/2])
        e, o = x.float()[..., 0::2], x.float()[..., 1::2]
        return torch.stack((e * c - o * s, o * c + e * s), -1).flatten(-2).bfloat16()
    if kind == "library bf16":                   # the library's bf16 path: bf16 tables, each product and the sum rounded to bf16
        cb, sb = c.bfloat16(), s.bfloat16()
        xb = x.bfloat16()
        rot = torch.cat((-xb[..., 64:], xb[..., :64]), -1)
        return xb * torch.cat((cb, cb), -1) + rot * torch.cat((sb, sb), -1)
    raise KeyError(kind)


def test_rope_checker_accepts_one_rounding_and_rejects_the_other_forms():
    """2^20 random elements (8192 rows of 128), angles up to 4000: the one-rounding f32 form stays inside the bound (it peaks at 0.98 of it);
    the sign-flipped sine, the interleaved-pair form and the library's bf16 form do not (the last by three orders of magnitude)"""
    x, cos, sin = _rope_inputs(8192, seed=6)
    peak = QR.check_rope("one rounding", _rope_f32(x, cos, sin), x, cos, sin)
    print("rope, one-rounding f32 form: worst error / bound %.3f" % peak)
    assert 0.5 < peak <= 1.0
    for kind in ("sign", "interleaved", "library bf16"):
        with pytest.raises(AssertionError):
            QR.check_rope(kind, _rope_f32(x, cos, sin, kind), x, cos, sin)
    want, mag = QR.rope_reference(x, cos, sin)
    over = ((_rope_f32(x, cos, sin, "library bf16").double() - want).abs() / (QR.TOL_ROW * want.abs() + QR.U_ROPE * mag)).max()
    print("rope, library bf16 form: worst error / bound %.1f" % float(over))
    assert float(over) > 100.0


def test_swiglu_checker_accepts_one_rounding_and_rejects_other_gates_and_two_roundings():
    g = torch.Generator().manual_seed(6)
    a, b = (2.0 * torch.randn((7, 256), generator=g)).bfloat16(), (2.0 * torch.randn((7, 256), generator=g)).bfloat16()
    silu = a.float() * torch.sigmoid(a.float())
    assert QR.check_swiglu("one rounding", (silu * b.float()).bfloat16(), a, b) <= QR.TOL_ROW + 2.0 ** -19
    with pytest.raises(AssertionError):     # the library's bf16 path: silu rounded to bf16, then the product
        QR.check_swiglu("two roundings", (silu.bfloat16().float() * b.float()).bfloat16(), a, b)
    with pytest.raises(AssertionError):
        QR.check_swiglu("swapped halves", (b.float() * torch.sigmoid(b.float()) * a.float()).bfloat16(), a, b)
    with pytest.raises(AssertionError):
        QR.check_swiglu("gelu gate", (torch.nn.functional.gelu(a.float(), approximate="tanh") * b.float()).bfloat16(), a, b)


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import qwen_ops
    lib = qwen_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    att = lambda **kw: lib.x2i_qwen_attention_bf16(*[kw.get(k, d) for k, d in (
        ("Q", fake), ("K", fake), ("VT", fake), ("lo", None), ("hi", None), ("O", fake), ("B", 1), ("Hq", 4), ("Hkv", 2), ("S", 77), ("Spad", 128),
        ("dk", 128), ("scale", 0.088), ("ldo", 512), ("obs", 77 * 512), ("st", None))])
    assert att(dk=32) < 0 and b"dk=32" in err()
    assert att(dk=96) < 0 and b"dk=96" in err()
    assert att(Hq=3) < 0 and b"Hkv" in err()
    assert att(Hkv=0) < 0
    assert att(Spad=100) < 0 and b"Spad" in err()
    assert att(Spad=64) < 0 and b"Spad" in err()              # Spad < S
    assert att(lo=fake) < 0 and b"both" in err()
    assert att(hi=fake) < 0 and b"both" in err()
    assert att(ldo=256, obs=77 * 256) < 0 and b"Hq*dk" in err()
    assert att(ldo=514) < 0 and b"aligned" in err()
    assert att(Q=C.c_void_p(0x1008)) < 0 and b"aligned" in err()
    for k in ("Q", "K", "VT", "O"):
        assert att(**{k: None}) < 0 and b"null" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert att(scale=bad) < 0 and b"scale" in err()
    rope = lambda **kw: lib.x2i_qwen_rope_split_bf16(*[kw.get(k, d) for k, d in (
        ("qkv", fake), ("ld", 1024), ("cos", fake), ("sin", fake), ("Q", fake), ("K", fake), ("VT", fake), ("B", 1), ("S", 77), ("Spad", 128),
        ("Hq", 4), ("Hkv", 2), ("dk", 128), ("st", None))])
    assert rope(dk=32) < 0 and b"dk=32" in err()
    assert rope(dk=96) < 0 and b"dk=96" in err()
    assert rope(ld=1016) < 0 and b"ld" in err()               # < (Hq + 2 Hkv) * dk
    assert rope(ld=1028) < 0
    assert rope(Spad=76) < 0 and rope(Spad=100) < 0 and rope(Hkv=0) < 0
    for k in ("qkv", "cos", "sin", "Q", "K", "VT"):
        assert rope(**{k: None}) < 0 and b"null" in err()
    assert rope(cos=C.c_void_p(0x1004)) < 0 and b"aligned" in err()
    assert lib.x2i_qwen_swiglu_bf16(fake, 24, fake, 12, 4, 12, None) < 0 and b"F=12" in err()
    assert lib.x2i_qwen_swiglu_bf16(fake, 128, None, 64, 4, 64, None) < 0 and b"null" in err()
    assert lib.x2i_qwen_swiglu_bf16(fake, 120, fake, 64, 4, 64, None) < 0 and b"strides" in err()    # ld_in < 2F
    assert lib.x2i_qwen_swiglu_bf16(fake, 128, fake, 60, 4, 64, None) < 0 and b"strides" in err()


# ---------------------------------------------------------------------------------------------------------------- host module
OK = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=256, num_hidden_layers=1, vocab_size=16, device="cpu")


def test_unsupported_configurations_and_arguments_raise():
    from x2i_amd._lib import X2IError
    from x2i_amd.qwen import Qwen2DecoderStack
    for bad in (dict(hidden_act="gelu"), dict(layer_types=["sliding_attention"]), dict(use_sliding_window=True), dict(rope_type="yarn"),
                dict(rope_type="linear"), dict(num_attention_heads=4), dict(hidden_size=512), dict(head_dim=96),      # head widths 32, 256, 96
                dict(num_key_value_heads=3), dict(intermediate_size=100), dict(mrope_section=[16, 24, 24]), dict(num_hidden_layers=0)):
        with pytest.raises(ValueError):
            Qwen2DecoderStack(**dict(OK, **bad))
    with pytest.raises(ValueError):
        Qwen2DecoderStack(dtype=torch.float32, **OK)
    with pytest.raises(TypeError):
        Qwen2DecoderStack(projection_dim=64, **OK)
    Qwen2DecoderStack(**dict(OK, rope_type="mrope", mrope_section=[8, 12, 12], layer_types=["full_attention"]))
    # a library configuration with sliding layers, and one with another rope type
    from transformers import Qwen2Config
    kw = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=256, num_hidden_layers=2, vocab_size=16)
    with pytest.raises(ValueError, match="sliding"):
        Qwen2DecoderStack(Qwen2Config(use_sliding_window=True, sliding_window=8, max_window_layers=1, **kw), device="cpu")
    with pytest.raises(ValueError, match="rope"):
        Qwen2DecoderStack(Qwen2Config(rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=1e4), **kw), device="cpu")
    m = Qwen2DecoderStack(**OK)
    x = torch.zeros((1, 6, 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        m(inputs_embeds=x, use_cache=True)
    with pytest.raises(ValueError):
        m(inputs_embeds=x, past_key_values=object())
    with pytest.raises(ValueError):
        m()
    with pytest.raises(ValueError):
        m(inputs_embeds=x, input_ids=torch.zeros((1, 6), dtype=torch.long))
    with pytest.raises(ValueError):      # three position axes without an mrope_section
        m(inputs_embeds=x, position_ids=torch.zeros((3, 1, 6), dtype=torch.long))
    with pytest.raises(X2IError):        # on the CPU the first launch refuses: no fallback
        m(inputs_embeds=x, attention_mask=torch.ones((1, 6), dtype=torch.long))


@pytest.mark.parametrize("vl", [False, True])
def test_parameter_names_are_the_librarys_and_views_share_stacked_storage(vl):
    from x2i_amd.qwen import Qwen2DecoderStack
    cfg, lib = QR.library_stack(256, 2, 1, 512, 2, vl=vl)
    sd = {k: v.bfloat16() for k, v in QR.random_stack_state_dict(lib, seed=1).items()}
    m = Qwen2DecoderStack(cfg, device="cpu")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in lib.state_dict().items()}
    assert "layers.1.self_attn.k_proj.bias" in sd and "layers.0.mlp.gate_proj.weight" in sd and "norm.weight" in sd and "embed_tokens.weight" in sd
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert m.config.mrope_section == ([16, 24, 24] if vl else None) and m.config.head_dim == 128 and m.config.rope_theta == 1000000.0
    # q|k|v and gate|up are views into stacked storage
    assert torch.equal(m._fused["1.qkv.w"][256:384], sd["layers.1.self_attn.k_proj.weight"])
    assert torch.equal(m._fused["0.qkv.b"][384:], sd["layers.0.self_attn.v_proj.bias"])
    assert torch.equal(m._fused["1.gu"][512:], sd["layers.1.mlp.up_proj.weight"])
    assert m.layers[0].self_attn.q_proj.weight.data_ptr() == m._fused["0.qkv.w"].data_ptr()
    # ... and stay views through _apply (tests/test_qwen_gpu.py moves a stack to the GPU)
    m = m.to("cpu").bfloat16()
    assert m.layers[1].mlp.up_proj.weight.data_ptr() == m._fused["1.gu"][512:].data_ptr()
    assert torch.equal(m.layers[1].self_attn.v_proj.bias, sd["layers.1.self_attn.v_proj.bias"])
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, **{"lm_head.weight": torch.zeros((16, 256))}), strict=True)
    short = dict(sd)
    short.pop("layers.0.self_attn.q_proj.bias")
    with pytest.raises(RuntimeError):
        m.load_state_dict(short, strict=True)
    with pytest.raises(ValueError):
        m.float()
    # from_hf copies an instantiated library decoder
    lib.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    m2 = Qwen2DecoderStack.from_hf(lib)
    for k, v in m2.state_dict().items():
        assert v.dtype == torch.bfloat16 and torch.equal(v, sd[k]), k


def test_harness_takes_the_hip_decoder_flag_and_defaults_stay():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("qwenvl")
    a = p.parse_args(["--synthetic"])
    assert a.hip_decoder is False and a.full_generate is False
    assert p.parse_args(["--synthetic", "--hip_decoder"]).hip_decoder is True
