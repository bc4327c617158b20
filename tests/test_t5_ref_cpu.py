"""CPU-side checks of the T5 encoder work (no GPU): the bias table against the library's compute_bias, the float64 restatement of the stack
against the library in float64, the checkers of tests/t5_ref.py against the mistakes they are there to catch, the extension header
include/x2i_t5.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and the host modules' refusals."""
import ctypes as C
import math
import os

import pytest
import torch

from tests import t5_ref as TR


def _lib_stack(d_model, heads, d_kv, d_ff, layers, vocab=64):
    return TR.library_stack(d_model, heads, d_kv, d_ff, layers, vocab)


# ---------------------------------------------------------------------------------------------------------------- bias table
@pytest.mark.parametrize("S", [1, 6, 77, 129, 300, 1024])
def test_bias_table_equals_the_librarys_compute_bias(S):
    """table[h][clamp(j - i, -R, R) + R] is bit-equal to T5Attention.compute_bias(S, S): the bucket function saturates at max_distance.
    Bias weights ~ N(0, 2^2): the default initialisation is near zero and would hide a wrong index."""
    from x2i_amd.t5 import relative_bias_table
    cfg, stack = _lib_stack(64, 3, 32, 128, 1)
    att = stack.block[0].layer[0].SelfAttention
    att.relative_attention_bias.weight.copy_(2.0 * torch.randn((32, 3), generator=torch.Generator().manual_seed(S)))
    want = att.compute_bias(S, S)[0]
    R = cfg.relative_attention_max_distance
    table = relative_bias_table(att.relative_attention_bias.weight, cfg.relative_attention_num_buckets, R)
    assert table.shape == (3, 2 * R + 1) and table.dtype == torch.float32
    assert torch.equal(table[:, TR.clamped_index(S, R)], want)
    assert len(torch.unique(want)) > 3 or S == 1


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def _keep_norm_statistics_in_float64(stack):
    """The library's T5LayerNorm casts its input to float32 for the mean of squares whatever the model's dtype, so a `.double()` stack still
    carries float32 statistics (about 1e-7 relative).  This replaces that one cast: the same formula with the statistics in the input's dtype."""
    import types
    from transformers.models.t5.modeling_t5 import T5LayerNorm

    def forward(self, hidden_states):
        variance = hidden_states.pow(2).mean(-1, keepdim=True)
        return self.weight * (hidden_states * torch.rsqrt(variance + self.variance_epsilon))
    for m in stack.modules():
        if isinstance(m, T5LayerNorm):
            m.forward = types.MethodType(forward, m)
    return stack


@pytest.mark.parametrize("d_model,heads,d_kv,d_ff,layers,S", [(64, 2, 32, 256, 2, 6), (128, 2, 64, 512, 2, 77)])
def test_float64_restatement_equals_the_library_in_float64(d_model, heads, d_kv, d_ff, layers, S):
    """To 1e-12 against the library's T5Stack in float64 with its norm statistics kept in float64 too, and to 1e-5 against the library as it is:
    its T5LayerNorm computes the mean of squares in float32 even in a float64 model, which no float64 restatement can follow to 1e-12.  The
    second bound: a float32 mean of D squares is within (log2 D + 2) 2^-24 < 6e-7 relative, the reciprocal square root halves that, and the
    five norms of a two-layer stack each pass it on to the output -- 1.5e-6 before any amplification by the blocks; 1e-5 leaves room for that
    and is four orders below the bf16 errors the GPU tests compare (measured: 1.6e-7 and 1.1e-7)."""
    from x2i_amd.t5 import relative_bias_table
    cfg, stack = _lib_stack(d_model, heads, d_kv, d_ff, layers)
    sd = TR.random_stack_state_dict(stack, seed=3)
    stack = stack.double()
    stack.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    x = torch.randn((2, S, d_model), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    as_is = stack(inputs_embeds=x).last_hidden_state
    want = _keep_norm_statistics_in_float64(stack)(inputs_embeds=x).last_hidden_state
    R = cfg.relative_attention_max_distance
    table = relative_bias_table(sd["block.0.layer.0.SelfAttention.relative_attention_bias.weight"].double(), cfg.relative_attention_num_buckets, R)
    got = TR.stack_reference(sd, x, num_heads=heads, d_kv=d_kv, eps=cfg.layer_norm_epsilon, table=table.double(), R=R)
    print("restatement vs library: float64 statistics %.3e, as it is %.3e" % (TR.rel_l2(got, want), TR.rel_l2(got, as_is)))
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert TR.rel_l2(got, want) <= 1e-12
    assert TR.rel_l2(got, as_is) <= 1e-5
    assert float(want.abs().max()) > 0.5 and float(want.std()) > 0.1      # a live output, not a collapsed one


# ---------------------------------------------------------------------------------------------------------------- the checkers reject
def _wrong_attention(Q, K, V, table, S, R, kind):
    """float64 attention with one deliberate mistake"""
    f = torch.float64
    pos = torch.arange(S)
    rel = pos[None, :] - pos[:, None]
    scale = 1.0
    if kind == "transposed":
        idx = (-rel).clamp(-R, R) + R
    elif kind == "off_by_one":
        idx = (rel + 1).clamp(-R, R) + R
    elif kind == "unclamped_modulo":
        idx = (rel + R) % (2 * R + 1)
    else:
        idx = rel.clamp(-R, R) + R
        if kind == "scaled":
            scale = Q.shape[-1] ** -0.5
    q, k, v = (t[:, :, :S].to(f) for t in (Q, K, V))
    out = torch.softmax((q @ k.transpose(-1, -2)) * scale + table.to(f)[:, idx], -1) @ v
    if kind == "tile_1pct":
        out[0, 1, 64:128] *= 1.01
    return out


@pytest.mark.parametrize("kind", ["transposed", "off_by_one", "unclamped_modulo", "scaled", "tile_1pct"])
def test_attention_checker_rejects(kind):
    B, H, S, dk, R = 1, 2, 300, 64, 128
    Q, K, V, table = TR.attention_inputs(B, H, S, dk, R, seed=11)
    ref = TR.attention_reference(Q, K, V, table, S, R)
    TR.check_attention("exact", _wrong_attention(Q, K, V, table, S, R, "none"), ref)          # the restatement without a mistake passes
    TR.check_attention("bf16 output", ref.bfloat16(), ref)                                      # ... and so does one rounding of it
    with pytest.raises(AssertionError):
        TR.check_attention(kind, _wrong_attention(Q, K, V, table, S, R, kind), ref)


def test_attention_checker_rejects_a_small_clamp_mistake():
    """R = 4 on S = 77: the clamp is hit inside one tile; a table read past the clamp (modulo the table length) is caught there too"""
    Q, K, V, table = TR.attention_inputs(2, 3, 77, 64, 4, seed=12)
    ref = TR.attention_reference(Q, K, V, table, 77, 4)
    TR.check_attention("exact", _wrong_attention(Q, K, V, table, 77, 4, "none"), ref)
    with pytest.raises(AssertionError):
        TR.check_attention("modulo", _wrong_attention(Q, K, V, table, 77, 4, "unclamped_modulo"), ref)


def test_rms_checker_rejects_a_mean_subtracting_norm():
    g = torch.Generator().manual_seed(5)
    x = (3.0 + torch.randn((5, 896), generator=g)).bfloat16()
    w = (1.0 + 0.1 * torch.randn((896,), generator=g)).bfloat16()
    normed = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    assert TR.check_rms("one rounding", (w.float() * normed).bfloat16(), x, w, 1e-6) <= TR.TOL_ROW
    with pytest.raises(AssertionError):     # the library's two roundings can be 2^-7 off: outside the bound
        TR.check_rms("two roundings", (w.float() * normed.bfloat16().float()).bfloat16(), x, w, 1e-6)
    xc = x.float() - x.float().mean(-1, keepdim=True)
    bad = (w.float() * (xc * torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + 1e-6))).bfloat16()
    with pytest.raises(AssertionError):
        TR.check_rms("mean-subtracting", bad, x, w, 1e-6)


def test_gated_gelu_checker_accepts_one_rounding_and_rejects_the_erf_form():
    g = torch.Generator().manual_seed(6)
    a, b = (2.0 * torch.randn((7, 256), generator=g)).bfloat16(), (2.0 * torch.randn((7, 256), generator=g)).bfloat16()
    # (the sigmoid form: torch's tanh form cancels in 1 + tanh(.) far below zero, which the kernels' x * sigmoid form does not)
    good = (TR.gelu_tanh_f64(a) * b.double()).bfloat16()
    x = torch.linspace(-4.0, 8.0, 1001, dtype=torch.float64)
    assert torch.allclose(TR.gelu_tanh_f64(x), torch.nn.functional.gelu(x, approximate="tanh"), rtol=1e-9, atol=0)
    TR.check_gated_gelu("one rounding", good, a, b)
    bad = (torch.nn.functional.gelu(a.double()) * b.double()).bfloat16()
    with pytest.raises(AssertionError):
        TR.check_gated_gelu("erf form", bad, a, b)


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import t5_ops
    lib = t5_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    assert lib.x2i_t5_attention_bf16(fake, fake, fake, fake, fake, 1, 2, 77, 128, 48, 128, 96, 77 * 96, None) < 0 and b"dk=48" in err()
    assert lib.x2i_t5_attention_bf16(fake, fake, fake, fake, fake, 1, 2, 77, 100, 64, 128, 128, 77 * 128, None) < 0 and b"Spad" in err()
    assert lib.x2i_t5_attention_bf16(fake, fake, fake, None, fake, 1, 2, 77, 128, 64, 128, 128, 77 * 128, None) < 0 and b"null" in err()
    assert lib.x2i_t5_attention_bf16(fake, fake, fake, fake, fake, 1, 2, 77, 128, 64, 4096, 128, 77 * 128, None) < 0 and b"R=4096" in err()
    assert lib.x2i_t5_attention_bf16(fake, fake, fake, fake, fake, 1, 2, 77, 128, 64, 128, 64, 77 * 64, None) < 0      # ldo < H * dk
    assert lib.x2i_t5_head_split_bf16(fake, 384, fake, fake, fake, 1, 77, 128, 2, 40, None) < 0 and b"dk=40" in err()
    assert lib.x2i_t5_head_split_bf16(fake, 380, fake, fake, fake, 1, 77, 128, 2, 64, None) < 0
    assert lib.x2i_t5_rms_rows_bf16(fake, 100, fake, 100, fake, 4, 100, 1e-6, None) < 0 and b"D=100" in err()
    assert lib.x2i_t5_gated_gelu_bf16(fake, 24, fake, 12, 4, 12, None) < 0 and b"F=12" in err()


# ---------------------------------------------------------------------------------------------------------------- host modules
def test_unsupported_configurations_and_masks_raise():
    from x2i_amd.t5 import T5EncoderModel, T5Stack
    ok = dict(d_model=64, d_kv=32, num_heads=2, d_ff=128, num_layers=1, vocab_size=16, device="cpu")
    for bad in (dict(is_decoder=True), dict(feed_forward_proj="relu"), dict(feed_forward_proj="gated-silu"), dict(dense_act_fn="relu"), dict(d_kv=48),
                dict(d_kv=256)):
        with pytest.raises(ValueError):
            T5Stack(**dict(ok, **bad))
    with pytest.raises(ValueError):
        T5Stack(dtype=torch.float32, **ok)
    m = T5Stack(**ok)
    x = torch.zeros((1, 6, 64), dtype=torch.bfloat16)
    mask = torch.ones((1, 6), dtype=torch.long)
    mask[0, 5] = 0
    with pytest.raises(ValueError):
        m(inputs_embeds=x, attention_mask=mask)
    with pytest.raises(ValueError):
        m()
    from x2i_amd._lib import X2IError
    with pytest.raises(X2IError):      # an all-ones mask is accepted; on the CPU the first launch then refuses: no fallback
        m(inputs_embeds=x, attention_mask=torch.ones((1, 6), dtype=torch.long))
    with pytest.raises(ValueError):
        T5EncoderModel(**ok)(input_ids=torch.zeros((1, 6), dtype=torch.long), output_hidden_states=True)


def test_parameter_names_are_the_librarys_and_views_share_stacked_storage():
    from x2i_amd.t5 import T5EncoderModel, T5Stack
    cfg, stack = _lib_stack(64, 2, 32, 128, 2)
    m = T5Stack(cfg, device="cpu")
    want = {k: tuple(v.shape) for k, v in stack.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    sd = TR.random_stack_state_dict(stack, seed=1)
    m.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    inner = 64
    assert torch.equal(m._fused["1.qkv"][inner:2 * inner].float(), sd["block.1.layer.0.SelfAttention.k.weight"])
    assert torch.equal(m._fused["0.wi"][128:].float(), sd["block.0.layer.1.DenseReluDense.wi_1.weight"])
    # the bias table follows the weight (cache keyed on its version counter)
    t0 = m.bias_table().clone()
    m.block[0].layer[0].SelfAttention.relative_attention_bias.weight.mul_(2.0)
    assert torch.equal(m.bias_table(), 2.0 * t0) and m.bias_table().shape == (2, 257)
    e = T5EncoderModel(cfg, device="cpu")
    assert e.encoder.embed_tokens.weight is e.shared.weight
    assert set(e.state_dict()) == {"shared.weight"} | {"encoder." + k for k in want}


def test_legacy_heads_keep_the_library_stack_by_default():
    import x2i_amd.proj as XP
    from x2i_amd.t5 import T5Stack
    kw = dict(in_channels=2, input_dim=64, output_dim0=32, output_dim1=64, num_layers=1, num_heads=2, head_dim=32, device="cpu")
    assert type(XP.Proj(**kw).t5stack).__module__.startswith("transformers.")
    m = XP.Proj(hip_t5=True, **kw)
    assert isinstance(m.t5stack, T5Stack)
    assert set(m.state_dict()) == set(XP.Proj(**kw).state_dict())


def test_encoder_model_reads_single_and_sharded_library_checkpoints(tmp_path):
    """from_pretrained on what the library's save_pretrained writes: config.json + model.safetensors, and shards behind an index file"""
    from transformers import T5EncoderModel as LibraryEncoder
    from x2i_amd.t5 import T5EncoderModel
    torch.manual_seed(0)
    lib = LibraryEncoder(TR.library_config(128, 2, 64, 512, 2, vocab=64)).eval()
    sd = {k: v.detach().float().bfloat16() for k, v in lib.state_dict().items()}
    lib.save_pretrained(str(tmp_path / "one"))
    lib.save_pretrained(str(tmp_path / "two"), max_shard_size="1200KB")
    assert os.path.exists(tmp_path / "one" / "model.safetensors")
    assert os.path.exists(tmp_path / "two" / "model.safetensors.index.json") and len([f for f in os.listdir(tmp_path / "two") if f.endswith(".safetensors")]) >= 2
    for d in ("one", "two"):
        m = T5EncoderModel.from_pretrained(str(tmp_path / d), device="cpu")
        got = m.state_dict()
        assert set(got) == set(sd) | {"encoder.embed_tokens.weight"}
        for k, v in got.items():
            assert v.dtype == torch.bfloat16 and torch.equal(v, sd[k if k in sd else "shared.weight"]), k
        assert (m.config.d_model, m.config.d_kv, m.config.num_heads, m.config.d_ff, m.config.num_layers, m.config.vocab_size) == (128, 64, 2, 512, 2, 64)
