"""The CLIP text encoder on the HIP path (include/x2i_clip.h, x2i_amd/clip.py, x2i_amd/text_encoders.py) on the GPU: each kernel against its
float64 checker of tests/clip_ref.py or bit for bit against torch, and the model, from_pretrained and the pair of prompt encoders against
the library in float64 (and no worse than 1.5 x the library's own bf16 run on the same GPU)."""
import os

import pytest
import torch

from tests import clip_ref as CR
from tests import t5_ref as TR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned, stack_errors  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 64 ** -0.5


@pytest.fixture(scope="module")
def clip_ops():
    from x2i_amd import clip_ops as o
    o.load()
    return o


# ---------------------------------------------------------------------------------------------------------------- attention
def run_attention(clip_ops, Q, K, V, S, extra_cols=0, extra_rows=0, scale=SCALE):
    """-> (O [B, H, S, dk] view, the whole sentinel-filled output buffer [B, S + extra_rows, H * dk + extra_cols])"""
    B, H, Spad, dk = Q.shape
    VT = V.transpose(-1, -2).contiguous()
    ldo = H * dk + extra_cols
    buf = poisoned(B, S + extra_rows, ldo)
    clip_ops.attention_causal(Q, K, VT, buf, B, H, S, Spad, dk, scale, ldo, (S + extra_rows) * ldo)
    return buf[:, :S, :H * dk].reshape(B, S, H, dk).permute(0, 2, 1, 3), buf


# (B, H, S), dk 64: one key, one row; ragged with three heads; the diagonal tile exactly full; one row reaches a second key tile; a second
# query block whose first tile is wholly in the past; five tiles, so early blocks skip most; the product shape
# Worst tile measured on the MI355X, in this order: 0, 2.16e-3, 1.81e-3, 2.86e-3, 2.05e-3, 2.29e-3, 2.60e-3 (bound TOL_O = 5e-3)
ATTENTION_CASES = [(1, 1, 1), (2, 3, 77), (1, 2, 64), (1, 2, 65), (1, 2, 130), (1, 2, 300), (2, 12, 77)]


@pytest.mark.parametrize("B,H,S", ATTENTION_CASES)
def test_attention_vs_fp64_per_tile(clip_ops, B, H, S):
    Q, K, V = CR.attention_inputs(B, H, S, 64, seed=1000 * S + H, device=DEV)
    ref = CR.attention_reference(Q, K, V, S, SCALE)
    O, buf = run_attention(clip_ops, Q, K, V, S, extra_cols=8, extra_rows=3)
    worst = CR.check_attention("clip_attention B=%d H=%d S=%d" % (B, H, S), O, ref, CR.TOL_O)
    print("clip_attention B=%d H=%d S=%d: worst tile rel-L2 %.3e (bound %.1e)" % (B, H, S, worst, CR.TOL_O))
    # nothing outside rows < S and columns < H * dk is written
    assert bool(is_sentinel(buf[:, S:]).all()) and bool(is_sentinel(buf[:, :, H * 64:]).all())
    assert not bool(is_sentinel(buf[:, :S, :H * 64]).any())
    # a relaunch is bit-identical, and sample 0 does not depend on the batch it is launched in
    O2, _ = run_attention(clip_ops, Q, K, V, S, extra_cols=8, extra_rows=3)
    assert torch.equal(O2, O)
    if B > 1:
        O1, _ = run_attention(clip_ops, Q[:1].contiguous(), K[:1].contiguous(), V[:1].contiguous(), S)
        assert torch.equal(O1[0], O[0])


@pytest.mark.parametrize("S", [77, 130])
def test_attention_row_0_is_its_own_value_row(clip_ops, S):
    """Row 0 attends to one key: its probability is 1 whatever the maximum bookkeeping does, so O[b][0] = V[b][h][0] within one rounding of P
    and one of O (2 * TOL_ROW per element)"""
    Q, K, V = CR.attention_inputs(2, 3, S, 64, seed=5 + S, device=DEV)
    O, _ = run_attention(clip_ops, Q, K, V, S)
    got, want = O[:, :, 0].double(), V[:, :, 0].double()
    assert bool(((got - want).abs() <= 2 * TR.TOL_ROW * want.abs()).all())


def test_attention_ignores_future_keys_and_values(clip_ops):
    """S = 77: K and V at positions >= 40 replaced by other finite values (-3 x + 100; the padding rows 77 .. 127 become 100).  Rows < 40
    are bit-identical, rows >= 40 are not: a mask applied by data, a leaked maximum or a wrong diagonal each fail this."""
    B, H, S = 2, 3, 77
    Q, K, V = CR.attention_inputs(B, H, S, 64, seed=21, device=DEV)
    O, _ = run_attention(clip_ops, Q, K, V, S)
    K2, V2 = K.clone(), V.clone()
    K2[:, :, 40:] = (-3.0 * K[:, :, 40:].float() + 100.0).bfloat16()
    V2[:, :, 40:] = (-3.0 * V[:, :, 40:].float() + 100.0).bfloat16()
    O2, _ = run_attention(clip_ops, Q, K2, V2, S)
    assert torch.equal(O2[:, :, :40], O[:, :, :40])
    changed = (O2[:, :, 40:] != O[:, :, 40:]).any(-1)
    assert bool(changed.all())
    CR.check_attention("clip_attention, changed future", O2, CR.attention_reference(Q, K2, V2, S, SCALE), CR.TOL_O)


@pytest.mark.parametrize("S,Spad", [(77, 128), (300, 320)])
def test_attention_masks_future_keys_by_index_under_adversarial_magnitudes(clip_ops, S, Spad):
    """Q and K shifted along one shared unit direction u per head, as test_t5_gpu's test_attention_masks_padding_keys_by_index... does, by
    sqrt(72) instead of 3 because these scores carry the scale 1/8: (q - c u).(k + c u) / 8 loses 9 on every valid pair.  The padding rows of
    K hold -c u and score near +9, with V = 50 there.  Second launch: every real key after position 20 flipped in sign, so that the future
    tokens of rows <= 20 -- inside the diagonal tile -- score near +9 as well.  Any of them let into the maximum or the sum would own the row."""
    B, H, c = 1, 2, 72.0 ** 0.5
    Q, K, V = CR.attention_inputs(B, H, S, 64, seed=7, Spad=Spad, device=DEV)
    u = torch.randn((B, H, 1, 64), generator=torch.Generator().manual_seed(8)).to(DEV)
    u /= u.norm(dim=-1, keepdim=True)
    Q[:, :, :S] = (Q[:, :, :S].float() - c * u).bfloat16()
    K[:, :, :S] = (K[:, :, :S].float() + c * u).bfloat16()
    K[:, :, S:] = (-c * u).bfloat16()
    V[:, :, S:] = 50.0
    ref = CR.attention_reference(Q, K, V, S, SCALE)
    O, _ = run_attention(clip_ops, Q, K, V, S)
    CR.check_attention("clip_attention anti", O, ref, CR.TOL_O)
    # and with the real future tokens scoring high as well: every key after position 20 flipped, for the rows up to 20
    K2 = K.clone()
    K2[:, :, 21:S] = (-K[:, :, 21:S].float()).bfloat16()
    O2, _ = run_attention(clip_ops, Q, K2, V, S)
    assert torch.equal(O2[:, :, :21], O[:, :, :21])
    CR.check_attention("clip_attention anti, flipped future", O2, CR.attention_reference(Q, K2, V, S, SCALE), CR.TOL_O)


@pytest.mark.parametrize("B,H,S", [(2, 3, 77), (1, 2, 130)])
def test_attention_is_the_qwen_kernel_without_groups_or_ranges(clip_ops, B, H, S):
    """x2i_clip_attention_bf16 launches the causal kernel of x2i_qwen_attention_bf16 with Hq = Hkv and no key ranges: the two entry points
    agree bit for bit.  Ragged in one query block; a second query block, one row reaching tile 2, Spad = 192 (no multiple of 128)"""
    from x2i_amd import qwen_ops
    Q, K, V = CR.attention_inputs(B, H, S, 64, seed=3000 * S + H, device=DEV)
    O, _ = run_attention(clip_ops, Q, K, V, S)
    buf = poisoned(B, S, H * 64)
    qwen_ops.attention(Q, K, V.transpose(-1, -2).contiguous(), buf, B, H, H, S, Q.shape[2], 64, SCALE, H * 64, S * H * 64)
    assert torch.equal(buf.reshape(B, S, H, 64).permute(0, 2, 1, 3), O)
    assert not bool(is_sentinel(buf).any())


def test_attention_refuses_other_head_widths(clip_ops):
    from x2i_amd._lib import X2IError
    Q, K, V = CR.attention_inputs(1, 1, 6, 64, seed=1, device=DEV)
    for dk in (32, 128):
        with pytest.raises(X2IError):
            clip_ops.attention_causal(Q, K, V, poisoned(1, 6, 128), 1, 1, 6, 64, dk, SCALE, 128, 6 * 128)


# ---------------------------------------------------------------------------------------------------------------- embed
def test_embed_is_the_torch_sum_and_clamps_foreign_ids(clip_ops):
    B, S, D, vocab = 3, 77, 128, 50
    g = torch.Generator().manual_seed(3)
    tok, pos = torch.randn((vocab, D), generator=g).bfloat16().to(DEV), torch.randn((80, D), generator=g).bfloat16().to(DEV)
    ids = torch.randint(0, vocab, (B, S), generator=g).to(DEV)
    ids[0, 0], ids[1, 5], ids[2, 76] = 0, vocab - 1, vocab - 1
    want = (tok[ids].float() + pos[:S].float()).bfloat16().reshape(B * S, D)
    X = poisoned(B * S + 2, D)
    clip_ops.embed(ids, tok, pos, out=X)
    assert torch.equal(X[:B * S], want) and bool(is_sentinel(X[B * S:]).all())
    # an id outside the table (a contract violation the host cannot see) is clamped: the launch reads nothing out of bounds and disturbs no other row
    bad = ids.clone()
    bad[1, 7], bad[2, 0] = vocab, -1
    X2 = poisoned(B * S + 2, D)
    clip_ops.embed(bad, tok, pos, out=X2)
    torch.cuda.synchronize()
    keep = torch.ones(B * S, dtype=torch.bool, device=DEV)
    keep[1 * S + 7] = keep[2 * S + 0] = False
    assert torch.equal(X2[:B * S][keep], want[keep]) and bool(is_sentinel(X2[B * S:]).all())


# ---------------------------------------------------------------------------------------------------------------- quick GELU
@pytest.mark.parametrize("rows,F", [(1, 64), (77, 3072), (3, 104)])
def test_quick_gelu_vs_fp64_per_element(clip_ops, rows, F):
    x = (2.0 * torch.randn((rows, F), generator=torch.Generator().manual_seed(rows * 100000 + F))).bfloat16().to(DEV)
    y = clip_ops.quick_gelu(x)
    assert y.shape == (rows, F)
    worst = CR.check_quick_gelu("clip_quick_gelu %dx%d" % (rows, F), y, x)
    print("clip_quick_gelu %dx%d: worst relative error %.3e (bound %.3e)" % (rows, F, worst, CR.TOL_ROW + 2.0 ** -19))
    # row strides: rows of a wider buffer in, rows of a wider sentinel-filled buffer out
    xw = torch.zeros((rows, F + 16), device=DEV, dtype=torch.bfloat16)
    xw[:, :F] = x
    yw = poisoned(rows, F + 8)
    clip_ops.quick_gelu(xw[:, :F], out=yw, rows=rows, ldx=F + 16, ldy=F + 8)
    assert torch.equal(yw[:, :F], y) and bool(is_sentinel(yw[:, F:]).all())


# ---------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("eos_token_id", [2, 41])
@pytest.mark.parametrize("S", [77, 300])
def test_pool_gathers_the_eos_row(clip_ops, eos_token_id, S):
    """Both rules at D = 128, bit-equal to torch indexing, with indices 0, middle and S - 1; a sample without an eos (or all ids equal) gives 0;
    S = 300: more positions than the workgroup has threads"""
    B, D, vocab = 4, 128, 64
    ids = CR.ids_with_eos_at(B, S, vocab, (0, S // 2, S - 1, S - 1), eos_token_id, seed=S)
    ids[3] = 7                                     # no eos; every id the same
    idx = CR.pool_index(ids, eos_token_id)
    assert idx.tolist() == [0, S // 2, S - 1, 0]
    Hs = torch.randn((B, S, D), generator=torch.Generator().manual_seed(2)).bfloat16().to(DEV)
    out = poisoned(B + 1, D + 8)
    clip_ops.pool(ids.to(DEV), Hs, eos_token_id, out=out, ldp=D + 8)
    assert torch.equal(out[:B, :D], Hs[torch.arange(B), idx.to(DEV)])
    assert bool(is_sentinel(out[B:]).all()) and bool(is_sentinel(out[:, D:]).all())


# ---------------------------------------------------------------------------------------------------------------- model
def _lib_and_hip(hidden, heads, layers, inter, seed, vocab=64, eos_token_id=2):
    from x2i_amd.clip import CLIPTextModel
    cfg, lib = CR.library_model(hidden, heads, layers, inter, vocab=vocab, eos_token_id=eos_token_id)
    sd = CR.random_model_state_dict(lib, seed=seed)
    lib.load_state_dict(sd, strict=True)
    hip = CLIPTextModel(cfg, device=DEV)
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    return cfg, lib, hip


def model_errors(name, out, lib, ids):
    """The criterion's two pairs, of last_hidden_state and of pooler_output: each (error of the HIP path, error of the library's bf16 run on
    the GPU), rel-L2 against the library in float64 on the CPU.  lib: the library module on the CPU holding bf16 values"""
    ref = lib.double()(ids, output_hidden_states=False)
    lib_bf16 = lib.to(device=DEV, dtype=torch.bfloat16)(ids.to(DEV), output_hidden_states=False)
    pairs = []
    for field in ("last_hidden_state", "pooler_output"):
        e_hip, e_lib = CR.rel_l2(getattr(out, field), getattr(ref, field)), CR.rel_l2(getattr(lib_bf16, field), getattr(ref, field))
        print("%s %s: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, field, e_hip, e_lib, e_hip / e_lib))
        pairs.append((e_hip, e_lib))
    return pairs


# (hidden, heads, layers, intermediate, B, S); a short prompt; one full-width layer.  Measured on MI355X, HIP / library bf16 against float64
# (last_hidden_state; pooler_output): 4.23e-3 / 4.40e-3; 4.46e-3 / 4.32e-3 -- 4.28e-3 / 4.47e-3; 4.48e-3 / 4.20e-3 -- 3.60e-3 / 3.78e-3; 3.65e-3 / 3.89e-3
# (ratio 0.94 .. 1.07; the criterion allows 1.5)
MODEL_CASES = [(128, 2, 2, 512, 2, 77), (256, 4, 2, 1024, 2, 20), (768, 12, 1, 3072, 2, 77)]


@pytest.mark.parametrize("hidden,heads,layers,inter,B,S", MODEL_CASES)
def test_model_vs_library_fp64_and_bf16(hidden, heads, layers, inter, B, S):
    cfg, lib, hip = _lib_and_hip(hidden, heads, layers, inter, seed=hidden + S)
    ids = CR.ids_with_eos_at(B, S, 64, (S // 2, S - 1)[:B], 2, seed=S)
    out = hip(ids.to(DEV), output_hidden_states=False)
    assert out[0] is out.last_hidden_state and out[1] is out.pooler_output
    assert out[0].shape == (B, S, hidden) and out[1].shape == (B, hidden) and out[0].dtype == out[1].dtype == torch.bfloat16
    assert torch.equal(out[1], out[0][torch.arange(B), CR.pool_index(ids, 2).to(DEV)])
    for e_hip, e_lib in model_errors("CLIPTextModel hidden=%d heads=%d layers=%d inter=%d B=%d S=%d" % (hidden, heads, layers, inter, B, S), out, lib, ids):
        assert_stack_criterion(e_hip, e_lib)


def test_model_forward_allocates_only_its_outputs_and_repeats_bit_for_bit():
    from x2i_amd.clip import CLIPTextModel
    hip = CLIPTextModel(hidden_size=128, num_attention_heads=2, intermediate_size=512, num_hidden_layers=2, vocab_size=64, eos_token_id=2,
                        device=DEV).init_random_(1)
    ids = torch.randint(0, 64, (2, 77), generator=torch.Generator().manual_seed(2)).to(DEV)
    first = hip(ids)
    keep = (first[0].clone(), first[1].clone())
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    out = hip(ids)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] - before == 2       # last_hidden_state and pooler_output
    assert torch.equal(out[0], keep[0]) and torch.equal(out[1], keep[1]) and out[0].shape == (2, 77, 128)
    assert float(out[0].float().std()) > 0.1


@pytest.mark.parametrize("spelling", ["library", "text_model"])
def test_from_pretrained_on_a_library_checkpoint(tmp_path, spelling):
    """A directory written by the library's save_pretrained; and the same file re-keyed to the `text_model.` prefix of the 4.x checkpoints"""
    from safetensors.torch import load_file, save_file
    from transformers import CLIPTextModel as LibraryModel
    from x2i_amd.clip import CLIPTextModel
    cfg, lib, _ = _lib_and_hip(128, 2, 2, 512, seed=9, eos_token_id=41)
    lib.save_pretrained(str(tmp_path))
    lib2 = LibraryModel.from_pretrained(str(tmp_path)).eval().requires_grad_(False)
    if spelling == "text_model":
        f = str(tmp_path / "model.safetensors")
        sd = load_file(f)
        assert not any(k.startswith("text_model.") for k in sd)
        save_file(CR.with_prefix(sd), f)
    hip = CLIPTextModel.from_pretrained(str(tmp_path), torch_dtype=torch.bfloat16, device=DEV)
    assert hip.config.eos_token_id == 41
    ids = CR.ids_with_eos_at(2, 77, 64, (30, 76), 41, seed=11)
    out = hip(ids.to(DEV), output_hidden_states=False)
    assert out.pooler_output.shape == (2, 128) and out.last_hidden_state.shape == (2, 77, 128)
    for e_hip, e_lib in model_errors("CLIPTextModel.from_pretrained (%s keys)" % spelling, out, lib2, ids):
        assert_stack_criterion(e_hip, e_lib)


def test_text_encoders_from_a_pipeline_directory(tmp_path):
    """Tiny `text_encoder/` and `text_encoder_2/` subfolders written by the library; get_t5_input_embeds(clip_ids [2, 77], t5_ids [2, 20]) ->
    bf16 [2, 128] and [2, 20, d_model], each under the criterion against the library pair"""
    from transformers import CLIPTextModel as LibraryCLIP, T5EncoderModel as LibraryT5
    from x2i_amd.text_encoders import TextEncoders
    _, clip_lib, _ = _lib_and_hip(128, 2, 2, 512, seed=13)
    clip_lib.save_pretrained(str(tmp_path / "text_encoder"))
    torch.manual_seed(0)
    t5_lib = LibraryT5(TR.library_config(128, 2, 64, 512, 2, vocab=64)).eval().requires_grad_(False)
    sd = TR.random_stack_state_dict(t5_lib.encoder, seed=14)
    sd["embed_tokens.weight"] = torch.randn((64, 128), generator=torch.Generator().manual_seed(15)).bfloat16().float()
    t5_lib.encoder.load_state_dict(sd, strict=True)
    t5_lib.save_pretrained(str(tmp_path / "text_encoder_2"))
    assert os.path.exists(tmp_path / "text_encoder" / "model.safetensors") and os.path.exists(tmp_path / "text_encoder_2" / "model.safetensors")
    te = TextEncoders.from_pretrained(str(tmp_path), DEV)
    clip_ids = CR.ids_with_eos_at(2, 77, 64, (12, 76), 2, seed=16)
    t5_ids = torch.randint(0, 64, (2, 20), generator=torch.Generator().manual_seed(17))
    pooled, embeds = te.get_t5_input_embeds(clip_ids, t5_ids)
    assert pooled.shape == (2, 128) and embeds.shape == (2, 20, 128) and pooled.dtype == embeds.dtype == torch.bfloat16
    assert pooled.device.type == embeds.device.type == "cuda"
    clip2 = LibraryCLIP.from_pretrained(str(tmp_path / "text_encoder")).eval().requires_grad_(False)
    t52 = LibraryT5.from_pretrained(str(tmp_path / "text_encoder_2")).eval().requires_grad_(False)
    e = stack_errors("TextEncoders pooled_prompt_embeds", pooled, clip2.float(), lambda m, dev, dt: m(clip_ids.to(dev), output_hidden_states=False).pooler_output)
    assert_stack_criterion(*e)
    e = stack_errors("TextEncoders prompt_embeds", embeds, t52.float(), lambda m, dev, dt: m(t5_ids.to(dev), output_hidden_states=False)[0])
    assert_stack_criterion(*e)
