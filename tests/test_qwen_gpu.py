"""The Qwen2 decoder prefill on the HIP path (include/x2i_qwen.h, x2i_amd/qwen.py, handoff.HipPrefill) on the GPU: each kernel against its
float64 checker of tests/qwen_ref.py or bit for bit against torch, and the stack and the hand-off against the library in float64 (and no
worse than 1.5 x the library's own bf16 run on the same GPU)."""
import pytest
import torch

from tests import qwen_ref as QR
from tests import t5_ref as TR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned, stack_errors  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def qwen_ops():
    from x2i_amd import qwen_ops as o
    o.load()
    return o


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- attention
def run_attention(qwen_ops, Q, K, V, S, k_lo=None, k_hi=None, extra_cols=0, extra_rows=0, scale=None):
    """-> (O [B, Hq, S, dk] view, the whole sentinel-filled output buffer [B, S + extra_rows, Hq * dk + extra_cols])"""
    B, Hq, Spad, dk = Q.shape
    Hkv = K.shape[1]
    VT = V.transpose(-1, -2).contiguous()
    ldo = Hq * dk + extra_cols
    buf = poisoned(B, S + extra_rows, ldo)
    qwen_ops.attention(Q, K, VT, buf, B, Hq, Hkv, S, Spad, dk, dk ** -0.5 if scale is None else scale, ldo, (S + extra_rows) * ldo, _i32(k_lo), _i32(k_hi))
    return buf[:, :S, :Hq * dk].reshape(B, S, Hq, dk).permute(0, 2, 1, 3), buf


# (B, Hq, Hkv, S, dk, k_lo, k_hi).  Without ranges: one key; ragged, groups of two; the diagonal tile exactly full; one row reaches a second
# tile; the 7B's group of seven over two query blocks; five tiles, groups of one; InternVL-1B's heads of 64.  With ranges: right padding; a
# range that starts inside tile 1 and inside the wave that holds rows 64..95; both ends, one start on a tile boundary; two single-key ranges.
ATTENTION_CASES = [
    (1, 1, 1, 1, 128, None, None), (2, 4, 2, 77, 128, None, None), (1, 2, 1, 64, 128, None, None), (1, 2, 1, 65, 128, None, None),
    (1, 7, 1, 130, 128, None, None), (1, 2, 2, 300, 128, None, None), (1, 14, 2, 130, 64, None, None),
    (2, 4, 2, 130, 128, [0, 0], [50, 130]), (2, 4, 2, 130, 128, [70, 0], [130, 130]), (2, 2, 1, 200, 128, [64, 5], [200, 199]),
    (1, 2, 1, 77, 128, [76], [77]), (1, 2, 1, 77, 128, [0], [1]),
]


@pytest.mark.parametrize("B,Hq,Hkv,S,dk,k_lo,k_hi", ATTENTION_CASES)
def test_attention_vs_fp64_per_tile(qwen_ops, B, Hq, Hkv, S, dk, k_lo, k_hi):
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=1000 * S + dk + Hq, device=DEV)
    ref = QR.attention_reference(Q, K, V, S, dk ** -0.5, k_lo, k_hi)
    O, buf = run_attention(qwen_ops, Q, K, V, S, k_lo, k_hi, extra_cols=8, extra_rows=3)
    name = "qwen_attention B=%d Hq=%d Hkv=%d S=%d dk=%d range %s..%s" % (B, Hq, Hkv, S, dk, k_lo, k_hi)
    worst = QR.check_attention(name, O, ref, QR.TOL_O, k_lo=k_lo)
    print("%s: worst tile rel-L2 %.3e (bound %.1e)" % (name, worst, QR.TOL_O))
    # nothing outside rows < S and columns < Hq * dk is written, and every element inside is
    assert bool(is_sentinel(buf[:, S:]).all()) and bool(is_sentinel(buf[:, :, Hq * dk:]).all())
    assert not bool(is_sentinel(buf[:, :S, :Hq * dk]).any())
    # a relaunch is bit-identical, and sample 0 does not depend on the batch it is launched in
    O2, _ = run_attention(qwen_ops, Q, K, V, S, k_lo, k_hi, extra_cols=8, extra_rows=3)
    assert torch.equal(O2, O)
    if B > 1:
        one = lambda v: None if v is None else v[:1]
        O1, _ = run_attention(qwen_ops, Q[:1].contiguous(), K[:1].contiguous(), V[:1].contiguous(), S, one(k_lo), one(k_hi))
        assert torch.equal(O1[0], O[0])


@pytest.mark.parametrize("Hq,Hkv,dk", [(7, 1, 128), (4, 2, 128), (6, 3, 64)])
def test_attention_group_mapping_known_answer(qwen_ops, Hq, Hkv, dk):
    """The value rows of key/value head g all equal g + 1: every output row of query head h is h // rep + 1 whatever the scores are, within
    one rounding of P and one of O (2 * TOL_ROW relative).  h % Hkv gives other numbers for every head past the first group."""
    B, S = 2, 130
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=31, device=DEV)
    for g in range(Hkv):
        V[:, g] = g + 1.0
    O, _ = run_attention(qwen_ops, Q, K, V, S)
    want = (torch.arange(Hq, device=DEV) // (Hq // Hkv) + 1.0).double()[None, :, None, None]
    assert bool(((O.double() - want).abs() <= 2 * TR.TOL_ROW * want).all())


@pytest.mark.parametrize("k_lo,k_hi", [([70, 0], [130, 130]), ([64, 129], [130, 130]), ([5, 100], [5, 90])])
def test_attention_rows_with_no_counted_key_are_exactly_zero(qwen_ops, k_lo, k_hi):
    """V = 50 and K = -c u outside the range (and in the padding beyond S), q = q' - c u: were a masked key let in, it would score near +9
    and own the row; were a row's masked scores exponentiated against a maximum that never left its initial value, the row would be 50.
    Rows before k_lo -- inside a computing wave ([70, 130): rows 64..69), in waves and blocks that compute nothing, and the rows of an
    empty range ([5, 5), [100, 90)) -- are exactly 0 and written; every other row has its float64 value."""
    B, Hq, Hkv, S, dk, c = 2, 4, 2, 130, 128, (9.0 * 128 ** 0.5) ** 0.5
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=41, device=DEV)
    u = torch.randn((B, Hkv, 1, dk), generator=torch.Generator().manual_seed(42)).to(DEV)
    u /= u.norm(dim=-1, keepdim=True)
    Q[:, :, :S] = (Q[:, :, :S].float() - c * u.repeat_interleave(Hq // Hkv, dim=1)).bfloat16()
    for b in range(B):
        lo, hi = k_lo[b], max(k_hi[b], k_lo[b])
        for sl in (slice(0, lo), slice(hi, None)):
            K[b, :, sl] = (-c * u[b]).bfloat16()
            V[b, :, sl] = 50.0
    ref = QR.attention_reference(Q, K, V, S, dk ** -0.5, k_lo, k_hi)
    O, buf = run_attention(qwen_ops, Q, K, V, S, k_lo, k_hi)
    assert not bool(is_sentinel(buf).any())
    for b in range(B):
        n = S if k_hi[b] <= k_lo[b] else k_lo[b]
        assert bool((O[b, :, :n] == 0).all()), "sample %d: rows < %d hold %r" % (b, n, float(O[b, :, :n].double().abs().max()))
        assert bool((O[b, :, n:] != 0).any(-1).all())
    QR.check_attention("qwen_attention, zero rows", O, ref, QR.TOL_O, k_lo=k_lo)


def test_attention_ignores_future_keys_and_values(qwen_ops):
    """S = 77: K and V at positions >= 40 replaced by other finite values (-3 x + 100; the padding rows 77 .. 127 become 100).  Rows < 40
    are bit-identical, rows >= 40 are not: a mask applied by data, a leaked maximum or a wrong diagonal each fail this."""
    B, Hq, Hkv, S, dk = 2, 4, 2, 77, 128
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=21, device=DEV)
    O, _ = run_attention(qwen_ops, Q, K, V, S)
    K2, V2 = K.clone(), V.clone()
    K2[:, :, 40:] = (-3.0 * K[:, :, 40:].float() + 100.0).bfloat16()
    V2[:, :, 40:] = (-3.0 * V[:, :, 40:].float() + 100.0).bfloat16()
    O2, _ = run_attention(qwen_ops, Q, K2, V2, S)
    assert torch.equal(O2[:, :, :40], O[:, :, :40])
    changed = (O2[:, :, 40:] != O[:, :, 40:]).any(-1)
    assert bool(changed.all())
    QR.check_attention("qwen_attention, changed future", O2, QR.attention_reference(Q, K2, V2, S, dk ** -0.5), QR.TOL_O)


@pytest.mark.parametrize("S,Spad,k_lo,k_hi", [(77, 128, None, None), (300, 320, [70], [290]), (200, 256, [5], [199])])
def test_attention_masks_by_index_under_adversarial_magnitudes(qwen_ops, S, Spad, k_lo, k_hi):
    """The construction of tests/test_clip_gpu.py at dk = 128: Q and K shifted along one shared unit direction u per key/value head by c with
    c^2 / sqrt(128) = 9, so that (q - c u).(k + c u) scale loses 9 on every counted pair.  Every key outside [k_lo, k_hi) and the padding
    beyond S hold -c u and score near +9, with V = 50 there.  Second launch: every counted key after position 20 of the range flipped in
    sign, so that the future tokens of the rows up to there -- inside the diagonal tile -- score near +9 as well."""
    B, Hq, Hkv, dk = 1, 2, 1, 128
    c = (9.0 * dk ** 0.5) ** 0.5
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=7, Spad=Spad, device=DEV)
    u = torch.randn((B, Hkv, 1, dk), generator=torch.Generator().manual_seed(8)).to(DEV)
    u /= u.norm(dim=-1, keepdim=True)
    lo, hi = (0, S) if k_lo is None else (k_lo[0], k_hi[0])
    Q[:, :, :S] = (Q[:, :, :S].float() - c * u).bfloat16()
    K[:, :, lo:hi] = (K[:, :, lo:hi].float() + c * u).bfloat16()
    for sl in (slice(0, lo), slice(hi, None)):
        K[:, :, sl] = (-c * u).bfloat16()
        V[:, :, sl] = 50.0
    ref = QR.attention_reference(Q, K, V, S, dk ** -0.5, k_lo, k_hi)
    O, _ = run_attention(qwen_ops, Q, K, V, S, k_lo, k_hi)
    QR.check_attention("qwen_attention anti", O, ref, QR.TOL_O, k_lo=k_lo)
    cut = lo + 21
    K2 = K.clone()
    K2[:, :, cut:hi] = (-K[:, :, cut:hi].float()).bfloat16()
    O2, _ = run_attention(qwen_ops, Q, K2, V, S, k_lo, k_hi)
    assert torch.equal(O2[:, :, :cut], O[:, :, :cut])
    QR.check_attention("qwen_attention anti, flipped future", O2, QR.attention_reference(Q, K2, V, S, dk ** -0.5, k_lo, k_hi), QR.TOL_O, k_lo=k_lo)


def test_attention_refusals(qwen_ops):
    from x2i_amd._lib import X2IError
    Q, K, V = QR.attention_inputs(1, 4, 2, 6, 128, seed=1, device=DEV)
    out = poisoned(1, 6, 512)
    call = lambda Hq=4, Hkv=2, Spad=64, dk=128, lo=None, hi=None: qwen_ops.attention(Q, K, V, out, 1, Hq, Hkv, 6, Spad, dk, 0.1, 512, 6 * 512, lo, hi)
    for bad in (dict(dk=32), dict(dk=96), dict(Hq=3), dict(Spad=40), dict(lo=_i32([0])), dict(hi=_i32([6]))):
        with pytest.raises(X2IError):
            call(**bad)
    assert bool(is_sentinel(out).all())     # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- RoPE + head split
@pytest.mark.parametrize("B,S,Hq,Hkv,dk,mrope", [(1, 1, 1, 1, 128, False), (2, 77, 4, 2, 128, True), (1, 130, 7, 1, 128, False), (1, 70, 14, 2, 64, True)])
def test_rope_split_vs_fp64_per_element(qwen_ops, B, S, Hq, Hkv, dk, mrope):
    """Tables from rope_tables: positions up to 4000, or three differing M-RoPE axes.  q and k per element against float64 from the same f32
    tables; VT bit-equal to the torch transposition; padding rows and columns untouched; the row stride honoured."""
    from x2i_amd.qwen import rope_tables
    g = torch.Generator().manual_seed(S * 100 + dk)
    if mrope:
        pos, sec = QR.mrope_positions(B, S, seed=S), ([16, 24, 24] if dk == 128 else [8, 12, 12])
        pos[1] += 3000
    else:
        pos, sec = torch.randint(0, 4001, (B, S), generator=g), None
        pos[0, 0] = 4000
    cos, sin = rope_tables(pos.to(DEV), dk, 1000000.0, sec)
    W, Spad, ld = (Hq + 2 * Hkv) * dk, qwen_ops.pad64(S), (Hq + 2 * Hkv) * dk + 16
    qkv = torch.zeros((B * S, ld), dtype=torch.bfloat16, device=DEV)
    qkv[:, :W] = (2.0 * torch.randn((B * S, W), generator=g)).bfloat16().to(DEV)
    Q, K, VT = poisoned(B, Hq, Spad, dk), poisoned(B, Hkv, Spad, dk), poisoned(B, Hkv, dk, Spad)
    qwen_ops.rope_split(qkv, cos, sin, Q, K, VT, B, S, Spad, Hq, Hkv, dk)
    q, k, v = (t.reshape(B, S, -1, dk) for t in qkv[:, :W].view(B, S, W).split([Hq * dk, Hkv * dk, Hkv * dk], dim=-1))
    eq = QR.check_rope("qwen_rope_split q", Q[:, :, :S].transpose(1, 2), q, cos, sin)
    ek = QR.check_rope("qwen_rope_split k", K[:, :, :S].transpose(1, 2), k, cos, sin)
    print("qwen_rope_split B=%d S=%d Hq=%d Hkv=%d dk=%d: worst error / bound q %.3f k %.3f" % (B, S, Hq, Hkv, dk, eq, ek))
    assert torch.equal(VT[:, :, :, :S], v.permute(0, 2, 3, 1))
    assert bool(is_sentinel(Q[:, :, S:]).all()) and bool(is_sentinel(K[:, :, S:]).all()) and bool(is_sentinel(VT[:, :, :, S:]).all())
    # position 0 is the identity
    if not mrope:
        c0, s0 = torch.ones_like(cos), torch.zeros_like(sin)
        qwen_ops.rope_split(qkv, c0, s0, Q, K, VT, B, S, Spad, Hq, Hkv, dk)
        assert torch.equal(Q[:, :, :S].transpose(1, 2), q) and torch.equal(K[:, :, :S].transpose(1, 2), k)


# ---------------------------------------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("rows,F", [(1, 64), (77, 512), (5, 11008), (3, 104)])
def test_swiglu_vs_fp64_per_element(qwen_ops, rows, F):
    g = torch.Generator().manual_seed(rows * 100000 + F)
    ab = (2.0 * torch.randn((rows, 2 * F), generator=g)).bfloat16().to(DEV)
    y = qwen_ops.swiglu(ab)
    assert y.shape == (rows, F)
    worst = QR.check_swiglu("qwen_swiglu %dx%d" % (rows, F), y, ab[:, :F], ab[:, F:])
    print("qwen_swiglu %dx%d: worst relative error %.3e (bound %.3e)" % (rows, F, worst, QR.TOL_ROW + 2.0 ** -19))
    # row strides: rows of a wider buffer in, rows of a wider sentinel-filled buffer out
    abw = torch.zeros((rows, 2 * F + 16), device=DEV, dtype=torch.bfloat16)
    abw[:, :2 * F] = ab
    yw = poisoned(rows, F + 8)
    qwen_ops.swiglu(abw[:, :2 * F], out=yw, rows=rows, ld_in=2 * F + 16, ldy=F + 8)
    assert torch.equal(yw[:, :F], y) and bool(is_sentinel(yw[:, F:]).all())


# ---------------------------------------------------------------------------------------------------------------- stack
def _masked(t, k_lo):
    """t [B, C, S, D] (or [B, S, D]) with the rows s < k_lo[b] -- where the library defines nothing -- set to zero on both sides of a comparison"""
    if k_lo is None:
        return t
    t = t.clone()
    for b, lo in enumerate(k_lo):
        t[b, ..., :lo, :] = 0
    return t


def _library_slab(m, x, mask, pos, dev, dt):
    out = m(inputs_embeds=x.to(device=dev, dtype=dt), attention_mask=None if mask is None else mask.to(dev), position_ids=None if pos is None else pos.to(dev),
            output_hidden_states=True, use_cache=False)
    return torch.stack(tuple(out.hidden_states), 1)


# (hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl): sample 0 right-padded to 50; sample 1 left-padded from 70 (four heads in two groups,
# two query blocks); heads of 64, no mask; Qwen2_5_VLTextModel under three differing position axes; one layer at the 3B's width
STACK_CASES = [(256, 2, 1, 512, 2, 2, 77, [0, 0], [50, 77], False), (512, 4, 2, 1024, 2, 2, 130, [0, 70], [130, 130], False),
               (128, 2, 2, 256, 2, 1, 20, None, None, False), (256, 2, 1, 512, 2, 2, 77, None, None, True),
               (2048, 16, 2, 11008, 1, 1, 77, None, None, False)]


@pytest.mark.parametrize("hidden,Hq,Hkv,d_ff,layers,B,S,k_lo,k_hi,vl", STACK_CASES)
def test_stack_vs_library_fp64_and_bf16(hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl):
    from x2i_amd.qwen import Qwen2DecoderStack
    cfg, lib = QR.library_stack(hidden, Hq, Hkv, d_ff, layers, vl=vl)
    sd = QR.random_stack_state_dict(lib, seed=hidden + S)
    lib.load_state_dict(sd, strict=True)
    hip = Qwen2DecoderStack(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)       # the views follow their stacked storage to the GPU
    assert hip.layers[0].self_attn.k_proj.weight.data_ptr() == hip._fused["0.qkv.w"][Hq * (hidden // Hq):].data_ptr() and hip.device.type == "cuda"
    x = torch.randn((B, S, hidden), generator=torch.Generator().manual_seed(S)).bfloat16()
    mask = None
    if k_lo is not None:
        mask = torch.zeros((B, S), dtype=torch.long)
        for b in range(B):
            mask[b, k_lo[b]:k_hi[b]] = 1
    pos = QR.mrope_positions(B, S, seed=S) if vl else None
    dev = lambda t: None if t is None else t.to(DEV)
    slab = hip(inputs_embeds=dev(x), attention_mask=dev(mask), position_ids=dev(pos))
    assert slab.shape == (B, layers + 1, S, hidden) and slab.dtype == torch.bfloat16 and slab.is_contiguous()
    assert torch.equal(slab[:, 0], dev(x))
    assert bool(torch.isfinite(slab.float()).all())          # the rows before k_lo included
    first = slab.clone()
    assert torch.equal(hip(inputs_embeds=dev(x), attention_mask=dev(mask), position_ids=dev(pos)), first)      # the cached workspace: a second call is bit-identical
    name = "Qwen2DecoderStack hidden=%d %dq/%dkv d_ff=%d layers=%d B=%d S=%d range %s..%s vl=%s" % (hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl)
    runs = {}

    def run(m, d, dt):
        runs[dt] = _masked(_library_slab(m, x, mask, pos, d, dt), k_lo)
        return runs[dt]
    e_hip, e_lib = stack_errors(name + " slab", _masked(first, k_lo), lib, run)
    assert_stack_criterion(e_hip, e_lib)
    # ... and the last entry alone (the final norm's output), from the same two library runs
    ref, lib_bf16 = runs[torch.float64][:, -1], runs[torch.bfloat16][:, -1]
    e_hip, e_lib = QR.rel_l2(_masked(first, k_lo)[:, -1], ref), QR.rel_l2(lib_bf16, ref)
    print("%s last: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)


def test_stack_forward_allocates_the_slab_and_two_tables_after_the_first_call():
    from x2i_amd.qwen import Qwen2DecoderStack
    hip = Qwen2DecoderStack(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=512, num_hidden_layers=2, vocab_size=64,
                            device=DEV).init_random_(1)
    x = torch.randn((2, 77, 256), generator=torch.Generator().manual_seed(2)).bfloat16().to(DEV)
    ids = torch.randint(0, 64, (2, 77), generator=torch.Generator().manual_seed(3)).to(DEV)
    keep = hip(inputs_embeds=x).clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    out = hip(inputs_embeds=x)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] - before == 3 and out.shape == (2, 3, 77, 256)       # the slab, cos, sin
    assert torch.equal(out, keep) and float(out[:, -1].float().std()) > 0.1
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    out = hip(input_ids=ids)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] - before == 3
    assert torch.equal(out[:, 0], hip.embed_tokens.weight[ids])


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hip_prefill_against_the_library_prefill_and_restores_the_forward():
    """A tiny random Qwen2ForCausalLM (hidden 256, 2 heads of 128, 1 kv head, 3 layers), sample 0 right-padded: HipPrefill's slab against
    handoff.prefill_hidden_states of the same model on the same GPU, both against the library in float64 on the CPU"""
    from transformers import Qwen2ForCausalLM
    from x2i_amd.handoff import HipPrefill, find_decoder, prefill_hidden_states
    cfg = QR.library_config(256, 2, 1, 512, 3)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    model.model.load_state_dict(QR.random_stack_state_dict(model.model, seed=5), strict=True)
    B, S = 2, 77
    ids = torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(6))
    mask = torch.ones((B, S), dtype=torch.long)
    mask[0, 50:] = 0
    ref = prefill_hidden_states(model.double(), dtype=torch.float64, input_ids=ids, attention_mask=mask)
    model = model.to(device=DEV, dtype=torch.bfloat16)
    lib_slab = prefill_hidden_states(model, input_ids=ids.to(DEV), attention_mask=mask.to(DEV)).clone()
    logits = model(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), use_cache=False).logits
    hp = HipPrefill(model)
    assert hp.stack.embed_tokens.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()       # the token table is shared
    slab = hp.prefill(model, input_ids=ids.to(DEV), attention_mask=mask.to(DEV))
    assert slab.shape == lib_slab.shape == (B, 4, S, 256) and slab.dtype == lib_slab.dtype == torch.bfloat16 and slab.device == lib_slab.device
    assert not torch.equal(slab, lib_slab)                   # the HIP stack ran
    for name, sl in (("slab", slice(None)), ("last", slice(-1, None))):
        e_hip, e_lib = QR.rel_l2(slab[:, sl], ref[:, sl]), QR.rel_l2(lib_slab[:, sl], ref[:, sl])
        print("HipPrefill %s: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, e_hip, e_lib, e_hip / e_lib))
        assert_stack_criterion(e_hip, e_lib)
    # the model's own forward is back: a plain library call gives the library's result again, and the hooks' slab too
    assert "forward" not in find_decoder(model).__dict__
    assert torch.equal(model(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), use_cache=False).logits, logits)
    assert torch.equal(prefill_hidden_states(model, input_ids=ids.to(DEV), attention_mask=mask.to(DEV)), lib_slab)
    # ... after an exception too; a second decoder pass is refused by name
    with pytest.raises(RuntimeError, match="full_generate"):
        hp.capture(lambda: (model(input_ids=ids.to(DEV), use_cache=False), model(input_ids=ids.to(DEV), use_cache=False)))
    assert "forward" not in find_decoder(model).__dict__
    assert torch.equal(hp.prefill(model, input_ids=ids.to(DEV), attention_mask=mask.to(DEV)), slab)
