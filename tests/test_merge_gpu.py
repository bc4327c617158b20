"""The prompt merge on the HIP path (include/x2i_merge.h, x2i_amd/merge.py, Qwen2DecoderStack's merge=, handoff.HipInternVLPrompt /
HipMiniCPMPrompt) on the GPU.  The kernels copy rows, plus one f32 multiply with one rounding, so every kernel comparison is bit for bit
against torch (cumsum; index_select / where) and tests/merge_ref.py.  The stack and the hand-offs are compared with the library in
float64 under the criterion of tests/test_qwen_gpu.py (no worse than 1.5 x the library's own bf16 run on the same GPU).

The tiny models at the end of the file restate, in this project's words, what the two chat models do between their towers and their decoder
(bounds, context tokens, scatter, slice and masked assignment); their towers are stubs that return seeded or cheaply computed rows."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from tests import merge_ref as MR
from tests import qwen_ref as QR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned, stack_errors  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 2048        # X2I_MERGE_RANK_CHUNK: rows per workgroup of the rank launches


@pytest.fixture(scope="module")
def merge_ops():
    from x2i_amd import merge_ops as o
    o.load()
    assert o.RANK_CHUNK == CHUNK
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- rank
def run_rank(merge_ops, ids, placeholder):
    n = ids.numel()
    src = torch.full((n + 8,), -77, dtype=torch.int32, device=DEV)
    total = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    ws = torch.empty((merge_ops.rank_workspace_ints(n),), dtype=torch.int32, device=DEV)
    merge_ops.rank(ids, placeholder, src[:n], total, ws)
    assert bool((src[n:] == -77).all())               # nothing past row n - 1 is written
    return src[:n], int(total)


# wave boundary, a larger block boundary, one below / at / one above the kernel's chunk (CHUNK rows per workgroup), two samples of 4097
@pytest.mark.parametrize("shape", [(1, 63), (1, 64), (1, 65), (1, 1023), (1, 1024), (1, 1025), (1, CHUNK - 1), (1, CHUNK), (1, CHUNK + 1), (2, 4097)])
def test_rank_is_the_exclusive_cumsum_of_the_placeholder_rows(merge_ops, shape):
    B, S = shape
    g = torch.Generator().manual_seed(B * 100000 + S)
    ids = torch.randint(0, 4, (B, S), generator=g).to(DEV)          # one row in four holds the placeholder 3
    ids[-1, -1] = 3
    hit = ids.reshape(-1) == 3
    want = torch.where(hit, torch.cumsum(hit.long(), 0) - 1, torch.full((B * S,), -1, device=DEV)).to(torch.int32)
    src, total = run_rank(merge_ops, ids, 3)
    assert torch.equal(src, want) and total == int(hit.sum())
    ref_src, ref_total = MR.rank_ref(ids, 3)
    assert torch.equal(src, ref_src) and total == ref_total
    assert torch.equal(run_rank(merge_ops, ids, 3)[0], src)          # a relaunch is identical


def test_rank_of_one_row_all_rows_and_no_row(merge_ops):
    one = torch.tensor([[5]], device=DEV)
    src, total = run_rank(merge_ops, one, 5)
    assert src.tolist() == [0] and total == 1
    src, total = run_rank(merge_ops, one, 6)
    assert src.tolist() == [-1] and total == 0
    n = CHUNK + 1
    ids = torch.full((1, n), 9, device=DEV)
    src, total = run_rank(merge_ops, ids, 9)
    assert torch.equal(src, torch.arange(n, dtype=torch.int32, device=DEV)) and total == n
    src, total = run_rank(merge_ops, ids, 8)
    assert bool((src == -1).all()) and total == 0
    # ids far outside int32 compare as 64-bit numbers
    ids = torch.tensor([[1 << 40, 7, (1 << 40) + 7, 7]], device=DEV)
    src, total = run_rank(merge_ops, ids, 7)
    assert src.tolist() == [-1, 0, -1, 1] and total == 2


def test_rank_refusals(merge_ops):
    from x2i_amd._lib import X2IError
    ids = torch.zeros((1, CHUNK + 1), dtype=torch.long, device=DEV)
    src = torch.full((CHUNK + 1,), -77, dtype=torch.int32, device=DEV)
    total = torch.zeros((1,), dtype=torch.int32, device=DEV)
    with pytest.raises(X2IError, match="workspace too small"):
        merge_ops.rank(ids, 0, src, total, torch.empty((1,), dtype=torch.int32, device=DEV))
    with pytest.raises(X2IError):
        merge_ops.rank(ids.int(), 0, src, total, torch.empty((2,), dtype=torch.int32, device=DEV))
    assert bool((src == -77).all())                   # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- merge
def merge_inputs(B, S, H, seed, V=50):
    """ids, a table, two feature arrays with unequal row strides (H + 16 and H) and unequal counts, and a src that takes about a third of
    the rows from array 0 and a fifth from array 1, in no particular order (a feature row may serve several prompt rows)"""
    g = torch.Generator().manual_seed(seed)
    n = B * S
    ids = torch.randint(0, V, (B, S), generator=g).to(DEV)
    table = torch.randn((V, H), generator=g).bfloat16().to(DEV)
    n0, n1 = n // 3 + 1, n // 5 + 2
    wide = torch.randn((n0, H + 16), generator=g).bfloat16().to(DEV)
    f0, f1 = wide[:, :H], torch.randn((n1, H), generator=g).bfloat16().to(DEV)
    pick = torch.rand((n,), generator=g)
    src = torch.full((n,), -1, dtype=torch.int32)
    v, a = (pick < 0.33).nonzero()[:, 0], ((pick >= 0.33) & (pick < 0.53)).nonzero()[:, 0]
    src[v] = torch.randint(0, n0, (len(v),), generator=g).to(torch.int32)
    src[a] = torch.randint(0, n1, (len(a),), generator=g).to(torch.int32) | (1 << 30)
    if n == 1:
        src[0] = 0
    return ids, table, f0, f1, src.to(DEV)


def expected_rows(ids, src, table, scale, f0, f1):
    """index_select / where, and torch's own bf16 tensor * Python float"""
    rows = torch.index_select(table, 0, ids.reshape(-1))
    if scale != 1.0:
        rows = rows * scale
    k, a = (src & MR.ROW_MASK).long(), (src >> MR.ARRAY_BIT) & 1
    r0 = torch.index_select(f0, 0, k.clamp(max=f0.shape[0] - 1))
    r1 = torch.index_select(f1, 0, k.clamp(max=f1.shape[0] - 1))
    return torch.where((src < 0)[:, None], rows, torch.where((a == 0)[:, None], r0, r1)).reshape(*ids.shape, -1)


@pytest.mark.parametrize("H", [8, 896, 3584])
@pytest.mark.parametrize("B,S", [(1, 1), (2, 77)])
@pytest.mark.parametrize("scale", [1.0, 12.0])
def test_merge_into_a_slab_entry_is_index_select_and_where_bit_for_bit(merge_ops, B, S, H, scale):
    ids, table, f0, f1, src = merge_inputs(B, S, H, seed=H * 1000 + S)
    err = torch.zeros((1,), dtype=torch.int32, device=DEV)
    want = expected_rows(ids, src, table, scale, f0, f1)
    assert torch.equal(bits(want), bits(MR.merge_ref(ids, src, table, scale, f0, f1)[0]))
    if scale != 1.0 and S > 1:
        assert not torch.equal(bits(want), bits(expected_rows(ids, src, table, 1.0, f0, f1)))
    # out = slab[:, 0] of a [B, C, S, H] slab whose other entries are poisoned
    slab = poisoned(B, 3, S, H)
    merge_ops.embed_merge(slab[:, 0], err, ids=ids, src=src, table=table, scale=scale, feat0=f0, feat1=f1)
    assert torch.equal(bits(slab[:, 0]), bits(want)) and bool(is_sentinel(slab[:, 1:]).all()) and int(err) == 0
    # rows of a wider, taller buffer: a row stride and a batch stride of its own; every element around the rows stays poisoned
    buf = poisoned(B, S + 2, H + 8)
    merge_ops.embed_merge(buf[:, 1:S + 1, :H], err, ids=ids, src=src, table=table, scale=scale, feat0=f0, feat1=f1)
    assert torch.equal(bits(buf[:, 1:S + 1, :H]), bits(want)) and int(err) == 0
    assert bool(is_sentinel(buf[:, 0]).all()) and bool(is_sentinel(buf[:, S + 1]).all()) and bool(is_sentinel(buf[:, :, H:]).all())
    # without src every row is a table row
    out = poisoned(B, S, H)
    merge_ops.embed_merge(out, err, ids=ids, table=table, scale=scale)
    rows = torch.index_select(table, 0, ids.reshape(-1))
    assert torch.equal(bits(out), bits((rows if scale == 1.0 else rows * scale).reshape(B, S, H)))


@pytest.mark.parametrize("H", [8, 896])
def test_merge_overwrite_mode_leaves_every_other_row_in_place(merge_ops, H):
    B, S = 2, 77
    ids, table, f0, f1, src = merge_inputs(B, S, H, seed=H + 5)
    err = torch.zeros((1,), dtype=torch.int32, device=DEV)
    before = torch.randn((B, S, H), generator=torch.Generator().manual_seed(1)).bfloat16().to(DEV)
    before[0, 0] = float("nan")
    out = before.clone()
    merge_ops.embed_merge(out, err, src=src, feat0=f0, feat1=f1)          # no table, no ids
    feat = expected_rows(ids, src, table, 1.0, f0, f1)
    want = torch.where((src < 0).reshape(B, S, 1), bits(before), bits(feat))
    assert torch.equal(bits(out), want) and int(err) == 0
    assert torch.equal(want, bits(MR.merge_ref(ids, src, None, 1.0, f0, f1, out=before)[0]))


def test_merge_out_of_range_rows_are_zero_rows_with_the_flag_set(merge_ops):
    """Specified behaviour of include/x2i_merge.h: the kernel compares ids[r] with V and a feature row with its array's count before it
    forms an address.  One id equal to V, one feature row equal to its count: zero rows, the flag, the neighbours intact."""
    from x2i_amd.merge import MergePlan
    B, S, H, V = 2, 77, 896, 50
    ids, table, f0, f1, src = merge_inputs(B, S, H, seed=3, V=V)
    tok = (src < 0).nonzero()[:, 0]
    vis = ((src >= 0) & (src < (1 << 30))).nonzero()[:, 0]
    aud = (src >= (1 << 30)).nonzero()[:, 0]
    good = expected_rows(ids, src, table, 1.0, f0, f1).reshape(B * S, H)
    for kind, row in (("id", int(tok[3])), ("vision", int(vis[2])), ("audio", int(aud[1]))):
        ids2, src2 = ids.clone(), src.clone()
        if kind == "id":
            ids2.view(-1)[row] = V
        elif kind == "vision":
            src2[row] = f0.shape[0]
        else:
            src2[row] = f1.shape[0] | (1 << 30)
        err = torch.zeros((1,), dtype=torch.int32, device=DEV)
        slab = poisoned(B, 2, S, H)
        merge_ops.embed_merge(slab[:, 0], err, ids=ids2, src=src2, table=table, feat0=f0, feat1=f1)
        got = slab[:, 0].reshape(B * S, H)
        keep = torch.ones((B * S,), dtype=torch.bool, device=DEV)
        keep[row] = False
        assert int(err) == 1, kind
        assert bool((bits(got[row]) == 0).all()) and torch.equal(bits(got[keep]), bits(good[keep])) and bool(is_sentinel(slab[:, 1]).all()), kind
        ref, flag = MR.merge_ref(ids2, src2, table, 1.0, f0, f1)
        assert flag == 1 and torch.equal(bits(ref.reshape(B * S, H)), bits(got))
        # the plan raises with check=True and keeps quiet with check=False
        for check in (True, False):
            plan = MergePlan(B, S, src2, [None, None], check=check).set_features(vision=f0, audio=f1)
            out = poisoned(B, S, H)
            if check:
                with pytest.raises(ValueError, match="outside the table or a feature row"):
                    plan.launch(out, ids2, table)
            else:
                plan.launch(out, ids2, table)
                assert int(plan.err) == 1
    # a placeholder total that differs from the feature rows
    ph = torch.zeros((B, S), dtype=torch.long, device=DEV)
    ph[1, 5:9] = 7
    plan = MergePlan.from_placeholder(ph, 7).set_features(vision=f1[:5])
    with pytest.raises(ValueError, match="4 placeholder rows and the features have 5"):
        plan.launch(poisoned(B, S, H), ph, table)


def test_merge_refusals(merge_ops):
    from x2i_amd._lib import X2IError
    ids, table, f0, f1, src = merge_inputs(2, 7, 16, seed=9)
    err = torch.zeros((1,), dtype=torch.int32, device=DEV)
    out = poisoned(2, 7, 16)
    bad = [dict(out=poisoned(2, 7, 12)), dict(table=table[:, :8]), dict(feat0=f1[:, :8]), dict(src=None, table=None), dict(scale=float("inf")),
           dict(ids=ids.int()), dict(src=src.long()), dict(n0=-1), dict(out=poisoned(2, 7, 32)[:, :, ::2])]
    for kw in bad:
        args = dict(out=out, ids=ids, src=src, table=table, feat0=f0, feat1=f1)
        args.update(kw)
        o = args.pop("out")
        with pytest.raises(X2IError):
            merge_ops.embed_merge(o, err, **args)
    assert bool(is_sentinel(out).all()) and int(err) == 0          # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- stack
def small_stack(hidden=256, Hq=2, Hkv=1, seed=1, vocab=64):
    from x2i_amd.qwen import Qwen2DecoderStack
    return Qwen2DecoderStack(hidden_size=hidden, num_attention_heads=Hq, num_key_value_heads=Hkv, intermediate_size=512, num_hidden_layers=2,
                             vocab_size=vocab, device=DEV).init_random_(seed)


def test_stack_with_a_plan_equals_the_stack_on_the_torch_merge_bit_for_bit():
    from x2i_amd.merge import MergePlan
    hip = small_stack()
    B, S, H, V = 2, 77, 256, 64
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V - 1, (B, S), generator=g).to(DEV)
    ids[0, 3:11] = V - 1
    ids[1, 40:44] = V - 1
    mask = torch.ones((B, S), dtype=torch.long, device=DEV)
    mask[0, 50:] = 0
    feats = torch.randn((3, 4, H), generator=g).bfloat16().to(DEV)
    embeds = hip.embed_tokens.weight.detach()[ids]
    embeds.view(B * S, H)[ids.reshape(-1) == V - 1] = feats.reshape(-1, H)          # the masked assignment over the flattened batch
    want = hip(inputs_embeds=embeds, attention_mask=mask).clone()
    plan = MergePlan.from_placeholder(ids, V - 1).set_features(vision=feats)
    got = hip(input_ids=ids, attention_mask=mask, merge=plan)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got[:, 0]), bits(embeds))
    # prefill takes the plan too and gives forward's slab
    cache = hip.new_cache(B, S + 1)
    assert torch.equal(bits(hip.prefill(cache, input_ids=ids, attention_mask=mask, merge=plan)), bits(want))
    # bounds, two arrays and a scale: against torch's own multiply and slice assignments
    audio = torch.randn((5, H), generator=g).bfloat16().to(DEV)
    image_bound = [torch.zeros((0, 2), dtype=torch.long, device=DEV), torch.tensor([[2, 6], [8, 12], [20, 24]], device=DEV)]
    audio_bounds = [[], [[30, 32], [40, 43]]]
    embeds = hip.embed_tokens.weight.detach()[ids] * 12.0
    embeds[1, 2:6], embeds[1, 8:12], embeds[1, 20:24] = feats[0], feats[1], feats[2]
    embeds[1, 30:32], embeds[1, 40:43] = audio[:2], audio[2:]
    plan = MergePlan.from_bounds(B, S, image_bound, audio_bounds, device=DEV).set_features(vision=feats, audio=audio)
    got = hip(input_ids=ids, attention_mask=mask, merge=plan, embed_scale=12.0)
    assert torch.equal(bits(got[:, 0]), bits(embeds))
    assert torch.equal(bits(got), bits(hip(inputs_embeds=embeds, attention_mask=mask)))
    with pytest.raises(ValueError, match="ask for 12 vision rows and the features have 8"):
        hip(input_ids=ids, merge=MergePlan.from_bounds(B, S, image_bound, device=DEV).set_features(vision=feats[:2]))
    with pytest.raises(ValueError, match="merge= goes with input_ids"):
        hip(inputs_embeds=embeds, merge=plan)


def test_from_bounds_crosses_to_the_host_once_for_all_bounds(monkeypatch):
    """Bounds on the GPU (five tensors over two samples and both kinds): ONE concatenated copy; src is the reference's"""
    from x2i_amd import merge
    B, S = 2, 50
    image_bound = [torch.zeros((0, 2), dtype=torch.long, device=DEV), torch.tensor([[2, 6], [8, 12], [20, 24]], device=DEV)]
    audio_bounds = [torch.tensor([[1, 3]], device=DEV), [torch.tensor([30, 32], device=DEV), torch.tensor([40, 43], device=DEV)]]
    copies, real = [], torch.cat
    monkeypatch.setattr(merge.torch, "cat", lambda ts, *a, **k: copies.append(len(ts)) or real(ts, *a, **k))
    plan = merge.MergePlan.from_bounds(B, S, image_bound, audio_bounds, device=DEV)
    assert copies == [5] and plan.expect == [12, 7] and plan.src.device.type == "cuda"
    want = MR.src_from_bounds_ref(B, S, [[], [[2, 6], [8, 12], [20, 24]]], [[[1, 3]], [[30, 32], [40, 43]]])
    assert torch.equal(plan.src.cpu(), want)


def test_stack_on_plain_input_ids_is_the_parents_gather_bit_for_bit():
    """The parent looked the ids up with one torch.index_select per sample; entry 0 is embed_tokens.weight[ids] and the slab that of the
    same rows handed over as inputs_embeds"""
    hip = small_stack(seed=2)
    ids = torch.randint(0, 64, (2, 77), generator=torch.Generator().manual_seed(3)).to(DEV)
    out = hip(input_ids=ids)
    assert torch.equal(bits(out[:, 0]), bits(hip.embed_tokens.weight[ids]))
    assert torch.equal(bits(out), bits(hip(inputs_embeds=hip.embed_tokens.weight[ids])))
    assert int(hip._ws[(2, 77)]["merge_err"]) == 0


def test_stack_with_a_group_of_seven_query_heads_vs_library_fp64_and_bf16():
    """Qwen2-0.5B's grouping (InternVL2.5-1B's decoder: 14 query heads on 2 key/value heads) at one key/value head: hidden 448, 7 heads of
    64, 2 layers, B = 2, S = 77, sample 0 right-padded to 50"""
    from x2i_amd.qwen import Qwen2DecoderStack
    from tests.test_qwen_gpu import _library_slab
    hidden, Hq, Hkv, d_ff, layers, B, S = 448, 7, 1, 1024, 2, 2, 77
    cfg, lib = QR.library_stack(hidden, Hq, Hkv, d_ff, layers)
    sd = QR.random_stack_state_dict(lib, seed=hidden + S)
    lib.load_state_dict(sd, strict=True)
    hip = Qwen2DecoderStack(cfg, device=DEV)
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    assert hip.config.head_dim == 64 and hip.config.num_attention_heads // hip.config.num_key_value_heads == 7
    ids = torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(S))
    mask = torch.ones((B, S), dtype=torch.long)
    mask[0, 50:] = 0
    slab = hip(input_ids=ids.to(DEV), attention_mask=mask.to(DEV))
    x = hip.embed_tokens.weight[ids.to(DEV)].cpu()
    assert torch.equal(bits(slab[:, 0].cpu()), bits(x)) and bool(torch.isfinite(slab.float()).all())
    runs = {}

    def run(m, d, dt):
        runs[dt] = _library_slab(m, x, mask, None, d, dt)
        return runs[dt]
    name = "Qwen2DecoderStack hidden=448 7q/1kv B=2 S=77 right-padded"
    e_hip, e_lib = stack_errors(name + " slab", slab, lib, run)
    assert_stack_criterion(e_hip, e_lib)
    ref, lib_bf16 = runs[torch.float64][:, -1], runs[torch.bfloat16][:, -1]
    e_hip, e_lib = QR.rel_l2(slab[:, -1], ref), QR.rel_l2(lib_bf16, ref)
    print("%s last: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)


# ---------------------------------------------------------------------------------------------------------------- tiny models
HID, VOCAB = 128, 64


def tiny_causal_lm(seed, scale_emb=None):
    from transformers import Qwen2ForCausalLM
    cfg = QR.library_config(HID, 2, 1, 256, 2, vocab=VOCAB)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    lm = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    lm.model.load_state_dict(QR.random_stack_state_dict(lm.model, seed=seed), strict=True)
    if scale_emb is not None:
        lm.config.scale_emb = scale_emb
    return lm


def _prompt_pass_of_generate(lm, embeds, attention_mask):
    """What both chat models end in: the language model's generate() on the merged embeddings (one new token: one decoder pass)"""
    return lm.generate(inputs_embeds=embeds, attention_mask=attention_mask, max_new_tokens=1, do_sample=False, pad_token_id=0)


class TinyInternVL(nn.Module):
    """An InternVL-like chat model: `language_model`, `img_context_token_id`, `extract_feature` (a stub tower: seeded rows [tiles, T, H])
    and a generate() that embeds the ids, assigns the feature rows to the context-token rows of the flattened batch and generates."""
    CTX, T = VOCAB - 1, 4

    def __init__(self, seed=5, lm=None, ctx=None, tokens_per_tile=None):
        """lm: a Qwen2ForCausalLM of any size (tools/prompt_bench.py builds the real configurations); default: the tiny one"""
        super().__init__()
        self.language_model = tiny_causal_lm(seed) if lm is None else lm
        self.img_context_token_id = self.CTX if ctx is None else ctx
        self.num_image_token = self.T if tokens_per_tile is None else tokens_per_tile
        self.eval()

    def extract_feature(self, pixel_values):
        w = self.language_model.get_input_embeddings().weight
        g = torch.Generator().manual_seed(17 + pixel_values.shape[0])
        return torch.randn((pixel_values.shape[0], self.num_image_token, w.shape[1]), generator=g).bfloat16().to(device=w.device, dtype=w.dtype)

    def merged(self, pixel_values, input_ids):
        embeds = self.language_model.get_input_embeddings()(input_ids)
        if pixel_values is not None:
            vit = self.extract_feature(pixel_values)
            B, N, C = embeds.shape
            embeds = embeds.reshape(B * N, C)
            selected = input_ids.reshape(B * N) == self.img_context_token_id
            assert selected.sum() != 0
            embeds[selected] = vit.reshape(-1, C)
            embeds = embeds.reshape(B, N, C)
        return embeds

    @torch.no_grad()
    def generate(self, pixel_values=None, input_ids=None, attention_mask=None, **kw):
        return _prompt_pass_of_generate(self.language_model, self.merged(pixel_values, input_ids), attention_mask)


class StubVpm(nn.Module):
    """pixel_values [n, 3, ps, patches * ps] -> last_hidden_state [n, patches, 8]: a fixed map of every patch's pixels, zero where masked"""

    def __init__(self, ps):
        super().__init__()
        self.ps = ps
        self.w = nn.Parameter(torch.randn((3 * ps * ps, 8), generator=torch.Generator().manual_seed(31)).bfloat16().float(), requires_grad=False)

    def forward(self, pixel_values, patch_attention_mask=None, tgt_sizes=None):
        n, _, ps, L = pixel_values.shape
        x = pixel_values.reshape(n, 3, ps, L // ps, ps).permute(0, 3, 1, 2, 4).reshape(n, L // ps, 3 * ps * ps)
        h = (x @ self.w.to(x.dtype)) * patch_attention_mask[:, 0, :, None].to(x.dtype)
        return SimpleNamespace(last_hidden_state=h)


class StubResampler(nn.Module):
    """[n, patches, 8] -> [n, Q, H]: the patch sum through a fixed map per query, plus the patch count of tgt_sizes"""

    def __init__(self, Q, hidden=HID):
        super().__init__()
        self.w = nn.Parameter(torch.randn((Q, 8, hidden), generator=torch.Generator().manual_seed(32)).bfloat16().float(), requires_grad=False)

    def forward(self, x, tgt_sizes=None):
        count = (tgt_sizes[:, 0] * tgt_sizes[:, 1]).to(x.dtype)
        return torch.einsum("nd,qdh->nqh", x.sum(1), self.w.to(x.dtype)) + 0.125 * count[:, None, None]


class TinyMiniCPM(nn.Module):
    """A MiniCPM-o-like model: `llm` (with config.scale_emb), `vpm`, `resampler`, `get_audio_embedding` (a stub: seeded rows, one per four
    feature frames) and a generate() that does the model's two merges literally -- a scatter over stacked aranges per sample for the
    image bounds, then per audio bound a slice assignment (chunk_input) or an index assignment per audio (otherwise)."""
    Q, PS = 4, 2

    def __init__(self, seed=6, chunk_input=True, scale_emb=12.0, lm=None, queries=None, patch_size=None, vision_batch_size=2):
        """lm: a Qwen2ForCausalLM of any size (tools/prompt_bench.py builds the real configuration); default: the tiny one"""
        super().__init__()
        self.llm = tiny_causal_lm(seed, scale_emb) if lm is None else lm
        self.hidden = self.llm.config.hidden_size
        self.Q, self.PS = self.Q if queries is None else queries, self.PS if patch_size is None else patch_size
        self.vpm, self.resampler = StubVpm(self.PS), StubResampler(self.Q, self.hidden)
        self.config = SimpleNamespace(vision_batch_size=vision_batch_size, init_audio=True, audio_chunk_length=1.0, chunk_input=chunk_input,
                                      patch_size=self.PS)
        self.eval()

    def get_audio_embedding(self, data, chunk_length=-1, dummy=True):
        w = self.llm.model.embed_tokens.weight
        out, k = [], 0
        for lens in data["audio_feature_lens"]:
            mine = []
            for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens):
                g = torch.Generator().manual_seed(41 + k)
                mine.append(torch.randn((int(n) // 4, self.hidden), generator=g).bfloat16().to(device=w.device, dtype=w.dtype))
                k += 1
            out.append(mine)
        return out

    def vision_rows(self, data):
        w = self.llm.model.embed_tokens.weight
        flat, counts = [], []
        for pixel_values in data["pixel_values"]:
            counts.append(len(pixel_values))
            flat.extend(i.flatten(end_dim=1).permute(1, 0) for i in pixel_values)
        if not flat:
            return [[] for _ in counts]
        tgt = torch.vstack([t for t in data["tgt_sizes"] if isinstance(t, torch.Tensor)]).type(torch.int32)
        max_patches = int(torch.max(tgt[:, 0] * tgt[:, 1]))
        x = torch.nn.utils.rnn.pad_sequence(flat, batch_first=True, padding_value=0.0)
        n, L, _ = x.shape
        x = x.permute(0, 2, 1).reshape(n, 3, -1, L).type(w.dtype)
        mask = torch.zeros((n, 1, max_patches), dtype=torch.bool, device=w.device)
        for i in range(n):
            mask[i, 0, :int(tgt[i][0] * tgt[i][1])] = True
        step = self.config.vision_batch_size
        hs = [self.vpm(x[i:i + step], patch_attention_mask=mask[i:i + step], tgt_sizes=tgt[i:i + step]).last_hidden_state for i in range(0, n, step)]
        emb = self.resampler(torch.cat(hs, dim=0), tgt)
        out, at = [], 0
        for c in counts:
            out.append(emb[at:at + c] if c else [])
            at += c
        return out

    def merged(self, data):
        emb = self.llm.model.embed_tokens(data["input_ids"])
        if hasattr(self.llm.config, "scale_emb"):
            emb = emb * self.llm.config.scale_emb
        new = emb.clone()
        for i, rows in enumerate(self.vision_rows(data)):
            bound = data["image_bound"][i]
            if len(rows) > 0 and len(bound) > 0:
                index = torch.stack([torch.arange(r[0], r[1], dtype=torch.long) for r in bound]).to(emb.device)
                new[i] = emb[i].scatter(0, index.view(-1, 1).repeat(1, emb.shape[-1]), rows.type(emb.dtype).view(-1, rows.shape[-1]))
        if len(data.get("audio_features", [])) > 0:
            audio = self.get_audio_embedding(data, self.config.audio_chunk_length)
            for i in range(len(new)):
                if self.config.chunk_input:
                    if not audio[i]:
                        continue
                    rows, at = torch.cat(audio[i], dim=0).to(new.dtype), 0
                    for bound in data["audio_bounds"][i]:
                        n = int(bound[1] - bound[0])
                        new[i, bound[0]:bound[1]] = rows[at:at + n]
                        at += n
                else:
                    for rows, bound in zip(audio[i], data["audio_bounds"][i]):
                        index = torch.arange(bound[0], bound[1], dtype=torch.long).to(new.device)
                        if rows.shape[0] != len(index):
                            raise ValueError("Shape mismatch: Trying to assign embeddings of shape %s to input indices of length %d" % (rows.shape, len(index)))
                        new[i, index] = rows.to(new.dtype)
        return new

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, **data):
        return _prompt_pass_of_generate(self.llm, self.merged(dict(data, input_ids=input_ids)), attention_mask)


def internvl_inputs(B=2, S=77):
    """sample 0 right-padded to 50 with one tile's context tokens, sample 1 with two tiles'"""
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(0, VOCAB - 1, (B, S), generator=g)
    mask = torch.ones((B, S), dtype=torch.long)
    mask[0, 50:] = 0
    ids[0, 50:] = 0
    ids[0, 3:7] = TinyInternVL.CTX
    ids[1, 10:18] = TinyInternVL.CTX
    return dict(input_ids=ids, attention_mask=mask, pixel_values=torch.zeros((3, 3, 4, 4)))


def minicpm_inputs(chunk_input, B=2, S=50):
    """sample 0 right-padded to 30, without features; sample 1 with three image bounds of Q rows and two audio bounds of 2 and 3 rows --
    one audio of 5 rows laid over both (chunk_input), or two audios of 2 and 3 rows"""
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, VOCAB, (B, S), generator=g)
    mask = torch.ones((B, S), dtype=torch.long)
    mask[0, 30:] = 0
    ps = TinyMiniCPM.PS
    sizes = [(2, 3), (2, 2), (1, 4)]
    images = [torch.randn((3, ps, h * w * ps), generator=g).bfloat16().float() for h, w in sizes]
    return dict(input_ids=ids, attention_mask=mask, pixel_values=[[], images], tgt_sizes=[[], torch.tensor(sizes)],
                image_bound=[torch.zeros((0, 2), dtype=torch.long), torch.tensor([[2, 6], [8, 12], [20, 24]])],
                audio_features=[torch.zeros((1, 4, 20))], audio_feature_lens=[[], torch.tensor([20] if chunk_input else [8, 12])],
                audio_bounds=[torch.zeros((0, 2), dtype=torch.long), torch.tensor([[30, 32], [40, 43]])])


def to_device(o, dev, dtype=None):
    if isinstance(o, torch.Tensor):
        return o.to(device=dev, dtype=dtype if dtype is not None and o.is_floating_point() else None)
    if isinstance(o, dict):
        return {k: to_device(v, dev, dtype) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [to_device(v, dev, dtype) for v in o]
    return o


def check_handoff(name, model, lm, inputs, make, run_prompt, merged):
    """The hand-off's slab against the model's own generate() path in float64 and in bf16 on the GPU (captured by hooks on the decoder),
    entry 0 against the model's own merged embeddings bit for bit, no lm_head call, and the instance restored"""
    from x2i_amd.handoff import HiddenStateSlab, find_decoder
    model = model.to(device=DEV, dtype=torch.bfloat16)
    gpu_inputs = to_device(inputs, DEV, torch.bfloat16)
    own = merged(model, gpu_inputs).clone()
    handoff = make(model)
    before = dict(model.__dict__)

    def fail(*a):
        raise AssertionError("the lm_head ran on the prompt")
    hook = lm(model).lm_head.register_forward_hook(fail)
    try:
        slab = run_prompt(handoff, gpu_inputs)
        with handoff:                                  # installed, the model's generate() is the hand-off's prompt pass
            via_generate = model.generate(**gpu_inputs)
    finally:
        hook.remove()
    via_generate = via_generate if isinstance(via_generate, tuple) else via_generate.hidden_states[0]
    assert torch.equal(bits(torch.stack(via_generate, 1)), bits(slab))
    assert model.__dict__.keys() == before.keys() and "generate" not in model.__dict__ and "forward" not in find_decoder(model).__dict__
    B, S = inputs["input_ids"].shape
    assert slab.shape == (B, 3, S, HID) and torch.equal(bits(slab[:, 0]), bits(own))

    def run(m, d, dt):
        return HiddenStateSlab(find_decoder(m), dt).capture(lambda: m.generate(**to_device(inputs, d, dt))).clone()
    e_hip, e_lib = stack_errors(name, slab, model.cpu().float(), run)
    assert_stack_criterion(e_hip, e_lib)
    return handoff


def test_internvl_handoff_against_the_models_own_generate_path():
    from x2i_amd.handoff import HipInternVLPrompt
    inputs = internvl_inputs()
    handoff = check_handoff("HipInternVLPrompt", TinyInternVL(), lambda m: m.language_model, inputs, HipInternVLPrompt,
                            lambda h, i: h.prompt(i["input_ids"], i["attention_mask"], i["pixel_values"]),
                            lambda m, i: m.merged(i["pixel_values"], i["input_ids"]))
    assert handoff.calls == 2
    # without pixels the ids run alone: the context tokens are ordinary rows of the table
    ids, mask = inputs["input_ids"].to(DEV), inputs["attention_mask"].to(DEV)
    alone = handoff.prompt(ids, mask)
    assert torch.equal(bits(alone[:, 0]), bits(handoff.stack.embed_tokens.weight[ids]))
    # context tokens and feature rows that differ in number: the model's own assert, here a ValueError
    with pytest.raises(ValueError, match="12 placeholder rows and the features have 8"):
        handoff.prompt(ids, mask, torch.zeros((2, 3, 4, 4), device=DEV))


@pytest.mark.parametrize("chunk_input", [True, False])
def test_minicpm_handoff_against_the_models_own_generate_path(chunk_input):
    from x2i_amd.handoff import HipMiniCPMPrompt
    inputs = minicpm_inputs(chunk_input)
    handoff = check_handoff("HipMiniCPMPrompt chunk_input=%s" % chunk_input, TinyMiniCPM(chunk_input=chunk_input), lambda m: m.llm, inputs,
                            HipMiniCPMPrompt, lambda h, i: h.prompt(**i), lambda m, i: m.merged(i))
    assert handoff.scale == 12.0
    gpu_inputs = to_device(inputs, DEV, torch.bfloat16)
    # bounds that ask for other rows than the sample's features have: refused before any launch
    short = dict(gpu_inputs, image_bound=[gpu_inputs["image_bound"][0], gpu_inputs["image_bound"][1][:2]])
    with pytest.raises(ValueError, match="vision rows per sample"):
        handoff.prompt(**short)
    if not chunk_input:
        wrong = dict(gpu_inputs, audio_bounds=[gpu_inputs["audio_bounds"][0], torch.tensor([[30, 33], [40, 42]], device=DEV)])
        with pytest.raises(ValueError, match="Shape mismatch"):
            handoff.prompt(**wrong)
