"""The Qwen2.5-VL vision tower on the HIP path (include/x2i_vit.h, x2i_amd/qwen_vision.py, handoff.HipVision) on the GPU: each kernel against
its float64 checker of tests/qwen_vision_ref.py or bit for bit against torch, and the tower and the hand-off against the library in float64
(and no worse than 1.5 x the library's own bf16 run on the same GPU)."""
import pytest
import torch

from tests import qwen_vision_ref as VR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def vit_ops():
    from x2i_amd import vit_ops as o
    o.load()
    return o


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- attention
def run_attention(vit_ops, Q, K, V, S, dk, lo=None, hi=None, extra_cols=0, extra_rows=0):
    """Q, K, V [B, H, Spad, dkp] -> (O [B, H, S, dk] view, the whole sentinel-filled output buffer [B, S + extra_rows, H * dk + extra_cols])"""
    B, H, Spad, _ = Q.shape
    VT = V.transpose(-1, -2).contiguous()
    ldo = H * dk + extra_cols
    buf = poisoned(B, S + extra_rows, ldo)
    vit_ops.attention(Q, K, VT, buf, B, H, S, Spad, dk, dk ** -0.5, ldo, (S + extra_rows) * ldo, _i32(lo), _i32(hi))
    return buf[:, :S, :H * dk].reshape(B, S, H, dk).permute(0, 2, 1, 3), buf


WINDOWS = [64, 16, 16, 4, 48, 36, 48, 36]      # the window segments of grids [(1,10,10), (2,6,14)]; the frames are [100, 84, 84]
# (B, H, S, dk, the segment lengths of every sample): one window of one merge unit; the windows of one 10 x 10 image; two grids, by windows
# (rows 128..255 of the second workgroup span three segments and its walk starts at tile 1) and by frames (a segment across the 128-row
# and the 64-key boundaries); one segment of five tiles (waves compute tiles before and after their own rows); heads of 64 and of 128 over
# two workgroups; another array per sample.
# Worst tile measured on the MI355X, in this order: 1.83e-3, 1.87e-3, 2.23e-3, 2.42e-3, 2.29e-3, 2.48e-3, 2.21e-3, 2.04e-3 (bound TOL_O = 5e-3;
# profiles/qwen_vision_gputest.log)
ATTENTION_CASES = [(1, 1, 4, 80, [[4]]), (1, 2, 100, 80, [[64, 16, 16, 4]]), (1, 2, 268, 80, [WINDOWS]), (1, 2, 268, 80, [[100, 84, 84]]),
                   (1, 1, 300, 80, [[300]]), (1, 2, 130, 64, [[130]]), (1, 1, 130, 128, [[130]]), (2, 3, 77, 80, [[64, 13], [5, 72]])]
_IDS = ["B%d-H%d-S%d-dk%d-%s" % (B, H, S, dk, "_".join("+".join(str(n) for n in s) for s in segs)) for B, H, S, dk, segs in ATTENTION_CASES]


def _ranges(segs):
    pairs = [VR.segment_ranges(s) for s in segs]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("B,H,S,dk,segs", ATTENTION_CASES, ids=_IDS)
def test_attention_vs_fp64_per_tile(vit_ops, B, H, S, dk, segs):
    lo, hi = _ranges(segs)
    Q, K, V = VR.attention_inputs(B, H, S, dk, seed=1000 * S + dk + H, device=DEV)
    ref = VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, lo, hi)
    O, buf = run_attention(vit_ops, Q, K, V, S, dk, lo, hi, extra_cols=8, extra_rows=3)
    name = "vit_attention B=%d H=%d S=%d dk=%d segments %s" % (B, H, S, dk, segs)
    worst = VR.check_attention(name, O, ref)
    print("%s: worst tile rel-L2 %.3e (bound %.1e)" % (name, worst, VR.TOL_O))
    # nothing outside rows < S and columns < H * dk is written, and every element inside is
    assert bool(is_sentinel(buf[:, S:]).all()) and bool(is_sentinel(buf[:, :, H * dk:]).all())
    assert not bool(is_sentinel(buf[:, :S, :H * dk]).any())
    # output rows that are only 8-byte aligned take the other store path: the same values, the same footprint
    O8, buf8 = run_attention(vit_ops, Q, K, V, S, dk, lo, hi, extra_cols=4, extra_rows=3)
    assert torch.equal(O8, O)
    assert bool(is_sentinel(buf8[:, S:]).all()) and bool(is_sentinel(buf8[:, :, H * dk:]).all()) and not bool(is_sentinel(buf8[:, :S, :H * dk]).any())
    # a relaunch is bit-identical, and sample 0 does not depend on the batch it is launched in
    O2, _ = run_attention(vit_ops, Q, K, V, S, dk, lo, hi, extra_cols=8, extra_rows=3)
    assert torch.equal(O2, O)
    if B > 1:
        O1, _ = run_attention(vit_ops, Q[:1].contiguous(), K[:1].contiguous(), V[:1].contiguous(), S, dk, lo[:1], hi[:1])
        assert torch.equal(O1[0], O[0])
    # the result does not depend on what the padding of a narrower head holds
    if VR.stored_width(dk) != dk:
        Qn, Kn, Vn = Q.clone(), K.clone(), V.clone()
        for t in (Qn, Kn, Vn):
            t[..., dk:] = NAN
        On, _ = run_attention(vit_ops, Qn, Kn, Vn, S, dk, lo, hi, extra_cols=8, extra_rows=3)
        assert torch.equal(On, O)
    # without the arrays every row's range is [0, S)
    if all(len(s) == 1 for s in segs):
        Onull, _ = run_attention(vit_ops, Q, K, V, S, dk, None, None, extra_cols=8, extra_rows=3)
        assert torch.equal(Onull, O)


@pytest.mark.parametrize("B,H,S,dk,segs", ATTENTION_CASES, ids=_IDS)
def test_attention_masks_by_index_under_adversarial_magnitudes(vit_ops, B, H, S, dk, segs):
    """The construction of tests/test_qwen_gpu.py with a sign per segment.  One unit direction u per head; the queries of segment s are
    shifted by -sign_s c u and its keys by +sign_s c u with c^2 / sqrt(dk) = 9 and sign_s = (-1)^s: a counted pair loses 9, and a pair of
    NEIGHBOURING segments -- the keys just outside a row's range, in the same tile -- gains 9.  The keys in [S, Spad), which count for no
    row, hold the shift that gains 9 against the last segment and V = 50.  The NaN padding of a narrower head stays in."""
    lo, hi = _ranges(segs)
    c = (9.0 * dk ** 0.5) ** 0.5
    Q, K, V = VR.attention_inputs(B, H, S, dk, seed=7 * S + dk, device=DEV)
    u = torch.randn((B, H, 1, dk), generator=torch.Generator().manual_seed(8)).to(DEV)
    u /= u.norm(dim=-1, keepdim=True)
    for b in range(B):
        start = 0
        for s, n in enumerate(segs[b]):
            sl, sign = slice(start, start + n), 1.0 - 2.0 * (s % 2)
            Q[b, :, sl, :dk] = (Q[b, :, sl, :dk].float() - sign * c * u[b]).bfloat16()
            K[b, :, sl, :dk] = (K[b, :, sl, :dk].float() + sign * c * u[b]).bfloat16()
            start += n
        K[b, :, S:, :dk] = (-sign * c * u[b]).bfloat16()
        V[b, :, S:, :dk] = 50.0
    for t in (Q, K, V):
        t[..., dk:] = NAN
    ref = VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, lo, hi)
    O, _ = run_attention(vit_ops, Q, K, V, S, dk, lo, hi)
    worst = VR.check_attention("vit_attention anti %s" % (segs,), O, ref)
    print("vit_attention anti B=%d H=%d S=%d dk=%d segments %s: worst tile rel-L2 %.3e" % (B, H, S, dk, segs, worst))


@pytest.mark.parametrize("B,H,S,dk,segs", ATTENTION_CASES, ids=_IDS)
def test_attention_known_answers_and_segment_isolation(vit_ops, B, H, S, dk, segs):
    """The value rows of segment s all equal s + 1: every output row of that segment is s + 1 whatever the scores are, within one rounding of
    P and one of O (2^-7 relative), and a neighbour's leak is off by at least 1.  Then K and V inside ONE segment of every sample are replaced
    (-3 x + 1): every row of that segment changes and every other row is bit-identical -- a row's result is a function of its own range."""
    lo, hi = _ranges(segs)
    Q, K, V = VR.attention_inputs(B, H, S, dk, seed=31 + S, device=DEV)
    want = torch.zeros((B, 1, S, 1), dtype=torch.float64, device=DEV)
    for b in range(B):
        start = 0
        for s, n in enumerate(segs[b]):
            V[b, :, start:start + n, :dk] = s + 1.0
            want[b, :, start:start + n] = s + 1.0
            start += n
    O, _ = run_attention(vit_ops, Q, K, V, S, dk, lo, hi)
    assert bool(((O.double() - want).abs() <= 2.0 ** -7 * want).all())
    Q, K, V = VR.attention_inputs(B, H, S, dk, seed=37 + S, device=DEV)
    O, _ = run_attention(vit_ops, Q, K, V, S, dk, lo, hi)
    K2, V2 = K.clone(), V.clone()
    inside = torch.zeros((B, S), dtype=torch.bool, device=DEV)
    for b in range(B):
        s = len(segs[b]) // 2                     # a middle segment
        s0 = sum(segs[b][:s])
        sl = slice(s0, s0 + segs[b][s])
        K2[b, :, sl, :dk] = (-3.0 * K[b, :, sl, :dk].float() + 1.0).bfloat16()
        V2[b, :, sl, :dk] = (-3.0 * V[b, :, sl, :dk].float() + 1.0).bfloat16()
        inside[b, sl] = True
    O2, _ = run_attention(vit_ops, Q, K2, V2, S, dk, lo, hi)
    same = (O2 == O).all(-1)                      # [B, H, S]
    assert bool(same[~inside[:, None].expand_as(same)].all())
    assert not bool(same[inside[:, None].expand_as(same)].any())
    VR.check_attention("vit_attention, one segment changed", O2, VR.attention_reference(Q, K2, V2, S, dk, dk ** -0.5, lo, hi))


def _hostile(kind, S):
    i = torch.arange(S)
    if kind == "non_monotonic":        # the rows' ranges walk backwards, in steps that cross tiles: row i reads the window opposite to it
        lo = ((S - 1 - i) // 7) * 7
        return lo.tolist(), (lo + 7).clamp_max(S).tolist()
    if kind == "excludes_own_row":     # every row reads the 10 keys that start 20 after it, wrapped: never itself
        lo = (i + 20) % (S - 10)
        return lo.tolist(), (lo + 10).tolist()
    if kind == "empty_rows":           # every third row, a whole wave (rows 32..63) and the last rows: hi == lo, and hi < lo
        lo, hi = torch.zeros(S, dtype=torch.long), torch.full((S,), S)
        lo[::3], hi[::3] = 40, 40
        lo[32:64], hi[32:64] = 70, 10
        lo[90:], hi[90:] = S, S
        return lo.tolist(), hi.tolist()
    assert kind == "clamped"           # -3 and 107 are [0, 100) after the clamp; unclamped they would still lie inside Spad = 128 and the arrays
    return [-3] * S, [107] * S


@pytest.mark.parametrize("kind", ["non_monotonic", "excludes_own_row", "empty_rows", "clamped"])
def test_attention_hostile_range_arrays(vit_ops, kind):
    """S = 100, Spad = 128: the arrays are taken as they are.  Keys that count for no row of a kind (and the keys in [S, Spad)) hold V = 50."""
    B, H, S, dk = 1, 2, 100, 80
    lo, hi = _hostile(kind, S)
    Q, K, V = VR.attention_inputs(B, H, S, dk, seed=53, Spad=128, device=DEV)
    ok = VR.counted(S, [lo], [hi], B)[0]
    unused = ~ok.any(0)
    V[:, :, :S][:, :, unused.to(DEV), :dk] = 50.0
    V[:, :, S:, :dk] = 50.0
    ref = VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, [lo], [hi])
    O, buf = run_attention(vit_ops, Q, K, V, S, dk, [lo], [hi], extra_cols=8, extra_rows=3)
    assert not bool(is_sentinel(buf[:, :S, :H * dk]).any()) and bool(is_sentinel(buf[:, S:]).all())
    empty = ~ok.any(-1)
    assert bool((O[0][:, empty.to(DEV)] == 0).all())            # exactly 0, and written
    assert bool((O[0][:, (~empty).to(DEV)] != 0).any(-1).all())
    worst = VR.check_attention("vit_attention hostile %s" % kind, O, ref)
    print("vit_attention hostile %s: %d empty rows, worst tile rel-L2 %.3e" % (kind, int(empty.sum()), worst))
    if kind == "clamped":
        Onull, _ = run_attention(vit_ops, Q, K, V, S, dk, None, None, extra_cols=8, extra_rows=3)
        assert torch.equal(Onull, O)


def test_attention_refusals(vit_ops):
    from x2i_amd._lib import X2IError
    Q, K, V = VR.attention_inputs(1, 2, 6, 80, seed=1, device=DEV)
    VT = V.transpose(-1, -2).contiguous()
    out = poisoned(1, 6, 256)
    r = _i32([[0] * 6])

    def call(H=2, S=6, Spad=64, dk=80, lo=None, hi=None, ldo=256, scale=0.1):
        vit_ops.attention(Q, K, VT, out, 1, H, S, Spad, dk, scale, ldo, 6 * 256, lo, hi)
    for bad in (dict(dk=32), dict(dk=96), dict(dk=72), dict(Spad=40), dict(S=70), dict(lo=r), dict(hi=r), dict(ldo=152), dict(ldo=162), dict(scale=0.0),
                dict(lo=r[:, :5], hi=r[:, :5])):
        with pytest.raises(X2IError):
            call(**bad)
    assert bool(is_sentinel(out).all())     # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- RoPE + head split
@pytest.mark.parametrize("S", [1, 77, 130])
@pytest.mark.parametrize("dk", [64, 80, 128])
def test_rope_split_vs_fp64_per_element(vit_ops, dk, S):
    """Tables as the tower makes them (angles up to 100 rad); q and k per element against float64 from the same f32 tables; VT bit-equal to
    the torch transposition; the padding (d >= dk, s >= S) untouched; the row stride honoured."""
    B, H = (2, 3) if S == 77 else (1, 2)
    g = torch.Generator().manual_seed(S * 100 + dk)
    ang = (100.0 * torch.rand((B, S, dk // 2), generator=g)).to(DEV)
    cos, sin = ang.cos(), ang.sin()
    W, Spad, dkp = 3 * H * dk, vit_ops.pad64(S), vit_ops.stored_width(dk)
    ld = W + 16
    qkv = torch.zeros((B * S, ld), dtype=torch.bfloat16, device=DEV)
    qkv[:, :W] = (2.0 * torch.randn((B * S, W), generator=g)).bfloat16().to(DEV)
    Q, K, VT = poisoned(B, H, Spad, dkp), poisoned(B, H, Spad, dkp), poisoned(B, H, dkp, Spad)
    vit_ops.rope_split(qkv, cos, sin, Q, K, VT, B, S, Spad, H, dk)
    q, k, v = qkv[:, :W].view(B, S, 3, H, dk).unbind(2)           # the library's reshape(S, 3, H, dk)
    eq = VR.check_rope("vit_rope_split q", Q[:, :, :S, :dk].transpose(1, 2), q, cos, sin)
    ek = VR.check_rope("vit_rope_split k", K[:, :, :S, :dk].transpose(1, 2), k, cos, sin)
    print("vit_rope_split B=%d S=%d H=%d dk=%d: worst error / bound q %.3f k %.3f" % (B, S, H, dk, eq, ek))
    assert torch.equal(VT[:, :, :dk, :S], v.permute(0, 2, 3, 1))
    for t in (Q[:, :, S:], Q[..., dk:], K[:, :, S:], K[..., dk:], VT[:, :, dk:], VT[..., S:]):
        assert bool(is_sentinel(t).all())
    # the zero angle is the identity
    vit_ops.rope_split(qkv, torch.ones_like(cos), torch.zeros_like(sin), Q, K, VT, B, S, Spad, H, dk)
    assert torch.equal(Q[:, :, :S, :dk].transpose(1, 2), q) and torch.equal(K[:, :, :S, :dk].transpose(1, 2), k)


def test_rope_split_refusals(vit_ops):
    from x2i_amd._lib import X2IError
    qkv = torch.zeros((6, 3 * 2 * 80), dtype=torch.bfloat16, device=DEV)
    Q, K, VT = poisoned(1, 2, 64, 128), poisoned(1, 2, 64, 128), poisoned(1, 2, 128, 64)
    cs = torch.ones((1, 6, 40), device=DEV)
    for bad in (dict(dk=96), dict(Spad=4), dict(ld=100), dict(ld=484)):
        kw = dict(dk=80, Spad=64, ld=None)
        kw.update(bad)
        c = cs if kw["dk"] == 80 else torch.ones((1, 6, kw["dk"] // 2), device=DEV)
        with pytest.raises(X2IError):
            vit_ops.rope_split(qkv, c, c, Q, K, VT, 1, 6, kw["Spad"], 2, kw["dk"], ld=kw["ld"])
    assert all(bool(is_sentinel(t).all()) for t in (Q, K, VT))


# ---------------------------------------------------------------------------------------------------------------- tower
TWO_GRIDS = [(1, 10, 10), (2, 6, 14)]
# (depth, hidden, heads, intermediate, out_hidden, fullatt, grid): the tiny tower with heads of 80 and one with heads of 64, on two grids (a
# video among them, 268 tokens) and on one image; one full-width layer of each kind (1280 hidden, 16 heads of 80, 3420 intermediate) at
# S = 100
TOWER_CASES = [(4, 160, 2, 172, 64, (1, 3), TWO_GRIDS), (4, 160, 2, 172, 64, (1, 3), [(1, 10, 10)]), (4, 128, 2, 172, 64, (1, 3), TWO_GRIDS),
               (4, 128, 2, 172, 64, (1, 3), [(1, 10, 10)]), (2, 1280, 16, 3420, 128, (1,), [(1, 10, 10)])]


@pytest.mark.parametrize("depth,hidden,heads,inter,out_hidden,fullatt,grid", TOWER_CASES)
def test_tower_vs_library_fp64_and_bf16(depth, hidden, heads, inter, out_hidden, fullatt, grid):
    from x2i_amd.qwen_vision import Qwen2_5VisionTower
    cfg, lib = VR.library_tower(depth, hidden, heads, inter, out_hidden, fullatt)
    sd = VR.random_tower_state_dict(lib, seed=hidden + len(grid))
    lib.load_state_dict(sd, strict=True)
    hip = Qwen2_5VisionTower(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)       # the views follow their padded storage to the GPU
    assert hip.blocks[0].mlp.up_proj.weight.data_ptr() == hip._fused["0.gu.w"][hip.Fp:].data_ptr() and hip.device.type == "cuda"
    px, g = VR.pixel_rows(grid, seed=hidden), torch.tensor(grid)
    S = px.shape[0]
    plan = hip.plan(g)
    px_dev = px.to(DEV)
    out = hip(px_dev, plan=plan)
    assert out.pooler_output.shape == (S // 4, out_hidden) and out.last_hidden_state.shape == (S, hidden) and out.pooler_output.dtype == torch.bfloat16
    first = (out.pooler_output.clone(), out.last_hidden_state.clone())
    # a second call with the same plan is bit-identical, and a planned forward only enqueues
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = hip(px_dev, plan=plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again.pooler_output, first[0]) and torch.equal(again.last_hidden_state, first[1])
    assert torch.equal(hip(px_dev, grid_thw=g.to(DEV)).pooler_output, first[0])         # without a plan: the same through grid_thw
    ref = lib.double()(px.double(), grid_thw=g)
    lib16 = lib.to(device=DEV, dtype=torch.bfloat16)(px_dev.bfloat16(), grid_thw=g.to(DEV))
    name = "Qwen2_5VisionTower depth=%d hidden=%d heads=%d inter=%d fullatt=%s grid %s" % (depth, hidden, heads, inter, fullatt, grid)
    for what, mine, theirs, want in (("pooler_output", first[0], lib16.pooler_output, ref.pooler_output),
                                     ("last_hidden_state", first[1], lib16.last_hidden_state, ref.last_hidden_state)):
        e_hip, e_lib = VR.rel_l2(mine, want), VR.rel_l2(theirs, want)
        print("%s %s: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, what, e_hip, e_lib, e_hip / e_lib))
        assert_stack_criterion(e_hip, e_lib)


# ---------------------------------------------------------------------------------------------------------------- hand-off
@pytest.fixture(scope="module")
def tiny_vl():
    """A tiny random Qwen2_5_VLForConditionalGeneration (tower: 2 layers, 2 heads of 80; decoder: hidden 256, 2 heads of 128, 2 layers) in bf16
    on the GPU, a prompt with two images, the conditioning slab of the library in float64 on the CPU and of the library in bf16 on the GPU"""
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
    from x2i_amd.handoff import prefill_hidden_states
    text = dict(vocab_size=64, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                max_position_embeddings=8192, rms_norm_eps=1e-6, hidden_act="silu", tie_word_embeddings=False, use_cache=False,
                rope_parameters=dict(rope_type="default", mrope_section=[16, 24, 24], rope_theta=1000000.0), bos_token_id=0, eos_token_id=1, pad_token_id=None)
    vis = dict(depth=2, hidden_size=160, num_heads=2, intermediate_size=172, out_hidden_size=256, fullatt_block_indexes=[1])
    cfg = Qwen2_5_VLConfig(text_config=text, vision_config=vis, image_token_id=60, video_token_id=61, vision_start_token_id=62, vision_end_token_id=63)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2_5_VLForConditionalGeneration(cfg).eval().requires_grad_(False)
    model.model.visual.load_state_dict(VR.random_tower_state_dict(model.model.visual, seed=5), strict=True)
    grid = torch.tensor([(1, 10, 10), (1, 6, 14)])
    ids = torch.tensor([[5, 6, 62] + [60] * 25 + [63, 7, 62] + [60] * 21 + [63, 8, 9, 10]])
    px = VR.pixel_rows(grid.tolist(), seed=9)
    ref = prefill_hidden_states(model.double(), dtype=torch.float64, input_ids=ids, pixel_values=px.double(), image_grid_thw=grid)
    model = model.to(device=DEV, dtype=torch.bfloat16)
    inputs = dict(input_ids=ids.to(DEV), pixel_values=px.to(DEV).bfloat16(), image_grid_thw=grid.to(DEV))
    return dict(model=model, inputs=inputs, ref=ref, lib_slab=prefill_hidden_states(model, **inputs).clone())


def test_hip_vision_against_the_library_tower_and_restores_the_forward(tiny_vl):
    """The conditioning slab with HipVision installed against the slab without it, both against the library in float64 on the CPU"""
    from x2i_amd.handoff import HipVision, find_visual, prefill_hidden_states
    model, inputs, ref, lib_slab = (tiny_vl[k] for k in ("model", "inputs", "ref", "lib_slab"))
    visual = find_visual(model)
    assert visual is model.model.visual
    hv = HipVision(model)
    with hv:
        assert "forward" in visual.__dict__
        slab = prefill_hidden_states(model, **inputs).clone()
    assert hv.calls == 1 and slab.shape == lib_slab.shape == ref.shape and not torch.equal(slab, lib_slab)      # the HIP tower ran
    e_hip, e_lib = VR.rel_l2(slab, ref), VR.rel_l2(lib_slab, ref)
    print("HipVision slab: rel-L2 against float64: HIP tower %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)
    # the tower's own forward is back: a plain library call gives the library's result again
    assert "forward" not in visual.__dict__
    assert torch.equal(prefill_hidden_states(model, **inputs), lib_slab)
    hv.install()
    hv.install()
    assert torch.equal(prefill_hidden_states(model, **inputs), slab)
    hv.remove()
    hv.remove()
    assert "forward" not in visual.__dict__ and torch.equal(prefill_hidden_states(model, **inputs), lib_slab)


def test_hip_vision_under_the_hip_decoder_prefill(tiny_vl):
    """The other kind of slab: handoff.HipPrefill (the decoder stack on the HIP path) with the library's tower and with the HIP tower"""
    from x2i_amd.handoff import HipPrefill, HipVision, find_visual
    model, inputs, ref, lib_slab = (tiny_vl[k] for k in ("model", "inputs", "ref", "lib_slab"))
    hp = HipPrefill(model)
    slab_dec = hp.prefill(model, **inputs).clone()
    with HipVision(model) as hv:
        slab_both = hp.prefill(model, **inputs).clone()
    assert hv.calls == 1 and slab_both.shape == ref.shape and not torch.equal(slab_both, slab_dec)
    e_both, e_dec, e_lib = VR.rel_l2(slab_both, ref), VR.rel_l2(slab_dec, ref), VR.rel_l2(lib_slab, ref)
    print("HipVision + HipPrefill slab: rel-L2 against float64: both on HIP %.3e, decoder alone %.3e, transformers bf16 on the GPU %.3e" % (e_both, e_dec, e_lib))
    assert_stack_criterion(e_both, e_lib)
    assert "forward" not in find_visual(model).__dict__ and torch.equal(hp.prefill(model, **inputs), slab_dec)
