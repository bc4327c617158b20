"""The Qwen2.5-VL vision tower without a GPU: the host work of a call (x2i_amd/qwen_vision.py: plan) against the library's own functions, the
padded packed weights and the float64 restatement of tests/qwen_vision_ref.py against the library in float64, the extension header
include/x2i_vit.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and every refusal."""
import ctypes as C

import pytest
import torch

from tests import qwen_vision_ref as VR

TWO_GRIDS = [(1, 10, 10), (2, 6, 14)]
GRIDS = [[(1, 10, 10)], TWO_GRIDS, [(1, 4, 4)], [(1, 18, 10), (1, 2, 2)]]
TINY = dict(depth=4, hidden_size=160, num_heads=2, intermediate_size=172, out_hidden_size=64, fullatt_block_indexes=[1, 3])


def _tiny(**kw):
    from x2i_amd.qwen_vision import Qwen2_5VisionTower
    f = dict(TINY, device="cpu")
    f.update(kw)
    return Qwen2_5VisionTower(**f)


# ---------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "_".join("x".join(str(v) for v in e) for e in g))
def test_plan_equals_the_librarys_functions(grid):
    from transformers.vision_utils import get_vision_attention_seqlens, get_vision_position_ids, get_vision_window_index
    cfg, lib = VR.library_tower(1, 160, 2, 172, 64, (0,))
    tower = _tiny()
    g = torch.tensor(grid)
    p = tower.plan(g)
    widx, cu_win = get_vision_window_index(g, spatial_merge_size=2, window_size=112, patch_size=14)
    cu, _ = get_vision_attention_seqlens(g, cfg)
    pos = get_vision_position_ids(g, 2)
    S = int(g.prod(-1).sum())
    assert p.S == S and p.Spad == (S + 63) // 64 * 64 and p.grid == tuple(tuple(e) for e in grid)
    assert torch.equal(p.window_index, widx) and torch.equal(p.reverse, torch.argsort(widx))
    assert torch.equal(p.cu_window_seqlens, cu_win) and p.cu_window_seqlens.dtype == cu_win.dtype == torch.int32
    assert torch.equal(p.cu_seqlens, cu) and p.cu_seqlens.dtype == cu.dtype
    assert torch.equal(p.position_ids, pos)
    # the token permutation is the library's gather of whole merge units, and the inverse undoes it on the merged rows
    x = torch.arange(S * 3.0).reshape(S, 3)
    assert torch.equal(x[p.perm], x.reshape(S // 4, 4, 3)[widx].reshape(S, 3))
    assert torch.equal(p.window_index[p.reverse], torch.arange(S // 4))
    # the half tables in window order, bit for bit the library's f32 expression
    emb = lib.rotary_pos_emb(pos).reshape(S // 4, 4, -1)[widx].reshape(S, -1)
    assert emb.shape == (S, 40) and p.cos.dtype == torch.float32
    assert torch.equal(p.cos[0], emb.cos()) and torch.equal(p.sin[0], emb.sin())
    # the key ranges are a Python-loop expansion of the two cu_seqlens
    for (lo, hi), c in (((p.win_lo, p.win_hi), cu_win), ((p.full_lo, p.full_hi), cu)):
        want = VR.cu_ranges(c.tolist())
        assert lo.dtype == hi.dtype == torch.int32 and lo.shape == hi.shape == (1, S) and lo.is_contiguous()
        assert lo[0].tolist() == want[0] and hi[0].tolist() == want[1]
    if grid == TWO_GRIDS:
        assert (cu_win[1:] - cu_win[:-1]).tolist() == [64, 16, 16, 4, 48, 36, 48, 36] and (cu[1:] - cu[:-1]).tolist() == [100, 84, 84]


def test_plan_refuses_grids_it_cannot_pack():
    tower = _tiny()
    for bad in ([], [(1, 5, 4)], [(1, 4, 3)], [(0, 4, 4)], [(1, 4)]):
        with pytest.raises(ValueError, match="merge unit"):
            tower.plan(bad)
    p = tower.plan([(1, 4, 4)])
    with pytest.raises(ValueError, match="GPU only"):        # a plan made on the CPU holds no workspaces
        tower(torch.zeros((16, 1176)), plan=p)
    with pytest.raises(ValueError, match="grid_thw or a plan"):
        tower(torch.zeros((16, 1176)))


# ---------------------------------------------------------------------------------------------------------------- packed weights
def test_padded_packed_weights_reproduce_the_unpadded_mlp_bit_for_bit():
    """float64 with the products of every output element added in the order of k (VR.ordered_linear): the zero rows of [gate; up], their zero
    biases and the zero columns of down_proj add exact zeros"""
    cfg, lib = VR.library_tower(**_lib_kw())
    sd = VR.random_tower_state_dict(lib, seed=3)
    tower = _tiny()
    tower.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    assert tower.Fp == 192 and tower.Kp == 1216
    f = torch.float64
    x = torch.randn((37, 160), generator=torch.Generator().manual_seed(4)).bfloat16().to(f)
    for i in (0, 3):
        p = "blocks.%d.mlp." % i
        want = VR.mlp_reference(x, *(sd[p + n].to(f) for n in ("gate_proj.weight", "gate_proj.bias", "up_proj.weight", "up_proj.bias", "down_proj.weight",
                                                               "down_proj.bias")))
        gu_w, gu_b, down = (tower._fused["%d.%s" % (i, n)].to(f) for n in ("gu.w", "gu.b", "down"))
        assert gu_w.shape == (384, 160) and down.shape == (160, 192)
        assert not bool(gu_w[172:192].any()) and not bool(gu_w[364:].any()) and not bool(gu_b[172:192].any()) and not bool(down[:, 172:].any())
        got = VR.packed_mlp_reference(x, gu_w, gu_b, down, tower.blocks[i].mlp.down_proj.bias.to(f))
        assert torch.equal(got, want) and float(want.abs().max()) > 0.1
    # the patch embedding: the Conv3d kernel is the first 1176 columns of the padded matrix, and the padded product adds exact zeros
    pe = tower._fused["pe"].to(f)
    w = sd["patch_embed.proj.weight"].to(f).reshape(160, -1)
    assert torch.equal(pe[:, :1176], w) and not bool(pe[:, 1176:].any())
    px = VR.pixel_rows([(1, 2, 2)], seed=5).to(f)
    assert torch.equal(VR.ordered_linear(torch.cat((px, torch.zeros((4, 40), dtype=f)), 1), pe), VR.ordered_linear(px, w))


def _lib_kw():
    return dict(depth=4, hidden=160, heads=2, inter=172, out_hidden=64, fullatt=(1, 3))


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
# The restatement differs from the library in float64 only where the library leaves float64: Qwen2_5_VLRMSNorm normalises in float32 (nine
# norms on this path, relative error 2^-24 = 6e-8 each, as in the decoder's restatement, which measured 7.6e-8) and the rotary table is
# evaluated in float32 on both sides.  Measured on the CPU: 1.32e-7 (last_hidden_state) and 1.39e-7 / 1.42e-7 (pooler_output) on the two
# inputs; the bound is three times the larger.  A tower that mixes up its window and full-attention layers is off by more than 1e-3.
RESTATEMENT_BOUND = 4.3e-7


@pytest.mark.parametrize("grid", [TWO_GRIDS, [(1, 10, 10)]])
def test_float64_restatement_equals_the_library_tower_in_float64(grid):
    from transformers.vision_utils import get_vision_attention_seqlens, get_vision_position_ids, get_vision_window_index
    cfg, lib = VR.library_tower(**_lib_kw())
    sd = VR.random_tower_state_dict(lib, seed=11)
    lib.load_state_dict(sd, strict=True)
    g = torch.tensor(grid)
    px = VR.pixel_rows(grid, seed=12)
    out = lib.double()(px.double(), grid_thw=g)
    widx, cu_win = get_vision_window_index(g, spatial_merge_size=2, window_size=112, patch_size=14)
    cu, _ = get_vision_attention_seqlens(g, cfg)
    last, pooled = VR.tower_reference(sd, px, widx, cu_win.tolist(), cu.tolist(), get_vision_position_ids(g, 2), num_heads=2, fullatt=(1, 3))
    e_last, e_pool = VR.rel_l2(last, out.last_hidden_state), VR.rel_l2(pooled, out.pooler_output)
    print("float64 restatement against the library in float64, grid %s: last_hidden_state %.3e pooler_output %.3e" % (grid, e_last, e_pool))
    assert e_last < RESTATEMENT_BOUND and e_pool < RESTATEMENT_BOUND, (e_last, e_pool)
    assert float(out.pooler_output.std()) > 0.05
    # the restatement tells window layers from full-attention layers, and the window order from the original one
    other, _ = VR.tower_reference(sd, px, widx, cu_win.tolist(), cu.tolist(), get_vision_position_ids(g, 2), num_heads=2, fullatt=(0, 2))
    assert VR.rel_l2(other, out.last_hidden_state) > 1e-3


def test_attention_reference_and_checker():
    """rows of an empty range are 0; the clamp; and a neighbour's leak fails the per-tile bound"""
    B, H, S, dk = 1, 2, 100, 80
    Q, K, V = VR.attention_inputs(B, H, S, dk, seed=1)
    lo, hi = VR.segment_ranges([64, 16, 16, 4])
    assert lo[63:66] == [0, 64, 64] and hi[63:66] == [64, 80, 80] and hi[-1] == 100
    ref = VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, [lo], [hi])
    assert VR.check_attention("same", ref, ref) == 0.0
    # every segment alone gives the same rows
    r1 = VR.attention_reference(Q[:, :, 64:80], K[:, :, 64:80], V[:, :, 64:80], 16, dk, dk ** -0.5)
    assert torch.allclose(ref[:, :, 64:80], r1, rtol=0, atol=1e-12)
    leak = VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, [lo], [[h + 1 if h < S else h for h in hi]])     # one key of the next segment
    with pytest.raises(AssertionError, match="rel-L2"):
        VR.check_attention("leak", leak, ref)
    e_lo, e_hi = list(lo), list(hi)
    e_lo[5], e_hi[5] = 70, 10
    assert not bool(VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, [e_lo], [e_hi])[:, :, 5].any())
    assert torch.equal(VR.attention_reference(Q, K, V, S, dk, dk ** -0.5, [[-3] * S], [[107] * S]), VR.attention_reference(Q, K, V, S, dk, dk ** -0.5))


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import vit_ops
    lib = vit_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    att = lambda **kw: lib.x2i_vit_attention_bf16(*[kw.get(k, d) for k, d in (
        ("Q", fake), ("K", fake), ("VT", fake), ("lo", None), ("hi", None), ("O", fake), ("B", 1), ("H", 4), ("S", 77), ("Spad", 128),
        ("dk", 80), ("scale", 0.11), ("ldo", 320), ("obs", 77 * 320), ("st", None))])
    assert att(dk=32) < 0 and b"dk=32" in err()
    assert att(dk=96) < 0 and b"dk=96" in err()
    assert att(dk=72) < 0 and b"dk=72" in err()
    assert att(H=0) < 0 and att(B=0) < 0
    assert att(Spad=100) < 0 and b"Spad" in err()
    assert att(Spad=64) < 0 and b"Spad" in err()              # Spad < S
    assert att(lo=fake) < 0 and b"both" in err()
    assert att(hi=fake) < 0 and b"both" in err()
    assert att(lo=C.c_void_p(0x1002), hi=fake) < 0 and b"aligned" in err()
    assert att(ldo=312, obs=77 * 312) < 0 and b"H*dk" in err()
    assert att(ldo=322) < 0 and b"aligned" in err()
    assert att(Q=C.c_void_p(0x1008)) < 0 and b"aligned" in err()
    for k in ("Q", "K", "VT", "O"):
        assert att(**{k: None}) < 0 and b"null" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert att(scale=bad) < 0 and b"scale" in err()
    rope = lambda **kw: lib.x2i_vit_rope_split_bf16(*[kw.get(k, d) for k, d in (
        ("qkv", fake), ("ld", 960), ("cos", fake), ("sin", fake), ("Q", fake), ("K", fake), ("VT", fake), ("B", 1), ("S", 77), ("Spad", 128),
        ("H", 4), ("dk", 80), ("st", None))])
    assert rope(dk=32) < 0 and b"dk=32" in err()
    assert rope(dk=96) < 0 and b"dk=96" in err()
    assert rope(ld=952) < 0 and b"ld" in err()                # < 3 * H * dk
    assert rope(ld=964) < 0
    assert rope(Spad=76) < 0 and rope(Spad=100) < 0 and rope(H=0) < 0 and rope(H=40000) < 0
    for k in ("qkv", "cos", "sin", "Q", "K", "VT"):
        assert rope(**{k: None}) < 0 and b"null" in err()
    assert rope(cos=C.c_void_p(0x1004)) < 0 and b"aligned" in err()


# ---------------------------------------------------------------------------------------------------------------- host module
def test_unsupported_configurations_raise():
    for bad, msg in ((dict(dtype=torch.float16), "bf16"), (dict(dtype=torch.float32), "bf16"), (dict(hidden_act="gelu"), "silu"),
                     (dict(hidden_size=144), "head widths"), (dict(hidden_size=192), "head widths"), (dict(num_heads=3), "head widths"),
                     (dict(depth=0), "layer"), (dict(window_size=14), "window_size")):
        with pytest.raises(ValueError, match=msg):
            _tiny(**bad)
    with pytest.raises(TypeError, match="unknown"):
        _tiny(num_layers=2)
    with pytest.raises(ValueError, match="bf16"):
        _tiny().float()
    for ok in (dict(hidden_size=128), dict(hidden_size=256), dict(hidden_size=1280, num_heads=16, depth=1)):
        _tiny(**ok)


def test_parameter_names_are_the_librarys_and_views_share_padded_storage():
    cfg, lib = VR.library_tower(**_lib_kw())
    tower = _tiny()
    lib_sd = lib.state_dict()
    sd = tower.state_dict()
    assert set(sd) == set(lib_sd) and all(sd[k].shape == lib_sd[k].shape for k in sd)
    want = VR.random_tower_state_dict(lib, seed=2)
    tower.load_state_dict({k: v.bfloat16() for k, v in want.items()}, strict=True)
    assert all(torch.equal(v.float(), want[k]) for k, v in tower.state_dict().items())
    with pytest.raises(RuntimeError):
        tower.load_state_dict({k: v for k, v in want.items() if k != "blocks.1.attn.qkv.bias"}, strict=True)
    m = tower.blocks[2].mlp
    assert m.gate_proj.weight.data_ptr() == tower._fused["2.gu.w"].data_ptr() and m.up_proj.weight.data_ptr() == tower._fused["2.gu.w"][192:].data_ptr()
    assert m.down_proj.weight.data_ptr() == tower._fused["2.down"].data_ptr() and m.down_proj.weight.stride() == (192, 1)
    assert tower.patch_embed.proj.weight.shape == (160, 3, 2, 14, 14) and tower.patch_embed.proj.weight.data_ptr() == tower._fused["pe"].data_ptr()
    # _apply re-points the views
    t2 = tower.to(torch.bfloat16)
    assert t2.blocks[2].mlp.up_proj.weight.data_ptr() == t2._fused["2.gu.w"][192:].data_ptr()
    # from_hf copies an instantiated tower
    from x2i_amd.qwen_vision import Qwen2_5VisionTower
    lib.load_state_dict(want, strict=True)
    copy = Qwen2_5VisionTower.from_hf(lib)
    assert copy.device.type == "cpu" and copy.config.fullatt_block_indexes == (1, 3) and copy.config.head_dim == 80
    assert all(torch.equal(v.float(), want[k]) for k, v in copy.state_dict().items())
    assert not bool(copy._fused["0.gu.w"][172:192].any()) and not bool(copy._fused["pe"][:, 1176:].any())


def test_harness_takes_the_hip_vision_flag_and_defaults_stay():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("qwenvl")
    a = p.parse_args(["--synthetic"])
    assert a.hip_vision is False and a.hip_decoder is False and a.full_generate is False
    b = p.parse_args(["--synthetic", "--hip_vision"])
    assert b.hip_vision is True and b.hip_decoder is False
    assert p.parse_args(["--synthetic", "--hip_vision", "--hip_decoder", "--full_generate"]).hip_vision is True


def test_find_visual_and_hip_vision_install_remove_without_a_gpu():
    """install / remove swap `forward` on the instance and restore what was there (nothing, or an earlier instance attribute)"""
    from x2i_amd import handoff
    cfg, lib = VR.library_tower(1, 160, 2, 172, 64, (0,))
    outer = torch.nn.Module()
    outer.model = torch.nn.Module()
    outer.model.visual = lib
    assert handoff.find_visual(outer) is lib and handoff.find_visual(outer.model) is lib
    with pytest.raises(RuntimeError, match="vision tower"):
        handoff.find_visual(torch.nn.Linear(2, 2))
    hv = handoff.HipVision(outer)
    assert "forward" not in lib.__dict__
    with hv:
        assert lib.__dict__["forward"] == hv._forward
    assert "forward" not in lib.__dict__
    mine = lambda *a, **k: None
    lib.forward = mine
    hv.install().install()
    hv.remove()
    assert lib.__dict__["forward"] is mine
