"""The MiniCPM-o SigLIP vision tower without a GPU: the bucketised position ids against the library's, the float64 restatement of
tests/siglip_ref.py against the library in float64, the zero padding of the heads and of the MLP, the packed weights of
x2i_amd/siglip.py, the extension header include/x2i_siglip.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), every refusal, and the wiring of
handoff.HipSiglip and --hip_vision."""
import ctypes as C

import pytest
import torch

from tests import siglip_ref as SR
from tests.test_qwen_vision_ref_cpu import RESTATEMENT_BOUND  # (a constant; its tests are not re-collected here)

GRIDS = [(1, 1), (3, 5), (9, 9), (20, 27), (32, 32), (1, 70)]
TINY = dict(hidden_size=144, num_attention_heads=2, num_hidden_layers=2, intermediate_size=300)


def _tiny(**kw):
    from x2i_amd.siglip import SiglipVisionTower
    f = dict(TINY, device="cpu")
    f.update(kw)
    return SiglipVisionTower(**f)


# ---------------------------------------------------------------------------------------------------------------- position ids
@pytest.mark.parametrize("h,w", GRIDS)
def test_position_ids_equal_the_librarys(h, w):
    """the restatement, the module's cached function and a plan's ids against what Idefics2VisionEmbeddings indexes its table with"""
    from x2i_amd.siglip import bucket_position_ids
    want = SR.library_position_ids(h, w)
    got = SR.position_ids([(h, w)], h * w)
    assert got.dtype == torch.int64 and got.shape == (1, h * w) and torch.equal(got[0], want)
    assert torch.equal(bucket_position_ids(h, w, SR.SIDE), want)
    assert int(want.max()) < SR.SIDE ** 2 and int(want[0]) == 0
    p = _tiny().plan([(h, w), (1, 1)], h * w + 3)              # in a padded batch: the padding patches get id 0
    assert torch.equal(p.position_ids[0, :h * w], want) and not bool(p.position_ids[0, h * w:].any()) and not bool(p.position_ids[1].any())
    assert p.ids.dtype == torch.int32 and p.ids.shape == (2 * (h * w + 3),) and torch.equal(p.ids.long(), p.position_ids.reshape(-1))
    assert p.row_hi.dtype == torch.int32 and p.row_hi.tolist() == [[h * w] * (h * w + 3), [1] * (h * w + 3)] and not bool(p.row_lo.any())


def test_position_ids_are_no_integer_formula():
    """(i * side) // h is what exact arithmetic would give; float32 moves some bucket edges, and the model's own torch calls are the
    contract.  Measured over h = 1 .. 70: the ids differ from the integer formula at h = 25, 49, 50, 55, 58 -- and from
    Idefics2VisionEmbeddings, which multiplies an index by a step where the model's code takes an arange with that step, at h = 49 and 58.
    The grids of the library comparisons (here and on the GPU) are among the 68 sizes where the two agree."""
    from x2i_amd.siglip import bucket_position_ids
    h = w = 49
    exact = (((torch.arange(h) * SR.SIDE) // h)[:, None] * SR.SIDE + (torch.arange(w) * SR.SIDE) // w).flatten()
    got = SR.position_ids([(h, w)], h * w)[0]
    assert torch.equal(bucket_position_ids(h, w, SR.SIDE), got)
    print("49 x 49: %d of %d ids differ from the integer formula, %d from Idefics2VisionEmbeddings" % (
        int((got != exact).sum()), h * w, int((got != SR.library_position_ids(h, w)).sum())))
    assert not torch.equal(got, exact)
    assert int((got - exact).abs().max()) <= SR.SIDE + 1        # an edge moves a patch by one bucket per axis, never further


def test_plan_refuses_what_the_position_table_cannot_reach():
    tower = _tiny()
    for bad in ([(71, 1)], [(1, 71)], [(3, 5), (80, 1)]):
        with pytest.raises(ValueError, match="position"):
            tower.plan(bad, 100)
    for bad, L in (([], 4), ([(2, 3)], 5), ([(0, 3)], 5), ([(2, 3, 1)], 9), ([(2, 3)], 0)):
        with pytest.raises(ValueError, match="tgt_sizes"):
            tower.plan(bad, L)
    p = tower.plan([(2, 3)], 6)
    with pytest.raises(ValueError, match="GPU only"):          # a plan made on the CPU holds no workspaces
        tower(torch.zeros((1, 3, 14, 14 * 6)), plan=p)
    with pytest.raises(ValueError, match="strips"):
        tower(torch.zeros((1, 3, 16, 14 * 6)), tgt_sizes=torch.tensor([[2, 3]]))
    with pytest.raises(ValueError, match="position"):          # the fallback without tgt_sizes is one row of L patches
        tower(torch.zeros((1, 3, 14, 14 * 71)))


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def _lib_and_sd(seed, hidden=144, heads=2, inter=300, layers=2):
    cfg, lib = SR.library_tower(hidden, heads, inter, layers)
    sd = SR.random_state_dict(lib, seed)
    lib.load_state_dict(sd, strict=True)
    return cfg, lib, sd


@pytest.mark.parametrize("h,w", [(4, 6), (9, 9), (1, 1)])
def test_float64_restatement_equals_the_library_tower_in_float64(h, w):
    """single unpadded images; the library sees the 2-D image, the restatement the strip.  Both sides stay in float64 throughout (nn.LayerNorm
    has no float32 island as the Qwen tower's RMS norm has), so the bound of tests/test_qwen_vision_ref_cpu.py is generous here."""
    cfg, lib, sd = _lib_and_sd(seed=11)
    strips, images = SR.random_strips([(h, w)], h * w, seed=12)
    assert torch.equal(SR.strip_to_image(strips[0], h, w), images[0]) and torch.equal(SR.image_to_strip(images[0], 14, h * w + 2)[:, :, :14 * h * w], strips[0])
    want =SR.library_forward(lib.double(), [im.double() for im in images])[0]
    got = SR.tower_reference(sd, strips, [(h, w)], num_heads=2)[0]
    e = SR.rel_l2(got, want)
    print("float64 restatement against the library in float64, grid %d x %d: %.3e" % (h, w, e))
    assert got.shape == want.shape == (h * w, 144) and e < RESTATEMENT_BOUND, e
    assert float(want.std()) > 0.1
    if h * w > 1:       # the restatement knows its position ids: another grid of the same patch count is another result
        other = SR.tower_reference(sd, strips, [(w, h) if h != w else (1, h * w)], num_heads=2)[0]
        assert SR.rel_l2(other, want) > 1e-3


def test_padded_batch_rows_equal_the_single_image_rows():
    """keys [0, n_b) for every row: a sample's valid rows do not depend on the batch it is padded into"""
    cfg, lib, sd = _lib_and_sd(seed=13)
    grids = [(3, 5), (9, 9), (1, 1)]
    strips, images = SR.random_strips(grids, 81, seed=14)
    out = SR.tower_reference(sd, strips, grids, num_heads=2)
    assert bool(torch.isfinite(out).all())
    for b, (h, w) in enumerate(grids):
        alone = SR.tower_reference(sd, strips[b:b + 1, :, :, :14 * h * w], [(h, w)], num_heads=2)[0]
        assert SR.rel_l2(out[b, :h * w], alone) < 1e-12


# float64 rounding: the padded products add exact zeros, but a BLAS call may block a sum of another length differently, so the two runs
# differ by a few units of 2^-53 per sum; two layers of sums of at most 320 terms stay below 1e-13, and the bound is ten times that.
PADDING_BOUND = 1e-12


def test_zero_padded_heads_and_mlp_leave_the_result_alone():
    cfg, lib, sd = _lib_and_sd(seed=15)
    grids = [(3, 5), (4, 4)]
    strips, _ = SR.random_strips(grids, 16, seed=16)
    want = SR.tower_reference(sd, strips, grids, num_heads=2)
    heads = SR.pad_heads(sd, 2, 72, 80)
    assert heads["encoder.layers.1.self_attn.q_proj.weight"].shape == (160, 144) and heads["encoder.layers.1.self_attn.out_proj.weight"].shape == (144, 160)
    both = SR.pad_mlp(heads, 320)
    assert both["encoder.layers.0.mlp.fc1.weight"].shape == (320, 144) and both["encoder.layers.0.mlp.fc2.weight"].shape == (144, 320)
    e_heads = SR.rel_l2(SR.tower_reference(heads, strips, grids, num_heads=2, scale_dim=72), want)
    e_both = SR.rel_l2(SR.tower_reference(both, strips, grids, num_heads=2, scale_dim=72), want)
    print("padded heads %.3e, padded heads and MLP %.3e (bound %.1e)" % (e_heads, e_both, PADDING_BOUND))
    assert e_heads < PADDING_BOUND and e_both < PADDING_BOUND
    # the scale is the real width's: with 80 ** -0.5 the padded tower is another tower
    assert SR.rel_l2(SR.tower_reference(heads, strips, grids, num_heads=2), want) > 1e-3


def test_packed_weights_are_the_zero_padded_parameters():
    cfg, lib, sd = _lib_and_sd(seed=17)
    tower = _tiny()
    tower.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    assert (tower.dkp, tower.Fp, tower.Kp, tower.side, tower.config.head_dim) == (80, 320, 640, 70, 72)
    want = SR.pad_mlp(SR.pad_heads(sd, 2, 72, 80), 320)
    for i in range(2):
        p = "encoder.layers.%d." % i
        qkv_w, qkv_b, out_w = tower._packed[i]
        assert qkv_w.shape == (480, 144) and qkv_b.shape == (480,) and out_w.shape == (144, 160)
        assert torch.equal(qkv_w.float(), torch.cat([want[p + "self_attn.%s_proj.weight" % n] for n in "qkv"]))
        assert torch.equal(qkv_b.float(), torch.cat([want[p + "self_attn.%s_proj.bias" % n] for n in "qkv"]))
        assert torch.equal(out_w.float(), want[p + "self_attn.out_proj.weight"])
        assert not bool(qkv_w.view(3, 2, 80, 144)[:, :, 72:].any()) and not bool(qkv_b.view(3, 2, 80)[:, :, 72:].any())
        assert not bool(out_w.view(144, 2, 80)[:, :, 72:].any())
        assert torch.equal(tower._fused["%d.fc1.w" % i].float(), want[p + "mlp.fc1.weight"])
        assert torch.equal(tower._fused["%d.fc1.b" % i].float(), want[p + "mlp.fc1.bias"])
        assert torch.equal(tower._fused["%d.fc2" % i].float(), want[p + "mlp.fc2.weight"])
    pe = tower._fused["pe"].float()
    assert pe.shape == (144, 640) and torch.equal(pe[:, :588], sd["embeddings.patch_embedding.weight"].reshape(144, 588)) and not bool(pe[:, 588:].any())
    # heads that need no padding are packed as they are
    assert [_tiny(hidden_size=h).dkp for h in (128, 160, 256)] == [64, 80, 128]
    full = _tiny(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, num_hidden_layers=1)
    assert (full.dkp, full.Fp, full.Kp, full.config.head_dim) == (80, 4352, 640, 72)


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import siglip_ops
    lib = siglip_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    rows = lambda **kw: lib.x2i_siglip_patch_rows_bf16(*[kw.get(k, d) for k, d in (
        ("strips", fake), ("sbs", 3 * 14 * 98), ("sld", 98), ("Xp", fake), ("ldx", 640), ("B", 2), ("L", 7), ("P", 14), ("Kp", 640), ("st", None))])
    assert rows(P=0) < 0 and b"P=0" in err()
    assert rows(P=33, Kp=3272, ldx=3272, sld=231, sbs=3 * 33 * 231) < 0 and b"P=33" in err()
    assert rows(B=0) < 0 and rows(L=0) < 0
    assert rows(Kp=584, ldx=584) < 0 and b"Kp=584" in err()     # < 3 * P * P
    assert rows(Kp=636) < 0 and b"Kp=636" in err()             # not a multiple of 8
    assert rows(ldx=632) < 0 and b"ldx" in err()               # < Kp
    assert rows(ldx=644) < 0 and b"ldx" in err()
    assert rows(sld=97) < 0 and b"strip_ld" in err()           # < P * L
    assert rows(sbs=3 * 14 * 98 - 1) < 0 and b"strip_batch_stride" in err()
    assert rows(Xp=C.c_void_p(0x1008)) < 0 and b"aligned" in err()
    assert rows(strips=C.c_void_p(0x1001)) < 0 and b"aligned" in err()
    for k in ("strips", "Xp"):
        assert rows(**{k: None}) < 0 and b"null" in err()
    add = lambda **kw: lib.x2i_siglip_add_positions_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("ldx", 144), ("ids", fake), ("pos", fake), ("n_pos", 4900), ("rows", 77), ("D", 144), ("st", None))])
    assert add(D=140, ldx=140) < 0 and b"D=140" in err()
    assert add(D=0) < 0 and add(rows=0) < 0 and add(n_pos=0) < 0
    assert add(ldx=136) < 0 and b"ldx" in err()
    assert add(ldx=148) < 0 and b"ldx" in err()
    assert add(ids=C.c_void_p(0x1002)) < 0 and b"aligned" in err()
    assert add(X=C.c_void_p(0x1008)) < 0 and add(pos=C.c_void_p(0x1008)) < 0
    for k in ("X", "ids", "pos"):
        assert add(**{k: None}) < 0 and b"null" in err()
    split = lambda **kw: lib.x2i_siglip_head_split_bf16(*[kw.get(k, d) for k, d in (
        ("qkv", fake), ("ld", 960), ("Q", fake), ("K", fake), ("VT", fake), ("B", 1), ("S", 77), ("Spad", 128), ("H", 4), ("dk", 80), ("st", None))])
    assert split(dk=72) < 0 and b"dk=72" in err()
    assert split(dk=32) < 0 and split(dk=96) < 0 and b"dk=96" in err()
    assert split(ld=952) < 0 and b"ld" in err()                # < 3 * H * dk
    assert split(ld=964) < 0
    assert split(Spad=76) < 0 and split(Spad=100) < 0 and split(H=0) < 0 and split(H=70000) < 0 and split(B=0) < 0
    for k in ("qkv", "Q", "K", "VT"):
        assert split(**{k: None}) < 0 and b"null" in err()
    assert split(Q=C.c_void_p(0x1008)) < 0 and b"aligned" in err()


# ---------------------------------------------------------------------------------------------------------------- host module
def test_unsupported_configurations_raise():
    for bad, msg in ((dict(dtype=torch.float16), "bf16"), (dict(dtype=torch.float32), "bf16"), (dict(hidden_act="gelu"), "gelu_pytorch_tanh"),
                     (dict(hidden_size=192), "head widths"), (dict(num_attention_heads=3), "head widths"), (dict(num_hidden_layers=0), "layer"),
                     (dict(num_channels=1), "channels"), (dict(patch_size=40), "patch_size")):
        with pytest.raises(ValueError, match=msg):
            _tiny(**bad)
    with pytest.raises(TypeError, match="unknown"):
        _tiny(depth=2)
    with pytest.raises(ValueError, match="bf16"):
        _tiny().float()


def test_parameter_names_are_the_librarys_and_the_packed_copies_follow_the_module():
    cfg, lib, want = _lib_and_sd(seed=2)
    tower = _tiny()
    lib_sd, sd = lib.state_dict(), tower.state_dict()
    assert set(sd) == set(lib_sd) and all(sd[k].shape == lib_sd[k].shape for k in sd)
    assert "embeddings.position_embedding.weight" in sd and sd["embeddings.position_embedding.weight"].shape == (4900, 144)
    tower.load_state_dict({k: v.bfloat16() for k, v in want.items()}, strict=True)
    assert all(torch.equal(v.float(), want[k]) for k, v in tower.state_dict().items())
    with pytest.raises(RuntimeError):
        tower.load_state_dict({k: v for k, v in want.items() if k != "encoder.layers.1.self_attn.k_proj.bias"}, strict=True)
    m = tower.encoder.layers[1].mlp
    assert m.fc1.weight.data_ptr() == tower._fused["1.fc1.w"].data_ptr() and m.fc2.weight.stride() == (320, 1)
    assert tower.embeddings.patch_embedding.weight.shape == (144, 3, 14, 14) and tower.embeddings.patch_embedding.weight.data_ptr() == tower._fused["pe"].data_ptr()
    # _apply re-points the views and makes the packed copies again
    before = tower._packed[0][0]
    t2 = tower.to(torch.bfloat16)
    assert t2.encoder.layers[1].mlp.fc1.weight.data_ptr() == t2._fused["1.fc1.w"].data_ptr()
    assert t2._packed[0][0] is not before and torch.equal(t2._packed[0][0], before)
    # from_hf copies an instantiated tower
    from x2i_amd.siglip import SiglipVisionTower
    copy = SiglipVisionTower.from_hf(lib)
    assert copy.device.type == "cpu" and copy.config.head_dim == 72 and copy.config.num_hidden_layers == 2 and copy.config.intermediate_size == 300
    assert all(torch.equal(v.float(), want[k]) for k, v in copy.state_dict().items()) and torch.equal(copy._packed[1][2], tower._packed[1][2])


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_harness_help_names_both_towers():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("minicpm")
    assert p.parse_args(["--synthetic"]).hip_vision is False
    assert p.parse_args(["--synthetic", "--hip_vision", "--full_generate"]).hip_vision is True
    text = " ".join(p.format_help().split())
    assert "MiniCPM-o" in text and "model.vpm" in text and "Qwen2.5-VL" in text


def test_find_vpm_and_hip_siglip_install_remove_without_a_gpu():
    """install / remove swap `forward` on the instance and restore what was there (nothing, or an earlier instance attribute)"""
    from x2i_amd import handoff
    from x2i_amd.infer.inference_minicpm import MiniCPMConditioner
    cfg, lib = SR.library_tower(144, 2, 300, 1)
    outer = torch.nn.Module()
    outer.vpm = lib
    assert handoff.find_vpm(outer) is lib
    bare = torch.nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="vpm"):
        handoff.find_vpm(bare)
    with pytest.raises(RuntimeError, match="vpm"):
        handoff.HipSiglip(bare)
    with pytest.raises(RuntimeError, match="vpm"):
        MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare, hip_vision=True)
    assert MiniCPMConditioner(None, "cpu", prefill_only=False, model=bare).vision is None
    hs = handoff.HipSiglip(outer)
    assert "forward" not in lib.__dict__ and hs.calls == 0
    with hs:
        assert lib.__dict__["forward"] == hs._forward
    assert "forward" not in lib.__dict__
    with pytest.raises(KeyError):
        with hs:
            raise KeyError("inside")
    assert "forward" not in lib.__dict__
    cond = MiniCPMConditioner(None, "cpu", prefill_only=False, model=outer, hip_vision=True)      # reaches HipSiglip.install()
    assert lib.__dict__["forward"] == cond.vision._forward
    cond.vision.remove()
    mine = lambda *a, **k: None
    lib.forward = mine
    hs.install().install()
    hs.remove()
    assert lib.__dict__["forward"] is mine
