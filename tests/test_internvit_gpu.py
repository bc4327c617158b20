"""The InternVL2.5 vision path on the HIP path (include/x2i_internvit.h, x2i_amd/internvit.py, handoff.HipInternVision) on the GPU: the row
kernels bit for bit against torch (and, for the LayerNorm, per element against float64), and the tower with its tail against the float64
restatement of tests/internvit_ref.py, no worse than 1.5 x the bf16 restatement run with torch on the same GPU.  No test reads the
reference tree."""
import pytest
import torch

from tests import internvit_ref as IR
from tests.test_t5_gpu import is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def iops():
    from x2i_amd import internvit_ops as o
    o.load()
    return o


def _bf(shape, seed, amp=1.0):
    return (amp * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).bfloat16().to(DEV)


# ---------------------------------------------------------------------------------------------------------------- patch rows
@pytest.mark.parametrize("B,gh,gw,P", [(2, 2, 3, 14), (1, 32, 32, 14)])
def test_patch_rows_is_the_torch_permutation(iops, B, gh, gw, P):
    """tiles that are a window of a wider tensor (row, channel and sample strides beyond the tile's, a start that is only 2-byte aligned), an
    output wider than Kp and longer than B * L: the footprint is rows < B * L, columns < Kp, and the tail columns 3 P^2 .. Kp-1 are zero.
    The grid 2 x 3 is not square, so rows exchanged for columns would show."""
    wide = _bf((B, 3, gh * P + 3, gw * P + 10), 100 * gh + B)
    img = wide[:, :, 2:2 + gh * P, 3:3 + gw * P]
    assert not img.is_contiguous()
    L = gh * gw
    want = img.reshape(B, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * L, 3 * P * P)
    for Kp in (640, 592):
        buf = poisoned(B * L + 2, Kp + 16)
        iops.patch_rows(img, buf, P, Kp)
        assert torch.equal(buf[:B * L, :3 * P * P], want)
        assert not bool(buf[:B * L, 3 * P * P:Kp].view(torch.int16).any())
        assert bool(is_sentinel(buf[B * L:]).all()) and bool(is_sentinel(buf[:, Kp:]).all())
    assert torch.equal(IR.patch_rows(img, P, 640), torch.cat((want, want.new_zeros((B * L, 52))), 1))      # (the restatement's helper agrees)
    again = poisoned(B * L + 2, 592 + 16)
    iops.patch_rows(img.contiguous(), again, P, 592)
    assert torch.equal(again, buf)              # the contiguous copy gives the same rows
    # and the rows are what the Conv2d sees: row b*L + r*gw + q is the patch at (r, q)
    r, q = gh - 1, gw - 2
    assert torch.equal(buf[(B - 1) * L + r * gw + q, :3 * P * P], img[B - 1, :, r * P:(r + 1) * P, q * P:(q + 1) * P].reshape(-1))


# ---------------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("B,L,D", [(2, 6, 64), (2, 1024, 1024)])
def test_embed_is_the_torch_bf16_add(iops, B, L, D):
    """bit-identical to torch's bf16 `cat([class, patches]) + position`; the class row of X is written without being read (it holds NaN);
    a relaunch on a fresh copy gives the same bits; nothing beyond X is touched"""
    pe, cls, pos = _bf((B, L, D), L + D), _bf((1, 1, D), 3), _bf((1, 1 + L, D), 4, 0.5)
    want = torch.cat([cls.expand(B, 1, -1), pe], dim=1) + pos
    assert want.dtype == torch.bfloat16
    out = []
    for _ in range(2):
        buf = poisoned(B + 1, 1 + L, D)
        buf[:B, 1:] = pe
        buf[:B, 0] = float("nan")
        iops.embed(buf[:B], cls, pos)
        assert bool(is_sentinel(buf[B:]).all())
        out.append(buf[:B].clone())
    assert torch.equal(out[0], want) and torch.equal(out[1], out[0])


# ---------------------------------------------------------------------------------------------------------------- shuffle + LayerNorm
SHUFFLE_CASES = [(2, 4, 64), (2, 2, 1024)]      # (B, g, D): four rows of 256 per sample; one row of 4096, the real width


def _shuffle_inputs(B, g, D):
    X = _bf((B, 1 + g * g, D), 7 * g + D, 3.0)
    X[:, 0] = float("nan")                      # the class row is never read
    w, b = (1 + 0.1 * torch.randn(4 * D, generator=torch.Generator().manual_seed(8))).bfloat16().to(DEV), _bf((4 * D,), 9, 0.1)
    return X, w, b


@pytest.mark.parametrize("v1", [False, True])
@pytest.mark.parametrize("B,g,D", SHUFFLE_CASES)
def test_shuffle_ln_vs_fp64(iops, B, g, D, v1):
    """every element within its float64-derived bound (tests/ew_ref.py's LayerNorm allowance, IR.shuffle_ln_expect), and the whole tensor
    within the 5e-3 of x2i_ln_affine_bf16's own test (tests/test_ops_gpu.py); rows and columns beyond the result untouched"""
    X, w, b = _shuffle_inputs(B, g, D)
    rows = B * (g // 2) ** 2
    buf = poisoned(rows + 1, 4 * D + 8)
    iops.shuffle_ln(X, w, b, 1e-5, buf, g, v1=v1)
    got = buf[:rows, :4 * D]
    assert bool(is_sentinel(buf[rows:]).all()) and bool(is_sentinel(buf[:, 4 * D:]).all()) and bool(torch.isfinite(got).all())
    want, bound = IR.shuffle_ln_expect(X, w, b, g, 1e-5, v1=v1)
    err = (got.double() - want).abs()
    worst = float((err / bound).max())
    print("internvit_shuffle_ln B=%d g=%d D=%d %s: worst |err| / bound %.3f, rel-L2 %.3e" % (B, g, D, "v1" if v1 else "v2", worst, IR.rel_l2(got, want)))
    assert bool((err <= bound).all()), "worst |err| / bound %.3f" % worst
    assert IR.rel_l2(got, want) < 5e-3
    other, _ = IR.shuffle_ln_expect(X, w, b, g, 1e-5, v1=not v1)
    assert g == 2 or IR.rel_l2(got, other) > 0.1      # (a 1 x 1 grid of cells has one order)


@pytest.mark.parametrize("v1", [False, True])
@pytest.mark.parametrize("B,g,D", SHUFFLE_CASES)
def test_shuffle_ln_is_gather_then_ln_affine(iops, B, g, D, v1):
    """bit-equal to a torch gather followed by x2i_ln_affine_bf16; also from an input with wider rows and samples further apart"""
    from x2i_amd import ops
    X, w, b = _shuffle_inputs(B, g, D)
    rows = B * (g // 2) ** 2
    gathered = IR.shuffle_gather(X[:, 1:], g, v1=v1).reshape(rows, 4 * D).contiguous()
    want = ops.ln_affine(gathered, w, b, 1e-5)
    got = torch.empty((rows, 4 * D), device=DEV, dtype=torch.bfloat16)
    iops.shuffle_ln(X, w, b, 1e-5, got, g, v1=v1)
    assert torch.equal(got, want)
    wide = poisoned(B, 3 + g * g, D + 16)
    wide[:, :1 + g * g, :D] = X
    again = torch.empty_like(got)
    iops.shuffle_ln(wide[:, :1 + g * g, :D], w, b, 1e-5, again, g, v1=v1)
    assert torch.equal(again, want)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(iops):
    """every validated argument, through the binding: nothing is launched (the outputs keep their sentinels)"""
    from x2i_amd._lib import X2IError
    img, out = torch.zeros((2, 3, 28, 42), dtype=torch.bfloat16, device=DEV), poisoned(12, 640)
    for bad in (dict(Kp=584), dict(Kp=636), dict(ldx=632), dict(P=33), dict(P=5), dict(img=img.float()), dict(img=img[:, :2]), dict(img=img[:, :, :, ::2]),
                dict(img=img.cpu()), dict(out=poisoned(11, 640)), dict(out=poisoned(12, 632))):
        kw = dict(img=img, out=out, P=14, Kp=640, ldx=None)
        kw.update(bad)
        with pytest.raises(X2IError):
            iops.patch_rows(kw["img"], kw["out"], kw["P"], kw["Kp"], ldx=kw["ldx"])
    assert bool(is_sentinel(out).all())
    X, cls, pos = poisoned(2, 7, 64), torch.zeros((64,), dtype=torch.bfloat16, device=DEV), torch.zeros((7, 64), dtype=torch.bfloat16, device=DEV)
    for bad in (dict(X=poisoned(2, 7, 72)[:, :, :64]), dict(X=poisoned(2, 7, 60)), dict(X=poisoned(7, 64)), dict(cls=cls[:56]), dict(cls=cls.float()),
                dict(pos=pos[:6]), dict(pos=pos.float()), dict(pos=torch.zeros((7, 72), dtype=torch.bfloat16, device=DEV)[:, :64]), dict(cls=cls.cpu())):
        kw = dict(X=X, cls=cls, pos=pos)
        kw.update(bad)
        with pytest.raises(X2IError):
            iops.embed(kw["X"], kw["cls"], kw["pos"])
    assert bool(is_sentinel(X).all())
    X, w, out = torch.zeros((2, 17, 64), dtype=torch.bfloat16, device=DEV), torch.zeros((256,), dtype=torch.bfloat16, device=DEV), poisoned(8, 256)
    for bad in (dict(g=3), dict(g=2), dict(X=X.float()), dict(X=X.transpose(1, 2)), dict(w=w[:248]), dict(w=w.float()), dict(out=poisoned(7, 256)),
                dict(out=poisoned(8, 248)), dict(ldy=252), dict(X=torch.zeros((2, 17, 60), dtype=torch.bfloat16, device=DEV), w=w[:240], out=poisoned(8, 240)),
                dict(X=torch.zeros((1, 5, 1032), dtype=torch.bfloat16, device=DEV), g=2, w=torch.zeros((4128,), dtype=torch.bfloat16, device=DEV),
                     out=poisoned(1, 4128))):
        kw = dict(X=X, w=w, out=out, g=4, ldy=None)
        kw.update(bad)
        with pytest.raises(X2IError):
            iops.shuffle_ln(kw["X"], kw["w"], kw["w"], 1e-5, kw["out"], kw["g"], ldy=kw["ldy"])
    assert bool(is_sentinel(out).all())


# ---------------------------------------------------------------------------------------------------------------- tower and tail
def _hip_vision(weights, cfg, llm, select_layer=-1, ps_version="v2", graph=False):
    from x2i_amd.internvit import InternVisionTower, InternVLVision
    vis = InternVLVision(InternVisionTower(device="cpu", **cfg), llm, select_layer=select_layer, ps_version=ps_version, graph=graph)
    vis.load_state_dict({k: v.bfloat16() for k, v in weights.items()}, strict=True)
    return vis.to(DEV)      # the Conv2d view follows its padded storage to the GPU, and the f32 LayerScale copies are made again there


FULL = dict(IR.TINY, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=2, image_size=448)
WIDE_RMS = dict(IR.TINY, hidden_size=256, num_attention_heads=2, norm_type="rms_norm", qk_normalization=True, qkv_bias=False)
# (configuration, H_llm, B, select_layer, ps_version): the fixture's configuration (S = 17, inside one key tile); two full-width layers on
# 32 x 32 patches (S = 1025: the 17th key tile holds one key, Spad = 1088); heads of 128 with RMS norms and q / k normalisation, under v1
# and select_layer -2.
# Measured on the MI355X, HIP / bf16 restatement against float64, test weights then activation probe (profiles/internvit_gputest.log):
#   tiny              5.00e-3 / 5.42e-3 (ratio 0.92),  probe 3.39e-3 / 1.52e-2 (0.22)
#   full width        4.99e-3 / 5.68e-3 (0.88),        probe 3.52e-3 / 1.51e-2 (0.23)
#   rms, heads of 128 4.44e-3 / 5.19e-3 (0.86),        probe 3.18e-3 / 1.41e-2 (0.23)
# (the criterion allows 1.5; on the probe weights the bf16 restatement's three roundings of `x + ls * branch` at ls = 2^15 x show, where
# the HIP path rounds once).  The tiny configuration at grid 6 x 6: 5.18e-3 / 5.70e-3 (0.91).
TOWER_CASES = [(IR.TINY, IR.TINY_LLM, 2, -1, "v2"), (FULL, 896, 2, -1, "v2"), (WIDE_RMS, 192, 2, -2, "v1")]


@pytest.mark.parametrize("cfg,llm,B,select_layer,ps_version", TOWER_CASES, ids=["tiny", "full_width", "rms_heads_of_128"])
def test_tower_and_tail_vs_fp64_and_bf16(cfg, llm, B, select_layer, ps_version):
    sd = IR.random_state_dict(cfg, llm, seed=cfg["hidden_size"] + B)
    x = IR.random_pixels(B, cfg["image_size"], seed=cfg["hidden_size"])
    g = cfg["image_size"] // cfg["patch_size"]
    seen = {}

    def run(weights, pixels):
        vis = _hip_vision(weights, cfg, llm, select_layer, ps_version)
        px = pixels.bfloat16().to(DEV)
        out = vis(px)
        assert out.dtype == torch.bfloat16 and out.shape == (B, (g // 2) ** 2, llm) and bool(torch.isfinite(out).all())
        # a second call with the same plan is bit-identical, and a planned forward only enqueues
        plan = vis.plan(B, g)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = vis(px, plan=plan)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(again, out)
        seen["vis"] = vis
        return out

    name = "InternVLVision hidden=%d heads=%d layers=%d grid %dx%d B=%d %s select_layer=%d %s" % (
        cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], g, g, B, cfg["norm_type"], select_layer, ps_version)
    IR.check_extract_feature(name, run, sd, x, cfg, device=DEV, select_layer=select_layer, ps_version=ps_version)
    # the tower alone is the model's vision_model: last_hidden_state with its class row, and hidden_states[select_layer]
    vis = seen["vis"]
    hs = vis.vision_model(pixel_values=x.bfloat16().to(DEV), select_layer=select_layer)
    assert hs.last_hidden_state.shape == (B, 1 + g * g, cfg["hidden_size"]) and torch.equal(hs.pooler_output, hs.last_hidden_state[:, 0])


def test_tower_at_another_grid_resamples_the_position_table():
    """84 x 84 pixels on the fixture's configuration: grid 6 x 6, 37 tokens, the position table resampled by the model's own call"""
    sd = IR.random_state_dict(IR.TINY, IR.TINY_LLM, seed=11)
    x = IR.random_pixels(2, 84, seed=12)
    vis = _hip_vision(sd, IR.TINY, IR.TINY_LLM)
    out = vis(x.bfloat16().to(DEV))
    ref = IR.extract_feature(sd, x.to(DEV), IR.TINY, torch.float64)
    lib = IR.extract_feature(sd, x.to(DEV), IR.TINY, torch.bfloat16)
    e_hip, e_lib = IR.rel_l2(out, ref), IR.rel_l2(lib, ref)
    print("InternVLVision tiny at grid 6x6: rel-L2 against float64: HIP %.3e, bf16 restatement %.3e (ratio %.2f)" % (e_hip, e_lib, e_hip / e_lib))
    assert out.shape == (2, 9, IR.TINY_LLM) and e_hip <= 1.5 * e_lib and e_hip < 3e-2


# ---------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_is_bit_identical_to_eager():
    """two different inputs through one captured plan: the first call of a shape runs eagerly, the second captures, the third replays; each
    equals the eager module's result bit for bit, and the results are copies (a later call does not change an earlier result)"""
    sd = IR.random_state_dict(IR.TINY, IR.TINY_LLM, seed=13)
    eager, graphed = _hip_vision(sd, IR.TINY, IR.TINY_LLM), _hip_vision(sd, IR.TINY, IR.TINY_LLM, graph=True)
    xs = [IR.random_pixels(2, 56, seed=s).bfloat16().to(DEV) for s in (14, 15, 16)]
    want = [eager(x) for x in xs]
    assert not torch.equal(want[0], want[1])
    got = [graphed(x) for x in xs]
    plan = graphed._plans[(2, 4)]
    assert plan.calls == 3 and plan.graph is not None and plan.sk_ws is not None
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(graphed(xs[0]), want[0]) and torch.equal(got[2], want[2]) and plan.calls == 4
    # another shape gets a plan and a graph of its own; graph=False on a call bypasses it
    assert torch.equal(graphed(xs[1][:1]), eager(xs[1][:1])) and set(graphed._plans) == {(2, 4), (1, 4)}
    assert torch.equal(graphed(xs[2], graph=False), want[2]) and plan.calls == 4
    from x2i_amd import ops
    ops.streamk_check()


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hip_internvision_replaces_and_restores():
    from x2i_amd.handoff import HipInternVision
    sd = IR.random_state_dict(IR.TINY, IR.TINY_LLM, seed=17)
    model = IR.StubChatModel(sd, device=DEV)
    x = IR.random_pixels(2, 56, seed=18).bfloat16().to(DEV)
    hv = HipInternVision(model)
    assert hv.vision.device.type == "cuda" and hv.vision.graph
    want = hv.vision(x, graph=False)
    with hv:
        assert "extract_feature" in model.__dict__
        got = [model.extract_feature(x) for _ in range(3)]      # eager, capture, replay
        assert hv.calls == 3 and model.own_calls == 0 and all(torch.equal(g_, want) for g_ in got)
    assert "extract_feature" not in model.__dict__
    # the model's own extract_feature is back, and the HIP result is the model's within the criterion's absolute bound
    theirs = model.extract_feature(x)
    assert model.own_calls == 1 and hv.calls == 3 and IR.rel_l2(want, theirs) < 3e-2
    with pytest.raises(KeyError):
        with hv:
            raise KeyError("inside")
    assert "extract_feature" not in model.__dict__
