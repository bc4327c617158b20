"""The MiniCPM-o SigLIP vision tower on the HIP path (include/x2i_siglip.h, x2i_amd/siglip.py, handoff.HipSiglip) on the GPU: the row kernels
bit for bit against torch, the attention in the regime the tower runs it in (heads of 72 zero-padded to 80, the scale of 72) against the
float64 checker of tests/qwen_vision_ref.py, and the tower and the hand-off against the library (Idefics2VisionTransformer) in float64
(and no worse than 1.5 x the library's own bf16 run on the same GPU)."""
import pytest
import torch

from tests import qwen_vision_ref as VR
from tests import siglip_ref as SR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def siglip_ops():
    from x2i_amd import siglip_ops as o
    o.load()
    return o


# ---------------------------------------------------------------------------------------------------------------- patch rows
@pytest.mark.parametrize("B,L,P", [(1, 1, 14), (2, 7, 14), (1, 130, 14)])
def test_patch_rows_is_the_torch_permutation(siglip_ops, B, L, P):
    """strips that are a window of a wider tensor (a row stride beyond P * L, a start that is only 2-byte aligned), an output wider than Kp
    and longer than B * L: the footprint is rows < B * L, columns < Kp, and the tail columns 3 P^2 .. Kp-1 are zero"""
    g = torch.Generator().manual_seed(100 * L + B)
    wide = torch.randn((B, 3, P, P * L + 10), generator=g).bfloat16().to(DEV)
    strips = wide[:, :, :, 3:3 + P * L]
    assert not strips.is_contiguous()
    want = strips.reshape(B, 3, P, L, P).permute(0, 3, 1, 2, 4).reshape(B * L, 3 * P * P)
    for Kp in (640, 592):
        buf = poisoned(B * L + 2, Kp + 16)
        siglip_ops.patch_rows(strips, buf, P, Kp)
        assert torch.equal(buf[:B * L, :3 * P * P], want)
        assert not bool(buf[:B * L, 3 * P * P:Kp].view(torch.int16).any())
        assert bool(is_sentinel(buf[B * L:]).all()) and bool(is_sentinel(buf[:, Kp:]).all())
    assert torch.equal(SR.patch_rows(strips, 640), torch.cat((want, want.new_zeros((B * L, 52))), 1))      # (the float64 tower's helper agrees)
    again = poisoned(B * L + 2, 592 + 16)
    siglip_ops.patch_rows(strips.contiguous(), again, P, 592)
    assert torch.equal(again, buf)              # the contiguous copy gives the same rows


def test_patch_rows_refusals(siglip_ops):
    from x2i_amd._lib import X2IError
    strips = torch.zeros((2, 3, 14, 14 * 7), dtype=torch.bfloat16, device=DEV)
    out = poisoned(14, 640)
    for bad in (dict(Kp=584), dict(Kp=636), dict(ldx=632), dict(P=7), dict(strips=strips.float()), dict(strips=strips.transpose(1, 2)),
                dict(strips=strips[:, :, :, ::2]), dict(out=poisoned(13, 640)), dict(out=poisoned(14, 632))):
        kw = dict(strips=strips, out=out, P=14, Kp=640, ldx=None)
        kw.update(bad)
        with pytest.raises(X2IError):
            siglip_ops.patch_rows(kw["strips"], kw["out"], kw["P"], kw["Kp"], ldx=kw["ldx"])
    assert bool(is_sentinel(out).all())         # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- position embedding
@pytest.mark.parametrize("rows,D", [(1, 8), (77, 144), (1024, 1152)])
def test_add_positions_is_the_torch_bf16_add(siglip_ops, rows, D):
    """bit-identical to torch's bf16 `x + table[ids]`; ids outside the table are clamped into it; a wider row stride; a relaunch on a fresh
    copy gives the same bits"""
    g = torch.Generator().manual_seed(rows + D)
    n_pos = 4900 if rows > 100 else 50
    x = torch.randn((rows, D), generator=g).bfloat16().to(DEV)
    pos = (0.5 * torch.randn((n_pos, D), generator=g)).bfloat16().to(DEV)
    ids = torch.randint(0, n_pos, (rows,), generator=g).to(torch.int32)
    ids[0] = n_pos - 1
    if rows > 3:
        ids[1], ids[2], ids[3] = -5, n_pos, n_pos + 1000
    ids = ids.to(DEV)
    want = x + pos[ids.long().clamp(0, n_pos - 1)]
    assert want.dtype == torch.bfloat16
    out = []
    for _ in range(2):
        buf = poisoned(rows + 1, D + 8)
        buf[:rows, :D] = x
        siglip_ops.add_positions(buf, ids, pos, rows=rows)
        assert bool(is_sentinel(buf[rows:]).all()) and bool(is_sentinel(buf[:, D:]).all())
        out.append(buf[:rows, :D].clone())
    assert torch.equal(out[0], want) and torch.equal(out[1], out[0])
    tight = x.clone()
    siglip_ops.add_positions(tight, ids, pos)
    assert torch.equal(tight, want)


def test_add_positions_refusals(siglip_ops):
    from x2i_amd._lib import X2IError
    x, pos = poisoned(6, 16), torch.zeros((5, 16), dtype=torch.bfloat16, device=DEV)
    ids = torch.zeros((6,), dtype=torch.int32, device=DEV)
    for bad in (dict(ids=ids.long()), dict(ids=ids[:5]), dict(pos=pos.float()), dict(pos=pos[:, :12]), dict(pos=torch.zeros((5, 24), dtype=torch.bfloat16, device=DEV)),
                dict(ldx=12), dict(ldx=20)):
        kw = dict(ids=ids, pos=pos, ldx=None)
        kw.update(bad)
        with pytest.raises(X2IError):
            siglip_ops.add_positions(x, kw["ids"], kw["pos"], ldx=kw["ldx"])
    assert bool(is_sentinel(x).all())


# ---------------------------------------------------------------------------------------------------------------- head split
@pytest.mark.parametrize("S", [1, 77, 130])
@pytest.mark.parametrize("dk", [64, 80, 128])
def test_head_split_is_the_torch_permutation(siglip_ops, dk, S):
    """Q, K, VT bit-equal to the torch reshape at the stored width (heads of 80 in rows of 128); the padding (d >= dk, s >= S) untouched; the
    row stride honoured"""
    B, H = (2, 3) if S == 77 else (1, 2)
    g = torch.Generator().manual_seed(S * 100 + dk)
    W, Spad, dkp = 3 * H * dk, siglip_ops.pad64(S), siglip_ops.stored_width(dk)
    qkv = torch.zeros((B * S, W + 16), dtype=torch.bfloat16, device=DEV)
    qkv[:, :W] = torch.randn((B * S, W), generator=g).bfloat16().to(DEV)
    Q, K, VT = poisoned(B, H, Spad, dkp), poisoned(B, H, Spad, dkp), poisoned(B, H, dkp, Spad)
    siglip_ops.head_split(qkv, Q, K, VT, B, S, Spad, H, dk)
    q, k, v = qkv[:, :W].view(B, S, 3, H, dk).unbind(2)
    assert torch.equal(Q[:, :, :S, :dk], q.transpose(1, 2)) and torch.equal(K[:, :, :S, :dk], k.transpose(1, 2))
    assert torch.equal(VT[:, :, :dk, :S], v.permute(0, 2, 3, 1))
    for t in (Q[:, :, S:], Q[..., dk:], K[:, :, S:], K[..., dk:], VT[:, :, dk:], VT[..., S:]):
        assert bool(is_sentinel(t).all())


def test_head_split_refusals(siglip_ops):
    from x2i_amd._lib import X2IError
    qkv = torch.zeros((6, 3 * 2 * 80), dtype=torch.bfloat16, device=DEV)
    Q, K, VT = poisoned(1, 2, 64, 128), poisoned(1, 2, 64, 128), poisoned(1, 2, 128, 64)
    for bad in (dict(dk=72), dict(dk=96), dict(Spad=4), dict(ld=100), dict(ld=484), dict(H=3)):
        kw = dict(dk=80, Spad=64, ld=None, H=2)
        kw.update(bad)
        with pytest.raises(X2IError):
            siglip_ops.head_split(qkv, Q, K, VT, 1, 6, kw["Spad"], kw["H"], kw["dk"], ld=kw["ld"])
    assert all(bool(is_sentinel(t).all()) for t in (Q, K, VT))


# ---------------------------------------------------------------------------------------------------------------- attention, padded regime
# (B, H, S, the key count n_b of every sample): the regime SiglipVisionTower runs x2i_vit_attention_bf16 in.  Heads of 72 padded to dk = 80
# and stored 128 wide: columns 72..79 of Q, K and V are zero, NaN sits in 80..127, the scale is 72 ** -0.5 and EVERY row of sample b, its
# padding rows included, has the keys [0, n_b).  Worst tile measured on the MI355X, in this order: 1.70e-3, 2.42e-3, 2.08e-3, 2.21e-3
# (bound TOL_O = 5e-3; profiles/siglip_gputest.log)
PADDED_CASES = [(1, 1, 4, [4]), (1, 2, 130, [130]), (2, 2, 100, [100, 37]), (1, 1, 300, [300])]


@pytest.mark.parametrize("B,H,S,counts", PADDED_CASES)
def test_attention_in_the_padded_regime_vs_fp64_per_tile(B, H, S, counts):
    from x2i_amd import vit_ops
    Spad = vit_ops.pad64(S)
    g = torch.Generator().manual_seed(1000 * S + H)
    Q, K, V = (torch.full((B, H, Spad, 128), NAN) for _ in range(3))
    for t, amp in ((Q, 1.5), (K, 1.5), (V, 1.0)):
        t[..., :80] = 0.0
        t[:, :, :S, :72] = amp * torch.randn((B, H, S, 72), generator=g)
    Q, K, V = (t.bfloat16().to(DEV) for t in (Q, K, V))
    lo = torch.zeros((B, S), dtype=torch.int32, device=DEV)
    hi = torch.tensor(counts, dtype=torch.int32)[:, None].expand(B, S).contiguous().to(DEV)
    buf = poisoned(B, S, H * 80)
    vit_ops.attention(Q, K, V.transpose(-1, -2).contiguous(), buf, B, H, S, Spad, 80, 72 ** -0.5, H * 80, S * H * 80, lo, hi)
    O = buf.reshape(B, S, H, 80).permute(0, 2, 1, 3)
    ref = VR.attention_reference(Q, K, V, S, 72, 72 ** -0.5, lo.tolist(), hi.tolist())
    name = "vit_attention, heads of 72 padded to 80: B=%d H=%d S=%d keys %s" % (B, H, S, counts)
    worst = VR.check_attention(name, O[..., :72], ref, VR.TOL_O)
    print("%s: worst tile rel-L2 %.3e (bound %.1e)" % (name, worst, VR.TOL_O))
    assert not bool(is_sentinel(buf).any()) and not bool(O[..., 72:].view(torch.int16).any())      # the padding columns come out exactly 0
    # the scale is the real width's: the reference at 80 ** -0.5 is another result
    if S >= 100:
        assert VR.rel_l2(VR.attention_reference(Q, K, V, S, 72, 80 ** -0.5, lo.tolist(), hi.tolist()), ref) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- tower
# (hidden, heads, intermediate, layers; grids): a tiny tower on one image; a padded batch of three images whose key ranges differ, where
# L = 81 crosses a 64-key tile; one full-width layer (1152 hidden, 16 heads of 72, 4304 intermediate) on 32 x 32 and 20 x 27 patches.
# Measured on the MI355X, HIP / library bf16 against float64: 5.23e-3 / 6.27e-3, 4.83e-3 / 5.83e-3, 3.94e-3 / 6.96e-3 (ratio 0.83, 0.83, 0.57;
# the criterion allows 1.5; profiles/siglip_gputest.log)
TOWER_CASES = [(144, 2, 300, 2, [(4, 6)]), (288, 4, 600, 2, [(3, 5), (9, 9), (1, 1)]), (1152, 16, 4304, 1, [(32, 32), (20, 27)])]


@pytest.mark.parametrize("hidden,heads,inter,layers,grids", TOWER_CASES)
def test_tower_vs_library_fp64_and_bf16(hidden, heads, inter, layers, grids):
    from x2i_amd.siglip import SiglipVisionTower
    cfg, lib = SR.library_tower(hidden, heads, inter, layers)
    sd = SR.random_state_dict(lib, seed=hidden + len(grids))
    lib.load_state_dict(sd, strict=True)
    hip = SiglipVisionTower(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)       # the views follow their padded storage to the GPU, and the head-padded copies are made again there
    assert hip.encoder.layers[0].mlp.fc1.weight.data_ptr() == hip._fused["0.fc1.w"].data_ptr() and hip._packed[0][0].device.type == "cuda"
    counts = [h * w for h, w in grids]
    B, L = len(grids), max(counts)
    strips, images = SR.random_strips(grids, L, seed=hidden)
    x = strips.bfloat16().to(DEV)
    sizes = torch.tensor(grids, dtype=torch.int32, device=DEV)
    mask = (torch.arange(L)[None, :] < torch.tensor(counts)[:, None])[:, None, :].to(DEV)
    out = hip(x, patch_attention_mask=mask, tgt_sizes=sizes)
    assert out.pooler_output is None and out.last_hidden_state.shape == (B, L, hidden) and out.last_hidden_state.dtype == torch.bfloat16
    first = out.last_hidden_state.clone()
    assert bool(torch.isfinite(first).all())
    # a second call with the same plan is bit-identical, and a planned forward only enqueues
    plan = hip.plan(grids, L)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = hip(x, plan=plan).last_hidden_state
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, first)
    # a sample's valid rows are bit-identical whether it runs alone or inside the padded batch
    if B > 1:
        for b, n in enumerate(counts):
            alone = hip(x[b:b + 1, :, :, :14 * n], patch_attention_mask=mask[b:b + 1, :, :n], tgt_sizes=sizes[b:b + 1]).last_hidden_state
            assert alone.shape == (1, n, hidden) and torch.equal(alone[0], first[b, :n]), "sample %d of %s" % (b, grids)
    # the library sees one 2-D image at a time, folded back from its strip; valid rows only
    folded = [SR.strip_to_image(strips[b], h, w) for b, (h, w) in enumerate(grids)]
    assert all(torch.equal(a, b) for a, b in zip(folded, images))
    images = folded
    ref =torch.cat(SR.library_forward(lib.double(), [im.double() for im in images]))
    lib16 = torch.cat(SR.library_forward(lib.to(device=DEV, dtype=torch.bfloat16), images))
    mine = torch.cat([first[b, :n] for b, n in enumerate(counts)])
    e_hip, e_lib = SR.rel_l2(mine, ref), SR.rel_l2(lib16, ref)
    print("SiglipVisionTower hidden=%d heads=%d inter=%d layers=%d grids %s: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e "
          "(ratio %.2f)" % (hidden, heads, inter, layers, grids, e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)


def test_tower_without_tgt_sizes_takes_the_masks_fallback():
    """the reference's fallback reads h = 1, w = the mask's count off a [1, L] mask: one row of patches"""
    from x2i_amd.siglip import SiglipVisionTower
    hip = SiglipVisionTower(hidden_size=144, num_attention_heads=2, intermediate_size=300, num_hidden_layers=1, device=DEV).init_random_(3)
    strips, _ = SR.random_strips([(1, 9), (1, 4)], 9, seed=4)
    x = strips.bfloat16().to(DEV)
    mask = (torch.arange(9)[None, :] < torch.tensor([9, 4])[:, None])[:, None, :].to(DEV)
    want = hip(x, patch_attention_mask=mask, tgt_sizes=torch.tensor([(1, 9), (1, 4)])).last_hidden_state
    assert torch.equal(hip(x, patch_attention_mask=mask).last_hidden_state, want)
    assert torch.equal(hip(x[:1]).last_hidden_state[0], want[0])
    assert not torch.equal(hip(x, tgt_sizes=torch.tensor([(3, 3), (2, 2)])).last_hidden_state[:, :4], want[:, :4])
    with pytest.raises(ValueError, match="plan is for"):
        hip(x[:1], plan=hip.plan([(1, 9), (1, 4)], 9))


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hip_siglip_replaces_the_forward_and_restores_it():
    from x2i_amd.handoff import HipSiglip, find_vpm
    cfg, lib = SR.library_tower(144, 2, 300, 2)
    lib.load_state_dict(SR.random_state_dict(lib, seed=21), strict=True)
    model = torch.nn.Module()
    model.vpm = lib.to(device=DEV, dtype=torch.bfloat16)
    vpm = find_vpm(model)
    grids = [(3, 5), (2, 2)]
    strips, images = SR.random_strips(grids, 15, seed=22)
    x, t = strips.bfloat16().to(DEV), torch.tensor(grids, dtype=torch.int32, device=DEV)
    m = (torch.arange(15)[None, :] < torch.tensor([15, 4])[:, None])[:, None, :].to(DEV)
    hs = HipSiglip(model)
    want = hs.tower(x, patch_attention_mask=m, tgt_sizes=t).last_hidden_state.clone()
    with hs:
        assert "forward" in vpm.__dict__
        got = model.vpm(x, patch_attention_mask=m, tgt_sizes=t).last_hidden_state
        assert torch.equal(got, want) and hs.calls == 1
        model.vpm(x, patch_attention_mask=m, tgt_sizes=t)
    assert hs.calls == 2 and "forward" not in vpm.__dict__
    # the library's own forward is back, and the HIP rows are the library's within the stack criterion's absolute bound
    theirs = SR.library_forward(model.vpm, images)
    assert hs.calls == 2 and SR.rel_l2(want[0], theirs[0]) < 3e-2 and SR.rel_l2(want[1, :4], theirs[1]) < 3e-2
    hs.install()
    hs.remove()
    assert "forward" not in vpm.__dict__
    with pytest.raises(KeyError):
        with hs:
            raise KeyError("inside")
    assert "forward" not in vpm.__dict__
