"""The MiniCPM-o Resampler on the HIP path (include/x2i_resampler.h, x2i_amd/resampler.py, handoff.HipResampler) on the GPU: the
learned-query attention against the float64 checker of tests/resampler_ref.py per (sample, head) tile, ln_pos and kv_split bit for bit
against existing entry points and torch, every refusal, and the module and the hand-off against float64 (and no worse than 1.5 x a bf16
module composed from torch.nn's own parts on the same GPU)."""
import pytest
import torch

from tests import resampler_ref as RR
from tests import siglip_ref as SR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SCALE = 128 ** -0.5


@pytest.fixture(scope="module")
def rops():
    from x2i_amd import resampler_ops as o
    o.load()
    return o


# ---------------------------------------------------------------------------------------------------------------- attention
# (B, H, NQ, L, Lpad, n_keys): one tile; a ragged tile and a single key; NQ off the wave size, and an empty sample; the model's 32 x 32 and
# 20 x 27 grids; a quarter split without counts; counts outside [0, L], which the kernel clamps.
# Worst tile measured on the MI355X, in this order: 1.80e-3, 2.01e-3, 2.29e-3, 2.51e-3, 1.79e-3, 1.83e-3 (bound TOL_O = 5e-3;
# profiles/resampler_gputest.log)
ATTENTION_CASES = [(1, 1, 64, 64, 64, [64]), (2, 2, 64, 200, 256, [200, 1]), (3, 2, 33, 320, 320, [320, 65, 0]),
                   (2, 4, 64, 1024, 1024, [1024, 540]), (1, 2, 8, 130, 192, None), (2, 1, 64, 100, 128, [107, -3])]


def attention_inputs(B, H, NQ, L, Lpad, counts, seed, noise_seed):
    """Q [H, NQpad, 128] with NaN in the rows >= NQ; K, V [B, H, Lpad, 128] with large finite noise at and beyond each sample's (clamped)
    key count, drawn from noise_seed alone"""
    g, gn = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(noise_seed)
    NQpad = (NQ + 31) // 32 * 32
    Q = torch.full((H, NQpad, 128), NAN)
    Q[:, :NQ] = 1.5 * torch.randn((H, NQ, 128), generator=g)
    K, V = 1.5 * torch.randn((B, H, Lpad, 128), generator=g), torch.randn((B, H, Lpad, 128), generator=g)
    nK, nV = 100.0 * torch.randn((B, H, Lpad, 128), generator=gn), 100.0 * torch.randn((B, H, Lpad, 128), generator=gn)
    for b in range(B):
        n = L if counts is None else min(max(counts[b], 0), L)
        K[b, :, n:], V[b, :, n:] = nK[b, :, n:], nV[b, :, n:]
    return Q.bfloat16().to(DEV), K.bfloat16().to(DEV), V.bfloat16().to(DEV)


def run_attention(rops, Q, K, V, counts, B, H, NQ, L, Lpad):
    """-> the whole sentinel-filled output buffer [B, NQ + 2, 128 H + 16]"""
    ldo = H * 128 + 16
    buf = poisoned(B, NQ + 2, ldo)
    n = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    rops.attention(Q, K, V.transpose(-1, -2).contiguous(), buf, B, H, NQ, L, Lpad, SCALE, ldo, (NQ + 2) * ldo, n)
    return buf


@pytest.mark.parametrize("B,H,NQ,L,Lpad,counts", ATTENTION_CASES)
def test_attention_vs_fp64_per_tile(rops, B, H, NQ, L, Lpad, counts):
    seed = 1000 * L + 10 * NQ + H
    Q, K, V = attention_inputs(B, H, NQ, L, Lpad, counts, seed, noise_seed=1)
    buf = run_attention(rops, Q, K, V, counts, B, H, NQ, L, Lpad)
    # the footprint: rows < NQ and columns < 128 H, all of them
    assert bool(is_sentinel(buf[:, NQ:]).all()) and bool(is_sentinel(buf[:, :, H * 128:]).all())
    assert not bool(is_sentinel(buf[:, :NQ, :H * 128]).any())
    O = RR.heads_of(buf[:, :NQ], H)
    assert bool(torch.isfinite(O).all())
    ref = RR.attention_reference(Q, K, V, counts, SCALE, NQ=NQ, L=L)
    name = "resampler_attention B=%d H=%d NQ=%d L=%d Lpad=%d n_keys %s" % (B, H, NQ, L, Lpad, counts)
    worst = RR.check_attention(name, O, ref, RR.TOL_O)
    print("%s: worst tile rel-L2 %.3e (bound %.1e)" % (name, worst, RR.TOL_O))
    # an empty sample's rows are exactly 0, and written
    for b in range(B):
        if counts is not None and min(max(counts[b], 0), L) == 0:
            assert not bool(buf[b, :NQ, :H * 128].view(torch.int16).any())
    # the mask is by index: other noise beyond the counts, the same bits
    Q2, K2, V2 = attention_inputs(B, H, NQ, L, Lpad, counts, seed, noise_seed=2)
    full = counts is None and Lpad == L or counts is not None and all(c >= Lpad for c in counts)
    assert torch.equal(Q2.view(torch.int16), Q.view(torch.int16)) and (full or not torch.equal(K2, K))
    assert torch.equal(run_attention(rops, Q2, K2, V2, counts, B, H, NQ, L, Lpad), buf)
    # a second launch gives the same bits
    assert torch.equal(run_attention(rops, Q, K, V, counts, B, H, NQ, L, Lpad), buf)
    # a sample launched alone equals its rows in the batch
    if B > 1:
        for b in range(B):
            alone = run_attention(rops, Q, K[b:b + 1].contiguous(), V[b:b + 1].contiguous(), None if counts is None else counts[b:b + 1], 1, H, NQ, L, Lpad)
            assert torch.equal(alone[0], buf[b]), "sample %d of %s" % (b, name)


def test_attention_refusals(rops):
    from x2i_amd._lib import X2IError
    B, H, NQ, L, Lpad = 1, 2, 64, 100, 128
    Q, K, V = attention_inputs(B, H, NQ, L, Lpad, None, 3, 4)
    VT = V.transpose(-1, -2).contiguous()
    big = torch.zeros(Q.numel() + 8, dtype=torch.bfloat16, device=DEV)
    n = torch.tensor([100], dtype=torch.int32, device=DEV)
    out = poisoned(B, NQ, 256)
    base = dict(Q=Q, K=K, VT=VT, out=out, NQ=NQ, L=L, Lpad=Lpad, scale=SCALE, ldo=256, obs=NQ * 256, n=n)
    for bad in (dict(Q=big[4:]), dict(K=torch.zeros(K.numel() + 8, dtype=torch.bfloat16, device=DEV)[4:]), dict(Lpad=96), dict(Lpad=120), dict(NQ=0), dict(NQ=65),
                dict(scale=0.0), dict(scale=-SCALE), dict(scale=float("inf")), dict(scale=NAN), dict(ldo=248), dict(ldo=252), dict(obs=NQ * 256 + 4),
                dict(Q=Q.float()), dict(VT=VT.float()), dict(n=n.long()), dict(L=0), dict(L=129)):
        kw = dict(base)
        kw.update(bad)
        with pytest.raises(X2IError):
            rops.attention(kw["Q"], kw["K"], kw["VT"], kw["out"], B, H, kw["NQ"], kw["L"], kw["Lpad"], kw["scale"], kw["ldo"], kw["obs"], kw["n"])
    with pytest.raises(X2IError):
        rops.attention(Q, K, VT, out.float(), B, H, NQ, L, Lpad, SCALE, 256, NQ * 256, n)
    torch.cuda.synchronize()
    assert bool(is_sentinel(out).all())         # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- ln_pos
@pytest.mark.parametrize("rows,D", [(1, 8), (77, 256), (1024, 3584)])
def test_ln_pos_is_ln_affine_then_add_positions(rops, rows, D):
    """XV bit-equal to ops.ln_affine, XK bit-equal to siglip_ops.add_positions on a copy of XV; rows with id -1 have XK == XV; ids beyond
    the table are clamped; wider row strides; the footprint"""
    from x2i_amd import ops, siglip_ops
    g = torch.Generator().manual_seed(rows + D)
    n_pos = 4900 if rows > 100 else 50
    x = (2.0 * torch.randn((rows, D), generator=g) + 0.5).bfloat16().to(DEV)
    w, b = (1.0 + 0.1 * torch.randn(D, generator=g)).bfloat16().to(DEV), (0.1 * torch.randn(D, generator=g)).bfloat16().to(DEV)
    pos = torch.randn((n_pos, D), generator=g).bfloat16().to(DEV)
    ids = torch.randint(0, n_pos, (rows,), generator=g).to(torch.int32)
    ids[0] = n_pos - 1
    if rows > 5:
        ids[1], ids[2], ids[3], ids[4], ids[5] = -1, n_pos, n_pos + 1000, -7, 0
    ids = ids.to(DEV)
    want_v = ops.ln_affine(x, w, b, 1e-6)
    want_k = siglip_ops.add_positions(want_v.clone(), ids.clamp_min(0), pos)
    want_k[ids < 0] = want_v[ids < 0]
    xw = torch.zeros((rows, D + 8), dtype=torch.bfloat16, device=DEV)
    xw[:, :D] = x
    XV, XK = poisoned(rows + 1, D + 16), poisoned(rows + 1, D + 8)
    rops.ln_pos(xw, w, b, 1e-6, ids, pos, XV, XK, rows=rows)
    assert torch.equal(XV[:rows, :D], want_v) and torch.equal(XK[:rows, :D], want_k)
    if rows > 5:
        assert torch.equal(XK[1, :D], XV[1, :D]) and torch.equal(XK[4, :D], XV[4, :D]) and not torch.equal(XK[5, :D], XV[5, :D])
    for t in (XV, XK):
        assert bool(is_sentinel(t[rows:]).all()) and bool(is_sentinel(t[:, D:]).all())
    assert torch.equal(xw[:, :D], x)
    tv, tk = torch.empty_like(x), torch.empty_like(x)       # tight rows, a relaunch
    rops.ln_pos(x, w, b, 1e-6, ids, pos, tv, tk)
    assert torch.equal(tv, want_v) and torch.equal(tk, want_k)


def test_ln_pos_refusals(rops):
    from x2i_amd._lib import X2IError
    rows, D = 6, 16
    x = torch.zeros((rows, D), dtype=torch.bfloat16, device=DEV)
    w = torch.ones(D, dtype=torch.bfloat16, device=DEV)
    pos, ids = torch.zeros((5, D), dtype=torch.bfloat16, device=DEV), torch.zeros(rows, dtype=torch.int32, device=DEV)
    XV, XK = poisoned(rows, D), poisoned(rows, D)
    off = torch.zeros(rows * D + 8, dtype=torch.bfloat16, device=DEV)[4:4 + rows * D].view(rows, D)
    base = dict(X=x, w=w, b=w, ids=ids, pos=pos, XV=XV, XK=XK, ldx=None, ldv=None, ldk=None)
    for bad in (dict(X=off), dict(ldx=12), dict(ldx=20), dict(ldv=12), dict(ldk=20), dict(ids=ids.long()), dict(ids=ids[:5]), dict(pos=pos.float()), dict(pos=pos[:, :12]),
                dict(pos=torch.zeros((5, 12), dtype=torch.bfloat16, device=DEV)), dict(w=w[:8]), dict(w=w.float()), dict(X=x.float()), dict(XK=XV)):
        kw = dict(base)
        kw.update(bad)
        with pytest.raises(X2IError):
            rops.ln_pos(kw["X"], kw["w"], kw["b"], 1e-6, kw["ids"], kw["pos"], kw["XV"], kw["XK"], ldx=kw["ldx"], ldv=kw["ldv"], ldk=kw["ldk"])
    both = poisoned(rows, D)
    with pytest.raises(X2IError, match="alias"):
        rops.ln_pos(both, w, w, 1e-6, ids, pos, both, XK)       # X may not be an output
    torch.cuda.synchronize()
    assert all(bool(is_sentinel(t).all()) for t in (XV, XK, both))


# ---------------------------------------------------------------------------------------------------------------- kv_split
@pytest.mark.parametrize("L", [1, 81, 1024])
def test_kv_split_is_the_torch_permutation(rops, L):
    """K, VT bit-equal to the torch reshape from two column ranges of one buffer; Lpad > L and what lies at s >= L untouched"""
    B, H = (2, 3) if L == 81 else (1, 2)
    g = torch.Generator().manual_seed(L)
    W, Lpad = H * 128, rops.pad64(L) + 64
    kv = torch.randn((B * L, 2 * W + 16), generator=g).bfloat16().to(DEV)
    K, VT = poisoned(B, H, Lpad, 128), poisoned(B, H, 128, Lpad)
    rops.kv_split(kv[:, :W], kv[:, W:2 * W], K, VT, B, L, Lpad, H)
    k, v = kv[:, :W].view(B, L, H, 128), kv[:, W:2 * W].view(B, L, H, 128)
    assert torch.equal(K[:, :, :L], k.transpose(1, 2)) and torch.equal(VT[..., :L], v.permute(0, 2, 3, 1))
    assert bool(is_sentinel(K[:, :, L:]).all()) and bool(is_sentinel(VT[..., L:]).all())
    # two separate buffers give the same
    K2, VT2 = poisoned(B, H, Lpad, 128), poisoned(B, H, 128, Lpad)
    rops.kv_split(kv[:, :W].contiguous(), kv[:, W:2 * W].contiguous(), K2, VT2, B, L, Lpad, H)
    assert torch.equal(K2, K) and torch.equal(VT2, VT)


def test_kv_split_refusals(rops):
    from x2i_amd._lib import X2IError
    B, L, Lpad, H = 1, 6, 64, 2
    kr = torch.zeros((B * L, 256), dtype=torch.bfloat16, device=DEV)
    off = torch.zeros(B * L * 256 + 8, dtype=torch.bfloat16, device=DEV)[4:4 + B * L * 256].view(B * L, 256)
    K, VT = poisoned(B, H, Lpad, 128), poisoned(B, H, 128, Lpad)
    base = dict(Kr=kr, Vr=kr, Lpad=Lpad, H=H, ldk=None, ldv=None, L=L)
    for bad in (dict(Kr=off), dict(Vr=off), dict(Lpad=4), dict(Lpad=60), dict(ldk=248), dict(ldv=260), dict(H=3), dict(Kr=kr.float()), dict(Vr=kr.float()), dict(L=0)):
        kw = dict(base)
        kw.update(bad)
        with pytest.raises(X2IError):
            rops.kv_split(kw["Kr"], kw["Vr"], K, VT, B, kw["L"], kw["Lpad"], kw["H"], ldk=kw["ldk"], ldv=kw["ldv"])
    with pytest.raises(X2IError):
        rops.kv_split(kr, kr, K.float(), VT, B, L, Lpad, H)
    torch.cuda.synchronize()
    assert bool(is_sentinel(K).all()) and bool(is_sentinel(VT).all())


# ---------------------------------------------------------------------------------------------------------------- module
def hip_module(sd, NQ, D, kv):
    from x2i_amd.resampler import Resampler
    hip = Resampler(num_queries=NQ, embed_dim=D, kv_dim=kv, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    return hip.to(DEV)


# (embed, kv_dim, queries; grids): the fixture's configuration on one frame; a padded batch of three frames whose key counts differ, where
# L = 81 crosses a 64-key tile and 40 queries take the two-row-group form; full width (3584, 28 heads, 1152, 64 queries) on 32 x 32 and
# 20 x 27 patches.  Measured on the MI355X, HIP / torch.nn bf16 against float64: 5.07e-3 / 5.32e-3, 4.51e-3 / 5.34e-3, 3.81e-3 / 4.95e-3 (ratio
# 0.95, 0.84, 0.77; the criterion allows 1.5; profiles/resampler_gputest.log)
MODULE_CASES = [(256, 64, 8, [(3, 5)]), (256, 128, 40, [(15, 1), (9, 9), (1, 1)]), (3584, 1152, 64, [(32, 32), (20, 27)])]


@pytest.mark.parametrize("D,kv,NQ,grids", MODULE_CASES)
def test_module_vs_fp64_and_torch_bf16(D, kv, NQ, grids):
    H = D // 128
    sd = RR.random_state_dict(NQ, D, kv, seed=D + kv)
    hip = hip_module(sd, NQ, D, kv)
    assert hip._pos.device.type == "cuda" and hip._projT.device.type == "cuda" and hip._Q is None
    B, L = len(grids), max(h * w for h, w in grids)
    x32 = RR.random_input(grids, L, kv, seed=D)
    x = x32.bfloat16().to(DEV)
    sizes = torch.tensor(grids, dtype=torch.int32, device=DEV)
    first = hip(x, sizes).clone()
    assert first.shape == (B, NQ, D) and first.dtype == torch.bfloat16 and bool(torch.isfinite(first).all())
    assert hip._Q.shape == (H, (NQ + 31) // 32 * 32, 128)
    # the padding rows of x reach nothing: other (finite) garbage there, the same bits
    y = RR.random_input(grids, L, kv, seed=D, garbage=7.0).bfloat16().to(DEV)
    assert all(torch.equal(y[b, :h * w], x[b, :h * w]) for b, (h, w) in enumerate(grids)) and (not torch.equal(y, x) or all(h * w == L for h, w in grids))
    assert torch.equal(hip(y, sizes), first)
    # a planned forward only enqueues, and gives the same bits
    plan = hip.plan(grids, L)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = hip(x, plan=plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, first)
    ref = RR.module_reference(sd, x32, grids, num_heads=H)
    lib = RR.LibraryResampler(NQ, D, H, kv)
    lib.load_state_dict(sd, strict=True)
    lib16 = lib.to(device=DEV, dtype=torch.bfloat16)(x, grids)
    e_hip, e_lib = RR.rel_l2(first, ref), RR.rel_l2(lib16, ref)
    print("Resampler embed=%d kv_dim=%d queries=%d grids %s: rel-L2 against float64: HIP %.3e, torch.nn bf16 on the GPU %.3e (ratio %.2f)"
          % (D, kv, NQ, grids, e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)


def test_module_chunks_of_16_equal_the_frames_one_at_a_time():
    """17 frames of one size cross the 16-frame chunk: every frame's rows are those of the frame run alone, bit for bit"""
    NQ, D, kv, grid = 8, 256, 64, (2, 3)
    hip = hip_module(RR.random_state_dict(NQ, D, kv, seed=17), NQ, D, kv)
    grids = [grid] * 17
    x = RR.random_input(grids, 6, kv, seed=18).bfloat16().to(DEV)
    out = hip(x, torch.tensor(grids)).clone()
    assert out.shape == (17, NQ, D) and not torch.equal(out[0], out[16])
    for b in range(17):
        assert torch.equal(hip(x[b:b + 1], torch.tensor([grid]))[0], out[b]), "frame %d" % b
    assert torch.equal(hip(x, torch.tensor(grids)), out)


def test_module_refuses_a_grid_beyond_the_table():
    hip = hip_module(RR.random_state_dict(8, 256, 64, seed=19), 8, 256, 64)
    with pytest.raises(ValueError, match="position table"):
        hip.plan([(71, 1)], 71)
    with pytest.raises(ValueError, match="position table"):
        hip(torch.zeros((1, 71, 64), dtype=torch.bfloat16, device=DEV), torch.tensor([(71, 1)]))
    with pytest.raises(ValueError, match="plan is for"):
        hip(torch.zeros((1, 15, 64), dtype=torch.bfloat16, device=DEV), plan=hip.plan([(3, 5), (2, 2)], 15))


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hip_resampler_replaces_the_forward_restores_it_and_composes_with_hip_siglip():
    from x2i_amd.handoff import HipResampler, HipSiglip, find_resampler
    cfg, tower = SR.library_tower(128, 2, 300, 2)
    tower.load_state_dict(SR.random_state_dict(tower, seed=31), strict=True)
    model = torch.nn.Module()
    model.vpm = tower.to(device=DEV, dtype=torch.bfloat16)
    res = RR.LibraryResampler(8, 256, 2, 128)
    res.load_state_dict(RR.random_state_dict(8, 256, 128, seed=32), strict=True)
    model.resampler = res.to(device=DEV, dtype=torch.bfloat16)
    assert find_resampler(model) is model.resampler
    grids = [(3, 5), (2, 2)]
    strips, _ = SR.random_strips(grids, 15, seed=33)
    px, t = strips.bfloat16().to(DEV), torch.tensor(grids, dtype=torch.int32, device=DEV)
    m = (torch.arange(15)[None, :] < torch.tensor([15, 4])[:, None])[:, None, :].to(DEV)
    hs, hr = HipSiglip(model), HipResampler(model)
    feats = hs.tower(px, patch_attention_mask=m, tgt_sizes=t).last_hidden_state
    want = hr.resampler(feats, t).clone()
    assert want.shape == (2, 8, 256)
    with hs, hr:
        assert "forward" in model.resampler.__dict__ and "forward" in model.vpm.__dict__
        got = model.resampler(model.vpm(px, patch_attention_mask=m, tgt_sizes=t).last_hidden_state, t)
        assert torch.equal(got, want) and hr.calls == 1 and hs.calls == 1
        model.resampler(feats, tgt_sizes=t)
    assert hr.calls == 2 and "forward" not in model.resampler.__dict__ and "forward" not in model.vpm.__dict__
    # the module's own forward is back, and the HIP rows are its rows within the stack criterion's absolute bound
    theirs = model.resampler(feats, t)
    assert hr.calls == 2 and RR.rel_l2(want, theirs) < 3e-2
    hr.install()
    hr.remove()
    assert "forward" not in model.resampler.__dict__
    with pytest.raises(KeyError):
        with hr:
            raise KeyError("inside")
    assert "forward" not in model.resampler.__dict__
