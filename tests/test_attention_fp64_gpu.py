"""The product attention kernels at the model's sequence length (S = 4608: 72 key tiles of 64, a 1024^2 image plus 512 text tokens; 24 heads)
and at ragged lengths near it, against the float64 reference of tests/attn_ref.py -- every output in full, every head, every 64-row tile:

  training forward   x2i_attention_lse_bf16 at scale 1/sqrt(128) (O and the log2-sum-exp rows handed to the backward)
  backward           x2i_attention_bwd_bf16 with default options (dQ and dK / dV passes as one launch), with its own statistics pass and with
                     the forward's statistics (the training step's path), dQ / dK / dV / lse2, D from x2i_attention_bwd_prep_bf16
  sampling forward   x2i_attention_vp_ws_bf16 (16 x 16 x 32 kernel, prescaled Q, span-permuted V^T, the stream-K workspace) as the sampling
                     path calls it, and the 32 x 32 x 16 hand-scheduled kernel on the natural layout

Input kinds (tests/attn_ref.py: make_inputs): `anti` fails a kernel whose padding keys enter the softmax, `spike` forces the online-softmax
rescale at a late key tile.  The reference runs on the GPU in float64 (torch): a test-side reference, not the product path."""
import math

import pytest
import torch

from tests import attn_ref as R
from tests.util import span_permute

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 1.0 / math.sqrt(128.0)
SENTINEL = 0x7F7F           # bf16 bits of 3.39e38: the padding rows of dQ / dK / dV before the call; the kernels store rows < S only


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


def poisoned(B, H, Spad):
    t = torch.empty((B, H, Spad, 128), device=DEV, dtype=torch.bfloat16)
    t.view(torch.int16).fill_(SENTINEL)
    return t


def untouched_beyond(t, S):
    return bool((t[:, :, S:].view(torch.int16) == SENTINEL).all())


def heads(o_tok, B, S, H):
    """token-major O [B, S, H * 128] -> [B, H, S, 128] (a view)"""
    return o_tok.view(B, S, H, 128).permute(0, 2, 1, 3)


# (B, H, S, kind): the model length; ragged (the masked last dQ tile); ragged with Spad % 256 = 128 (a half dQ block, dead dK / dV rows);
# 270 dQ and 540 dK / dV blocks (not multiples of 8: the uneven branch of the XCD block remap)
TRAIN_CASES = [(1, 24, 4608, "random"), (2, 24, 4600, "random"), (2, 24, 4600, "anti"), (1, 24, 4470, "random"), (1, 24, 4470, "anti"),
               (1, 24, 4470, "spike"), (3, 5, 4600, "random"), (3, 5, 4600, "anti")]


@pytest.mark.parametrize("B,H,S,kind", TRAIN_CASES)
def test_training_attention_forward_and_backward_vs_fp64(ops, B, H, S, kind):
    from x2i_amd import _lib
    Spad = ops.pad128(S)
    D = H * 128
    Q, K, V, dO = R.make_inputs(kind, B, H, S, Spad, seed=B * 100000 + H * 10000 + S, device=DEV)
    ref = R.reference(Q, K, V, dO, S, SCALE)
    tag = f"B={B} H={H} S={S} {kind}"
    # training forward: O and lse2 (+big beyond S)
    VT = ops.transpose(V.view(B * H, Spad, 128)).view(B, H, 128, Spad)
    O = torch.full((B, S, D), 7.0, device=DEV, dtype=torch.bfloat16)
    lse_f = torch.full((B, H, Spad), -7.0, device=DEV)
    ops.attention_lse(Q, K, VT, O, lse_f, B, H, S, Spad, D, S * D, SCALE)
    w = {"O": R.check_tiles(f"{tag} attention_lse O", heads(O, B, S, H), ref["O"], R.TOL_O),
         "lse2 fwd": R.check_rows(f"{tag} attention_lse lse2", lse_f, ref["lse2"], R.TOL_LSE2)}
    assert bool((lse_f[:, :, S:] > 1e29).all())
    # D = rowsum(dO * O) from the token-major dO and the forward's bf16 O, against float64 on the same O; 0 on the padding rows
    dO_tok = dO[:, :, :S].permute(0, 2, 1, 3).reshape(B, S, D).contiguous()
    Dv = torch.full((B, H, Spad), -7.0, device=DEV)
    ops.attention_bwd_prep(dO_tok, O, Dv, B, H, S, Spad, do_bs=S * D, lddo=D, o_bs=S * D, ldo=D)
    w["D"] = R.check_rows(f"{tag} attention_bwd_prep D", Dv, (dO[:, :, :S].double() * heads(O, B, S, H).double()).sum(-1), R.TOL_D)
    assert bool((Dv[:, :, S:] == 0).all())
    # backward: the statistics from the forward (the training step's path, have_lse = 1) and from its own statistics pass (have_lse = 0)
    QT, KT = ops.transpose(Q.view(B * H, Spad, 128)), ops.transpose(K.view(B * H, Spad, 128))
    dOh = dO.view(B * H, Spad, 128)
    dOT = ops.transpose(dOh)
    grads = {}
    for have_lse in (1, 0):
        lse = lse_f if have_lse else torch.full((B, H, Spad), -7.0, device=DEV)
        dQ, dK, dV = poisoned(B, H, Spad), poisoned(B, H, Spad), poisoned(B, H, Spad)
        ops.attention_bwd(Q, K, V, QT, KT, dOh, dOT, lse, Dv, dQ, dK, dV, B, H, S, Spad, SCALE, have_lse=bool(have_lse))
        if not have_lse:
            w["lse2 bwd"] = R.check_rows(f"{tag} statistics pass lse2", lse, ref["lse2"], R.TOL_LSE2)
            assert bool((lse[:, :, S:] > 1e29).all())
        for n, t, bound in (("dQ", dQ, R.TOL_DQ), ("dK", dK, R.TOL_DK), ("dV", dV, R.TOL_DV)):
            e = R.check_tiles(f"{tag} have_lse={have_lse} {n}", t, ref[n], bound)
            w[n] = max(w.get(n, 0.0), e)
            assert untouched_beyond(t, S), f"{tag} have_lse={have_lse}: {n} rows >= S written"
        grads[have_lse] = (dQ, dK, dV)
    if S == 4608:
        # the two passes one after the other: the fused launch's blocks, bit for bit
        old = _lib.set_option("attn_bwd_overlap", 0)
        try:
            serial = [poisoned(B, H, Spad) for _ in range(3)]
            ops.attention_bwd(Q, K, V, QT, KT, dOh, dOT, lse_f, Dv, *serial, B, H, S, Spad, SCALE, have_lse=True)
        finally:
            _lib.set_option("attn_bwd_overlap", old)
        for a, b_ in zip(serial, grads[1]):
            assert torch.equal(a, b_)
    print(f"\n  {tag}: worst tile " + ", ".join(f"{k} {v:.2e}" for k, v in w.items()))


# (B, S, kind) at H = 24: batch 1 .. 4 at the model length (1.7 .. 6.75 rounds of work items: stream-K cuts, the persistent form) and the ragged
# model length
SAMPLE_CASES = [(1, 4608, "random"), (2, 4608, "peaked"), (3, 4608, "spike"), (4, 4608, "random"), (3, 4600, "anti"), (3, 4600, "spike")]


@pytest.mark.parametrize("B,S,kind", SAMPLE_CASES)
def test_sampling_attention_vs_fp64(ops, B, S, kind):
    """ops.attention(..., vt_perm=True) with Q carrying softmax_scale * log2(e) and scale = ln 2, as the sampling path calls it (x2i_amd/flux.py),
    with the stream-K workspace of the current stream; reference softmax(ln2 Qs K^T) V on the bf16 Qs the kernel saw."""
    H = 24
    Spad = ops.pad128(S)
    D = H * 128
    ln2 = math.log(2.0)
    assert ops.attention_prefers_vt_perm(H, S, ln2)
    Q, K, V, _ = R.make_inputs(kind, B, H, S, Spad, seed=7000 + B * 10000 + S, device=DEV)
    Qs = (Q.float() * (SCALE * R.LOG2E)).bfloat16()
    ref = R.reference(Qs, K, V, None, S, ln2)
    VTP = span_permute(ops.transpose(V.view(B * H, Spad, 128)).view(B, H, 128, Spad))
    O = torch.full((B, S, D), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.attention(Qs, K, VTP, O, B, H, S, Spad, D, S * D, ln2, vt_perm=True)
    e = R.check_tiles(f"B={B} S={S} {kind} attention vt_perm O", heads(O, B, S, H), ref["O"], R.TOL_O)
    ops.streamk_check(sync=True)
    print(f"\n  sampling B={B} H={H} S={S} {kind}: worst tile O {e:.2e}")


@pytest.mark.parametrize("S,kind", [(4608, "random"), (4600, "anti")])
def test_sampling_attention_natural_layout_vs_fp64(ops, S, kind):
    """The hand-scheduled 32 x 32 x 16 kernel (csrc/attention_w4.hip): the automatic choice for a prescaled Q on the natural V^T layout."""
    B, H = 2, 24
    Spad = ops.pad128(S)
    D = H * 128
    ln2 = math.log(2.0)
    Q, K, V, _ = R.make_inputs(kind, B, H, S, Spad, seed=8000 + S, device=DEV)
    Qs = (Q.float() * (SCALE * R.LOG2E)).bfloat16()
    ref = R.reference(Qs, K, V, None, S, ln2)
    VT = ops.transpose(V.view(B * H, Spad, 128)).view(B, H, 128, Spad)
    O = torch.full((B, S, D), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.attention(Qs, K, VT, O, B, H, S, Spad, D, S * D, ln2)
    e = R.check_tiles(f"B={B} S={S} {kind} attention natural layout O", heads(O, B, S, H), ref["O"], R.TOL_O)
    print(f"\n  natural layout B={B} H={H} S={S} {kind}: worst tile O {e:.2e}")
