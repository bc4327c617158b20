"""The float64 GEMM reference and the per-element checker of tests/gemm_ref.py, on the host at small shapes (a few 256^2 tiles with ragged
edges, K up to 3072, a fused QKV case with two heads, two samples and tok_off > 0).  A correct-kernel stand-in -- f32 accumulation over the
64-wide K-tiles in order, the epilogue in f32 with one rounding -- passes every bound on every operand kind; each kernel fault below, applied to
that stand-in, is rejected with a message that names the faulty tile -- and several of them slip past the sampled-row rel-L2 check the GEMM
tests used before."""
import math

import pytest
import torch

from tests import gemm_ref as R

bf = torch.bfloat16
M, N, K, B = 600, 520, 3072, 2          # 3 x 3 tiles per item, the last row / column of tiles partial
FT = (1, 1)                             # the tile the single-tile faults hit


def operands(kind, seed, M=M, N=N, K=K, batch=B, res=True):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((batch, M, K), generator=g)
    if kind == "tagged":
        A = torch.stack([A[z] * R.tag_scales(M, K, z) for z in range(batch)])
    A = A.to(bf)
    W = (0.02 * torch.randn((N, K), generator=g)).to(bf)
    bias = (0.5 * torch.randn((N,), generator=g)).to(bf)
    gate = torch.randn((batch, N), generator=g)
    if not res:
        return A, W, bias, None, None
    if kind == "cancel":
        lin = torch.stack([R.linear_f64(A[z], W, bias)[0] for z in range(batch)])
        resv = (-gate[:, None, :].double() * lin).to(bf)
    else:
        resv = (R.lin_scale(K) * torch.randn((batch, M, N), generator=g)).to(bf)
    return A, W, bias, gate, resv


def f32_fma(g, v, r):
    """fmaf(g, v, r) for f32 tensors: the exact product and sum in float64, one rounding to f32"""
    return (g.double() * v.double() + r.double()).float()


def acc_f32(A, W, fault=None):
    """f32 accumulation of A [M, K] W^T over the 64-wide K-tiles, in order.  fault: ("drop", kt) leaves K-tile kt out of tile FT, ("twice",
    kt0, kt1) adds K-tiles kt0..kt1-1 a second time in tile FT."""
    acc = torch.zeros((A.shape[0], W.shape[0]))
    parts = []
    for k0 in range(0, A.shape[1], 64):
        p = A[:, k0:k0 + 64].float() @ W[:, k0:k0 + 64].float().T
        acc += p
        parts.append(p)
    if fault is not None:
        rs, cs = slice(FT[0] * 256, FT[0] * 256 + 256), slice(FT[1] * 256, FT[1] * 256 + 256)
        if fault[0] == "drop":
            acc[rs, cs] -= parts[fault[1]][rs, cs]
        elif fault[0] == "twice":
            for kt in range(fault[1], fault[2]):
                acc[rs, cs] += parts[kt][rs, cs]
    return acc


def standin_gemm(A, W, bias, gate, res, act=R.ACT_NONE, fault=None):
    """x2i_gemm_bf16 as a correct kernel computes it (fault None) or with one kernel fault: [batch, M, N] bf16"""
    out = []
    for z in range(A.shape[0]):
        f = fault if (z == 0 or (fault and fault[0] in ("gate_item", "double_round"))) else None   # single-tile faults: in item 0
        acc = acc_f32(A[z], W, f if f and f[0] in ("drop", "twice") else None)
        b = bias.float()
        rs, cs = slice(FT[0] * 256, FT[0] * 256 + 256), slice(FT[1] * 256, FT[1] * 256 + 256)
        if f and f[0] == "bias_tile":                # tile FT reads the bias of the next 256-column tile
            b = b.clone()
            b[FT[1] * 256:FT[1] * 256 + 256] = bias.float()[FT[1] * 256 + 256:FT[1] * 256 + 512].clone() if N >= FT[1] * 256 + 512 else \
                torch.cat([bias.float()[FT[1] * 256 + 256:], bias.float()[:FT[1] * 256 + 512 - N]])
            v = acc + bias.float()
            v[rs, cs] = (acc + b)[rs, cs]
        else:
            v = acc + b
        if act == R.ACT_GELU_TANH:               # gelu_tanh_f: x / (1 + exp2(x (a + b x^2))), in f32
            v = v / (1.0 + torch.exp2(v * (v * v * -0.10294324 - 2.3022082)))
        if res is not None:
            gz = gate[z - 1 if (f and f[0] == "gate_item" and z > 0) else z]
            if f and f[0] == "double_round":
                v = v.to(bf).float()
            v = f32_fma(gz, v, res[z].float())
        if f and f[0] == "trunc":
            t = v.clone()
            t[rs, cs] = (t[rs, cs].view(torch.int32) & ~0xFFFF).view(torch.float32)
            out.append(t.to(bf))
        else:
            out.append(v.to(bf))
    return torch.stack(out)


def gemm_failure(A, W, bias, gate, res, C, act=R.ACT_NONE):
    rep = R.check_gemm(R.Report("launch"), A, W, bias, C, act=act, gate=gate, res=res)
    try:
        rep.done()
    except AssertionError as e:
        return str(e)
    return None


def sampled_rel_l2(C, A, W, bias, gate, res, rows=(0, 1, 255, 520, 599)):
    """the old style of check: fp32 reference on a few hand-picked rows (here in tile rows 0 and 2), whole-slice rel-L2"""
    worst = 0.0
    for z in range(A.shape[0]):
        r = torch.tensor(rows)
        lin = A[z][r].float() @ W.float().T + bias.float()
        want = res[z][r].float() + gate[z] * lin if res is not None else lin
        worst = max(worst, float((C[z][r].float() - want).norm() / want.norm()))
    return worst


_cache = {}


def case(kind):
    if kind not in _cache:
        ops_ = operands(kind, 11 + len(kind))
        _cache[kind] = ops_, standin_gemm(*ops_)
    return _cache[kind]


@pytest.mark.parametrize("kind", R.KINDS)
def test_correct_standin_passes_every_bound(kind):
    (A, W, bias, gate, res), C = case(kind)
    rep = R.check_gemm(R.Report(f"standin {kind}"), A, W, bias, C, gate=gate, res=res)
    worst = rep.done()
    assert worst < 1.0
    # plain, GELU-tanh and f32 outputs on the same operands
    C0 = standin_gemm(A, W, bias, None, None)
    assert R.check_gemm(R.Report("plain"), A, W, bias, C0).done() < 1.0
    C1 = standin_gemm(A, W, bias, None, None, act=R.ACT_GELU_TANH)
    assert R.check_gemm(R.Report("gelu"), A, W, bias, C1, act=R.ACT_GELU_TANH).done() < 1.0
    Cf = torch.stack([acc_f32(A[z], W) + bias.float() for z in range(B)])
    assert R.check_gemm(R.Report("f32"), A, W, bias, Cf, out_f32=True).done() < 1.0
    print(f"\n  {kind}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("fault,kind,old_misses", [
    (("drop", 17), "random", True),
    (("twice", 30, 36), "random", True),
    (("double_round",), "cancel", False),
    (("trunc",), "random", True),
    (("bias_tile",), "random", True),
])
def test_single_tile_faults_are_rejected_naming_the_tile(fault, kind, old_misses):
    (A, W, bias, gate, res), C = case(kind)
    bad = standin_gemm(A, W, bias, gate, res, fault=fault)
    msg = gemm_failure(A, W, bias, gate, res, bad)
    assert msg is not None, fault
    if fault[0] != "double_round":   # (a launch-wide fault: every tile fails)
        assert msg.startswith(f"launch, item 0: tile ({FT[0]}, {FT[1]})") and "[1 failing tiles in the launch]" in msg, msg
    else:
        assert "item" in msg and "tile (" in msg, msg
    # the old check (rel-L2 < 1e-2 on sampled rows) does not see it
    assert (sampled_rel_l2(bad, A, W, bias, gate, res) < R.OLD_SAMPLED_BOUND) == old_misses, fault


def test_gate_of_the_previous_item_is_rejected_naming_the_item():
    (A, W, bias, gate, res), C = case("random")
    bad = standin_gemm(A, W, bias, gate, res, fault=("gate_item",))
    msg = gemm_failure(A, W, bias, gate, res, bad)
    assert msg is not None and "item 1" in msg and "item 0" not in msg, msg


def test_truncation_of_a_gelu_epilogue_is_rejected():
    (A, W, bias, _, _), _ = case("random")
    good = standin_gemm(A, W, bias, None, None, act=R.ACT_GELU_TANH)
    bad = standin_gemm(A, W, bias, None, None, act=R.ACT_GELU_TANH, fault=("trunc",))
    assert gemm_failure(A, W, bias, None, None, good, act=R.ACT_GELU_TANH) is None
    msg = gemm_failure(A, W, bias, None, None, bad, act=R.ACT_GELU_TANH)
    assert msg is not None and f"tile ({FT[0]}, {FT[1]})" in msg


# ---------------------------------------------------------------------------------------------------------------- encoder launches
# What the encoder modules' launches add to the checker (tests/gemm_replay.py, tests/test_encoder_gemm_fp64_gpu.py): a weight per item,
# A rows that overlap in memory, a residual in the output's own storage, and the GELU-erf / SiLU / ReLU epilogues.  Small shapes: two items,
# one ragged tile each.
M2, N2, D2 = 70, 100, 64
LDA2, K2 = 2 * D2, 3 * D2                # the stride-2 convolution as a GEMM: a row starts 2 D after the last and is 3 D long


def act_f32(v, act):
    """the activations as csrc/x2i_common.h writes them, in f32"""
    if act == R.ACT_GELU_TANH:
        return v / (1.0 + torch.exp2(v * (v * v * -0.10294324 - 2.3022082)))
    if act == R.ACT_GELU_ERF:
        return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
    if act == R.ACT_SILU:
        return v / (1.0 + torch.exp2(-1.4426950408889634 * v))
    if act == R.ACT_RELU:
        return v.clamp_min(0.0)
    return v


def standin2(A, W, bias, *, act=R.ACT_NONE, gate=None, res=None, fault=None):
    """x2i_gemm_bf16 on A [batch, M, K] (any view), W [N, K] or [batch, N, K], gate [batch, N], res [batch, M, N]: bf16 [batch, M, N].
    fault: "w_prev" (item z multiplies the weight of item z - 1), "act_tanh" (the tanh GELU whatever was asked), "double_round" (a bf16
    rounding before the residual add), "gate_shift" (column n takes the gate of channel n + 1)."""
    out = []
    for z in range(A.shape[0]):
        Wz = W if W.dim() == 2 else W[z - 1 if (fault == "w_prev" and z > 0) else z]
        v = acc_f32(A[z], Wz) + (bias.float() if bias is not None else 0.0)
        v = act_f32(v, R.ACT_GELU_TANH if fault == "act_tanh" else act)
        if res is not None:
            g = gate[z] if gate is not None else torch.ones(v.shape[1])
            if fault == "gate_shift":
                g = torch.roll(g, -1)
            if fault == "double_round":
                v = v.to(bf).float()
            v = f32_fma(g, v, res[z].float())
        out.append(v.to(bf))
    return torch.stack(out)


def failure2(A, W, bias, C, **kw):
    try:
        R.check_gemm(R.Report("launch"), A, W, bias, C, **kw).done()
    except AssertionError as e:
        return str(e)
    return None


def names_item_row_col(msg, item=None):
    import re
    return msg is not None and re.search(r"item %s: .*\(m=\d+, n=\d+\)" % (r"\d+" if item is None else item), msg) is not None


def small_operands(kind, seed, K=K2, w_batch=False):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((B, M2, K), generator=g)
    if kind == "tagged":
        A = torch.stack([A[z] * R.tag_scales(M2, K, z) for z in range(B)])
    W = (0.02 * torch.randn((B, N2, K) if w_batch else (N2, K), generator=g)).to(bf)
    bias = (0.5 * torch.randn((N2,), generator=g)).to(bf)
    return A.to(bf), W, bias


def overlapped_A(kind, seed):
    """(the strided view [B, M2, K2] with lda = LDA2 < K2, the same storage read densely with lda = K2): the storage is filled, and `tagged`
    scales the storage (a copy_ into an overlapping view is refused)"""
    per_item = M2 * K2                    # (room for the dense reading too)
    st = torch.randn(B * per_item, generator=torch.Generator().manual_seed(seed))
    if kind == "tagged":
        n = (M2 - 1) * LDA2 + K2
        for z in range(B):
            st[z * per_item:z * per_item + n] *= R.tag_scales_flat(n, LDA2, z).float()
    st = st.to(bf)
    return st.as_strided((B, M2, K2), (per_item, LDA2, 1)), st.as_strided((B, M2, K2), (per_item, K2, 1))


@pytest.mark.parametrize("kind", R.KINDS)
def test_standin_passes_with_a_weight_per_item_and_a_shared_a(kind):
    A, W, bias = small_operands(kind, 31, w_batch=True)
    assert failure2(A, W, bias, standin2(A, W, bias)) is None
    shared = A[:1].expand(B, M2, K2)          # a_batch_stride = 0: every item reads the same rows
    assert shared.stride(0) == 0
    assert failure2(shared, W, bias, standin2(shared, W, bias)) is None
    # the previous item's weight is rejected, in item 1 and not in item 0
    msg = failure2(A, W, bias, standin2(A, W, bias, fault="w_prev"))
    assert names_item_row_col(msg, 1) and "item 0" not in msg, msg
    with pytest.raises(AssertionError):
        R.check_gemm(R.Report("shape"), A, W[:1], bias, standin2(A, W, bias))       # a batch of weights that is not the launch's


@pytest.mark.parametrize("kind", R.KINDS)
def test_standin_passes_with_overlapping_a_rows_and_the_dense_reading_is_rejected(kind):
    A, dense = overlapped_A(kind, 32)
    assert A.stride() == (M2 * K2, LDA2, 1) and torch.equal(A[0, 1, :D2], A[0, 0, LDA2:])       # the rows do overlap
    _, W, bias = small_operands("random", 33)
    assert failure2(A, W, bias, standin2(A, W, bias)) is None
    msg = failure2(A, W, bias, standin2(dense, W, bias))
    assert names_item_row_col(msg), msg
    assert "(m=0," not in msg                     # row 0 reads the same elements either way
    if kind == "tagged":                          # the storage tags differ from row to row and from 64-block to 64-block
        t = R.tag_scales_flat(2 * LDA2, LDA2)
        assert float(t[0]) != float(t[64]) and float(t[0]) != float(t[LDA2]) and bool((torch.log2(t) == torch.log2(t).round()).all())


@pytest.mark.parametrize("kind", R.KINDS)
def test_standin_passes_with_the_residual_in_the_outputs_storage(kind):
    """out=X, res=X: the residual is filled into the shared storage, a clone of it is what the reference reads"""
    A, W, bias = small_operands(kind, 34)
    g = torch.Generator().manual_seed(35)
    gate = torch.randn((B, N2), generator=g)
    if kind == "cancel":
        X = torch.stack([(-gate[z].double() * R.linear_f64(A[z], W, bias)[0]).to(bf) for z in range(B)])
    else:
        X = (R.lin_scale(K2) * torch.randn((B, M2, N2), generator=g)).to(bf)
    before = X.clone()
    X.copy_(standin2(A, W, bias, gate=gate, res=X))
    assert failure2(A, W, bias, X, gate=gate, res=before) is None
    assert failure2(A, W, bias, X, gate=gate, res=X) is not None            # the storage after the launch is not the residual
    # a second bf16 rounding before the add; the gate read one channel off
    X2 = before.clone()
    X2.copy_(standin2(A, W, bias, gate=gate, res=X2, fault="double_round"))
    msg = failure2(A, W, bias, X2, gate=gate, res=before)
    assert names_item_row_col(msg), (kind, msg)
    X3 = before.clone()
    X3.copy_(standin2(A, W, bias, gate=gate, res=X3, fault="gate_shift"))
    msg = failure2(A, W, bias, X3, gate=gate, res=before)
    assert names_item_row_col(msg), (kind, msg)


@pytest.mark.parametrize("act", [R.ACT_GELU_ERF, R.ACT_SILU, R.ACT_RELU], ids=["gelu_erf", "silu", "relu"])
def test_standin_passes_with_each_activation(act):
    A, W, bias = small_operands("random", 36 + act, K=1024)
    A = (A.float() * 3.0).to(bf)                  # lin reaches +-6: the tails of the activations, and the cancelling side of 1 + erf
    lin = R.linear_f64(A[0], W, bias)[0]
    assert float(lin.min()) < -5.0 and float(lin.max()) > 5.0
    rep = R.check_gemm(R.Report("act"), A, W, bias, standin2(A, W, bias, act=act), act=act)
    share = rep.done()
    print(f"\n  act {act}: share of the f32 allowance used by the stand-in {share:.3f}")
    assert share < 1.0
    # and as a second output: C = v, C2 = act(v)
    C = standin2(A, W, bias)
    C2 = torch.stack([act_f32(acc_f32(A[z], W) + bias.float(), act).to(bf) for z in range(B)])
    assert R.check_gemm(R.Report("act2"), A, W, bias, C, C2=C2, act2=act).done() < 1.0


def test_tanh_gelu_where_erf_was_asked_is_rejected():
    A, W, bias = small_operands("random", 38, K=1024)
    msg = failure2(A, W, bias, standin2(A, W, bias, act=R.ACT_GELU_ERF, fault="act_tanh"), act=R.ACT_GELU_ERF)
    assert names_item_row_col(msg), msg
    # ... and the widened erf term does not let the tanh form through on the negative side alone either
    neg = (-0.25 * A.float().abs()).to(bf), W.abs(), None         # lin near -3.3: GELU near -1.6e-3, the two forms 3e-4 apart
    msg = failure2(*neg, standin2(*neg, act=R.ACT_GELU_ERF, fault="act_tanh"), act=R.ACT_GELU_ERF)
    assert names_item_row_col(msg), msg
    assert failure2(*neg, standin2(*neg, act=R.ACT_GELU_ERF), act=R.ACT_GELU_ERF) is None


# ---------------------------------------------------------------------------------------------------------------- fused QKV
H, ST, SI, NS = 2, 40, 300, 2          # two heads (one 256-column tile per section), 40 text + 300 image tokens, two samples
S = ST + SI
SPAD = (S + 127) // 128 * 128
KQ = 512


def rope_tables(S_):
    pos = torch.arange(S_, dtype=torch.float64)[:, None]
    freq = 1.0 / (10000.0 ** (torch.arange(64, dtype=torch.float64) / 64))
    ang = (pos * freq).repeat_interleave(2, -1)
    return torch.cos(ang).float(), torch.sin(ang).float()


def qkv_problem(seed, M_, kind="random"):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((1, M_, KQ), generator=g)
    if kind == "tagged":
        A = A * R.tag_scales(M_, KQ)
    W = (0.02 * torch.randn((3 * H * 128, KQ), generator=g)).to(bf)
    bias = (0.5 * torch.randn((3 * H * 128,), generator=g)).to(bf)
    nq, nk = (1.0 + 0.1 * torch.randn(128, generator=g)).to(bf), (1.0 + 0.1 * torch.randn(128, generator=g)).to(bf)
    return A.to(bf), W, bias, nq, nk


def standin_qkv(A, W, bias, nq, nk, cos, sin, Q, K, VT, *, tok_off, rps, q_scale, vt_perm, eps=1e-6, fault=None):
    """x2i_gemm_qkv_bf16 in f32 as a correct kernel computes it (or with one fault), written into Q / K / VT"""
    M_ = A.shape[1]
    x = (acc_f32(A[0], W) + bias.float()).to(bf).float().view(M_, 3, H, 128)
    rows = torch.arange(M_)
    b, s = R.tokens_of(rows, 0, tok_off, rps)
    st = s.clone()
    if fault == "rope_next":                      # RoPE of token s + 1 on the rows of the second sample
        st = torch.where(b == 1, (s + 1).clamp_max(cos.shape[0] - 1), s)
    c, sn = cos[st], sin[st]
    qs = torch.tensor(q_scale, dtype=torch.float32)
    wq, wk = nq.float() * qs, nk.float()
    if fault == "swap_qk":
        wq, wk = nk.float() * qs, nq.float()
    if fault == "qscale_k":
        wk = nk.float() * qs
    for sec, w, dst in ((0, wq, Q), (1, wk, K)):
        xs = x[:, sec]
        r = torch.rsqrt((xs * xs).sum(-1, keepdim=True) / 128 + eps)
        a = xs * r * w
        o = torch.empty_like(a)
        o[..., 0::2] = (a[..., 0::2].double() * c[:, None, 0::2] - (a[..., 1::2] * sn[:, None, 0::2]).double()).float()
        o[..., 1::2] = (a[..., 1::2].double() * c[:, None, 1::2] + (a[..., 0::2] * sn[:, None, 1::2]).double()).float()
        dst[b, :, s, :] = o.to(bf)
    pos = R.vt_pos(s, vt_perm)
    if fault == "vt_span":                        # one 32-token span of sample 0 written in sequence order
        span = (b == 0) & (s >= 64) & (s < 96)
        pos = torch.where(span, s, pos)
    VT[b, :, :, pos] = x[:, 2].to(bf)


def qkv_failure(A, W, bias, nq, nk, cos, sin, Q, K, VT, *, tok_off, rps, q_scale, vt_perm, name="qkv"):
    rep = R.check_qkv(R.Report(name), A, W, bias, nq, nk, cos, sin, Q, K, VT, H=H, tok_off=tok_off, rows_per_sample=rps, q_scale=q_scale,
                      vt_perm=vt_perm)
    try:
        rep.done()
    except AssertionError as e:
        return str(e)
    return None


def qkv_buffers():
    Q = R.poison_(torch.empty((NS, H, SPAD, 128), dtype=bf))
    K = R.poison_(torch.empty((NS, H, SPAD, 128), dtype=bf))
    VT = R.poison_(torch.empty((NS, H, 128, SPAD), dtype=bf))
    return Q, K, VT


QS = 1.0 / math.sqrt(128.0) * 1.4426950408889634


def run_pair(fault=None, vt_perm=True, kind="random"):
    """the double block's pair: image rows (tok_off = ST, rows_per_sample = SI) and text rows (tok_off = 0), both samples, one buffer set.
    Returns (failure message or None) over both problems, and the buffers."""
    cos, sin = rope_tables(S)
    pairs = torch.stack((cos[:, 0::2], sin[:, 0::2]), -1).contiguous()
    img = qkv_problem(1, NS * SI, kind)
    txt = qkv_problem(2, NS * ST, kind)
    Q, K, VT = qkv_buffers()
    ti, tt = img, txt
    if fault == "swap_streams":                   # the image rows get the text stream's norm weights and vice versa
        ti, tt = img[:3] + txt[3:], txt[:3] + img[3:]
    standin_qkv(*ti, cos, sin, Q, K, VT, tok_off=ST, rps=SI, q_scale=QS, vt_perm=vt_perm, fault=fault)
    standin_qkv(*tt, cos, sin, Q, K, VT, tok_off=0, rps=ST, q_scale=QS, vt_perm=vt_perm)
    msgs = [qkv_failure(*img, pairs, None, Q, K, VT, tok_off=ST, rps=SI, q_scale=QS, vt_perm=vt_perm, name="qkv image"),
            qkv_failure(*txt, cos, sin, Q, K, VT, tok_off=0, rps=ST, q_scale=QS, vt_perm=vt_perm, name="qkv text")]
    return [m for m in msgs if m], (Q, K, VT)


@pytest.mark.parametrize("vt_perm", [False, True])
@pytest.mark.parametrize("kind", ["random", "tagged"])
def test_qkv_standin_passes_and_leaves_the_padding(vt_perm, kind):
    msgs, (Q, K, VT) = run_pair(vt_perm=vt_perm, kind=kind)
    assert not msgs, msgs
    R.check_qkv_padding("standin", Q, K, VT, S, vt_perm)


@pytest.mark.parametrize("fault,want", [
    ("swap_qk", "section q"),
    ("qscale_k", "section k"),
    ("rope_next", "sample 1"),
    ("vt_span", "section v"),
    ("swap_streams", "qkv image"),
])
def test_qkv_faults_are_rejected_naming_sample_head_section(fault, want):
    msgs, _ = run_pair(fault=fault)
    assert msgs, fault
    assert want in msgs[0] or (fault == "qscale_k" and any("section k" in m for m in msgs)), msgs
    if fault == "rope_next":
        assert "sample 0" not in msgs[0] and "section q" in msgs[0] or "section k" in msgs[0], msgs   # rows SI.. of the image launch
    if fault == "vt_span":
        assert "sample 0" in msgs[0] and "tile (0, 2)" in msgs[0], msgs


def test_qkv_padding_write_is_rejected():
    _, (Q, K, VT) = run_pair()
    Q[1, 1, S + 3, 5] = 0
    with pytest.raises(AssertionError, match=r"Q padding row written: sample 1, head 1, row 343"):
        R.check_qkv_padding("standin", Q, K, VT, S, True)
    _, (Q, K, VT) = run_pair()
    VT[0, 0, 7, SPAD - 1] = 0
    with pytest.raises(AssertionError, match=r"V\^T padding column written: sample 0, head 0, dim 7, position 383"):
        R.check_qkv_padding("standin", Q, K, VT, S, True)


# ---------------------------------------------------------------------------------------------------------------- untouched regions
def test_writes_outside_the_launch_are_rejected():
    """out rows >= M and columns before c_offset: a [B*S, 5 D]-style buffer written at columns [c_offset, c_offset + N) of M rows"""
    rows, ld, c_off, n = 300, 96, 32, 64
    buf = R.poison_(torch.empty(rows * ld + 7, dtype=bf))
    view = ((rows - 20, n), (ld, 1), c_off)
    mask = R.write_mask(buf, [view])
    buf.as_strided(*view).fill_(1.0)
    R.check_untouched("ok", buf, mask, row_len=ld)
    past = buf.clone()
    past[(rows - 20) * ld + c_off + 3] = 1.0            # one row past M
    with pytest.raises(AssertionError, match=r"first at element .* \(row 280, col 35\)"):
        R.check_untouched("past M", past, mask, row_len=ld)
    before = buf.clone()
    before[5 * ld + c_off - 1] = 1.0                    # one column before c_offset
    with pytest.raises(AssertionError, match=r"\(row 5, col 31\)"):
        R.check_untouched("before c_offset", before, mask, row_len=ld)
    f = R.poison_(torch.empty(64, dtype=torch.float32))
    f[3] = 0.0
    with pytest.raises(AssertionError, match="element 3"):
        R.check_untouched("f32", f, torch.zeros(64, dtype=torch.bool))


def test_bf16_helpers_are_exact():
    x = torch.randn(100000, dtype=torch.float64) * torch.exp2(torch.randint(-130, 100, (100000,)).double())
    r = R.bf16_rne(x)
    assert torch.equal(r, x.float().to(bf).double()) or \
        bool(((r - x).abs() <= 0.5 * R.ulp_bf16(x)).all())            # (torch's double -> bf16 may round twice; ours never does)
    assert torch.equal(R.bf16_rne(r), r)
    mid = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)   # ties: to even
    assert R.bf16_rne(mid).tolist() == [1.0, 1.0 + 4 * 2.0 ** -8]
    assert R.ulp_bf16(torch.tensor([1.0, 1.5, 2.0 ** -130], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -133]
