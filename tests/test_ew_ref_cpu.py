"""The float64 references and the per-row checker of tests/ew_ref.py on the host.  f32 stand-ins that follow the kernels' arithmetic
(csrc/elementwise.hip: per-lane chains and the 64-lane butterfly of wave_sum, ln_mod1's operation order, one rounding per output) pass every
bound on every operand kind; each kernel fault below, applied to the stand-in, is rejected with a message that names the sample and the row
-- and several of them slip past the whole-tensor rel-L2 / abs checks the kernel tests used before."""
import re

import pytest
import torch

from tests import ew_ref as E

bf = torch.bfloat16
LN_B, LN_S, LN_S0, LN_D = 3, 37, 13, 1024      # S, S0 not multiples of 4: waves of 4 rows straddle samples and streams


# ---------------------------------------------------------------------------------------------------------------- f32 helpers
def fma32(a, b, c):
    """fmaf on f32 tensors: exact product and sum in float64, one rounding to f32"""
    return (a.double() * b.double() + c.double()).float()


def wave_sum_chain(v, sq=False):
    """the f32 row sum of ln_kernel: lane l sums its 16-byte chunks c = l + 64 i (8 elements each) in order (sq: fmaf(d, d, acc)), then
    wave_sum's butterfly.  v f32 [R, D], D % 512 == 0."""
    R, D = v.shape
    L = v.view(R, D // 512, 64, 8)
    acc = torch.zeros((R, 64))
    for i in range(D // 512):
        for j in range(8):
            x = L[:, i, :, j]
            acc = fma32(x, x, acc) if sq else acc + x
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, 0]


def ln_standin(X, mod, fault=None, eps=1e-6):
    """x2i_ln_modulate_bf16 on X bf16 [B, S, D] with mod f32 [B, 4 D] = (shift0 | scale0 | shift1 | scale1), rows s < S0 on the first pair;
    4-row waves as ln_rows_kernel.  fault: one_pass, no_eps, trunc, mod_bf16, stale (every row of a 4-row wave uses the vectors of the
    wave's first row's sample),
    s0_off (S0 + 1)."""
    B, S, D = X.shape
    x = X.reshape(B * S, D).float()
    row = torch.arange(B * S)
    b, s = row // S, row % S
    S0 = LN_S0 + (1 if fault == "s0_off" else 0)
    side = (s >= S0).long()
    if fault == "stale":
        b = ((row // 4) * 4) // S
    m = mod.view(B, 4, D)
    sh, sc = m[b, 2 * side], m[b, 2 * side + 1]
    mean = wave_sum_chain(x) / D
    if fault == "one_pass":
        var = wave_sum_chain(x, sq=True) / D - mean * mean
    else:
        d = x - mean[:, None]
        var = wave_sum_chain(d, sq=True) / D
    epsf = torch.tensor(0.0 if fault == "no_eps" else eps, dtype=torch.float32)
    rstd = torch.rsqrt(var + epsf)
    one = 1.0 + sc
    if fault == "mod_bf16":
        one = one.to(bf).float()
    y = fma32((x - mean[:, None]) * rstd[:, None], one, sh)
    if fault == "trunc":
        return (y.view(torch.int32) & ~0xFFFF).view(torch.float32).to(bf).view(B, S, D)
    return y.to(bf).view(B, S, D)


def ln_failure(X, mod, Y):
    D = X.shape[-1]
    rep = E.check_ln(E.Report("ln"), X, Y, LN_S0, mod[:, 0:], mod[:, D:], mod[:, 2 * D:], mod[:, 3 * D:], 1e-6)
    try:
        rep.done()
    except AssertionError as e:
        return str(e)
    return None


def ln_old_rel_l2(X, mod, Y):
    """the old check (test_ln_modulate_two_streams): fp32 LayerNorm, whole-tensor rel-L2"""
    D = X.shape[-1]
    ln = torch.nn.functional.layer_norm(X.float(), (D,), eps=1e-6)
    ref = torch.empty_like(ln)
    ref[:, :LN_S0] = ln[:, :LN_S0] * (1 + mod[:, None, D:2 * D]) + mod[:, None, 0:D]
    ref[:, LN_S0:] = ln[:, LN_S0:] * (1 + mod[:, None, 3 * D:]) + mod[:, None, 2 * D:3 * D]
    return float((Y.float() - ref).norm() / ref.norm())


_ln_cache = {}


def ln_case(kind):
    if kind not in _ln_cache:
        g = torch.Generator().manual_seed(7 + E.LN_KINDS.index(kind))
        X = E.ln_rows(LN_B * LN_S, LN_D, kind, g, "cpu").view(LN_B, LN_S, LN_D)
        mod = E.mod_vectors(LN_B * 4 * LN_D, kind, g, "cpu").view(LN_B, 4 * LN_D)
        _ln_cache[kind] = X, mod
    return _ln_cache[kind]


def where_of(msg):
    m = re.search(r"worst at sample (\d+), row \(token\) (\d+)", msg)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("kind", E.LN_KINDS)
def test_ln_standin_passes(kind):
    X, mod = ln_case(kind)
    assert ln_failure(X, mod, ln_standin(X, mod)) is None


def test_ln_const_rows_are_exact():
    X, mod = ln_case("const")
    Y = ln_standin(X, mod)
    D = LN_D
    for r in range(0, LN_B * LN_S, 3):
        b, s = divmod(r, LN_S)
        sh = mod[b, 0:D] if s < LN_S0 else mod[b, 2 * D:3 * D]
        assert torch.equal(Y[b, s], sh.to(bf)), (b, s)


# fault, kind it must fail on, whether the old rel-L2 check misses it
LN_FAULTS = [("one_pass", "large_mean", True),
             ("no_eps", "const", False),
             ("trunc", "random", True),
             ("mod_bf16", "random", True),
             ("stale", "random", False),
             ("s0_off", "random", False)]


@pytest.mark.parametrize("fault,kind,old_misses", LN_FAULTS, ids=[f[0] for f in LN_FAULTS])
def test_ln_fault_rejected(fault, kind, old_misses):
    X, mod = ln_case(kind)
    Y = ln_standin(X, mod, fault)
    msg = ln_failure(X, mod, Y)
    assert msg is not None, fault
    b, s = where_of(msg)
    assert 0 <= b < LN_B and 0 <= s < LN_S
    if fault == "s0_off":                   # only row S0 of every sample changes
        assert s == LN_S0 and msg.endswith(f"[{LN_B} failing rows in the launch]"), msg
    if fault == "stale":                    # the first rows of a sample whose wave began in the sample before
        first = ((b * LN_S) // 4) * 4
        assert b > 0 and first < b * LN_S and s < 4 and msg.endswith("[5 failing rows in the launch]"), msg
    if fault == "no_eps":                   # the constant rows: 0 * inf
        assert (b * LN_S + s) % 3 in (0, 1), msg
    old = ln_old_rel_l2(X, mod, Y)
    assert (old < E.OLD_LN_REL_L2) == old_misses, (fault, old)


# ---------------------------------------------------------------------------------------------------------------- skinny linear
def silu32(x):
    return x / (1.0 + torch.exp(-x))


def skinny_standin(X, W, bias, act_in, act_out, y_old=None, fault=None):
    """x2i_skinny_linear: lanes chain k = 8 l + 512 i + j (fmaf), wave_sum, + bias, act_out, (+ y_old) in f32.  Chunks of 8 samples.
    fault: drop_last_k (the k >= 512 pass of K = 768 left out), chunk_row (samples 8.. read X one row early), bias_twice (under
    accumulate), act_after (act_in applied to the sum instead of x)."""
    B, K = X.shape
    x = X.float()
    if fault == "chunk_row":
        x = torch.cat((x[:8], x[7:B - 1]))
    a = x if act_in == E.ACT_NONE else silu32(x)
    if fault == "act_after":
        a = x
    N = W.shape[0]
    nk = K // 8
    Wl = W.float().view(N, nk, 8)
    al = a.view(B, nk, 8)
    acc = torch.zeros((B, N, 64))
    for i in range((K + 511) // 512):
        if fault == "drop_last_k" and i > 0:
            break
        for j in range(8):
            c = torch.arange(64) + 64 * i
            ok = c < nk
            cc = c.clamp_max(nk - 1)
            w = Wl[:, cc, j] * ok          # [N, 64]
            acc = fma32(w[None], al[:, cc, j][:, None, :] * ok, acc)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    v = acc[..., 0]
    if fault == "act_after":
        v = silu32(v)
    if bias is not None:
        v = v + bias.float()
    if act_out == E.ACT_SILU:
        v = silu32(v)
    if y_old is not None:
        v = y_old + v
        if fault == "bias_twice":
            v = v + bias.float()
    return v


def skinny_failure(X, W, bias, Y, act_in, act_out, y_old=None):
    rep = E.check_skinny(E.Report("skinny"), X, W, bias, Y, act_in=act_in, act_out=act_out, y_old=y_old)
    try:
        rep.done()
    except AssertionError as e:
        return str(e)
    return None


def sk_operands(kind, B, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((B, K), generator=g)
    W = (0.05 * torch.randn((N, K), generator=g)).to(bf)
    bias = (0.5 * torch.randn((N,), generator=g)).to(bf)
    if kind == "cancel":        # sample 0: bias = -bf16(W silu(x0)): its pre-activation is a rounding residual
        bias = (-(W.double() @ E.act_f64(X[0].double(), E.ACT_SILU))).to(bf)
    return X, W, bias


@pytest.mark.parametrize("kind", E.SK_KINDS)
@pytest.mark.parametrize("B,K", [(1, 256), (9, 768), (13, 3072)])
def test_skinny_standin_passes(kind, B, K):
    X, W, bias = sk_operands(kind, B, 200, K, B + K)
    Y = skinny_standin(X, W, bias, E.ACT_SILU, E.ACT_NONE)
    assert skinny_failure(X, W, bias, Y, E.ACT_SILU, E.ACT_NONE) is None
    Y2 = skinny_standin(X.to(bf), W, None, E.ACT_NONE, E.ACT_SILU, y_old=Y)
    assert skinny_failure(X.to(bf), W, None, Y2, E.ACT_NONE, E.ACT_SILU, y_old=Y) is None


SK_FAULTS = [("drop_last_k", 768, False, None), ("chunk_row", 256, False, 8), ("bias_twice", 256, False, None),
             ("act_after", 256, False, None)]


@pytest.mark.parametrize("fault,K,old_misses,sample", SK_FAULTS, ids=[f[0] for f in SK_FAULTS])
def test_skinny_fault_rejected(fault, K, old_misses, sample):
    B, N = 9, 200
    X, W, bias = sk_operands("random", B, N, K, 5)
    y_old = torch.randn((B, N)) if fault == "bias_twice" else None
    Y = skinny_standin(X, W, bias, E.ACT_SILU, E.ACT_NONE, y_old=y_old, fault=fault)
    msg = skinny_failure(X, W, bias, Y, E.ACT_SILU, E.ACT_NONE, y_old=y_old)
    assert msg is not None, fault
    b, _ = where_of(msg)
    if sample is not None:
        assert b == sample and "samples [8]" in msg, msg
    want = E.skinny_expect(X, W, bias, act_in=E.ACT_SILU, y_old=y_old)[0]
    old = float((Y.double() - want).norm() / want.norm())
    assert (old < E.OLD_SKINNY_REL_L2) == old_misses, (fault, old)


# ---------------------------------------------------------------------------------------------------------------- gated residual, sinusoid, Euler
def test_gated_residual_wrong_sample_gate():
    g = torch.Generator().manual_seed(3)
    B, S, D = 3, 20, 256
    X = torch.randn((B, S, D), generator=g).to(bf)
    T = torch.randn((B, S, D), generator=g).to(bf)
    G = torch.randn((B, D), generator=g)
    good = fma32(G[:, None, :], T.float(), X.float()).to(bf)
    assert E.check_gated(E.Report("gated"), X, T, G, good).done() < 1.0
    bad = good.clone()
    bad[2] = fma32(G[1][None], T[2].float(), X[2].float()).to(bf)
    with pytest.raises(AssertionError, match=r"worst at sample 2, row \(token\) \d+"):
        E.check_gated(E.Report("gated"), X, T, G, bad).done()


def sinusoid_standin(t, dim, round_bf16, fault=None):
    half = dim // 2
    k = torch.arange(dim) % half
    f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * k.float() / half)
    a = t[:, None] * f[None, :]
    first = torch.arange(dim) < half
    if fault == "swap":
        first = ~first
    v = torch.where(first[None], torch.cos(a), torch.sin(a))
    return v.to(bf).float() if round_bf16 else v


T_SIN = torch.tensor([0.0, 1.0, 250.0, 752.0, 1000.0, 3500.0, 0.001])


@pytest.mark.parametrize("round_bf16", [False, True])
def test_sinusoid_standin_and_swap(round_bf16):
    for dim in (256, 128):
        want, bound, delta = E.sinusoid_expect(T_SIN, dim, round_bf16)
        smp, tok = torch.arange(len(T_SIN)), torch.zeros(len(T_SIN), dtype=torch.long)
        assert E.check_rows("sin", sinusoid_standin(T_SIN, dim, round_bf16), want, bound, delta, sample=smp, token=tok)[0] is None
        msg, _ = E.check_rows("sin", sinusoid_standin(T_SIN, dim, round_bf16, "swap"), want, bound, delta, sample=smp, token=tok)
        assert msg is not None and "worst at sample" in msg
    # the new bound is far below the old absolute 2e-3 everywhere
    assert float(E.sinusoid_expect(T_SIN[:5], 256, False)[1].max()) < E.OLD_SIN_ABS / 4


def test_euler_bound_rejects_truncation():
    g = torch.Generator().manual_seed(4)
    x, e = torch.randn(4096, generator=g).to(bf), torch.randn(4096, generator=g).to(bf)
    dt = -0.25
    v = fma32(torch.tensor(dt), e.float(), x.float())
    want, bound, delta = E.euler_expect(x, e, dt)
    i = torch.arange(4096)
    assert E.check_rows("euler", v.to(bf)[:, None], want[:, None], bound[:, None], delta[:, None], sample=i * 0, token=i)[0] is None
    tr = (v.view(torch.int32) & ~0xFFFF).view(torch.float32).to(bf)
    assert E.check_rows("euler", tr[:, None], want[:, None], bound[:, None], delta[:, None], sample=i * 0, token=i)[0] is not None


# ---------------------------------------------------------------------------------------------------------------- qkv_split
def qkv_split_standin(rows, nq, nk, cos, sin, B, S, H, Spad, fault=None):
    """x2i_qkv_split_bf16 with S0 = 0: norm_rope8 in f32, V^T zero-filled to 64-token tiles; fault vt_pad: the transpose tiles run to Spad"""
    HD = H * 128
    Q = E.poison_(torch.empty((B, H, Spad, 128), dtype=bf))
    K, VT = E.poison_(torch.empty_like(Q)), E.poison_(torch.empty((B, H, 128, Spad), dtype=bf))
    for sec, nw, out in ((0, nq, Q), (1, nk, K)):
        x = rows[:, :, sec * HD:(sec + 1) * HD].float().view(B, S, H, 128)
        ss = (x * x).sum(-1, keepdim=True)
        r = torch.rsqrt(ss / 128 + 1e-6)
        y = x * r * nw.float()
        c, s = cos[None, :, None, :], sin[None, :, None, :]
        o = torch.empty_like(y)
        o[..., 0::2] = y[..., 0::2] * c[..., 0::2] - y[..., 1::2] * s[..., 0::2]
        o[..., 1::2] = y[..., 1::2] * c[..., 1::2] + y[..., 0::2] * s[..., 1::2]
        out[:, :, :S] = o.to(bf).permute(0, 2, 1, 3)
    end = Spad if fault == "vt_pad" else E.vt_zero_end(S)
    VT[..., :end] = 0
    VT[..., :S] = rows[:, :, 2 * HD:].view(B, S, H, 128).permute(0, 2, 3, 1)
    return Q, K, VT


def test_qkv_split_checker():
    g = torch.Generator().manual_seed(6)
    B, S, H, Spad = 2, 70, 2, 256
    rows = torch.randn((B, S, 3 * H * 128), generator=g).to(bf)
    nq, nk = (1 + 0.1 * torch.randn(128, generator=g)).to(bf), (1 + 0.1 * torch.randn(128, generator=g)).to(bf)
    ang = torch.randn((S, 64), generator=g).repeat_interleave(2, -1) * 3
    cos, sin = torch.cos(ang), torch.sin(ang)
    Q, K, VT = qkv_split_standin(rows, nq, nk, cos, sin, B, S, H, Spad)
    assert E.check_qkv_split(E.Report("qkv_split"), rows, None, None, nq, nk, cos, sin, Q, K, VT, S=S, S0=0, H=H).done() < 1.0
    E.check_qkv_split_padding("qkv_split", Q, K, VT, S)
    Q, K, VT = qkv_split_standin(rows, nq, nk, cos, sin, B, S, H, Spad, fault="vt_pad")
    with pytest.raises(AssertionError, match=r"V\^T padding position 128 written"):
        E.check_qkv_split_padding("qkv_split", Q, K, VT, S)
