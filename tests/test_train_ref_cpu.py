"""The float64 references and bounds of tests/train_ref.py on the host.  f32 stand-ins that follow the arithmetic order of the kernels of
csrc/train.hip (per-thread chains, the DPP wave sum and the 8-slot LDS sum of block_sums, the wave-per-row butterfly, reduce_rows' 16 waves
of 8 accumulators) pass every bound on every operand kind with a worst share <= 1; each kernel fault below, applied to the stand-in, is
rejected with a message that names the sample and the row -- and for each the whole-tensor rel-L2 check of tests/test_train_gpu.py is
evaluated on the same launch: several slip past it."""
import re

import pytest
import torch

from tests import ew_ref as E
from tests import train_ref as T
from tests.gemm_ref import ACT_GELU_ERF, ACT_GELU_TANH, ACT_SILU
from tests.test_ew_ref_cpu import fma32

bf = torch.bfloat16
LANE = torch.arange(64)


# ---------------------------------------------------------------------------------------------------------------- f32 sums
def block_sums32(acc):
    """block_sums of csrc/train.hip on per-thread values acc f32 [..., nt] (nt % 64 == 0): wave_sum_lane63's DPP order (quad_perm [1,0,3,2],
    [2,3,0,1], row_half_mirror, row_mirror inside the 16-lane rows, then (row 3 + row 2) + (row 1 + row 0) in lane 63), then the 8 LDS slots
    in order (slots of absent waves hold 0)"""
    nw = acc.shape[-1] // 64
    v = acc.reshape(*acc.shape[:-1], nw, 4, 16)
    i = torch.arange(16)
    for x in (1, 2, 7, 15):
        v = v + v[..., i ^ x]
    r = v[..., 15]
    wave = (r[..., 3] + r[..., 2]) + (r[..., 1] + r[..., 0])
    a = torch.zeros(wave.shape[:-1])
    for w in range(8):
        if w < nw:
            a = a + wave[..., w]
    return a


def row_sum32(a, b=None, *, form):
    """f32 sum over the last axis of a (or of a * b by fmaf) as ln_mod_bwd does it.  form 1: thread c owns columns 8 c .. 8 c + 7 (chain of 8),
    block_sums; form 0: lane l owns the 16-byte chunks l + 64 i (chain over i, j), wave_sum's butterfly."""
    D = a.shape[-1]
    nv = D // 8
    nt = 64 * ((nv + 63) // 64)
    pad = (0, nt * 8 - D)
    a = torch.nn.functional.pad(a, pad).reshape(*a.shape[:-1], nt // 64, 64, 8)
    b = None if b is None else torch.nn.functional.pad(b, pad).reshape(a.shape)
    if form == 1:
        acc = torch.zeros(a.shape[:-1])
        for j in range(8):
            acc = acc + a[..., j] if b is None else fma32(a[..., j], b[..., j], acc)
        return block_sums32(acc.reshape(*acc.shape[:-2], nt))
    acc = torch.zeros((*a.shape[:-3], 64))
    for i in range(nt // 64):
        for j in range(8):
            acc = acc + a[..., i, :, j] if b is None else fma32(a[..., i, :, j], b[..., i, :, j], acc)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., LANE ^ o]
    return acc[..., 0]


def butterfly64(acc):
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., LANE ^ o]
    return acc[..., 0]


def failure(rep):
    try:
        rep.done()
    except AssertionError as e:
        return str(e)
    return None


def where_of(msg):
    m = re.search(r"worst at sample (\d+), row \(token\) (\d+), cols (\d+)\.\.(\d+)", msg)
    assert m, msg
    return int(m.group(1)), int(m.group(2))


def idx(n):
    return torch.arange(n)


def check3(rep, got, exp, what=""):
    """got [B, S, N] against (want, bound, delta) [B, S, N]: sample b, row s"""
    B, S, N = got.shape
    want, bound, delta = exp
    smp = idx(B).repeat_interleave(S)
    tok = idx(S).repeat(B)
    rep.check(got.reshape(B * S, N), want.reshape(B * S, N), bound.reshape(B * S, N), delta.reshape(B * S, N), sample=smp, token=tok, what=what)
    return rep


# ---------------------------------------------------------------------------------------------------------------- ln_mod_bwd
def ln_bwd_standin(X, dY, m, dXin, dx0, *, R, scale=True, form=1, fault=None, eps=1e-6):
    """x2i_ln_mod_bwd_bf16 in f32 on X, dY, dXin (or None) bf16 [B, S, D], m f32 [B, D] / [D]; dx0: what dXout held before.  Returns
    (dX bf16 [B, S, D], partial f32 [B, nw, 2, D]).  fault: see LN_FAULTS."""
    B, S, D = X.shape
    x, dy = X.float(), dY.float()
    invD = torch.tensor(1.0 / D, dtype=torch.float32)

    def mean_of(s):
        return s * invD if form == 1 else s / D
    mean = mean_of(row_sum32(x, form=form))[..., None]
    d = x - mean
    if fault == "one_pass":
        var = mean_of(row_sum32(x, x, form=form))[..., None] - mean * mean
    else:
        var = mean_of(row_sum32(d, d, form=form))[..., None]
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    xh = d * rstd
    mm = m[0:1].expand_as(m) if fault == "mult_sample0" else m
    if scale or fault == "affine_as_scale":
        mul = 1.0 + mm
    else:
        mul = mm
    mul = mul.view(B, 1, D) if scale else mul.view(1, 1, D)
    gm = dy * mul
    sg = row_sum32(dy if fault == "mean_before_mult" else gm, form=form)
    mg, mgx = mean_of(sg)[..., None], mean_of(row_sum32(gm, xh, form=form))[..., None]
    t = fma32(-xh, mgx, gm - mg)
    din = torch.zeros_like(x) if (dXin is None or fault == "no_dxin") else dXin.float()
    dx = fma32(rstd, t, din).to(bf)
    nw = (S + R - 1) // R
    part = torch.zeros((B, nw, 2, D))
    for w in range(nw):
        end = min(S, (w + 1) * R)
        rows = list(range(w * R, end))
        if (end - w * R) % 2 == 1:                       # a half-live step of LB_RB = 2 rows
            if fault == "skip_last_ragged":
                dx[:, end - 1] = dx0[:, end - 1]
            if fault == "dead_row_next" and end < S:
                rows.append(end)
        for s in rows:
            part[:, w, 0] = fma32(dy[:, s], xh[:, s], part[:, w, 0])
            part[:, w, 1] = part[:, w, 1] + dy[:, s]
    if fault == "swap_partials":
        part = part.flip(2)
    return dx, part


def ln_bwd_case(kind, B, S, D, seed, *, dy_outlier=False, dxin_scale=1.0, mod_scale=None):
    g = torch.Generator().manual_seed(seed)
    X = E.ln_rows(B * S, D, kind, g, "cpu").view(B, S, D)
    dY = torch.randn((B, S, D), generator=g)
    if dy_outlier:
        ch = torch.randint(0, D, (4,), generator=g)
        dY[..., ch] *= 2.0 ** 9
    m = E.mod_vectors(B * D, kind, g, "cpu").view(B, D) if mod_scale is None else mod_scale * torch.randn((B, D), generator=g)
    dXin = (dxin_scale * torch.randn((B, S, D), generator=g)).to(bf)
    return X, dY.to(bf), m, dXin


def ln_bwd_check(X, dY, m, dXin, dx, part, *, R, scale=True):
    ex, ep = T.ln_mod_bwd_expect(X, dY, m, dXin, R=R, mult_is_scale=scale)
    rep = check3(E.Report("ln_mod_bwd"), dx, ex, " dX")
    B, nw = part.shape[:2]
    check3(rep, part.reshape(B, nw, -1), tuple(v.reshape(B, nw, -1) for v in ep), " partial")
    return rep


def ln_old_catches(X, dY, m, dXin, dx, part, *, R, scale=True):
    """the check of test_ln_modulate_backward_vs_autograd: rel-L2 of dX and of the two reduced column sums"""
    ex, ep = T.ln_mod_bwd_expect(X, dY, m, dXin, R=R, mult_is_scale=scale)
    return (T.rel_l2(dx, ex[0]) >= T.OLD_LN_BWD_DX_REL_L2 or T.rel_l2(part.sum(1)[:, 0], ep[0].sum(1)[:, 0]) >= T.OLD_LN_BWD_PARTIAL_REL_L2 or
            T.rel_l2(part.sum(1)[:, 1], ep[0].sum(1)[:, 1]) >= T.OLD_LN_BWD_PARTIAL_REL_L2)


LN_SHAPES = [(2, 21, 520, 5), (3, 7, 256, 1), (2, 11, 1024, 3), (2, 9, 1024, 16)]


@pytest.mark.parametrize("kind", E.LN_KINDS)
@pytest.mark.parametrize("form", [1, 0])
def test_ln_bwd_standin_passes(kind, form):
    worst = 0.0
    for j, (B, S, D, R) in enumerate(LN_SHAPES):
        X, dY, m, dXin = ln_bwd_case(kind, B, S, D, 11 * j + E.LN_KINDS.index(kind), dy_outlier=j == 0)
        for din in (dXin, None):
            dx, part = ln_bwd_standin(X, dY, m, din, E.poison_(torch.empty_like(X)), R=R, form=form)
            worst = max(worst, ln_bwd_check(X, dY, m, din, dx, part, R=R).done())
        if j == 2:                                       # an affine LayerNorm weight
            dx, part = ln_bwd_standin(X, dY, m[0], None, None, R=R, scale=False, form=form)
            worst = max(worst, ln_bwd_check(X, dY, m[0], None, dx, part, R=R, scale=False).done())
    assert worst <= 1.0, worst


def test_ln_bwd_const_rows_are_exact():
    B, S, D, R = 2, 9, 3072, 3
    X, dY, m, dXin = ln_bwd_case("const", B, S, D, 5)
    ex, ep = T.ln_mod_bwd_expect(X, dY, m, None, R=R)
    assert T.const_mean_err(D) == 0.0 and T.const_mean_err(520) == 0.0
    for form in (1, 0):
        dx, part = ln_bwd_standin(X, dY, m, None, None, R=R, form=form)
        rows = torch.arange(B * S).view(B, S) % 3 == 0
        g = dY.double() * (1 + m.double())[:, None]
        rstd = 1.0 / (E.f32(1e-6)) ** 0.5
        plain = rstd * (g - g.mean(-1, keepdim=True))    # xhat = 0: dx = rstd (g - mean g)
        assert float((ex[0][rows] - plain[rows]).abs().max()) < 1e-9 * float(plain.abs().max())
        assert ln_bwd_check(X, dY, m, None, dx, part, R=R).done() <= 1.0
    assert bool((ep[2][:, :, 1] > 0).all()) and float(T.ln_mod_bwd_expect(X, dY, m, None, R=1)[1][2][:, :, 1].max()) == 0.0


# fault, operand kind, (B, S, D, R), affine, whether the old rel-L2 check misses it
LN_FAULTS = [("one_pass", "large_mean", (2, 21, 520, 5), False, True),       # 1 % of rstd, diluted by a dXin of the same size as dX
             ("skip_last_ragged", "random", (1, 4607, 256, 8), False, True),      # the single-row fault, at a training step's row count
             ("dead_row_next", "random", (2, 21, 520, 5), False, False),
             ("mult_sample0", "random", (2, 21, 520, 5), False, True),            # the wrong-sample fault (see ln_fault_case)
             ("mean_before_mult", "mod_edge", (2, 21, 520, 5), False, False),
             ("no_dxin", "random", (2, 21, 520, 5), False, False),
             ("swap_partials", "random", (2, 21, 520, 5), False, False),
             ("affine_as_scale", "random", (2, 21, 520, 5), True, False)]


def ln_fault_case(fault, kind, shape):
    B, S, D, R = shape
    if fault == "mult_sample0":
        # the residual-stream gradient after many blocks of the backward chain is an order of magnitude above one LayerNorm's own term, and
        # FLUX's scale modulations are around 0.1: the sample mix-up changes dX by 6e-3 of its norm
        return ln_bwd_case(kind, B, S, D, 3, dxin_scale=8.0, mod_scale=0.1)
    return ln_bwd_case(kind, B, S, D, 3)


@pytest.mark.parametrize("fault,kind,shape,affine,old_misses", LN_FAULTS, ids=[f[0] for f in LN_FAULTS])
def test_ln_bwd_fault_rejected(fault, kind, shape, affine, old_misses):
    B, S, D, R = shape
    X, dY, m, dXin = ln_fault_case(fault, kind, shape)
    mm = m[0] if affine else m
    dx0 = dXin.clone()                                   # dXin aliases dXout
    good = ln_bwd_standin(X, dY, mm, dXin, dx0, R=R, scale=not affine)
    assert ln_bwd_check(X, dY, mm, dXin, *good, R=R, scale=not affine).done() <= 1.0
    dx, part = ln_bwd_standin(X, dY, mm, dXin, dx0, R=R, scale=not affine, fault=fault)
    msg = failure(ln_bwd_check(X, dY, mm, dXin, dx, part, R=R, scale=not affine))
    assert msg is not None, fault
    b, s = where_of(msg)
    assert 0 <= b < B and 0 <= s < S
    if fault == "skip_last_ragged":
        assert (b, s) == (0, S - 1) and "dX" in msg and msg.endswith("[1 failing rows in the launch]"), msg
    if fault == "mult_sample0":
        assert b >= 1 and "samples [1]" in msg, msg
    if fault in ("dead_row_next", "swap_partials"):
        assert "partial" in msg, msg
    assert ln_old_catches(X, dY, mm, dXin, dx, part, R=R, scale=not affine) == (not old_misses), fault


# ---------------------------------------------------------------------------------------------------------------- gate_bwd
def gate_bwd_standin(dX, Tt, gate, G, *, S, R, fault=None):
    """x2i_gate_bwd_bf16 on the first S rows of [B, St, D] buffers: (dT bf16 [B, S, D], partial [B, nw, D] or None)"""
    B, St, D = dX.shape
    d = dX.float()[:, :S]
    gt = torch.ones((B, 1, D)) if gate is None else (gate[0:1].expand_as(gate) if fault == "gate_sample0" else gate).view(B, 1, D)
    o = torch.zeros_like(d) if G is None else G.float()[:, :S].clone()
    nw = (S + R - 1) // R
    if fault == "drop_G_ragged" and S % R:
        o[:, (nw - 1) * R:] = 0
    dT = fma32(gt, d, o).to(bf)
    if gate is None:
        return dT, None
    part = torch.zeros((B, nw, D))
    for w in range(nw):
        end = min(St, (w + 1) * R) if fault == "partial_past_S" else min(S, (w + 1) * R)
        for s in range(w * R, end):
            part[:, w] = fma32(dX.float()[:, s], Tt.float()[:, s], part[:, w])
    return dT, part


def gate_check(dX, Tt, gate, G, dT, part, *, S, R):
    sl = lambda v: None if v is None else v[:, :S]
    et, ep = T.gate_bwd_expect(sl(dX), sl(Tt), gate, sl(G), R=R)
    rep = check3(E.Report("gate_bwd"), dT, et, " dT")
    if ep is not None:
        check3(rep, part, ep, " partial")
    return rep


def gate_case(B=3, St=40, D=520, seed=9):
    g = torch.Generator().manual_seed(seed)
    return (tuple(torch.randn((B, St, D), generator=g).to(bf) for _ in range(3)) + (torch.randn((B, D), generator=g),))


@pytest.mark.parametrize("S,R", [(37, 8), (37, 3), (9, 16), (40, 5)])
def test_gate_bwd_standin_passes(S, R):
    dX, Tt, G, gate = gate_case()
    worst = 0.0
    for gt, gg in ((gate, G), (gate, None), (None, G), (None, None)):
        dT, part = gate_bwd_standin(dX, Tt, gt, gg, S=S, R=R)
        worst = max(worst, gate_check(dX, Tt, gt, gg, dT, part, S=S, R=R).done())
    assert worst <= 1.0
    ex = T.gate_bwd_expect(dX, None, None, None, R=R)[0]
    assert float(ex[2].max()) == 0.0                     # the plain copy is exact


GATE_FAULTS = [("drop_G_ragged", False), ("gate_sample0", False), ("partial_past_S", False)]


@pytest.mark.parametrize("fault,old_misses", GATE_FAULTS, ids=[f[0] for f in GATE_FAULTS])
def test_gate_bwd_fault_rejected(fault, old_misses):
    S, R = 37, 8
    dX, Tt, G, gate = gate_case()
    dT, part = gate_bwd_standin(dX, Tt, gate, G, S=S, R=R, fault=fault)
    msg = failure(gate_check(dX, Tt, gate, G, dT, part, S=S, R=R))
    assert msg is not None, fault
    b, s = where_of(msg)
    if fault == "drop_G_ragged":
        assert s >= 32 and msg.endswith(f"[{3 * 5} failing rows in the launch]"), msg
    if fault == "gate_sample0":
        assert b >= 1 and "samples [1, 2]" in msg, msg
    if fault == "partial_past_S":
        assert "partial" in msg and s == 4, msg           # the last row group
    et, ep = T.gate_bwd_expect(dX[:, :S], Tt[:, :S], gate, G[:, :S], R=R)
    old = T.rel_l2(dT, et[0]) >= T.OLD_GATE_BWD_REL_L2 or T.rel_l2(part.sum(1), ep[0].sum(1)) >= T.OLD_GATE_BWD_REL_L2
    assert old == (not old_misses), fault


# ---------------------------------------------------------------------------------------------------------------- reduce_rows
def reduce_standin(inp, *, alpha=1.0, old=None, fault=None):
    """reduce_rows_kernel on inp f32 [nz, np, len]: 16 waves, wave w takes rows w, w + 16, ..: the 8-deep unrolled loop while
    k + 112 < np, then single rows; a 3-level tree; the 16 wave sums added in order.  fault: tail16 (rows from 16 (np // 16) on skipped),
    tail128 (the rows behind the unrolled loop skipped once it has run), alpha_old (alpha applied to the old value too)."""
    nz, np_, n = inp.shape
    t = torch.zeros((nz, n))
    a = torch.tensor(alpha, dtype=torch.float32)
    for w in range(16):
        acc = [torch.zeros((nz, n)) for _ in range(8)]
        k = w
        unrolled = False
        while k + 7 * 16 < np_:
            for q in range(8):
                acc[q] = acc[q] + inp[:, k + q * 16]
            k += 128
            unrolled = True
        while k < np_:
            if not ((fault == "tail128" and unrolled) or (fault == "tail16" and k >= 16 * (np_ // 16))):
                acc[0] = acc[0] + inp[:, k]
            k += 16
        t = t + (((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])))
    if old is None:
        return a * t
    return a * (old + t) if fault == "alpha_old" else fma32(a, t, old)


def reduce_check(inp, out, *, alpha=1.0, old=None):
    nz = inp.shape[0]
    want, bound, delta = T.reduce_rows_expect(inp, alpha=alpha, old=old)
    rep = E.Report("reduce_rows")
    rep.check(out, want, bound, delta, sample=idx(nz), token=idx(nz) * 0, unit=1)
    return rep


def reduce_case(nz, np_, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    inp = torch.randn((nz, np_, n), generator=g)
    inp[:, :, 0] = torch.where(idx(np_)[None] % 2 == 0, 1.0, -1.0) * (1 + 2.0 ** -12 * torch.randn((nz, np_), generator=g))   # cancels
    return inp, torch.randn((nz, n), generator=g)


@pytest.mark.parametrize("np_", [1, 15, 16, 17, 112, 113, 128, 129, 241, 576])
def test_reduce_standin_passes(np_):
    inp, old = reduce_case(3, np_, 65)
    w1 = reduce_check(inp, reduce_standin(inp)).done()
    w2 = reduce_check(inp, reduce_standin(inp, alpha=0.375, old=old), alpha=0.375, old=old).done()
    assert max(w1, w2) <= 1.0


# fault, np, whether the old check (the np <= 7 launches of test_train_gpu.py, rel-L2 5e-3) misses it
REDUCE_FAULTS = [("tail16", 129, False), ("tail128", 241, True), ("tail128", 576, True),
                 ("alpha_old", 17, True)]                # (the old launches accumulate with alpha = 1)


@pytest.mark.parametrize("fault,np_,old_misses", REDUCE_FAULTS, ids=[f"{f[0]}-{f[1]}" for f in REDUCE_FAULTS])
def test_reduce_fault_rejected(fault, np_, old_misses):
    inp, old = reduce_case(2, np_, 65)
    acc = dict(alpha=0.375, old=old) if fault == "alpha_old" else {}
    assert reduce_check(inp, reduce_standin(inp, **acc), **acc).done() <= 1.0
    msg = failure(reduce_check(inp, reduce_standin(inp, fault=fault, **acc), **acc))
    assert msg is not None and "worst at sample" in msg, fault
    # the old tests reduce np = 3, 5, 7 partial rows (the row groups of their three shapes), accumulating with alpha = 1
    caught = False
    for n_old in (3, 5, 7):
        i2, o2 = reduce_case(2, n_old, 65, seed=n_old)
        kw = dict(alpha=1.0, old=o2 * 0)
        want = T.reduce_rows_expect(i2, **kw)[0]
        caught |= T.rel_l2(reduce_standin(i2, fault=fault, **kw), want) >= T.OLD_LN_BWD_PARTIAL_REL_L2
    assert caught == (not old_misses), fault


# ---------------------------------------------------------------------------------------------------------------- softmax
def lane_chain(a, b=None):
    """sum over the last axis (a multiple of 8 wide) as the one-wave-per-row kernels: lane l chains the chunks l + 64 i, then the butterfly"""
    n = a.shape[-1]
    nc = n // 8
    tot = 64 * ((nc + 63) // 64) * 8
    a = torch.nn.functional.pad(a, (0, tot - n)).reshape(*a.shape[:-1], tot // 512, 64, 8)
    b = None if b is None else torch.nn.functional.pad(b, (0, tot - n)).reshape(a.shape)
    acc = torch.zeros((*a.shape[:-3], 64))
    for i in range(a.shape[-3]):
        for j in range(8):
            acc = acc + a[..., i, :, j] if b is None else fma32(a[..., i, :, j], b[..., i, :, j], acc)
    return butterfly64(acc)


def softmax_standin(x, Cv, scale):
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    v = x.float()
    mask = idx(x.shape[-1]) < Cv
    mx = torch.where(mask, v, torch.tensor(-3.0e38)).amax(-1, keepdim=True) * sl2
    e = torch.where(mask, torch.exp2(v * sl2 - mx), torch.tensor(0.0))
    inv = 1.0 / lane_chain(e)[..., None]
    return (e * inv).to(bf)


def softmax_bwd_standin(P, dP, Cv, scale, fault=None):
    p, g = P.float(), dP.float()
    mask = (idx(P.shape[-1]) < Cv).float()
    dot = lane_chain(p if fault == "dot_past_cv" else p * mask, g)[..., None]
    out = torch.where(mask.bool(), (torch.tensor(scale, dtype=torch.float32) * p) * (g - dot), g if fault == "pad_nonzero" else torch.tensor(0.0))
    return out.to(bf)


SM_SHAPES = [(16, 128, 100), (8, 640, 513), (4, 1024, 1024), (5, 64, 1)]


def softmax_case(rows, Ct, seed):
    g = torch.Generator().manual_seed(seed)
    x = (10.0 * torch.randn((rows, Ct), generator=g)).clamp(-30, 30)
    x[:, 0] = 30.0                                       # one column dominates
    return x.to(bf), torch.randn((rows, Ct), generator=g).to(bf)


@pytest.mark.parametrize("rows,Ct,Cv", SM_SHAPES)
def test_softmax_standins_pass(rows, Ct, Cv):
    x, dP = softmax_case(rows, Ct, Ct + Cv)
    smp, tok = idx(rows) * 0, idx(rows)
    for scale in (0.3, 1.0):
        P = softmax_standin(x, Cv, scale)
        rep = E.Report("softmax_pad")
        rep.check(P[:, :Cv], *T.softmax_pad_expect(x, Cv, scale), sample=smp, token=tok)
        assert rep.done() <= 1.0
        Pg = P.clone()
        Pg[:, Cv:] = 0.5                                 # what P holds beyond Cv must not matter
        dS = softmax_bwd_standin(Pg, dP, Cv, scale)
        rep = E.Report("softmax_bwd")
        rep.check(dS[:, :Cv], *T.softmax_bwd_expect(Pg, dP, Cv, scale), sample=smp, token=tok)
        assert rep.done() <= 1.0 and bool((dS[:, Cv:].view(torch.int16) == 0).all())


@pytest.mark.parametrize("fault", ["dot_past_cv", "pad_nonzero"])
def test_softmax_bwd_fault_rejected(fault):
    rows, Ct, Cv, scale = 16, 128, 100, 0.3
    x, dP = softmax_case(rows, Ct, 3)
    P = softmax_standin(x, Cv, scale)
    P[:, Cv:] = 0.5
    dS = softmax_bwd_standin(P, dP, Cv, scale, fault)
    buf = dS.clone().view(1, rows, Ct)
    if fault == "pad_nonzero":
        with pytest.raises(AssertionError, match=r"padding column not \+0: sample 0, row \d+, cols 10\d"):
            T.check_softmax_layout("softmax_bwd", buf, 1, rows, rows, Ct, Cv, Ct)
        return
    rep = E.Report("softmax_bwd")
    rep.check(dS[:, :Cv], *T.softmax_bwd_expect(P, dP, Cv, scale), sample=idx(rows) * 0, token=idx(rows))
    msg = failure(rep)
    assert msg is not None and where_of(msg)[0] == 0
    # the old check: rel-L2 5e-3 against the same formula -- on a P whose padding is zero, where this fault changes nothing
    P0 = P.clone()
    P0[:, Cv:] = 0
    old = T.rel_l2(softmax_bwd_standin(P0, dP, Cv, scale, fault)[:, :Cv], T.softmax_bwd_expect(P0, dP, Cv, scale)[0])
    assert old < T.OLD_SOFTMAX_REL_L2


# ---------------------------------------------------------------------------------------------------------------- act_bwd
def act_grad32(x, act):
    if act == ACT_GELU_TANH:
        k = torch.tensor(0.7978845608028654, dtype=torch.float32)
        t = torch.tanh(k * (x + 0.044715 * x * x * x))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * k * (1.0 + 3.0 * 0.044715 * x * x)
    if act == ACT_GELU_ERF:
        return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    sg = 1.0 / (1.0 + torch.exp(-x))
    return sg * (1.0 + x * (1.0 - sg))


def act_grid():
    """pre over [-12, 12] on the bf16 grid plus +-0, +-2^-20, +-100"""
    g = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(bf).float()
    g = g[torch.isfinite(g) & (g.abs() <= 12)]
    return torch.cat((g, torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 100.0, -100.0]))).to(bf)


@pytest.mark.parametrize("act", [ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU])
def test_act_bwd_standin_passes_and_sign_flip_rejected(act):
    pre = act_grid()
    n = pre.numel()
    g = torch.Generator().manual_seed(act)
    dA = torch.randn(n, generator=g).to(bf)
    for f32out in (False, True):
        d, p = (dA.float(), pre.float()) if f32out else (dA, pre)
        got = d.float() * act_grad32(p.float(), act)
        got = got if f32out else got.to(bf)
        want, bound, delta = T.act_bwd_expect(d, p, act, out_f32=f32out)
        rep = E.Report("act_bwd")
        rep.check(got[:, None], want[:, None], bound[:, None], delta[:, None], sample=idx(n) * 0, token=idx(n), unit=1)
        assert rep.done() <= 1.0
        bad = d.float() * act_grad32(-p.float(), act)     # act'(-x)
        rep = E.Report("act_bwd")
        rep.check(bad[:, None] if f32out else bad.to(bf)[:, None], want[:, None], bound[:, None], delta[:, None], sample=idx(n) * 0, token=idx(n),
                  unit=1)
        assert failure(rep) is not None


# ---------------------------------------------------------------------------------------------------------------- qkv_split_bwd
def qkv_bwd_standin(rows, dy, nw, c, s, H, fault=None):
    """dq / dk rows in f32: rows bf16 [m, H 128], dy bf16 [m, H, 128], c / s f32 [m, 128]; 16 lanes of 8 elements per head"""
    m = rows.shape[0]
    x, g, w = rows.float().view(m, H, 128), dy.float(), nw.float().view(1, 1, 128)
    c, s = c.view(m, 1, 128), s.view(m, 1, 128)
    ge, go = g[..., 0::2], g[..., 1::2]
    dn = torch.empty_like(g)
    if fault == "rope_forward":
        dn[..., 0::2] = ge * c[..., 0::2] - go * s[..., 0::2]
        dn[..., 1::2] = go * c[..., 1::2] + ge * s[..., 1::2]
    else:
        dn[..., 0::2] = ge * c[..., 0::2] + go * s[..., 1::2]
        dn[..., 1::2] = -ge * s[..., 0::2] + go * c[..., 1::2]

    def sum128(v):
        a = v.view(m, H, 16, 8)
        acc = torch.zeros((m, H, 16))
        for j in range(8):
            acc = acc + a[..., j]
        l16 = torch.arange(16)
        for o in (8, 4, 2, 1):
            acc = acc + acc[..., l16 ^ o]
        return acc[..., :1]
    ss, dot = sum128(x * x), sum128(dn * w * x)
    r = torch.rsqrt(ss * (1.0 / 128.0) + 1e-6)
    k = r * r * r * (1.0 if fault == "no_128" else 1.0 / 128.0) * dot
    return (r * w * dn - x * k).to(bf).view(m, H * 128)


def qkv_bwd_case(m=33, H=3, seed=2):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn((m, H * 128), generator=g)
    rows[5] *= 2.0 ** 9                                   # an outlier row
    dy = torch.randn((m, H, 128), generator=g).to(bf)
    nw0, nw1 = ((1 + 0.2 * torch.randn(128, generator=g)).to(bf) for _ in range(2))
    ang = 3.0 * torch.randn((m, 64), generator=g).repeat_interleave(2, -1)
    return rows.to(bf), dy, nw0, nw1, torch.cos(ang), torch.sin(ang)


def test_qkv_split_bwd_standin_and_faults():
    m, H = 33, 3
    rows, dy, nw0, nw1, c, s = qkv_bwd_case(m, H)
    exp = T.qkv_split_bwd_rows(rows, dy, nw0, c.double(), s.double(), H=H)
    smp, tok = idx(m) * 0, idx(m)

    def run(got):
        rep = E.Report("qkv_split_bwd")
        rep.check(got, *exp, sample=smp, token=tok, unit=128)
        return rep
    assert run(qkv_bwd_standin(rows, dy, nw0, c, s, H)).done() <= 1.0
    for fault, got in (("rope_forward", qkv_bwd_standin(rows, dy, nw0, c, s, H, "rope_forward")),
                       ("wrong_weight", qkv_bwd_standin(rows, dy, nw1, c, s, H)),
                       ("no_128", qkv_bwd_standin(rows, dy, nw0, c, s, H, "no_128"))):
        msg = failure(run(got))
        assert msg is not None and "worst at sample 0, row (token)" in msg, fault
        assert T.rel_l2(got, exp[0]) >= T.OLD_QKV_BWD_REL_L2, fault      # (the old rel-L2 check catches these three too)


# ---------------------------------------------------------------------------------------------------------------- kd_loss
def kd_standin(t, s, temp, ls, fault=None):
    """kd_loss_kernel in f32 (one wave per row): (row_loss f32 [rows], grad bf16 [rows, D])"""
    D = t.shape[-1]
    t, s = t.float(), s.float()
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temp, dtype=torch.float32)
    ls = torch.tensor(ls, dtype=torch.float32)
    out = []
    for x in (t, s):
        x = x - (lane_chain(x) / D)[..., None]
        sd = torch.sqrt(lane_chain(x, x) / (D if fault == "biased_std" else D - 1))[..., None]
        c = 1.0 / (torch.tensor(1e-7, dtype=torch.float32) + sd)
        k = c * inv_t
        z = x * k
        mx = z.amax(-1, keepdim=True)
        lse = mx + torch.log(lane_chain(torch.exp(z - mx)))[..., None]
        out.append((x, sd, c, z - lse))
    (_, _, _, lq), (us, sds, cs, lp) = out
    p = torch.exp(lp)
    d = lp - lq
    rl = lane_chain(p, d)[..., None]
    dsh = p * (d - rl) * inv_t
    md = (lane_chain(dsh) / D)[..., None]
    kk = torch.where(sds > 0, cs * cs * lane_chain(dsh, us)[..., None] / ((D - 1) * sds), torch.tensor(0.0))
    if fault == "no_second_term":
        kk = kk * 0
    return rl[..., 0], (ls * (cs * (dsh - md) - kk * us)).to(bf)


def kd_case(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    t = 0.7 * torch.randn((rows, D), generator=g)
    s = 0.9 * torch.randn((rows, D), generator=g) + 0.3 * t
    if rows >= 5:
        s[1] = 0.75                                      # constant student
        t[2] = -1.5                                      # constant teacher
        s[3, 7] = 2.0 ** 12                              # one outlier
    return t.to(bf), s.to(bf)


def kd_check(t, s, temp, ls, rl, grad):
    rows = t.shape[0]
    el, eg = T.kd_loss_expect(t, s, temp, ls)
    rep = E.Report("kd_loss")
    rep.check(rl[:, None], *(v[:, None] for v in el), sample=idx(rows) * 0, token=idx(rows), unit=1, what=" row loss")
    rep.check(grad, *eg, sample=idx(rows) * 0, token=idx(rows), what=" grad")
    return rep


@pytest.mark.parametrize("rows,D", [(1, 256), (5, 3072), (7, 4096)])
@pytest.mark.parametrize("temp", [1.0, 3.0])
def test_kd_standin_passes(rows, D, temp):
    t, s = kd_case(rows, D, rows + D)
    rl, grad = kd_standin(t, s, temp, 0.25)
    assert kd_check(t, s, temp, 0.25, rl, grad).done() <= 1.0
    assert bool(torch.isfinite(T.kd_loss_expect(t, s, temp, 0.25)[1][0]).all())


def test_kd_reference_is_the_stated_formula():
    """normalize (unbiased std, 1e-7 +), softmax(z / T), KL(teacher || student): autograd of x2i_amd/distill.py's formula in float64"""
    import torch.nn.functional as F
    from x2i_amd.distill import normalize
    t, s = kd_case(1, 256, 4)
    t2, s2 = torch.cat((t, t)), torch.cat((s, s * 1.5 + 0.25))
    sr = s2.double().requires_grad_(True)
    term = F.kl_div(F.softmax(normalize(t2.double()) / 3.0, dim=-1).log(), F.softmax(normalize(sr) / 3.0, dim=-1), reduction="sum")
    (0.25 * term).backward()
    el, eg = T.kd_loss_expect(t2, s2, 3.0, 0.25)
    assert abs(float(el[0].sum()) - float(term.detach())) < 1e-6 * abs(float(term.detach()))      # (1e-7 as its f32 value, 1 / T as f32: 1e-7 relative)
    assert T.rel_l2(eg[0], sr.grad) < 1e-6


@pytest.mark.parametrize("fault", ["biased_std", "no_second_term"])
def test_kd_fault_rejected(fault):
    t, s = kd_case(5, 3072, 1)
    rl, grad = kd_standin(t, s, 3.0, 0.25, fault)
    msg = failure(kd_check(t, s, 3.0, 0.25, rl, grad))
    assert msg is not None and "worst at sample 0, row (token)" in msg, fault
    old = T.rel_l2(grad, T.kd_loss_expect(t, s, 3.0, 0.25)[1][0])
    assert old < T.OLD_KD_GRAD_REL_L2, (fault, old)      # both slip past the old 1e-2: 1 / D against 1 / (D - 1) is 1.6e-4 of the gradient,
    #                                                      the second term 1.6e-3


# ---------------------------------------------------------------------------------------------------------------- skinny_bwd, conv5x5_wgrad, sums
def skinny_bwd_standin(dy, W, N, chunk, fault=None):
    """skinny_bwd_kernel on the first N rows of W [Np, K] / columns of dy [B, Np]: partial f32 [nchunk, B, K]"""
    B, K = dy.shape[0], W.shape[1]
    nchunk = (N + chunk - 1) // chunk
    part = torch.zeros((nchunk, B, K))
    Wf = W.float()
    for i in range(nchunk):
        hi = min(W.shape[0], (i + 1) * chunk) if fault == "past_N" else min(N, (i + 1) * chunk)
        for n in range(i * chunk, hi):
            part[i] = fma32(dy[:, n:n + 1], Wf[n][None], part[i])
    return part


@pytest.mark.parametrize("B,N,K,chunk", [(1, 100, 8, 1000), (3, 257, 136, 256), (8, 70, 264, 30)])
def test_skinny_bwd_standin_and_fault(B, N, K, chunk):
    g = torch.Generator().manual_seed(N)
    Np = N + 5
    dy, W = torch.randn((B, Np), generator=g), (0.05 * torch.randn((Np, K), generator=g)).to(bf)
    ep, eo = T.skinny_bwd_expect(dy[:, :N], W[:N], chunk)
    nchunk = ep[0].shape[0]

    def check(part):
        rep = E.Report("skinny_bwd")
        rep.check(part.reshape(nchunk * B, K), *(v.reshape(nchunk * B, K) for v in ep), sample=idx(nchunk * B) % B, token=idx(nchunk * B) // B,
                  what=" partial")
        out = reduce_standin(part.reshape(1, nchunk, B * K)).view(B, K)
        rep.check(out, *eo, sample=idx(B), token=idx(B) * 0, what=" reduced")
        return rep
    assert check(skinny_bwd_standin(dy, W, N, chunk)).done() <= 1.0
    if N % chunk:
        msg = failure(check(skinny_bwd_standin(dy, W, N, chunk, "past_N")))
        assert msg is not None and f"row (token) {nchunk - 1}" in msg, msg       # the last chunk
        bad = reduce_standin(skinny_bwd_standin(dy, W, N, chunk, "past_N").reshape(1, nchunk, B * K)).view(B, K)
        assert T.rel_l2(bad, eo[0]) >= T.OLD_SKINNY_BWD_REL_L2


def conv_wgrad_standin(x, dy, S, fault=None):
    """conv5x5_wgrad_kernel + reduce_rows on the first S rows of the planes x bf16 [B, C, Sp, H], dy bf16 [B, Sp, H] (the planes are S rows
    high for the kernel: rows >= S exist only for the fault that reads them): dw f32 [C, 25]"""
    B, C, Sp, H = x.shape
    nh, nchunk = H // 8, (S + 15) // 16
    xf = torch.zeros((B, C, nchunk * 16 + 4, nh, 8))
    xf[:, :, :Sp] = x.float().view(B, C, Sp, nh, 8)[:, :, :nchunk * 16 + 4]
    dpad = torch.zeros((B, S + 4, H + 16))
    dpad[:, 2:S + 2, 8:H + 8] = dy.float()[:, :S]
    acc = torch.zeros((B, C, nchunk, nh, 25))
    for rr in range(16):
        sp = torch.arange(nchunk) * 16 + rr
        live = (sp < (Sp if fault == "rows_past_S" else S)).float().view(1, 1, nchunk, 1)
        xv = xf[:, :, sp.clamp_max(nchunk * 16 + 3)] * live[..., None]            # [B, C, nchunk, nh, 8]
        for ds in range(5):
            r = sp - ds + 2                                                       # dy row (r in [0, S) else nothing)
            ok = ((r >= 0) & (r < S)).float().view(1, nchunk, 1)
            drow = dpad[:, (r + 2).clamp(0, S + 3)] * ok                          # [B, nchunk, H + 16]
            for dh in range(5):
                for j in range(8):
                    # x[s'][8 hc + j] pairs with dy[r][8 hc + j + 2 - dh]
                    col = torch.arange(nh) * 8 + j + 2 - dh + 8
                    dv = drow[:, :, col]                                          # [B, nchunk, nh]
                    if fault == "edge_pair" and (j + 2 - dh < 0 or j + 2 - dh > 7):
                        dv = dv.clone()
                        dv[:, :, 5 if j + 2 - dh > 7 else 6] = 0                  # the pair between the chunks 5 and 6
                    acc[..., ds * 5 + dh] = fma32(xv[..., j], dv[:, None], acc[..., ds * 5 + dh])
    lanes = torch.zeros((B, C, nchunk, 256, 25))
    assert nh <= 256
    lanes[:, :, :, :nh] = acc
    w4 = lanes.view(B, C, nchunk, 4, 64, 25)
    for o in (32, 16, 8, 4, 2, 1):
        w4 = w4 + w4[..., LANE ^ o, :]
    w4 = w4[..., 0, :]
    part = w4[..., 0, :] + w4[..., 1, :] + w4[..., 2, :] + w4[..., 3, :]          # [B, C, nchunk, 25]
    return reduce_standin(part.permute(1, 0, 2, 3).reshape(C, B * nchunk, 25))


@pytest.mark.parametrize("S", [24, 17])
def test_conv5x5_wgrad_standin_and_faults(S):
    B, C, H = 2, 2, 96
    g = torch.Generator().manual_seed(S)
    x, dy = torch.randn((B, C, S + 3, H), generator=g).to(bf), torch.randn((B, S + 3, H), generator=g).to(bf)
    exp = T.conv5x5_wgrad_expect(x[:, :, :S], dy[:, :S])

    def run(got):
        rep = E.Report("conv5x5_wgrad")
        rep.check(got, *exp, sample=idx(C) * 0, token=idx(C), unit=5)
        return rep
    assert run(conv_wgrad_standin(x, dy, S)).done() <= 1.0
    for fault in ("edge_pair", "rows_past_S"):
        got = conv_wgrad_standin(x, dy, S, fault)
        assert failure(run(got)) is not None, fault
        # the old check: rel-L2 2e-2 of the whole gradient -- one neighbour pair of H / 8 is 1 / 12 of the dh = 0, 1, 3, 4 taps' sums here
        assert (T.rel_l2(got, exp[0]) < T.OLD_PROJ_REL_L2) == (False), fault


def test_sums_and_clip_references():
    g = torch.Generator().manual_seed(8)
    for n in (1, 255, 100003):
        x = torch.randn(n, generator=g)
        for sq in (False, True):
            want, bound, delta = T.sum_all_expect(x, sq)
            ref = (x.double() ** 2).sum() if sq else x.double().sum()
            assert float(want) == float(ref) and float(bound) >= float(delta) > 0
            f32sum = ((x * x) if sq else x).sum()         # any f32 summation order is within the bound
            assert abs(float(f32sum) - float(want)) <= float(bound)
    for ss, mx in ((4.0, 3.0), (4.0, 2.0), (4.0, 1.0), (0.0, 1.0)):
        want, bound, delta = T.clip_coef_expect(torch.tensor([ss]), mx)
        nrm = ss ** 0.5
        assert abs(float(want[0]) - min(1.0, mx / (nrm + 1e-6))) < 1e-12 and float(want[1]) == nrm
        assert (float(delta[0]) == 0.0) == (mx / (nrm + 1e-6) > 1.001)
    x, dy = torch.randn((2, 3, 5, 8), generator=g).to(bf), torch.randn((2, 5, 8), generator=g).to(bf)
    want = T.plane_dot_expect(x, dy, alpha=0.5, nchunk=4)[0]
    assert torch.allclose(want, 0.5 * (x.double() * dy.double()[:, None]).sum((0, 2, 3)))
