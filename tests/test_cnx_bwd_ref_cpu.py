"""The checker of tests/cnx_bwd_ref.py checked, on the CPU.

Stand-ins: an f32 one-pass evaluation in torch that follows the kernels' order (csrc/conv_bwd.hip: a thread's pixels of a chunk, the block's
rows, reduce_rows' sixteen strided chains, the group's channels and the samples in order, fmas through float64), and a one-pass evaluation
with another summation order (torch's f32 sums).  Both stay inside every bound for every operand kind and shape of the GPU module's list:
this is what "derived, not tuned" rests on.  The largest share is printed.

Planted faults: each is rejected by the new check with a message that names the place; which of the old whole-tensor assertions of
tests/test_controlnext_train_gpu.py (cnx_bwd_ref.OLD_*) accept it is printed.

Also: the undecided-element cap of every (case, kind) the GPU module runs, from the reference alone; the Python restatements of gn_plan and
stem_plan against the workspace queries of the built library."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import cnx_bwd_ref as R
from tests.conv_ref import GN_KINDS
from tests.gemm_ref import ACT_NONE, ACT_RELU, ACT_SILU

F32 = torch.float32
STEM_SHAPES = [(1, 8, 8, 64), (3, 50, 36, 64), (2, 51, 37, 64), (2, 51, 37, 32), (1, 128, 130, 64)]
LINEAR_SHAPES = [(1, 1, 1), (3, 24, 16), (8, 128, 256), (9, 40, 50), (2, 128, 256), (2, 256, 256), (2, 256, 128)]


# ---------------------------------------------------------------------------------------------------------------- f32 stand-ins
def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def seq_sum(t, dim):
    s = torch.zeros_like(t.select(dim, 0))
    for k in range(t.shape[dim]):
        s = s + t.select(dim, k)
    return s


def reduce_rows_f32(p):
    """x2i_reduce_rows_f32 over dim 0: sixteen strided chains, then the sixteen in order"""
    return seq_sum(torch.stack([seq_sum(p[w::16], 0) for w in range(min(16, p.shape[0]))]), 0)


def chunk_sum(a, b, pl, order):
    """sum over the pixels of a b (fma; b None: of a) for a, b f32 [B, HW, C] -> [B, C]"""
    if order == "flat":
        return (a * b if b is not None else a).sum(1)
    B, HW, Cc = a.shape
    chunk, nchunk, rows, T = pl["chunk"], pl["nchunk"], pl["rows"], pl["T"]

    def lay(t):                        # pixel p_begin + k rows + r of a chunk -> [B, nchunk, k, r, C]; what is not there adds exact zeros
        t = F.pad(t, (0, 0, 0, nchunk * chunk - HW)).view(B, nchunk, chunk, Cc)
        return F.pad(t, (0, 0, 0, T * rows - chunk)).view(B, nchunk, T, rows, Cc)
    A_, B_ = lay(a), (lay(b) if b is not None else None)
    acc = torch.zeros((B, nchunk, rows, Cc), dtype=F32)
    for k in range(T):
        acc = fma(A_[:, :, k], B_[:, :, k], acc) if b is not None else acc + A_[:, :, k]
    return reduce_rows_f32(seq_sum(acc, 2).transpose(0, 1))


def act_grad_f32(z, act):
    if act == ACT_RELU:
        return (z > 0).float()
    if act == ACT_SILU:
        s = 1.0 / (1.0 + torch.exp(-z))
        return s * (1.0 + z * (1.0 - s))
    return torch.ones_like(z)


def gn_bwd_f32(c, o, order="kernel", fault=None):
    """x2i_groupnorm_nhwc_bwd_bf16 in f32 on the operands o of case c: dict dx bf16, dw, db, dpre f32 (or None)"""
    (B, HW, Cc, G), act = c["shape"], c["act"]
    cg = Cc // G
    pl = R.gn_bwd_plan(B, HW, Cc, G)
    x, g, w, b = o["x"].float(), o["dy"].float(), o["w"].float(), o["b"].float()
    pa = o["pre_add"]
    z = x + pa[:, None, :] if pa is not None else x
    z1 = z
    if fault == "last_pixel":          # the last pixel of the ragged last chunk left out of S1
        assert HW % pl["chunk"]
        z1 = z.clone()
        z1[:, HW - 1] = 0
    m1, m2 = chunk_sum(z1, None, pl, order), chunk_sum(z, z, pl, order)
    n = torch.tensor(float(HW), dtype=F32) * cg
    mean = seq_sum(m1.view(B, G, cg), 2) / n
    var = (seq_sum(m2.view(B, G, cg), 2) / n - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + torch.tensor(1e-5 if fault == "eps" else c["eps"], dtype=F32))
    ch = lambda t: t.repeat_interleave(cg, 1)
    mc, rc = ch(mean), ch(rstd)
    xh = (z - mc[:, None]) * rc[:, None]
    lin = xh if fault == "act_at_xhat" else fma(w, xh, b)
    dz = g * act_grad_f32(lin, act)
    s0, s1 = chunk_sum(dz, None, pl, order), chunk_sum(dz, xh, pl, order)
    a, q = torch.zeros((B, G), dtype=F32), torch.zeros((B, G), dtype=F32)
    for j in range(cg):
        a = fma(w.view(G, cg)[:, j], s0.view(B, G, cg)[:, :, j], a)
        q = fma(w.view(G, cg)[:, j], s1.view(B, G, cg)[:, :, j], q)
    Ac, Qc = ch(a / n), ch(q / n)
    out = dict(dw=None, db=None, dpre=None)
    if pa is not None:
        sxh = (m1 - float(HW) * mc) * rc
        out["dpre"] = rc * (w * s0 - float(HW) * Ac - (0.0 if fault == "dpre_no_q" else Qc * sxh))
    if c["dw"] != "none":
        qs, as_ = seq_sum(s1, 0), seq_sum(s0, 0)
        out["dw"] = qs if o["prev_dw"] is None or fault == "dw_no_prev" else o["prev_dw"] + qs
        out["db"] = as_ if o["prev_db"] is None else o["prev_db"] + as_
    Ad, Qd = Ac.clone(), Qc.clone()
    if fault == "neighbour_group":     # A and Q of group 1 used for the last channel of group 0
        Ad[:, cg - 1], Qd[:, cg - 1] = Ac[:, cg], Qc[:, cg]
    d = rc[:, None] * (w * dz - Ad[:, None] - xh * Qd[:, None])
    if c["in_relu"]:
        d = torch.where((x >= 0) if fault == "mask_ge" else (x > 0), d, torch.zeros_like(d))
    if o["dx_in"] is not None:
        oo = d + o["dx_in"].float()
        if fault == "dx_in_chunk":     # dx_in skipped in chunk 3 of the last sample
            oo[B - 1, 3 * pl["chunk"]:4 * pl["chunk"]] = d[B - 1, 3 * pl["chunk"]:4 * pl["chunk"]]
        d = oo
    out["dx"] = d.to(torch.bfloat16)
    return out


def linear_wgrad_f32(dy, x, act_in, prev_w, prev_b, order="kernel", fault=None):
    a = x / (1.0 + torch.exp(-x)) if act_in == ACT_SILU and fault != "no_silu" else x
    if order == "flat":
        s, sb = dy.T @ a, dy.sum(0)
    else:
        s, sb = torch.zeros((dy.shape[1], x.shape[1]), dtype=F32), torch.zeros(dy.shape[1], dtype=F32)
        for k in range(dy.shape[0]):
            s, sb = fma(dy[k][:, None], a[k][None, :], s), sb + dy[k]
    db = sb if prev_b is None else prev_b + sb
    if fault == "db_slot":             # db written one slot off
        db = torch.cat((torch.zeros(1) if prev_b is None else prev_b[:1], db[:-1]))
    return (s if prev_w is None else prev_w + s), db


def stem_wgrad_f32(x, dy, prev_w, prev_b, order="kernel", fault=None):
    """x2i_conv_stem_wgrad_bf16 in f32: x bf16 [B, H, W, 3], dy bf16 [B, OH, OW, Cout]"""
    B, H, W, _ = x.shape
    Cout = dy.shape[-1]
    pl = R.stem_plan(B, H, W, Cout)
    g = dy.float()
    if fault == "oh_floor":            # OH = H / 2 for (H + 1) / 2: the last output row and column never visited
        g = g.clone()
        g[:, H // 2:], g[:, :, W // 2:] = 0, 0
    if order == "flat":
        dw = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (Cout, 3, 3, 3), g.permute(0, 3, 1, 2), stride=2, padding=1)
        db = g.sum((0, 1, 2))
    else:
        pat = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1, stride=2).transpose(1, 2).reshape(pl["P"], 27)     # (ci, ky, kx)
        pat = torch.cat((pat, torch.ones(pl["P"], 1)), 1)
        T4 = -(-pl["chunk"] // 4)

        def lay(t):
            t = F.pad(t, (0, 0, 0, pl["nblk"] * pl["chunk"] - pl["P"])).view(pl["nblk"], pl["chunk"], -1)
            return F.pad(t, (0, 0, 0, T4 * 4 - pl["chunk"])).view(pl["nblk"], T4, 4, -1)
        G_, P_ = lay(g.reshape(pl["P"], Cout)), lay(pat)
        acc = torch.zeros((pl["nblk"], 4, Cout, 28), dtype=F32)
        for k in range(T4):
            acc = fma(G_[:, k, :, :, None], P_[:, k, :, None, :], acc)
        red = reduce_rows_f32(((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3])
        dw, db = red[:, :27].reshape(Cout, 3, 3, 3), red[:, 27]
    return (dw if prev_w is None else prev_w + dw), (db if prev_b is None else prev_b + db)


# ---------------------------------------------------------------------------------------------------------------- old checks
def old_gn_checks(c, o, got):
    """the assertions of test_groupnorm_bwd_against_float64_autograd on `got` against a float64 reference: {name: passed}"""
    e = R.gn_bwd_expect_case(c, o)
    res = {"rel-L2(dx)": R.rel_l2(got["dx"], e["dx"][0]) < R.OLD_GN_DX_REL_L2}
    if got["dw"] is not None:
        res["rel-L2(dw)"] = R.rel_l2(got["dw"], e["dw"][0]) < R.OLD_GN_DWDB_REL_L2
        res["rel-L2(db)"] = R.rel_l2(got["db"], e["db"][0]) < R.OLD_GN_DWDB_REL_L2
    if got["dpre"] is not None:
        gx = e["dx"][0] - (o["dx_in"].double() if o["dx_in"] is not None else 0.0)
        res["dpre"] = bool(((got["dpre"].double() - e["dpre"][0]).abs() <= R.OLD_GN_DPRE_SCALE * gx.abs().sum(1).max()).all())
    return res


def new_gn_check(c, o, got, name="gn_bwd"):
    return R.check_gn_bwd(name, R.gn_bwd_expect_case(c, o), got["dx"], c["shape"][3], dx_in=o["dx_in"], dw=got["dw"], db=got["db"],
                          dpre=got["dpre"])


def rejected(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    for n in needles:
        assert n in msg, (n, msg)
    return msg


# ---------------------------------------------------------------------------------------------------------------- the stand-ins hold
WORST = {}


@pytest.mark.parametrize("shape", R.GN_BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gn_bwd_standins_stay_inside_every_bound(shape):
    cases = [c for c in R.gn_bwd_cases() if c["shape"] == shape]
    for i, c in enumerate(cases):
        for k, kind in enumerate(GN_KINDS):
            o = R.gn_bwd_operands(c, kind, "tagged" if (i + k) % 2 else "random", 1000 + 31 * i + k)
            for order in ("kernel", "flat"):
                sh = new_gn_check(c, o, gn_bwd_f32(c, o, order), f"{R.case_id(c)} {kind} {order}")
                for key, v in sh.items():
                    WORST[(key, kind, order)] = max(WORST.get((key, kind, order), 0.0), v)
    print("\n  worst share of the allowance so far: " + ", ".join(f"{k[0]}/{k[1]}/{k[2]} {v:.3f}" for k, v in sorted(WORST.items())))


def _linear_operands(B, N, K, seed, acc):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    return rn(B, N), 3.0 * rn(B, K), (rn(N, K) if acc else None), (rn(N) if acc else None)


@pytest.mark.parametrize("B,N,K", LINEAR_SHAPES)
def test_linear_wgrad_standins_stay_inside_every_bound(B, N, K):
    worst = 0.0
    for act in (ACT_NONE, ACT_SILU):
        for acc in (False, True):
            dy, x, pw, pb = _linear_operands(B, N, K, 7 + B + N, acc)
            (ww, wb_), (bw, bb) = R.linear_wgrad_expect(dy, x, act, pw, pb)
            for order in ("kernel", "flat"):
                dw, db = linear_wgrad_f32(dy, x, act, pw, pb, order)
                worst = max(worst, R.check_vec("linear_wgrad dw", dw, ww, wb_, R.where_linear(K)),
                            R.check_vec("linear_wgrad db", db, bw, bb, lambda i: f"db[n={i}]"))
    print(f"\n  linear_wgrad {B, N, K}: worst share {worst:.3f}")


def _stem_operands(B, H, W, Cout, seed, acc, kind="random"):
    gen = torch.Generator().manual_seed(seed)
    x, dy = R.wgrad_operands(kind, B, H, W, 3, (H + 1) // 2, (W + 1) // 2, Cout, 3, 3, gen)
    rn = lambda *s: torch.randn(s, generator=gen)
    return x, dy, (rn(Cout, 3, 3, 3) if acc else None), (rn(Cout) if acc else None)


@pytest.mark.parametrize("B,H,W,Cout", STEM_SHAPES)
def test_stem_wgrad_standins_stay_inside_every_bound(B, H, W, Cout):
    worst = 0.0
    for kind, acc in (("random", False), ("tagged", True)):
        x, dy, pw, pb = _stem_operands(B, H, W, Cout, 11 + H, acc, kind)
        (ww, wb_), (bw, bb) = R.stem_wgrad_expect(x, dy, pw, pb)
        for order in ("kernel", "flat"):
            dw, db = stem_wgrad_f32(x, dy, pw, pb, order)
            worst = max(worst, R.check_vec("stem dw", dw, ww, wb_, R.where_wgrad(3, 3, 3)), R.check_vec("stem db", db, bw, bb, lambda i: f"db[co={i}]"))
    print(f"\n  conv_stem_wgrad {B, H, W, Cout}: worst share {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- planted faults
def _case(shape, act, **kw):
    c = dict(shape=shape, act=act, eps=1e-6 if act == ACT_SILU else 1e-5, in_relu=False, pre=False, dx_in="none", dw="plain")
    c.update(kw)
    return c


# (fault, case, operand kind, what the message must name)
GN_FAULTS = [
    ("last_pixel", _case((3, 65, 8, 1), ACT_SILU, dx_in="sep"), "random", ("sample ", "pixel ", "channel ", "group ")),
    ("neighbour_group", _case((2, 560, 128, 4), ACT_SILU, dx_in="sep", dw="acc"), "random", ("sample ", "pixel ", "channel 31", "group 0")),
    ("dx_in_chunk", _case((2, 560, 64, 2), ACT_RELU, dx_in="sep"), "random", ("sample 1", "pixel ", "channel ", "group ")),
    ("mask_ge", _case((2, 560, 256, 8), ACT_NONE, in_relu=True), "random", ("in_relu", "sample ", "pixel ", "channel ", "group ")),
    ("act_at_xhat", _case((2, 560, 128, 4), ACT_SILU, pre=True, dx_in="sep"), "random", ("sample ", "pixel ", "channel ", "group ")),
    ("dpre_no_q", _case((2, 560, 256, 8), ACT_SILU, pre=True, dx_in="sep"), "random", ("dpre", "sample ", "channel ", "group ")),
    ("eps", _case((2, 70, 1024, 512), ACT_NONE, dx_in="sep", eps=1e-6), "const", ("sample ", "pixel ", "channel ", "group ")),
    ("dw_no_prev", _case((5, 300, 128, 8), ACT_SILU, dw="acc"), "random", ("dw", "channel ", "group ")),
]


@pytest.mark.parametrize("fault,c,kind,needles", GN_FAULTS, ids=[f[0] for f in GN_FAULTS])
def test_planted_groupnorm_bwd_fault_is_rejected(fault, c, kind, needles):
    o = R.gn_bwd_operands(c, kind, "random", 77)
    new_gn_check(c, o, gn_bwd_f32(c, o), "sound")                          # the stand-in without the fault passes
    bad = gn_bwd_f32(c, o, fault=fault)
    msg = rejected(lambda: new_gn_check(c, o, bad, fault), fault, *needles)
    old = old_gn_checks(c, o, bad)
    if kind == "random":                                                  # (the old assertions accept the sound stand-in on their own operand kind)
        assert all(old_gn_checks(c, o, gn_bwd_f32(c, o)).values())
    print(f"\n  {fault}: new check: {msg}\n  {fault}: old assertions: " + ", ".join(f"{k} {'PASSES' if v else 'rejects'}" for k, v in old.items()) +
          ("  -> the old test lets it through" if all(old.values()) else ""))
    if fault in ("last_pixel", "neighbour_group"):                        # wrong in dx alone, and inside the old norm of dx
        assert old["rel-L2(dx)"], old


def test_planted_linear_wgrad_faults_are_rejected():
    B, N, K = 3, 24, 16
    dy, x, pw, pb = _linear_operands(B, N, K, 5, True)
    (ww, wb_), (bw, bb) = R.linear_wgrad_expect(dy, x, ACT_SILU, pw, pb)
    dw, _ = linear_wgrad_f32(dy, x, ACT_SILU, pw, pb, fault="no_silu")
    msg = rejected(lambda: R.check_vec("no_silu dw", dw, ww, wb_, R.where_linear(K)), "no_silu", "dw[n=", "][k=")
    _, db = linear_wgrad_f32(dy, x, ACT_SILU, pw, pb, fault="db_slot")
    msg2 = rejected(lambda: R.check_vec("db_slot db", db, bw, bb, lambda i: f"db[n={i}]"), "db_slot", "db[n=")
    print(f"\n  {msg}\n  {msg2}\n  old assertions: none (x2i_linear_wgrad_f32 had no GPU test)")


def test_planted_stem_wgrad_fault_is_rejected():
    B, H, W, Cout = 2, 51, 37, 64
    x, dy, pw, pb = _stem_operands(B, H, W, Cout, 9, False)
    (ww, wb_), (bw, bb) = R.stem_wgrad_expect(x, dy)
    dw, db = stem_wgrad_f32(x, dy, None, None, fault="oh_floor")
    msg = rejected(lambda: R.check_vec("oh_floor dw", dw, ww, wb_, R.where_wgrad(3, 3, 3)), "oh_floor", "dw[co=", "[ky=")
    rejected(lambda: R.check_vec("oh_floor db", db, bw, bb, lambda i: f"db[co={i}]"), "db[co=")
    mag = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2).abs(), (Cout, 3, 3, 3), dy.double().permute(0, 3, 1, 2).abs(), stride=2, padding=1)
    old_dw = bool(((dw.double() - ww).abs() <= R.old_stem_gamma(B * 26 * 19) * R.u * mag + 1e-30).all())
    old_db = torch.allclose(db.double(), bw, rtol=R.OLD_STEM_DB_RTOL, atol=R.OLD_STEM_DB_ATOL)
    print(f"\n  {msg}\n  old assertions at this shape: dw {'PASSES' if old_dw else 'rejects'}, db {'PASSES' if old_db else 'rejects'} "
          "(the old test never ran an odd H or W)")


# ---------------------------------------------------------------------------------------------------------------- cap, plans
def test_undecided_cap_holds_from_the_reference_alone():
    worst = 0.0
    for i, c in enumerate(R.gn_bwd_cases() + R.RECORDED_RELU_CASES):
        if c["act"] != ACT_RELU:
            continue
        for k, kind in enumerate(GN_KINDS):
            for dyk in ("random", "tagged"):
                o = R.gn_bwd_operands(c, kind, dyk, 100 + 7 * i + k)
                if kind == "const":
                    assert float(o["b"].float().abs().min()) >= R.MIN_RELU_BIAS
                e = R.gn_bwd_expect_case(c, o)
                assert e["undecided"] <= R.UNDECIDED_CAP * e["numel"], (R.case_id(c), kind, e["undecided"], e["numel"])
                worst = max(worst, e["undecided"] / e["numel"])
    print(f"\n  largest undecided share over the ReLU cases: {worst:.2e} (cap {R.UNDECIDED_CAP:g})")


def _q(fn, *args):
    n = C.c_int64(-7)
    rc = fn(*args, C.byref(n))
    return rc, n.value


def test_plans_match_the_workspace_queries():
    from x2i_amd import _lib
    lib = _lib.load()
    for B, HW, Cc, G in R.GN_BWD_SHAPES + [(2, 560, 128, 2), (2, 560, 128, 8), (2, 64 * 64, 128, 4), (2048, 100, 64, 2)]:
        assert _q(lib.x2i_groupnorm_bwd_workspace_floats, B, HW, Cc, G) == (0, R.gn_bwd_plan(B, HW, Cc, G)["ws"]), (B, HW, Cc, G)
    for B, H, W, Cout in STEM_SHAPES + [(2, 1024, 1024, 64), (1, 2, 2, 64), (2, 128, 128, 64)]:
        assert _q(lib.x2i_conv_stem_wgrad_workspace_floats, B, H, W, Cout) == (0, R.stem_plan(B, H, W, Cout)["ws"]), (B, H, W, Cout)
    rows = {R.gn_bwd_plan(*s)["rows"] for s in R.GN_BWD_SHAPES}
    assert rows == {256, 32, 16, 8, 4, 2}
    assert R.gn_bwd_plan(1, 7300, 64, 2)["nchunk"] == 115 and R.gn_bwd_plan(3, 64, 8, 2)["nchunk"] == 1 and R.gn_bwd_plan(3, 65, 8, 1)["nchunk"] == 2
    assert R.gn_bwd_plan(2, 560, 64, 2)["chunk"] == 63 and 560 % 63
