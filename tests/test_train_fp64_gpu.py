"""Unit launches of the training backward's row and element kernels (csrc/train.hip) against the float64 references and derived bounds of
tests/train_ref.py: every output element of every launch, NaN fails, elements whose allowance is 0 must be exact, every written buffer starts
as the sentinel (or a saved copy for in-place operators) and everything outside the launch's write set is checked unchanged.

The shapes are the smallest that reach each path of the kernels: ragged and odd row groups (half-live steps of ln_mod_bwd_rows_kernel),
workgroups of 64 .. 512 threads, the wave-per-row fallback (train_rows_wg = 0, or a partial buffer off 16-byte alignment), padded strides
and the offsets of an image-row sub-range of a shared [B, S_total, ld] buffer, reduce_rows' 8-deep loop (np > 112), softmax rows longer than
one 64-lane pass, act_bwd's grid-stride loop, qkv_split_bwd's two-source addressing, skinny_bwd's second column pass and cut chunks, kd_loss
on constant rows.  The worst share of the f32 allowance used per kernel is printed at the end (WORST)."""
import time

import pytest
import torch

from tests import ew_ref as E
from tests import train_ref as T
from tests.gemm_ref import ACT_GELU_ERF, ACT_GELU_TANH, ACT_SILU, sentinel_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf = torch.bfloat16
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


def note(name, share):
    WORST[name] = max(WORST.get(name, 0.0), share)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def idx(n):
    return torch.arange(n, device=DEV)


def randn(shape, g, scale=1.0, dtype=torch.float32):
    return (scale * torch.randn(shape, device=DEV, generator=g)).to(dtype)


def poisoned(n, dtype):
    return E.poison_(torch.empty(n, device=DEV, dtype=dtype))


def check3(rep, got, exp, what=""):
    """got [B, S, N] (a view) against (want, bound, delta) [B, S, N]: sample b, row s"""
    B, S, N = got.shape
    smp, tok = idx(B).repeat_interleave(S), idx(S).repeat(B)
    rep.check(got.reshape(B * S, N), *(v.reshape(B * S, N) for v in exp), sample=smp, token=tok, what=what)


class forms:
    """run the body under train_rows_wg = form, restore the option afterwards"""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from x2i_amd import _lib
        self.old = _lib.get_option("train_rows_wg")
        _lib.set_option("train_rows_wg", self.form)

    def __exit__(self, *a):
        from x2i_amd import _lib
        _lib.set_option("train_rows_wg", self.old)


class Layout:
    """[B, S, D] views of one operand inside a flat buffer: contiguous, or the image rows St .. St + S of a shared [B, St + S + 2, ld] buffer
    with a padded leading dimension (what x2i_amd/train.py passes: an offset of St rows and a batch stride of the whole sequence)"""

    def __init__(self, B, S, D, pad, St):
        self.B, self.S, self.D = B, S, D
        self.ld = D + pad
        self.bs = (St + S + 2) * self.ld if (pad or St) else S * D
        self.off = St * self.ld
        self.numel = B * self.bs + 8
        self.view_spec = ((B, S, D), (self.bs, self.ld, 1), self.off)

    def view(self, buf):
        return buf.as_strided(*self.view_spec)

    def filled(self, values, dtype=bf):
        """a buffer of random data with `values` [B, S, D] in the view"""
        buf = torch.randn(self.numel, device=DEV).to(dtype)
        self.view(buf).copy_(values)
        return buf

    def kw(self, bs, ld, off):
        return {bs: self.bs, ld: self.ld, off: self.off}


# ---------------------------------------------------------------------------------------------------------------- ln_mod_bwd, gate_bwd
ROW_SHAPES = [(2, 37, 3072, 8), (3, 37, 4096, 3), (2, 21, 520, 5), (3, 7, 256, 1), (1, 40, 3072, 16), (2, 9, 1024, 16)]
# operand kind of X, dXin ("alias" dXout / None / a "separate" tensor), 4 outlier channels in dY, partial one float off 16-byte alignment
LN_VARIANTS = [("random", "alias", False, False), ("large_mean", None, False, False), ("outlier", "separate", False, False),
               ("const", "alias", True, False), ("mod_edge", None, False, True), ("random", "separate", False, False)]


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("B,S,D,R", ROW_SHAPES)
def test_ln_mod_bwd_vs_fp64(ops, B, S, D, R, padded):
    t0 = time.time()
    St = 11 if padded else 0
    LX, LY, LD = (Layout(B, S, D, p if padded else 0, St) for p in (32, 64, 24))
    nw = (S + R - 1) // R
    for form in (1, 0):
        with forms(form):
            for j, (kind, din, dy_out, mis) in enumerate(LN_VARIANTS):
                affine = j == len(LN_VARIANTS) - 1                       # the last variant: an affine LayerNorm weight (mult_is_scale = False)
                g = gen(1000 * j + S + D)
                xbuf = LX.filled(E.ln_rows(B * S, D, kind, g, DEV).view(B, S, D))
                dy = randn((B, S, D), g)
                if dy_out:
                    dy[..., torch.randint(0, D, (4,), device=DEV, generator=g)] *= 2.0 ** 9
                dybuf = LY.filled(dy)
                mult_bs = D + (12 if padded else 0)
                mbuf = E.mod_vectors(B * mult_bs, kind, g, DEV)
                m = mbuf[:D] if affine else mbuf.view(B, mult_bs)[:, :D]
                dxbuf = poisoned(LD.numel, bf)
                din_vals = randn((B, S, D), g, dtype=bf) if din else None
                dinbuf = None
                if din == "alias":
                    LD.view(dxbuf).copy_(din_vals)
                    dinbuf = dxbuf
                elif din == "separate":
                    dinbuf = LD.filled(din_vals)
                    din_copy = dinbuf.clone()
                pbuf = poisoned(B * nw * 2 * D + 4, torch.float32)
                part = pbuf[1:] if mis else pbuf
                ops.ln_mod_bwd(xbuf, dybuf, mbuf, dinbuf, dxbuf, part, B=B, S=S, D=D, R=R, mult_is_scale=not affine, mult_bs=0 if affine else mult_bs,
                               **LX.kw("x_bs", "ldx", "x_offset"), **LY.kw("dy_bs", "ldy", "dy_offset"), **LD.kw("dx_bs", "lddx", "dx_offset"))
                torch.cuda.synchronize()
                name = f"ln_mod_bwd B={B} S={S} D={D} R={R} {'padded' if padded else 'contiguous'} form={form} {kind} dXin={din} " \
                       f"{'affine ' if affine else ''}{'partial+4B' if mis else ''}"
                ex, ep = T.ln_mod_bwd_expect(LX.view(xbuf), LY.view(dybuf), m, din_vals, R=R, mult_is_scale=not affine)
                rep = E.Report(name)
                check3(rep, LD.view(dxbuf), ex, " dX")
                pv = part[:B * nw * 2 * D].view(B, nw, 2 * D)
                check3(rep, pv, tuple(v.reshape(B, nw, 2 * D) for v in ep), " partial")
                key = "wg" if (form == 1 and not mis) else "wave"
                note(f"ln_mod_bwd {key}", rep.done())
                E.check_untouched(name + " dX", dxbuf, E.write_mask(dxbuf, [LD.view_spec]), row_len=LD.ld)
                o = 1 if mis else 0
                E.check_untouched(name + " partial", pbuf, E.write_mask(pbuf, [((B * nw * 2 * D,), (1,), o)]))
                if din == "separate":
                    assert torch.equal(dinbuf.view(torch.int16), din_copy.view(torch.int16)), name + ": dXin changed"
    print(f"\n  ln_mod_bwd B={B} S={S} D={D} R={R} ({time.time() - t0:.1f} s): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


# gate, G, partial one float off alignment
GATE_VARIANTS = [(True, True, False), (True, False, False), (False, True, False), (False, False, False), (True, True, True)]


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("B,S,D,R", ROW_SHAPES)
def test_gate_bwd_vs_fp64(ops, B, S, D, R, padded):
    St = 11 if padded else 0
    LDX, LT, LG, LDT = (Layout(B, S, D, p if padded else 0, St) for p in (8, 32, 64, 24))
    nw = (S + R - 1) // R
    for form in (1, 0):
        with forms(form):
            for j, (has_gate, has_G, mis) in enumerate(GATE_VARIANTS):
                g = gen(100 * j + S + D)
                scale = 2.0 ** 10 if j == 1 else 1.0                    # (once with large residual-stream values)
                dxbuf, tbuf, gbuf = (L.filled(randn((B, S, D), g, scale)) for L in (LDX, LT, LG))
                gate_bs = D + (12 if padded else 0)
                gate = randn((B, gate_bs), g) if has_gate else None
                dtbuf = poisoned(LDT.numel, bf)
                pbuf = poisoned(B * nw * D + 4, torch.float32)
                part = pbuf[1:] if mis else pbuf
                ops.gate_bwd(dxbuf, tbuf if has_gate else None, gate, gbuf if has_G else None, dtbuf, part if has_gate else None, B=B, S=S, D=D, R=R,
                             gate_bs=gate_bs, **LDX.kw("dx_bs", "lddx", "dx_offset"), **LT.kw("t_bs", "ldt", "t_offset"),
                             **LG.kw("g_bs", "ldg", "g_offset"), **LDT.kw("dt_bs", "lddt", "dt_offset"))
                torch.cuda.synchronize()
                name = f"gate_bwd B={B} S={S} D={D} R={R} {'padded' if padded else 'contiguous'} form={form} gate={has_gate} G={has_G} " \
                       f"{'partial+4B' if mis else ''}"
                et, ep = T.gate_bwd_expect(LDX.view(dxbuf), LT.view(tbuf), gate[:, :D] if has_gate else None, LG.view(gbuf) if has_G else None, R=R)
                rep = E.Report(name)
                check3(rep, LDT.view(dtbuf), et, " dT")
                if has_gate:
                    check3(rep, part[:B * nw * D].view(B, nw, D), ep, " partial")
                note(f"gate_bwd {'wg' if (form == 1 and not mis) else 'wave'}", rep.done())
                E.check_untouched(name + " dT", dtbuf, E.write_mask(dtbuf, [LDT.view_spec]), row_len=LDT.ld)
                views = [((B * nw * D,), (1,), 1 if mis else 0)] if has_gate else []
                E.check_untouched(name + " partial", pbuf, E.write_mask(pbuf, views))


# ---------------------------------------------------------------------------------------------------------------- reduce_rows
@pytest.mark.parametrize("np_", [1, 15, 16, 17, 112, 113, 128, 129, 241, 576])
def test_reduce_rows_vs_fp64(ops, np_):
    for n in (1, 63, 64, 65, 3072):
        for nz in (1, 3):
            g = gen(np_ + n + nz)
            in_ps, in_off, out_off = n + 3, 2, 3
            in_zs, out_zs = np_ * in_ps + 5, n + 7
            ibuf = randn(nz * in_zs + in_off + 8, g)
            iv = ibuf.as_strided((nz, np_, n), (in_zs, in_ps, 1), in_off)
            sign = torch.where(idx(np_) % 2 == 0, 1.0, -1.0)[None]
            iv[:, :, 0] = sign * (1 + 2.0 ** -12 * randn((nz, np_), g))    # a column whose partials cancel
            for acc in (False, True):
                obuf = poisoned(nz * out_zs + out_off + 8, torch.float32)
                ospec = ((nz, n), (out_zs, 1), out_off)
                old = None
                if acc:
                    old = randn((nz, n), g)
                    obuf.as_strided(*ospec).copy_(old)
                alpha = 0.375 if acc else (1.0 if nz == 1 else -1.5)
                ops.reduce_rows(ibuf, obuf, np_=np_, len_=n, nz=nz, in_zs=in_zs, in_ps=in_ps, out_zs=out_zs, accumulate=acc, alpha=alpha,
                                in_offset=in_off, out_offset=out_off)
                torch.cuda.synchronize()
                name = f"reduce_rows np={np_} len={n} nz={nz} accumulate={acc}"
                rep = E.Report(name)
                rep.check(obuf.as_strided(*ospec), *T.reduce_rows_expect(iv, alpha=alpha, old=old), sample=idx(nz), token=idx(nz) * 0, unit=1)
                note("reduce_rows", rep.done())
                E.check_untouched(name, obuf, E.write_mask(obuf, [ospec]))


def test_reduce_rows_scalar_loss_sum(ops):
    g = gen(5)
    x = randn(5000, g).abs()
    out = poisoned(4, torch.float32)
    ops.reduce_rows(x, out, np_=5000, len_=1, in_ps=1, out_offset=1)
    torch.cuda.synchronize()
    rep = E.Report("reduce_rows loss sum np=5000")
    rep.check(out[1:2].view(1, 1), *T.reduce_rows_expect(x.view(1, 5000, 1)), sample=idx(1), token=idx(1), unit=1)
    note("reduce_rows", rep.done())
    E.check_untouched("reduce_rows loss sum", out, E.write_mask(out, [((1,), (1,), 1)]))


# ---------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("nz,Rt,Rv,Ct,Cv,ld", [(2, 16, 13, 128, 100, 128), (1, 8, 8, 640, 513, 648), (3, 5, 0, 64, 1, 64), (1, 4, 4, 1024, 1024, 1024),
                                               (2, 6, 5, 576, 7, 584), (1, 3, 3, 512, 505, 512)])
def test_softmax_pad_and_bwd_vs_fp64(ops, nz, Rt, Rv, Ct, Cv, ld):
    """(the last two: Cv in the first / the last 8-column chunk of a 64-lane pass)"""
    rows = nz * Rv
    smp, tok = idx(nz).repeat_interleave(Rv), idx(Rv).repeat(nz)
    for scale in (0.3, 1.0):
        g = gen(Ct + Cv)
        x = (10.0 * randn((nz, Rt, Ct), g)).clamp(-30, 30)
        x[:, ::2, 0] = 30.0                               # one column dominates every other row
        pbuf = poisoned(nz * Rt * ld, bf)
        pv = pbuf.view(nz, Rt, ld)
        pv[:, :, :Ct] = x.to(bf)
        xin = pv[:, :Rv, :Ct].reshape(rows, Ct).clone()
        ops.softmax_pad_(pbuf, nz, Rt, Rv, Ct, Cv, scale, ld=ld)
        torch.cuda.synchronize()
        name = f"softmax_pad nz={nz} Rt={Rt} Rv={Rv} Ct={Ct} Cv={Cv} ld={ld} scale={scale}"
        if rows:
            rep = E.Report(name)
            rep.check(pv[:, :Rv, :Cv].reshape(rows, Cv), *T.softmax_pad_expect(xin, Cv, scale), sample=smp, token=tok)
            note("softmax_pad", rep.done())
        T.check_softmax_layout(name, pbuf, nz, Rt, Rv, Ct, Cv, ld)
        # backward on the bf16 P the kernel reads; what P holds in its padding must not matter
        pv[:, Rv:, :Ct] = 0.5
        pv[:, :Rv, Cv:Ct] = 0.5
        P0 = pbuf.clone()
        dbuf = poisoned(nz * Rt * ld, bf)
        dv = dbuf.view(nz, Rt, ld)
        dv[:, :, :Ct] = randn((nz, Rt, Ct), g, dtype=bf)
        din = dv[:, :Rv, :Ct].reshape(rows, Ct).clone()
        ops.softmax_bwd_(pbuf, dbuf, nz, Rt, Rv, Ct, Cv, scale, ld=ld)
        torch.cuda.synchronize()
        name = "softmax_bwd" + name[len("softmax_pad"):]
        if rows:
            rep = E.Report(name)
            rep.check(dv[:, :Rv, :Cv].reshape(rows, Cv), *T.softmax_bwd_expect(P0.view(nz, Rt, ld)[:, :Rv, :Ct].reshape(rows, Ct), din, Cv, scale),
                      sample=smp, token=tok)
            note("softmax_bwd", rep.done())
        T.check_softmax_layout(name, dbuf, nz, Rt, Rv, Ct, Cv, ld)
        assert torch.equal(pbuf.view(torch.int16), P0.view(torch.int16)), name + ": P changed"


# ---------------------------------------------------------------------------------------------------------------- act_bwd
def act_grid():
    """pre over [-12, 12] on the bf16 grid plus +-0, +-2^-20, +-100"""
    v = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32, device=DEV).to(torch.int16).view(bf).float()
    v = v[torch.isfinite(v) & (v.abs() <= 12)]
    return torch.cat((v, torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 100.0, -100.0], device=DEV)))


def _act_check(name, got, d0, pre, act, f32out, key):
    rows = got.shape[0]
    rep = E.Report(name)
    for r0 in range(0, rows, 2048):
        r1 = min(rows, r0 + 2048)
        rep.check(got[r0:r1], *T.act_bwd_expect(d0[r0:r1], pre[r0:r1], act, out_f32=f32out), sample=idx(r1 - r0) * 0, token=idx(r1 - r0) + r0)
    note(key, rep.done())


@pytest.mark.parametrize("act", [ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU], ids=["gelu_tanh", "gelu_erf", "silu"])
def test_act_bwd_vs_fp64(ops, act):
    grid = act_grid()
    cols, ldd, ldp, d_off, p_off = 136, 152, 144, 16, 8
    rows = (grid.numel() + cols - 1) // cols
    g = gen(act)
    pre = torch.cat((grid, 12.0 * (2 * torch.rand(rows * cols - grid.numel(), device=DEV, generator=g) - 1))).view(rows, cols)
    pbuf = randn(rows * ldp + p_off + 8, g, dtype=bf)
    pspec, dspec = ((rows, cols), (ldp, 1), p_off), ((rows, cols), (ldd, 1), d_off)
    pbuf.as_strided(*pspec).copy_(pre)
    dbuf = poisoned(rows * ldd + d_off + 8, bf)
    dbuf.as_strided(*dspec).copy_(randn((rows, cols), g, 2.0))
    d0 = dbuf.as_strided(*dspec).clone()
    ops.act_bwd_(dbuf, pbuf, act, rows=rows, cols=cols, ldd=ldd, ldp=ldp, d_offset=d_off, p_offset=p_off)
    torch.cuda.synchronize()
    name = f"act_bwd bf16 act={act}"
    _act_check(name, dbuf.as_strided(*dspec), d0, pbuf.as_strided(*pspec), act, False, "act_bwd bf16")
    E.check_untouched(name, dbuf, E.write_mask(dbuf, [dspec]), row_len=ldd)
    # the contiguous f32 form: the same grid and f32 values between its points
    p32 = torch.cat((pre.reshape(-1), 12.0 * (2 * torch.rand(1001, device=DEV, generator=g) - 1)))
    n = p32.numel()
    d32buf = poisoned(n + 8, torch.float32)
    d32buf[:n] = randn(n, g, 2.0)
    d0 = d32buf[:n].clone()
    ops.act_bwd_(d32buf, p32, act, rows=1, cols=n)
    torch.cuda.synchronize()
    _act_check(f"act_bwd f32 act={act}", d32buf[:n].view(1, n), d0.view(1, n), p32.view(1, n), act, True, "act_bwd f32")
    E.check_untouched(f"act_bwd f32 act={act}", d32buf, E.write_mask(d32buf, [((n,), (1,), 0)]))


def test_act_bwd_grid_stride_loop(ops):
    """rows * cols / 8 > 16384 * 256 work items: the grid-stride loop of act_bwd_kernel iterates"""
    rows, cols = 8200, 4104
    assert rows * cols // 8 > 16384 * 256
    g = gen(77)
    pre = randn((rows, cols), g, 3.0, bf)
    dbuf = poisoned(rows * cols + 64, bf)
    dv = dbuf[:rows * cols].view(rows, cols)
    dv.copy_(randn((rows, cols), g))
    d0 = dv.clone()
    ops.act_bwd_(dbuf, pre, ACT_GELU_TANH, rows=rows, cols=cols)
    torch.cuda.synchronize()
    _act_check("act_bwd bf16 33.6 M elements", dv, d0, pre, ACT_GELU_TANH, False, "act_bwd bf16")
    assert bool(sentinel_bits(dbuf[rows * cols:]).all())


# ---------------------------------------------------------------------------------------------------------------- qkv_split_bwd
@pytest.mark.parametrize("S,S0", [(33, 0), (33, 9), (33, 33), (130, 1)])
@pytest.mark.parametrize("H", [1, 3])
def test_qkv_split_bwd_vs_fp64(ops, H, S, S0):
    B, HD = 2, H * 128
    C3 = 3 * HD
    S1 = S - S0
    Spad = ops.pad128(S) + 128
    ld0, ld1, ldd0, ldd1 = C3 + 8, C3 + 24, C3 + 16, C3 + 40
    g = gen(H + S + S0)

    def rows_buf(n, ld):
        t = randn((max(n, 1), ld), g)
        t[::7] *= 2.0 ** 9                                # outlier rows
        return t.to(bf)
    q0, q1 = rows_buf(B * S0, ld0), rows_buf(B * S1, ld1)
    d0, d1 = poisoned(max(B * S0, 1) * ldd0, bf), poisoned(max(B * S1, 1) * ldd1, bf)
    nrm = [(1 + 0.2 * randn(128, g)).to(bf) for _ in range(4)]
    # the model's RoPE tables: S0 text tokens at the origin, the image tokens on a grid (FluxPosEmbed, axes (16, 56, 56))
    ids = torch.zeros((S, 3), device=DEV)
    w = 6
    ids[S0:, 1], ids[S0:, 2] = idx(S1) // w, idx(S1) % w
    cos, sin = ops.rope_table(ids, (16, 56, 56))
    dQ, dK, dV = (randn((B, H, Spad, 128), g, dtype=bf) for _ in range(3))
    text = S0 > 0
    ops.qkv_split_bwd(q0 if text else None, q1, ld0, ld1, d0 if text else None, d1, ldd0, ldd1, B, S, S0, H, nrm[0] if text else None,
                      nrm[1] if text else None, nrm[2], nrm[3], cos, sin, dQ, dK, dV, Spad)
    torch.cuda.synchronize()
    name = f"qkv_split_bwd H={H} S={S} S0={S0}"
    rep = E.Report(name)
    for src, n, qb, db, ld, ldd, nq, nk, lo in ((0, S0, q0, d0, ld0, ldd0, nrm[0], nrm[1], 0), (1, S1, q1, d1, ld1, ldd1, nrm[2], nrm[3], S0)):
        if n == 0:
            assert bool(sentinel_bits(db).all()), f"{name}: d{src} written though its stream is empty"
            continue
        tok = (idx(n) + lo).repeat(B)
        smp = idx(B).repeat_interleave(n)
        c, s = cos[lo:lo + n].double().repeat(B, 1), sin[lo:lo + n].double().repeat(B, 1)
        got = db.view(B * n, ldd)
        for sec, nw_, dy in ((0, nq, dQ), (1, nk, dK)):
            dyr = dy[:, :, lo:lo + n].permute(0, 2, 1, 3).reshape(B * n, H, 128)
            exp = T.qkv_split_bwd_rows(qb.view(-1, ld)[:B * n, sec * HD:(sec + 1) * HD], dyr, nw_, c, s, H=H)
            rep.check(got[:, sec * HD:(sec + 1) * HD], *exp, sample=smp, token=tok, unit=128, col0=sec * HD, what=f" d{'qk'[sec]} source {src}")
        dv = dV[:, :, lo:lo + n].permute(0, 2, 1, 3).reshape(B * n, HD).double()
        zero = torch.zeros_like(dv)
        rep.check(got[:, 2 * HD:C3], dv, zero, zero, sample=smp, token=tok, unit=128, col0=2 * HD, what=f" dv source {src}")
        E.check_untouched(f"{name} d{src}", db, E.write_mask(db, [((B * n, C3), (ldd, 1), 0)]), row_len=ldd)
    note("qkv_split_bwd", rep.done())


# ---------------------------------------------------------------------------------------------------------------- skinny_linear_bwd
@pytest.mark.parametrize("N,K,chunk", [(5000, 256, 512), (1000, 4096, 300), (257, 2056, 256), (100, 8, 1000)])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_skinny_linear_bwd_vs_fp64(ops, B, N, K, chunk):
    g = gen(B + N + K)
    dy = randn((B, N), g)
    dy[:, ::97] *= 64.0
    Wbuf = randn((N, K + 8), g, 0.05, bf)
    W = Wbuf[:, :K]
    nchunk = (N + chunk - 1) // chunk
    part = poisoned(nchunk * B * K + 8, torch.float32)
    lib = ops._lib.load()
    ops.check(lib.x2i_skinny_linear_bwd(ops._p(dy), dy.stride(0), ops._p(W), W.stride(0), ops._p(part), B, N, K, chunk, ops._stream()), "skinny_linear_bwd")
    out = poisoned(B * K + 8, torch.float32)
    ops.reduce_rows(part, out, np_=nchunk, len_=B * K)
    torch.cuda.synchronize()
    name = f"skinny_bwd B={B} N={N} K={K} chunk={chunk}"
    ep, eo = T.skinny_bwd_expect(dy, W, chunk)
    rep = E.Report(name)
    rep.check(part[:nchunk * B * K].view(nchunk * B, K), *(v.reshape(nchunk * B, K) for v in ep), sample=idx(nchunk * B) % B,
              token=idx(nchunk * B) // B, what=" partial (row = chunk)")
    rep.check(out[:B * K].view(B, K), *eo, sample=idx(B), token=idx(B) * 0, what=" reduced")
    note("skinny_bwd", rep.done())
    E.check_untouched(name + " partial", part, E.write_mask(part, [((nchunk * B * K,), (1,), 0)]))
    E.check_untouched(name + " out", out, E.write_mask(out, [((B * K,), (1,), 0)]))
    assert torch.equal(ops.skinny_linear_bwd(dy, W, chunk=chunk), out[:B * K].view(B, K)), name + ": ops.skinny_linear_bwd differs from its two stages"


# ---------------------------------------------------------------------------------------------------------------- kd_loss_rows
@pytest.mark.parametrize("rows", [1, 5, 37])
@pytest.mark.parametrize("D", [256, 3072, 4096])
def test_kd_loss_rows_vs_fp64(ops, D, rows):
    ldt, lds, ldg = D + 8, D + 24, D + 16
    for temp in (1.0, 3.0):
        g = gen(D + rows)
        t = randn((rows, D), g, 0.7)
        s = randn((rows, D), g, 0.9) + 0.3 * t
        if rows >= 5:
            s[1] = 0.75                                   # constant student: zero std, the normalisation's second term is 0
            t[2] = -1.5                                   # constant teacher
            s[3, 7] = 2.0 ** 12                           # one outlier
        tb, sb = randn((rows, ldt), g, dtype=bf), randn((rows, lds), g, dtype=bf)
        tb[:, :D], sb[:, :D] = t.to(bf), s.to(bf)
        el, eg = T.kd_loss_expect(tb[:, :D], sb[:, :D], temp, 0.25)
        for with_grad in (True, False):
            grad = poisoned(rows * ldg, bf)
            rl = poisoned(rows + 3, torch.float32)
            ops.kd_loss_rows(tb, sb, grad if with_grad else None, rl, rows=rows, D=D, temperature=temp, loss_scale=0.25, ldt=ldt, lds=lds, ldg=ldg)
            torch.cuda.synchronize()
            name = f"kd_loss rows={rows} D={D} T={temp} grad={with_grad}"
            rep = E.Report(name)
            rep.check(rl[:rows, None], *(v[:, None] for v in el), sample=idx(rows) * 0, token=idx(rows), unit=1, what=" row loss")
            if with_grad:
                rep.check(grad.view(rows, ldg)[:, :D], *eg, sample=idx(rows) * 0, token=idx(rows), what=" grad")
            note("kd_loss", rep.done())
            E.check_untouched(name + " row loss", rl, E.write_mask(rl, [((rows,), (1,), 0)]))
            E.check_untouched(name + " grad", grad, E.write_mask(grad, [((rows, D), (ldg, 1), 0)] if with_grad else []), row_len=ldg)


# ---------------------------------------------------------------------------------------------------------------- projector side
@pytest.mark.parametrize("B,C,S,H", [(2, 3, 24, 128), (1, 2, 17, 2056), (1, 1, 5, 8)])
def test_conv5x5_wgrad_vs_fp64(ops, B, C, S, H):
    g = gen(S + H)
    x, dy = randn((B, C, S, H), g, dtype=bf), randn((B, S, H), g, dtype=bf)
    out = ops.conv5x5_wgrad(x, dy)
    torch.cuda.synchronize()
    rep = E.Report(f"conv5x5_wgrad B={B} C={C} S={S} H={H}")
    rep.check(out, *T.conv5x5_wgrad_expect(x, dy), sample=idx(C) * 0, token=idx(C), unit=5)
    note("conv5x5_wgrad", rep.done())


@pytest.mark.parametrize("nchunk", [64, 7, 1])
def test_plane_dot_ragged_last_chunk(ops, nchunk):
    g = gen(nchunk)
    x, dy = randn((2, 3, 24, 40), g, dtype=bf), randn((2, 24, 40), g, dtype=bf)          # 120 vectors per plane: no multiple of 64 or 7
    out = ops.plane_dot(x, dy, alpha=0.5, nchunk=nchunk)
    torch.cuda.synchronize()
    rep = E.Report(f"plane_dot nchunk={nchunk}")
    rep.check(out[None], *(v[None] for v in T.plane_dot_expect(x, dy, alpha=0.5, nchunk=nchunk)), sample=idx(1), token=idx(1), unit=1)
    note("plane_dot", rep.done())


@pytest.mark.parametrize("n", [1, 255, 256, 100003])
def test_sum_all_vs_fp64(ops, n):
    g = gen(n)
    for dtype in (torch.float32, bf):
        x = (randn(n, g) + 0.25).to(dtype)
        for sq in (False, True):
            out = poisoned(1, torch.float32)
            ops.sum_all(x, squares=sq, out=out)
            torch.cuda.synchronize()
            rep = E.Report(f"sum_all n={n} {dtype} squares={sq}")
            rep.check(out[None], *(v[None] for v in T.sum_all_expect(x, sq)), sample=idx(1), token=idx(1), unit=1)
            note("sum_all", rep.done())


def test_clip_coef_vs_fp64(ops):
    for ss, mx in ((4.0, 3.0), (4.0, 2.0), (4.0, 1.0), (0.0, 1.0), (1.2345e7, 1.0), (3.0e-9, 1.0)):
        sumsq = torch.tensor([ss], device=DEV)
        out = ops.clip_coef(sumsq, mx)
        torch.cuda.synchronize()
        rep = E.Report(f"clip_coef sumsq={ss} max_norm={mx}")
        rep.check(out[None], *(v[None] for v in T.clip_coef_expect(sumsq, mx)), sample=idx(1), token=idx(1), unit=1)
        note("clip_coef", rep.done())
    assert float(ops.clip_coef(torch.tensor([0.0], device=DEV), 1.0)[0]) == 1.0


# ---------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("batch,R,C", [(3, 72, 136), (2, 8, 200), (1, 128, 64)])
def test_transpose_bit_exact_and_nothing_else_written(ops, batch, R, C):
    g = gen(R + C)
    ld_in, ld_out = C + 8, R + 16
    in_bs, out_bs = R * ld_in + 64, C * ld_out + 32
    ibuf = randn(batch * in_bs + 8, g, dtype=bf)
    obuf = poisoned(batch * out_bs + 16, bf)
    ops.transpose(ibuf, obuf, batch=batch, R=R, C=C, in_bs=in_bs, ld_in=ld_in, out_bs=out_bs, ld_out=ld_out, in_offset=8, out_offset=16)
    torch.cuda.synchronize()
    src = ibuf.as_strided((batch, R, C), (in_bs, ld_in, 1), 8)
    ospec = ((batch, C, R), (out_bs, ld_out, 1), 16)
    assert torch.equal(obuf.as_strided(*ospec).view(torch.int16), src.transpose(1, 2).contiguous().view(torch.int16))
    E.check_untouched(f"transpose batch={batch} R={R} C={C}", obuf, E.write_mask(obuf, [ospec]), row_len=ld_out)


def test_print_worst():
    """(last: the table of worst shares over everything this module ran)"""
    print("\n  worst share of the f32 allowance per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
