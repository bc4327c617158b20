"""ops.ln_affine, ops.softmax_rows_, the f32 ops.adamw_ and the forms of t5_ops.rms_rows the stacks use, every output element of every launch
against the float64 references and derived bounds of tests/rows_ref.py (rms_rows: tests/t5_ref.check_rms): NaN fails, elements whose
allowance is 0 must be exact, outputs start as the sentinel (or as a saved copy for in-place operands), everything outside the write set --
guards on both sides included -- is checked unchanged and the inputs are checked unchanged bit for bit.  No case skips itself: inputs that
miss their kind's coverage condition fail the test.

The shapes are the smallest that reach each path: one lane, a ragged second chunk of lane 0 alone (D = 520), a partly filled seventh pass
(D = 3200) and the cap (D = 4096) of ln_kernel; one thread, every thread, one thread in register chunk 1 (cols = 2056) and the cap
(cols = 16384) of softmax_rows_kernel with maxima in different waves; AdamW launches of less than, exactly and one more than a workgroup
and one above the 8192-workgroup grid, which only the grid-stride loop finishes.  The worst share of the f32 allowance used per kernel is
printed at the end (WORST)."""
import time

import pytest
import torch

from tests import rows_ref as R
from tests import t5_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf = torch.bfloat16
WORST = {}
GUARD = 64                       # sentinel elements on each side of an output (a multiple of 8: the views stay 16-byte aligned)


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture(scope="module")
def t5_ops():
    from x2i_amd import t5_ops as o
    o.load()
    return o


def note(name, share):
    WORST[name] = max(WORST.get(name, 0.0), share)


def gen(*key):
    return torch.Generator(device=DEV).manual_seed(R.seed_of(*key))


def idx(n):
    return torch.arange(n, device=DEV)


def guarded(shape, dtype, lead=GUARD):
    """(poisoned flat buffer, contiguous view of `shape` inside it behind `lead` sentinel elements and before GUARD more, its view spec)"""
    n, stride = 1, []
    for s in reversed(shape):
        stride.insert(0, n)
        n *= s
    buf = R.poison_(torch.empty(lead + n + GUARD, device=DEV, dtype=dtype))
    return buf, buf[lead:lead + n].view(shape), (tuple(shape), tuple(stride), lead)


def same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def check2(rep, got, exp, what=""):
    rows = idx(got.shape[0])
    rep.check(got, *exp, sample=torch.zeros_like(rows), token=rows, what=what)


# ---------------------------------------------------------------------------------------------------------------- ln_affine
@pytest.mark.parametrize("rows,D", R.LN_SHAPES)
def test_ln_affine_vs_fp64(ops, rows, D):
    t0 = time.time()
    cases = [c for c in R.ln_cases() if c[:2] == (rows, D)]
    assert len(cases) >= len(R.LN_EPS) * len(R.LN_AFFINE_KINDS)
    for _, _, eps, kind, variant in cases:
        g = gen("ln", rows, D, eps, kind, variant)
        x = R.ln_affine_rows(rows, D, kind, g, DEV)
        w, b = R.ln_wb(D, variant, g, DEV)
        name = f"ln_affine {rows}x{D} eps={eps} {kind} {variant}"
        R.ln_condition(x, w, b, kind, eps)
        x0, w0, b0 = x.clone(), w.clone(), b.clone()
        buf, out, spec = guarded((rows, D), bf)
        assert ops.ln_affine(x, w, b, eps, out=out) is out
        torch.cuda.synchronize()
        exp = R.ln_affine_expect(x0, w0, b0, eps)
        rep = R.Report(name)
        check2(rep, out, exp)
        note("ln_affine", rep.done())
        R.check_untouched(name, buf, R.write_mask(buf, [spec]))
        assert same_bits(x, x0) and same_bits(w, w0) and same_bits(b, b0), name + ": an input changed"
        const = R.const_rows(x0.double())[:, 0]
        if bool(const.any()):
            assert same_bits(out[const], b0.expand(rows, D)[const]), name + ": a constant row is not the bias"
    # without `out` the result is a new tensor shaped like X with the same bits
    assert same_bits(ops.ln_affine(x, w, b, eps), out)
    print(f"\n  ln_affine {rows}x{D}: {len(cases)} launches ({time.time() - t0:.1f} s), worst share so far {WORST['ln_affine']:.3f}")


def test_ln_affine_refusals_leave_the_output_alone(ops):
    from x2i_amd._lib import X2IError
    g = gen("ln refusals")
    for rows, D in ((3, 60), (2, 4104)):           # D % 8 != 0; beyond the cap of 4096
        x = torch.randn((rows, D), device=DEV, generator=g).to(bf)
        w, b = R.ln_wb(D, "plain", g, DEV)
        buf, out, _ = guarded((rows, D), bf)
        with pytest.raises(X2IError, match="D=%d" % D):
            ops.ln_affine(x, w, b, 1e-6, out=out)
        torch.cuda.synchronize()
        assert bool(R.sentinel_bits(buf).all())
    rows, D = 3, 64
    w, b = R.ln_wb(D, "plain", g, DEV)
    xbuf = torch.randn(rows * D + 8, device=DEV, generator=g).to(bf)
    wbuf = torch.ones(D + 8, device=DEV, dtype=bf)
    for off in ("X", "out", "weight", "bias"):     # a pointer 8 bytes off 16-byte alignment
        x = xbuf[4:4 + rows * D].view(rows, D) if off == "X" else xbuf[:rows * D].view(rows, D)
        buf, out, _ = guarded((rows, D), bf, lead=GUARD + 4 if off == "out" else GUARD)
        with pytest.raises(X2IError, match="alignment"):
            ops.ln_affine(x, wbuf[4:4 + D] if off == "weight" else w, wbuf[4:4 + D] if off == "bias" else b, 1e-6, out=out)
        torch.cuda.synchronize()
        assert bool(R.sentinel_bits(buf).all()), off


# ---------------------------------------------------------------------------------------------------------------- softmax_rows_
def run_softmax(ops, x, scale):
    """x bf16 [rows, cols] -> (the buffer, the view the launch ran on in place, its spec)"""
    buf, view, spec = guarded(tuple(x.shape), bf)
    view.copy_(x)
    assert ops.softmax_rows_(view, scale) is view
    torch.cuda.synchronize()
    return buf, view, spec


@pytest.mark.parametrize("rows,cols", R.SM_SHAPES)
def test_softmax_rows_vs_fp64(ops, rows, cols):
    t0 = time.time()
    for scale in R.SM_SCALES:
        for kind in R.SM_KINDS:
            x = R.softmax_rows_in(rows, cols, kind, scale, gen("softmax", rows, cols, scale, kind), DEV)
            name = f"softmax_rows {rows}x{cols} scale={scale:.4g} {kind}"
            R.softmax_condition(x, kind, scale)
            x0 = x.clone()
            buf, y, spec = run_softmax(ops, x, scale)
            exp = R.softmax_rows_expect(x0, scale)
            rep = R.Report(name)
            check2(rep, y, exp)
            note("softmax_rows", rep.done())
            R.check_untouched(name, buf, R.write_mask(buf, [spec]))
            assert same_bits(x, x0), name + ": the source of the copy changed"
            # each element rounds once to bf16, by at most 2^-9 of itself and of 1: the row sums to 1 within cols 2^-9
            s = y.double().sum(-1)
            assert bool(((s - 1.0).abs() <= cols * 2.0 ** -9).all()), f"{name}: a row sums to {float(s[(s - 1.0).abs().argmax()]):.6f}"
            if kind == "flat" and cols & (cols - 1) == 0:
                assert bool((y.double() == 1.0 / cols).all()), name + ": a constant row of a power-of-two width is not 1 / cols exactly"
            # a relaunch on a fresh copy is bit-identical, and a row does not depend on the rows around it
            assert same_bits(run_softmax(ops, x0, scale)[1], y), name + ": a relaunch differs"
            assert same_bits(run_softmax(ops, x0[-1:], scale)[1], y[-1:]), name + ": the last row alone differs"
            if rows > 1:
                assert same_bits(run_softmax(ops, x0.flip(0).contiguous(), scale)[1].flip(0), y), name + ": the rows in reverse order differ"
    print(f"\n  softmax_rows {rows}x{cols}: {len(R.SM_SCALES) * len(R.SM_KINDS)} cases ({time.time() - t0:.1f} s), "
          f"worst share so far {WORST['softmax_rows']:.3f}")


def test_softmax_rows_refusals_leave_the_buffer_alone(ops):
    from x2i_amd._lib import X2IError
    for rows, cols in ((4, 12), (1, 16392)):       # cols % 8 != 0; beyond the cap of 16384
        buf, view, _ = guarded((rows, cols), bf)
        view.copy_(torch.randn((rows, cols), device=DEV, generator=gen("softmax refusal", cols)))
        saved = buf.clone()
        with pytest.raises(X2IError, match="cols=%d" % cols):
            ops.softmax_rows_(view, 1.0)
        torch.cuda.synchronize()
        assert same_bits(buf, saved)


# ---------------------------------------------------------------------------------------------------------------- adamw_
def adamw_step(ops, name, n, p, g, m, v, bufs, coef_t, wd, step):
    """one launch on the views p / g / m / v of the poisoned buffers `bufs`, every element of p', m', v' checked from the state read"""
    p0, g0, m0, v0 = p.clone(), g.clone(), m.clone(), v.clone()
    gbuf0 = bufs["g"].clone()
    coef0 = None if coef_t is None else coef_t.clone()
    assert ops.adamw_(p, g, m, v, weight_decay=wd, step=step, coef=coef_t, **R.ADAMW_HYP) is p
    torch.cuda.synchronize()
    exp = R.adamw_expect(p0, g0, m0, v0, None if coef_t is None else float(coef0[0]), R.adamw_scalars(weight_decay=wd, step=step, **R.ADAMW_HYP))
    shares = {}
    for key, got in (("p", p), ("m", m), ("v", v)):
        rep = R.Report(f"{name} {key}'")
        R.check_flat(rep, got, exp[key])
        shares[key] = rep
    for key, rep in shares.items():
        note("adamw " + key, rep.done())
    for key in "pmv":
        R.check_untouched(f"{name} {key}", bufs[key], R.write_mask(bufs[key], [bufs[key + "_spec"]]))
    assert same_bits(bufs["g"], gbuf0), name + ": the gradient buffer changed"
    assert coef_t is None or same_bits(coef_t, coef0), name + ": coef changed"
    return exp, p0


@pytest.mark.parametrize("config", list(R.ADAMW_CONFIGS))
@pytest.mark.parametrize("n", R.ADAMW_SIZES)
def test_adamw_vs_fp64(ops, n, config):
    t0 = time.time()
    coef, wd, step, rnd = R.ADAMW_CONFIGS[config]
    if n == max(R.ADAMW_SIZES):
        assert n > 8192 * 256, "the largest launch must be beyond the grid: only the grid-stride loop reaches its end"
    g0 = gen("adamw", n, config)
    ps, ms, vs = R.adamw_state(n, rnd, g0, DEV)
    gs = R.adamw_gradient(n, g0, DEV)
    R.adamw_condition(n, gs, ms, vs, rnd)
    # p inside a poisoned bf16 buffer; g, m, v at an odd element offset of larger poisoned f32 buffers, as FlatAdamW slices its flat storage
    bufs = {}
    bufs["p"], p, bufs["p_spec"] = guarded((n,), bf)
    views = {}
    for key, src in (("g", gs), ("m", ms), ("v", vs)):
        bufs[key], views[key], bufs[key + "_spec"] = guarded((n,), torch.float32, lead=GUARD + 1)
        views[key].copy_(src)
    p.copy_(ps)
    g, m, v = views["g"], views["m"], views["v"]
    assert g.storage_offset() % 2 == 1 and m.storage_offset() % 2 == 1 and v.storage_offset() % 2 == 1
    coef_t = None if coef is None else torch.tensor([coef, 12.5], device=DEV, dtype=torch.float32)
    lo, hi = R.adamw_zero_stretch(n)
    for k in range(3 if n == 5000 else 1):           # three consecutive steps, each checked from the state the kernel left
        if k:
            g.copy_(R.adamw_gradient(n, gen("adamw", n, config, k), DEV))
        name = f"adamw n={n} {config} step {step + k}"
        exp, p0 = adamw_step(ops, name, n, p, g, m, v, bufs, coef_t, wd, step + k)
        if k == 0 and hi > lo:          # a zero gradient on zero moments: m' = v' = 0 and the parameter takes the decay alone
            assert not bool(m[lo:hi].any()) and not bool(v[lo:hi].any()), name + ": a moment of the zero stretch moved"
            assert not bool(exp["m"][2][lo:hi].any()) and not bool(exp["v"][2][lo:hi].any())
            if wd == 0.0:
                assert same_bits(p[lo:hi], p0[lo:hi]) and not bool(exp["p"][2][lo:hi].any()), name + ": wd = 0 moved a parameter of the zero stretch"
            else:
                assert bool((p[lo:hi].double().abs() <= p0[lo:hi].double().abs()).all()), name + ": the decay grew a parameter"
    print(f"\n  adamw n={n} {config} ({time.time() - t0:.1f} s): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith("adamw")))


# ---------------------------------------------------------------------------------------------------------------- rms_rows
def rms_note(worst):
    note("rms_rows", worst / TR.TOL_ROW)


def test_rms_rows_zero_row_gives_exact_zeros(t5_ops):
    g = gen("rms zero")
    rows, D = 5, 896
    x = (3.0 + torch.randn((rows, D), device=DEV, generator=g)).to(bf)
    x[2] = 0
    w = torch.randn(D, device=DEV, generator=g).to(bf)
    for eps in (1e-6, 1e-5):
        buf, y, spec = guarded((rows, D), bf)
        t5_ops.rms_rows(x, w, eps, out=y)
        torch.cuda.synchronize()
        rms_note(TR.check_rms(f"rms_rows zero row eps={eps}", y, x, w, eps))        # (a bound of 0 on the zero row: exact)
        assert not bool(y[2].any()) and not bool(torch.isnan(y.float()).any())
        R.check_untouched("rms_rows zero row", buf, R.write_mask(buf, [spec]))


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_rms_rows_eps_dominant(t5_ops, eps):
    """rows whose mean square is below eps / 4: the result is x w / sqrt(eps) to first order, and the other eps is caught"""
    g = gen("rms eps", eps)
    rows, D = 6, 1024
    x = (R.ln_affine_rows(rows, D, "eps_dominant", g, DEV).double() * 2.0 ** -8).to(bf)
    w = (1.0 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(bf)
    assert bool(((x.double() ** 2).mean(-1) < 1e-6 / 4).all()), "eps_dominant: mean square not below eps / 4"
    other = 1e-6 if eps == 1e-5 else 1e-5
    a, b = TR.rms_reference(x, w, eps), TR.rms_reference(x, w, other)
    assert bool(((a - b).abs() > TR.TOL_ROW * (a.abs() + b.abs())).any()), "eps_dominant: the other eps moves no element by more than its bound"
    x0 = x.clone()
    buf, y, spec = guarded((rows, D), bf)
    t5_ops.rms_rows(x, w, eps, out=y)
    torch.cuda.synchronize()
    rms_note(TR.check_rms(f"rms_rows eps_dominant eps={eps}", y, x0, w, eps))
    R.check_untouched("rms_rows eps_dominant", buf, R.write_mask(buf, [spec]))
    assert same_bits(x, x0)


def test_rms_rows_in_place_on_the_middle_columns(t5_ops):
    """InternViT's k_norm: Y is X, ldx = ldy = 3 D, the columns [D, 2 D) of a [rows, 3 D] buffer; every other column stays"""
    g = gen("rms in place")
    rows, D, eps = 7, 1024, 1e-6
    qkv = (3.0 + torch.randn((rows, 3 * D), device=DEV, generator=g)).to(bf)
    w = torch.randn(D, device=DEV, generator=g).to(bf)
    q0 = qkv.clone()
    t5_ops.rms_rows(qkv[:, D:2 * D], w, eps, out=qkv[:, D:2 * D], rows=rows, ldx=3 * D, ldy=3 * D)
    torch.cuda.synchronize()
    rms_note(TR.check_rms("rms_rows in place", qkv[:, D:2 * D], q0[:, D:2 * D], w, eps))
    assert same_bits(qkv[:, :D], q0[:, :D]) and same_bits(qkv[:, 2 * D:], q0[:, 2 * D:]), "a column outside [D, 2 D) changed"


def test_rms_rows_decode_form(t5_ops):
    """Qwen2 decoding: 3 rows a slab stride apart (ldx much larger than D), a contiguous output"""
    g = gen("rms decode")
    rows, D, eps, ldx = 3, 896, 1e-6, 29 * 896
    slab = (3.0 + torch.randn((rows, ldx), device=DEV, generator=g)).to(bf)
    w = torch.randn(D, device=DEV, generator=g).to(bf)
    s0 = slab.clone()
    buf, y, spec = guarded((rows, D), bf)
    t5_ops.rms_rows(slab[:, 5 * D:6 * D], w, eps, out=y, rows=rows, ldx=ldx)
    torch.cuda.synchronize()
    rms_note(TR.check_rms("rms_rows decode", y, s0[:, 5 * D:6 * D], w, eps))
    R.check_untouched("rms_rows decode", buf, R.write_mask(buf, [spec]))
    assert same_bits(slab, s0)


def test_print_worst():
    """(last: the table of worst shares over everything this module ran; rms_rows: its worst relative error over t5_ref.TOL_ROW)"""
    print("\n  worst share of the f32 allowance per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert {"ln_affine", "softmax_rows", "adamw p", "adamw m", "adamw v", "rms_rows"} <= set(WORST)
    assert all(v <= 1.0 for v in WORST.values())
