"""The float64 references and bounds of tests/rows_ref.py on the host.  f32 stand-ins that follow the kernels' arithmetic in the kernels' own
order (the chunk chain of a lane or thread, the 64-lane butterfly of wave_sum, then the waves; every product and sum rounded, nothing
contracted) stay inside every bound on every case tests/test_rows_fp64_gpu.py launches; each kernel fault below, planted in the stand-in, is
rejected on one of those cases; and the whole-tensor criteria the three kernels were judged by before accept a wrong eps and a dropped
AdamW tail."""
import pytest
import torch

from tests import rows_ref as R

bf = torch.bfloat16
WORST = {}


def fma32(a, b, c):
    """fmaf on f32 tensors: exact product and sum in float64, one rounding to f32"""
    return (a.double() * b.double() + c.double()).float()


def gen(*key):
    return torch.Generator().manual_seed(R.seed_of(*key))


def butterfly(acc):
    """wave_sum over the last dimension (64 lanes); every lane ends with the same value"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    return acc[..., 0]


def failure(rep):
    try:
        rep.done()
    except AssertionError as e:
        return str(e)
    return None


def check2(name, got, exp):
    rows = torch.arange(got.shape[0])
    rep = R.Report(name)
    rep.check(got, *exp, sample=torch.zeros_like(rows), token=rows)
    return rep


# ---------------------------------------------------------------------------------------------------------------- ln_affine
def ln_lane_sum(v, sq=False):
    """ln_kernel's row sum of v f32 [rows, D]: lane l chains the values of its chunks l, l + 64, ... (sq: fmaf(d, d, acc)), then wave_sum.
    Lanes beyond a ragged last pass add nothing (zeros here: x + 0 and fma(0, 0, x) are exact)."""
    rows, D = v.shape
    L = torch.nn.functional.pad(v, (0, -D % 512)).view(rows, -1, 64, 8)
    acc = torch.zeros((rows, 64))
    for i in range(L.shape[1]):
        for j in range(8):
            x = L[:, i, :, j]
            acc = fma32(x, x, acc) if sq else acc + x
    return butterfly(acc)


def ln_affine_standin(x, w, b, eps, fault=None):
    """ln_kernel<true> in f32.  fault: eps5 (eps 1e-5 whatever was asked), one_pass (variance as E[x^2] - mean^2), bias_chunk (the bias of the
    neighbouring 8-column chunk), no_weight, mean_d8 (the mean over the first D - 8 columns)."""
    D = x.shape[-1]
    xf = x.float()
    mean = ln_lane_sum(xf[:, :D - 8]) / (D - 8) if fault == "mean_d8" else ln_lane_sum(xf) / D
    if fault == "one_pass":
        var = ln_lane_sum(xf, sq=True) / D - mean * mean
    else:
        var = ln_lane_sum(xf - mean[:, None], sq=True) / D
    rstd = torch.rsqrt(var + torch.tensor(1e-5 if fault == "eps5" else eps, dtype=torch.float32))
    t = (xf - mean[:, None]) * rstd[:, None]
    if fault != "no_weight":
        t = t * w.float()
    bias = b.view(-1, 8).roll(1, 0).reshape(-1) if fault == "bias_chunk" else b
    return (t + bias.float()).to(bf)


def ln_case(rows, D, eps, kind, variant):
    g = gen("ln", rows, D, eps, kind, variant)
    x = R.ln_affine_rows(rows, D, kind, g, "cpu")
    w, b = R.ln_wb(D, variant, g, "cpu")
    return x, w, b


def test_ln_affine_standin_stays_inside_the_bound_on_every_case():
    for rows, D, eps, kind, variant in R.ln_cases():
        x, w, b = ln_case(rows, D, eps, kind, variant)
        R.ln_condition(x, w, b, kind, eps)
        exp = R.ln_affine_expect(x, w, b, eps)
        name = f"ln_affine {rows}x{D} eps={eps} {kind} {variant}"
        WORST["ln_affine"] = max(WORST.get("ln_affine", 0.0), check2(name, ln_affine_standin(x, w, b, eps), exp).done())
        const = R.const_rows(x.double())[:, 0]
        if bool(const.any()):          # a constant row is bf16(b) exactly
            assert torch.equal(ln_affine_standin(x, w, b, eps)[const], b.expand(rows, D)[const]) and not bool(exp[2][const].any())
    print(f"\n  ln_affine stand-in: worst share of delta {WORST['ln_affine']:.3f}")
    assert WORST["ln_affine"] <= 1.0


# fault, the case of tests/test_rows_fp64_gpu.py it must fail on
LN_FAULTS = [("eps5", (3, 520, 1e-6, "eps_dominant", "plain")),
             ("one_pass", (9, 4096, 1e-6, "const", "plain")),       # (rows constant but for two elements: E[x^2] - mean^2 is noise above eps)
             ("bias_chunk", (7, 768, 1e-6, "random", "plain")),
             ("no_weight", (6, 1152, 1e-5, "random", "plain")),
             ("mean_d8", (5, 64, 1e-6, "random", "plain"))]


@pytest.mark.parametrize("fault,case", LN_FAULTS, ids=[f[0] for f in LN_FAULTS])
def test_ln_affine_fault_rejected(fault, case):
    assert case in list(R.ln_cases())
    x, w, b = ln_case(*case)
    eps = case[2]
    exp = R.ln_affine_expect(x, w, b, eps)
    assert failure(check2("ln_affine", ln_affine_standin(x, w, b, eps), exp)) is None
    msg = failure(check2("ln_affine", ln_affine_standin(x, w, b, eps, fault), exp))
    assert msg is not None and "rows over the bound" in msg, fault


def test_old_ln_criterion_accepts_the_wrong_eps():
    """tests/test_ops_gpu.py::test_ln_affine: N(0, 3^2) rows, eps = 1e-6, rel-L2 < 5e-3 against F.layer_norm.  With a variance of 9 a kernel
    that uses 1e-5 instead passes it -- and the per-element bound on the same rows passes it too (the outputs move by 5e-7 of themselves):
    only rows whose variance is below eps show the constant, which is what the eps_dominant kind is for."""
    g = gen("old ln")
    D = 896
    x = (3.0 * torch.randn((21, D), generator=g)).to(bf)
    w, b = R.ln_wb(D, "plain", g, "cpu")
    y = ln_affine_standin(x, w, b, 1e-6, "eps5")
    ref = torch.nn.functional.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-6)
    assert float((y.float() - ref).norm() / ref.norm()) < R.OLD_REL_L2
    assert failure(check2("ln_affine", y, R.ln_affine_expect(x, w, b, 1e-6))) is None
    x, w, b = ln_case(3, 520, 1e-6, "eps_dominant", "plain")
    assert failure(check2("ln_affine", ln_affine_standin(x, w, b, 1e-6, "eps5"), R.ln_affine_expect(x, w, b, 1e-6))) is not None


# ---------------------------------------------------------------------------------------------------------------- softmax_rows_
def softmax_standin(x, scale, fault=None):
    """softmax_rows_kernel in f32: thread t holds the chunks t, t + 256, ...; it chains their values chunk by chunk, wave_sum joins the 64
    lanes of a wave and red[0] + red[1] + red[2] + red[3] the waves.  fault: no_scale, max_head (the maximum over the first 2048 columns
    only), drop_wave (the sum without wave 3's share), exp (e^x in place of 2^x)."""
    rows, cols = x.shape
    sl = torch.tensor(1.0 if fault == "no_scale" else scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    v = x.float() * sl
    mx = (v[:, :2048] if fault == "max_head" else v).amax(-1, keepdim=True)
    e = torch.exp(v - mx) if fault == "exp" else torch.exp2(v - mx)
    E = torch.nn.functional.pad(e, (0, -cols % 2048)).view(rows, -1, 256, 8)
    acc = torch.zeros((rows, 256))
    for c in range(E.shape[1]):
        for j in range(8):
            acc = acc + E[:, c, :, j]
    red = butterfly(acc.view(rows, 4, 64))
    if fault == "drop_wave":
        red[:, 3] = 0
    total = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    inv = 1.0 / total
    return (e * inv[:, None]).to(bf)


def sm_case(rows, cols, scale, kind):
    return R.softmax_rows_in(rows, cols, kind, scale, gen("softmax", rows, cols, scale, kind), "cpu")


def test_softmax_standin_stays_inside_the_bound_on_every_case():
    worst = 0.0
    for rows, cols in R.SM_SHAPES:
        for scale in R.SM_SCALES:
            for kind in R.SM_KINDS:
                x = sm_case(rows, cols, scale, kind)
                R.softmax_condition(x, kind, scale)
                exp = R.softmax_rows_expect(x, scale)
                y = softmax_standin(x, scale)
                worst = max(worst, check2(f"softmax_rows {rows}x{cols} scale={scale:.4g} {kind}", y, exp).done())
                assert bool(((y.double().sum(-1) - 1.0).abs() <= cols * 2.0 ** -9).all())
                if kind == "flat" and cols & (cols - 1) == 0:
                    assert not bool(exp[2].any()) and bool((y.double() == 1.0 / cols).all())
    print(f"\n  softmax_rows stand-in: worst share of delta {worst:.3f}")
    assert worst <= 1.0


SM_FAULTS = [("no_scale", (3, 256, 0.25, "random")),
             ("max_head", (2, 2056, 1.0, "max_last")),
             ("drop_wave", (3, 2048, 1.0, "random")),
             ("exp", (40, 96, 1.0, "random"))]


@pytest.mark.parametrize("fault,case", SM_FAULTS, ids=[f[0] for f in SM_FAULTS])
def test_softmax_fault_rejected(fault, case):
    rows, cols, scale, kind = case
    assert (rows, cols) in R.SM_SHAPES and scale in R.SM_SCALES and kind in R.SM_KINDS
    x = sm_case(*case)
    exp = R.softmax_rows_expect(x, scale)
    assert failure(check2("softmax_rows", softmax_standin(x, scale), exp)) is None
    msg = failure(check2("softmax_rows", softmax_standin(x, scale, fault), exp))
    assert msg is not None and "rows over the bound" in msg, fault


def test_softmax_bound_allows_zero_only_below_the_smallest_normal():
    x = sm_case(3, 2048, 1.0, "spike")
    want, bound, delta = R.softmax_rows_expect(x, 1.0)
    small = want < R.F32_MIN_NORMAL
    assert bool(small.any()) and bool((bound[small] >= want[small]).all())
    assert bool((bound[~small] < 0.01 * want[~small]).all())


# ---------------------------------------------------------------------------------------------------------------- adamw_
def adamw_standin(p, g, m, v, coef, wd, step, fault=None):
    """adamw_kernel in f32, every product and sum rounded.  Returns (p', m', v').  fault: bc_prev (the bias corrections of step - 1), l2
    (weight decay added to the gradient instead of decoupled), no_coef, v_unclipped (v from the unclipped gradient), tail (the last n % 256
    elements left alone)."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    hyp = R.ADAMW_HYP
    lr, b1, b2, eps, wdf = t(hyp["lr"]), t(hyp["beta1"]), t(hyp["beta2"]), t(hyp["eps"]), t(wd)
    s = step - 1 if fault == "bc_prev" else step
    bc1, bc2 = t(1.0 - hyp["beta1"] ** s), t(1.0 - hyp["beta2"] ** s)
    cf = t(1.0 if coef is None or fault == "no_coef" else coef)
    pw = p.float()
    graw = g + wdf * pw if fault == "l2" else g
    gg = cf * graw
    gv = graw if fault == "v_unclipped" else gg
    mm = b1 * m + (1.0 - b1) * gg
    vv = b2 * v + (1.0 - b2) * gv * gv
    decay = t(1.0) if fault == "l2" else 1.0 - lr * wdf
    pn = (pw * decay - lr * (mm / bc1) / (torch.sqrt(vv / bc2) + eps)).to(bf)
    if fault == "tail":
        k = p.numel() - p.numel() % 256
        pn[k:], mm[k:], vv[k:] = p[k:], m[k:], v[k:]
    return pn, mm, vv


def adamw_case(n, config):
    coef, wd, step, rnd = R.ADAMW_CONFIGS[config]
    g0 = gen("adamw", n, config)
    p, m, v = R.adamw_state(n, rnd, g0, "cpu")
    g = R.adamw_gradient(n, g0, "cpu")
    return p, g, m, v, coef, wd, step, rnd


def adamw_report(name, got, exp):
    rep = R.Report(name)
    for key, val in zip("pmv", got):
        R.check_flat(rep, val, exp[key], what=" " + key)
    return rep


@pytest.mark.parametrize("config", list(R.ADAMW_CONFIGS))
def test_adamw_standin_stays_inside_the_bound_on_every_case(config):
    worst = 0.0
    for n in R.ADAMW_SIZES:
        p, g, m, v, coef, wd, step, rnd = adamw_case(n, config)
        R.adamw_condition(n, g, m, v, rnd)
        for k in range(3 if n == 5000 else 1):          # three consecutive steps, each from the state the step before left
            if k:
                g = R.adamw_gradient(n, gen("adamw", n, config, k), "cpu")
            exp = R.adamw_expect(p, g, m, v, coef, R.adamw_scalars(weight_decay=wd, step=step + k, **R.ADAMW_HYP))
            got = adamw_standin(p, g, m, v, coef, wd, step + k)
            worst = max(worst, adamw_report(f"adamw n={n} {config} step {step + k}", got, exp).done())
            lo, hi = R.adamw_zero_stretch(n)
            if k == 0 and hi > lo:         # zero gradient on zero moments: the decay alone, exactly
                assert not bool(got[1][lo:hi].any()) and not bool(got[2][lo:hi].any()) and not bool(exp["m"][2][lo:hi].any())
                if wd == 0.0:
                    assert torch.equal(got[0][lo:hi], p[lo:hi]) and not bool(exp["p"][2][lo:hi].any())
            p, m, v = got
    print(f"\n  adamw stand-in {config}: worst share of delta {worst:.3f}")
    assert worst <= 1.0


ADAMW_FAULTS = [("bc_prev", 5000, "coef_wd_step1000"), ("l2", 5000, "coef_wd_step1000"), ("no_coef", 257, "coef_wd_step1000"),
                ("v_unclipped", 256, "coef_wd_step1000"), ("tail", 257, "nocoef_wd0_step1")]


@pytest.mark.parametrize("fault,n,config", ADAMW_FAULTS, ids=[f[0] for f in ADAMW_FAULTS])
def test_adamw_fault_rejected(fault, n, config):
    assert n in R.ADAMW_SIZES
    p, g, m, v, coef, wd, step, _ = adamw_case(n, config)
    exp = R.adamw_expect(p, g, m, v, coef, R.adamw_scalars(weight_decay=wd, step=step, **R.ADAMW_HYP))
    assert failure(adamw_report("adamw", adamw_standin(p, g, m, v, coef, wd, step), exp)) is None
    msg = failure(adamw_report("adamw", adamw_standin(p, g, m, v, coef, wd, step, fault), exp))
    assert msg is not None and "rows over the bound" in msg, fault
    if fault == "tail":
        assert "row (token) 1, cols 0..0" in msg, msg        # element 256, the one element behind the last whole block


def test_old_adamw_criteria_accept_the_dropped_tail():
    """tests/test_train_gpu.py::test_clip_and_adamw_vs_fp32_restatement_and_torch: fewer than 0.2 % of the elements differ from an fp32
    restatement and rel-L2 < 1e-4.  A launch above the grid (the only kind that enters the grid-stride loop) that leaves its last n % 256
    elements alone passes both; the per-element check names the first of them."""
    n = R.ADAMW_SIZES[-1]
    assert n > R.ADAMW_GRID and n % 256 == 5
    p, g, m, v, coef, wd, step, _ = adamw_case(n, "nocoef_wd0_step1")
    good = adamw_standin(p, g, m, v, coef, wd, step)
    bad = adamw_standin(p, g, m, v, coef, wd, step, "tail")
    assert float((bad[0] != good[0]).float().mean()) < R.OLD_ADAMW_MISMATCH
    assert float((bad[0].double() - good[0].double()).norm() / good[0].double().norm()) < R.OLD_ADAMW_REL_L2
    exp = R.adamw_expect(p, g, m, v, coef, R.adamw_scalars(weight_decay=wd, step=step, **R.ADAMW_HYP))
    msg = failure(adamw_report("adamw", bad, exp))
    assert msg is not None and f"row (token) {n // 256}" in msg, msg


def test_grid_stride_size_is_above_the_grid_and_ragged():
    n = R.ADAMW_SIZES[-1]
    assert n > 8192 * 256 and n % 256 and (n + 255) // 256 > 8192
