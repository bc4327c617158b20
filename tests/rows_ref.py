"""float64 references, derived per-element bounds and the shared test inputs of three row / element kernels that every stack uses:
ops.ln_affine (ln_kernel<true>, csrc/elementwise.hip), ops.softmax_rows_ (softmax_rows_kernel, csrc/controlnext.hip) and the f32 ops.adamw_
(adamw_kernel, csrc/train.hip).  No GPU-only code here: tests/test_rows_ref_cpu.py runs the references against f32 stand-ins on the host,
tests/test_rows_fp64_gpu.py against the kernels.  It builds on tests/ew_ref.py (Report / check_rows, the LayerNorm mean and rstd terms and the
operand kinds) and tests/gemm_ref.py (the sentinel helpers, _round_bound).

Every function returns (want, bound, delta) in float64: `want` is the exact value of the operator on the operands the kernel read (bf16 / f32
-> float64 is exact), `delta` bounds what the kernel's f32 evaluation may differ from it by, and bound = delta + the output's own rounding
(1/2 ulp_bf16(|want| + delta) for bf16, u |want| for f32 outputs: gemm_ref._round_bound).  u = U_F32 = 2^-24; SLACK = 1 + 2^-10 covers the
second-order terms of the first-order counts below.

  Affine LayerNorm (ln_kernel<true>).  y = ((x - mu) rstd) w + b, w / b bf16.  Mean, variance and rstd are ln_kernel's common code, bounded as
    ew_ref.ln_expect does -- with one correction for widths that are no multiple of 512: lane l holds the chunks l, l + 64, ..., so the longest
    chain has L = 8 ceil(D / 512) elements, not D / 64 (D = 520: lane 0 holds 16 values, D / 64 = 8.1; D = 64: eight lanes hold 8 values each,
    D / 64 = 1).  An element passes through at most L - 1 chain adds, 6 butterfly levels and the division:
      E_mu = ln_mean_err(x) (L + 6) / (D / 64 + 6)   (= ln_mean_err(x) where 512 divides D; 0 on constant rows),
      e_r  = (L + 10) u / 2 + E_mu^2 / (2 (var + eps)) + LN_RSQRT_ULPS u.
    output.  d = x - mu~ (1 rounding), d rstd~ (1), (.) w (1), (.) + b (1, relative to |y|): four roundings as written.  -ffp-contract=fast may
      turn the last two into one fma, which only removes a rounding, so the uncontracted count is allowed:
      delta = SLACK (rstd |w| (E_mu + |x - mu| (e_r + 3 u)) + u |y|).
    A constant row: mu~ = x exactly (ew_ref), d = 0, 0 rstd w = 0, 0 + b = b: want = b, delta = 0, the element must be bf16(b) = b exactly.
  Row softmax (softmax_rows_kernel).  want = softmax(s x), s the f32 scale the launch receives.  In the exp2 domain t_i = x_i s log2(e).
    The host forms sl = f32(s * 1.4426950408889634f): the constant is f32(log2 e) (u) and the product rounds (u): sl = s log2(e) (1 + e_s),
    |e_s| <= 2 u, the same for every element.  v_i = f32(x_i sl) = t_i (1 + e_s)(1 + e_i), |e_i| <= u; mx = max v_j exactly (fmaxf is exact, and
    rounding is monotone: the maximum is taken at a maximum of t).  w_i = f32(v_i - mx) = (d_i (1 + e_s) + t_i e_i - t_max e_m)(1 + e_w) with
    d_i = t_i - t_max.  t_max e_m moves every exponent alike, and softmax is shift-invariant: the error of mx itself cancels between the
    numerators and their sum.  What remains is each element's own exponent error
      err_i = u |t_i| + 3 u |d_i|          (e_i on t_i; e_s, up to 2 u, and e_w on d_i)
    and the hardware exp2 (EXP2_ULPS u relative): numerator i is exact up to rho_i = 2^err_i (1 + EXP2_ULPS u) - 1.
    sum.  A thread chains its 8 ceil(cols / 2048) <= 64 values, wave_sum adds 6 levels, three adds join the waves: (chain + 9) u relative to
      the sum (all terms positive), on top of the numerators' own errors, which enter with their weights: rho_S = sum_j p_j rho_j.  Terms whose
      exponent is below -126 may be flushed to 0 by v_exp_f32: at most cols 2^-126 of a sum that is >= 1 (the maximum contributes 2^0).
    output.  inv = 1 / sum (correctly rounded, u), e_i inv (u), then bf16:
      delta_i = SLACK p_i (rho_i + rho_S + (chain + 9) u + cols 2^-126 + 2 u) / (1 - rho_S - (chain + 9) u).
    An element whose exact value may lie below the smallest normal f32 (p_i - delta_i < 2^-126) may come out as 0 or as any denormal:
    delta_i = max(delta_i, p_i) there.  A constant row of a power-of-two width: v - mx = 0, exp2(0) = 1, the sum cols and 1 / cols are exact:
    want = 1 / cols = bf16(1 / cols), delta = 0.
  AdamW (adamw_kernel), f32 moments, bf16 parameter.  The launch receives f32 lr, b1, b2, eps, wd, bc1 = f32(1 - beta1^step), bc2
    (adam8_ref.scalars restates them; 1 - b is one f32 subtraction, exact for b >= 1/2, and cannot be contracted: an input here).  The kernel's
    expression is plain C++ (no __f*_rn), so under -ffp-contract=fast any product may be fused into the sum that follows it.  A fusion only
    removes a rounding: every multiply and add is counted.
    m'.  gg = cf g (u); t = (1 - b1) gg (u): 2 u |t|; b1 m (u); the sum (u |m'|, the output's own rounding):
         delta_m = SLACK u (|b1 m| + 2 |t|), bound_m = delta_m + u |m'|.
    v'.  t = ((1 - b2) gg) gg: gg twice (2 u), two products (2 u); b2 v (u): delta_v = SLACK u (b2 v + 4 t), bound_v = delta_v + u v'.
    p'.  From the exact m', v' with dm = bound_m, dv = bound_v propagated.  sqrtf and / are correctly rounded (DIV_SQRT_U = u): build.py
         compiles with -O3 -ffp-contract=fast and neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt, and the code object
         runs with f32 denormals on (the compiler emits the v_div_scale / v_div_fmas / v_div_fixup sequence and a refined v_sqrt_f32).
         mh = m / bc1: dmh = dm / bc1 + DU |mh|;  vh = v / bc2: dvh = dv / bc2 + DU vh;  s = sqrt(vh): ds = SLACK s dvh / (2 vh) + DU s;
         den = s + eps: dden = ds + u den;  num = lr mh: dnum = lr dmh + u |num|;  q = num / den: dq = (dnum + |q| dden) / (den - dden) +
         DU |q|;  decay = 1 - lr wd: the product and the difference round, or one fma does: ddecay = u (lr wd + decay), 0 when wd = 0 (then
         decay = 1 exactly);  p' = p decay - q: the product (u |p decay|, nothing when decay = 1) and the difference (u |p'|, nothing when
         q = 0 exactly: x - 0 = x):  delta_p = SLACK (dq + |p| ddecay + [decay != 1] u |p decay| + [q != 0] u |p'|);  bf16 output.
         A zero gradient on zero moments gives m' = v' = 0 and q = 0 with delta 0: the parameter takes the decay alone, and with wd = 0
         stays bit for bit.

Constants.  No constant is fitted to a kernel's output.  Next to each: the largest share of the f32 part (delta) any launch of
tests/test_rows_fp64_gpu.py used on MI355X, (|err| - rounding part)+ / delta as ew_ref's statistic."""
import math
import zlib

import torch

from tests import adam8_ref
from tests.ew_ref import LN_KINDS, LN_MEAN_SLACK, LN_RSQRT_ULPS, Report, check_rows, const_rows, f32, ln_mean_err, ln_rows  # noqa: F401
from tests.gemm_ref import U_F32, _round_bound, check_untouched, poison_, sentinel_bits, ulp_bf16, write_mask  # noqa: F401

SLACK = 1.0 + 2.0 ** -10
# LN_MEAN_SLACK, LN_RSQRT_ULPS: ew_ref's (rsqrtf is 1 ulp on gfx950, 2 allowed).  Measured share of ln_affine's delta: see LN_SHARE_MEASURED
# v_exp_f32: 1 ulp (AMD Instinct CDNA3 / CDNA4 ISA reference, V_EXP_F32: "base-2 exponent ... 1 ULP accuracy, denormals are flushed"); 2 allowed
EXP2_ULPS = 2.0                  # measured with the sum's terms: at most 0.905 of softmax's delta (SOFTMAX_SHARE_MEASURED)
# sqrtf and the f32 division of the AdamW expression: correctly rounded under the library's compiler flags (see the docstring), relative error u
DIV_SQRT_U = U_F32               # measured with p's other terms: at most 0.824 of delta_p (ADAMW_SHARE_MEASURED)
F32_MIN_NORMAL = 2.0 ** -126
LOG2E = 1.4426950408889634

# measured on MI355X by tests/test_rows_fp64_gpu.py (printed there as WORST; not an input to any bound)
LN_SHARE_MEASURED = 0.056        # (7 x 768; the mean and rstd terms are worst cases over D values, the kernel's errors mostly cancel)
SOFTMAX_SHARE_MEASURED = 0.905   # (3 x 16384; 0.313 at every narrower shape)
ADAMW_SHARE_MEASURED = (0.824, 0.946, 0.979)     # (p, m, v), the launch of 2 097 925 elements: among two million elements one product and one
#                                                  sum both round by nearly half an ulp the same way, which is all of delta_m / delta_v
RMS_SHARE_MEASURED = 0.971       # worst relative error over t5_ref.TOL_ROW (3.87e-3 of 3.98e-3: one bf16 rounding just above a power of two)

# the old whole-tensor criteria, kept only to show what they let through (tests/test_rows_ref_cpu.py)
OLD_REL_L2 = 5e-3                # test_ln_affine, test_softmax_rows_and_batched_weight_gemm
OLD_ADAMW_REL_L2 = 1e-4          # test_clip_and_adamw_vs_fp32_restatement_and_torch ...
OLD_ADAMW_MISMATCH = 2e-3        # ... and its share of elements that differ from an fp32 restatement


# ---------------------------------------------------------------------------------------------------------------- ln_affine
def ln_chain(D):
    """the longest per-lane chain of ln_kernel: lane 0 holds ceil(D / 512) chunks of 8 values"""
    return 8 * ((D + 511) // 512)


def ln_affine_expect(x, w, b, eps):
    """Affine LayerNorm of the rows x [rows, D] (bf16) with weight / bias [D] (bf16): (want, bound, delta) float64 [rows, D]"""
    x, w, b = x.double(), w.double(), b.double()
    D = x.shape[-1]
    L = ln_chain(D)
    mu = x.sum(-1, keepdim=True) / D
    xc = x - mu
    var = (xc * xc).sum(-1, keepdim=True) / D
    epsf = f32(eps)
    rstd = torch.rsqrt(var + epsf)
    want = xc * rstd * w + b
    e_mu = ln_mean_err(x) * ((L + 6) / (D / 64 + 6))
    e_r = 0.5 * (L + 10) * U_F32 + 0.5 * e_mu ** 2 / (var + epsf) + LN_RSQRT_ULPS * U_F32
    delta = SLACK * (rstd * w.abs() * (e_mu + xc.abs() * (e_r + 3 * U_F32)) + U_F32 * want.abs())
    const = const_rows(x)
    delta = torch.where(const, torch.zeros_like(delta), delta)
    want = torch.where(const, b.expand_as(want), want)
    return want, _round_bound(want, delta, False), delta


LN_SHAPES = [(1, 8), (5, 64), (3, 520), (7, 768), (6, 1152), (4, 1024), (2, 3200), (9, 4096)]
LN_EPS = (1e-6, 1e-5)
LN_AFFINE_KINDS = LN_KINDS + ("eps_dominant",)


def seed_of(*key):
    """a stable generator seed from the parameters of a case"""
    return zlib.crc32(repr(key).encode())


def ln_cases():
    """(rows, D, eps, kind, weight / bias variant) of every ln_affine launch: every kind at both eps on every shape, once a weight with a
    zero and a negative chunk, once a bias of 2^9"""
    for rows, D in LN_SHAPES:
        for eps in LN_EPS:
            for kind in LN_AFFINE_KINDS:
                yield rows, D, eps, kind, "plain"
    for eps in LN_EPS:
        yield 3, 520, eps, "random", "zero_neg"
        yield 7, 768, eps, "outlier", "big_bias"


def ln_affine_rows(R, D, kind, gen, device):
    """bf16 [R, D] inputs: ew_ref.ln_rows' kinds (mod_edge is its random kind: the affine branch has no modulation vector), and
    eps_dominant  c + {-1, 0, 1} bf16 ulps around c in +-[0.04, 0.05] (ulp 2^-12): a variance near 4e-8, far below both eps"""
    if kind != "eps_dominant":
        return ln_rows(R, D, kind, gen, device)
    c = (0.04 + 0.01 * torch.rand((R, 1), device=device, generator=gen)).to(torch.bfloat16).double()
    k = torch.randint(-1, 2, (R, D), device=device, generator=gen).double()
    k[:, 0], k[:, 1] = 1.0, -1.0           # never a constant row
    sign = torch.where(torch.arange(R, device=device)[:, None] % 2 == 1, -1.0, 1.0)
    return (sign * (c + k * 2.0 ** -12)).to(torch.bfloat16)


def ln_wb(D, variant, gen, device):
    """bf16 weight and bias [D]: 1 + 0.1 N(0, 1) and 0.1 N(0, 1); `zero_neg`: the first 8-column chunk of the weight 0 and the last one
    negated (one chunk at D = 8: its first half 0, its second negated); `big_bias`: a bias of 2^9"""
    w = (1.0 + 0.1 * torch.randn(D, device=device, generator=gen)).to(torch.bfloat16)
    b = (0.1 * torch.randn(D, device=device, generator=gen)).to(torch.bfloat16)
    if variant == "zero_neg":
        h = 8 if D > 8 else 4
        w[:h] = 0
        w[D - h:] = -w[D - h:].abs()
    elif variant == "big_bias":
        b = torch.full_like(b, 2.0 ** 9)
    else:
        assert variant == "plain", variant
    return w, b


def ln_condition(x, w, b, kind, eps):
    """the coverage condition of an input kind; AssertionError if the generated rows miss it"""
    xd = x.double()
    D = xd.shape[-1]
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1)
    if kind == "large_mean":          # a one-pass variance cancels at least 12 bits
        assert bool((mu[:, 0] ** 2 > 2.0 ** 12 * var).all()), "large_mean: mean^2 <= 2^12 var"
    elif kind == "outlier":
        assert bool((xd.abs().amax(-1) >= 2.0 ** 11).all()), "outlier: no channel at 2^11"
    elif kind == "const":
        assert bool(const_rows(xd).any()), "const: no constant row"
        if xd.shape[0] > 1:
            assert bool((~const_rows(xd)).any()), "const: only constant rows"
    elif kind == "eps_dominant":
        assert bool((var < f32(min(LN_EPS)) / 4).all()) and bool((var > 0).all()), "eps_dominant: variance not below eps / 4"
        other = LN_EPS[1] if eps == LN_EPS[0] else LN_EPS[0]
        w0, b0, _ = ln_affine_expect(x, w, b, eps)
        w1, b1, _ = ln_affine_expect(x, w, b, other)
        assert bool(((w0 - w1).abs() > b0 + b1).any()), "eps_dominant: the other eps moves no element by more than its bound"
    else:
        assert kind in ("random", "mod_edge"), kind
        assert not bool(const_rows(xd).any())
    assert D % 8 == 0


# ---------------------------------------------------------------------------------------------------------------- softmax_rows_
SM_SHAPES = [(1, 8), (40, 96), (3, 256), (3, 2048), (2, 2056), (2, 4104), (3, 16384)]
SM_SCALES = (1.0, 0.25, 512 ** -0.5)
SM_KINDS = ("random", "spike", "max_last", "flat", "twin", "low")


def sm_chain(cols):
    """values a thread of softmax_rows_kernel adds in a chain: 8 per register chunk, ceil(cols / 2048) chunks"""
    return 8 * ((cols + 2047) // 2048)


def softmax_rows_expect(x, scale):
    """softmax(scale x) over the rows x [rows, cols] (bf16), scale a Python float (the launch receives its f32 value): (want, bound, delta)"""
    x = x.double()
    cols = x.shape[-1]
    t = x * (f32(scale) * LOG2E)
    d = t - t.amax(-1, keepdim=True)
    e = torch.exp2(d)
    want = e / e.sum(-1, keepdim=True)
    err = U_F32 * (t.abs() + 3.0 * d.abs())
    rho = torch.exp2(err) * (1.0 + EXP2_ULPS * U_F32) - 1.0
    rho_s = (want * rho).sum(-1, keepdim=True)
    tree = (sm_chain(cols) + 9) * U_F32
    delta = SLACK * want * (rho + rho_s + tree + cols * F32_MIN_NORMAL + 2 * U_F32) / (1.0 - rho_s - tree)
    delta = torch.where(want - delta < F32_MIN_NORMAL, torch.maximum(delta, want), delta)
    if cols & (cols - 1) == 0:
        flat = const_rows(x)
        delta = torch.where(flat, torch.zeros_like(delta), delta)
        want = torch.where(flat, torch.full_like(want, 1.0 / cols), want)
    return want, _round_bound(want, delta, False), delta


def sm_wave_of(col):
    """(wave, thread, register chunk) of softmax_rows_kernel that holds column `col`"""
    ch = col // 8
    return (ch % 256) // 64, ch % 256, ch // 256


def sm_twin_cols(cols):
    """the two columns of the `twin` kind: column 3 (wave 0, thread 0) and the last column -- moved back to the last thread of the pass
    before where the last column falls into wave 0 of a later pass -- so that the two maxima sit in different waves wherever a row spans
    more than one (cols > 512), in different lanes where it spans more than one chunk, and in one lane at cols = 8"""
    c2 = cols // 8 - 1
    if c2 >= 64 and c2 % 256 < 64:
        c2 -= c2 % 256 + 1
    return 3, c2 * 8 + 7


def softmax_rows_in(R, cols, kind, scale, gen, device):
    """bf16 [R, cols] scores of one kind (see SM_KINDS and softmax_condition)"""
    sl = f32(scale) * LOG2E
    x = 4.0 * torch.randn((R, cols), device=device, generator=gen)
    if kind == "spike":            # one column per row ahead by 1.1 * 160 exp2 units and the spread of the rest
        col = torch.randint(0, cols, (R, 1), device=device, generator=gen)
        x.scatter_(1, col, torch.full((R, 1), 176.0 / sl + 48.0, device=device))
    elif kind == "max_last":
        x[:, -1] = 141.0 / sl + 48.0
    elif kind == "flat":
        x = (3.0 * torch.randn((R, 1), device=device, generator=gen)).expand(R, cols)
    elif kind == "twin":
        c1, c2 = sm_twin_cols(cols)
        x[:, c1] = x[:, c2] = 24.0
    elif kind == "low":
        x = -3.0e4 + 256.0 * torch.randn((R, cols), device=device, generator=gen)
    else:
        assert kind == "random", kind
    return x.to(torch.bfloat16).contiguous()


def softmax_condition(x, kind, scale):
    """the coverage condition of an input kind; AssertionError if the generated rows miss it"""
    R, cols = x.shape
    t = x.double() * (f32(scale) * LOG2E)
    tmax = t.amax(-1, keepdim=True)
    if kind == "spike":
        want = softmax_rows_expect(x, scale)[0]
        top = t == tmax
        assert bool((top.sum(-1) == 1).all()), "spike: the maximum is not alone"
        if cols > 1:
            assert bool((torch.where(top, torch.full_like(t, -math.inf), t).amax(-1, keepdim=True) < tmax - 160.0).all()), "spike: lead <= 160"
            assert bool((want[~top] < F32_MIN_NORMAL).all()), "spike: another element is a normal f32"
    elif kind == "max_last":
        head = t[:, :min(2048, cols - 1)]        # the first register chunk's columns (all but the last column of a short row)
        assert bool((t[:, -1:] == tmax).all()) and bool((t[:, -1] - head.amax(-1) > 128.0).all()), \
            "max_last: exp2(t_last - max over the first chunk) does not overflow"
    elif kind == "flat":
        assert bool(const_rows(x.double()).all())
    elif kind == "twin":
        c1, c2 = sm_twin_cols(cols)
        top = t == tmax
        assert bool((top.sum(-1) == 2).all()) and bool(top[:, c1].all()) and bool(top[:, c2].all()), "twin: the maximum is not exactly twice"
        w1, w2 = sm_wave_of(c1), sm_wave_of(c2)
        assert w1[0] != w2[0] if cols > 512 else (w1[1] != w2[1] if cols > 8 else c1 != c2), "twin: both maxima in one wave"
    elif kind == "low":
        assert bool((x.double() < -2.0e4).all()), "low: a score above -2e4"
        assert not bool(const_rows(x.double()).any())
    else:
        assert kind == "random", kind
        assert cols == 8 or not bool(const_rows(x.double()).any())


# ---------------------------------------------------------------------------------------------------------------- adamw_
ADAMW_GRID = 8192 * 256                      # elements one pass of the launch's largest grid covers
ADAMW_SIZES = [1, 255, 256, 257, 5000, ADAMW_GRID + 3 * 256 + 5]
ADAMW_HYP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
# (clip coefficient, weight decay, step, random incoming moments): adam8's two
ADAMW_CONFIGS = {"nocoef_wd0_step1": (None, 0.0, 1, False), "coef_wd_step1000": (0.37, 1e-2, 1000, True)}


def adamw_scalars(*, weight_decay, step, **hyp):
    """adam8_ref.scalars (the f32 values the launch receives) and the f32 weight decay itself"""
    sc = adam8_ref.scalars(weight_decay=weight_decay, step=step, **hyp)
    sc["wd"] = f32(weight_decay)
    return sc


def adamw_expect(p, g, m, v, coef, sc):
    """One ops.adamw_ step from the state the kernel read: p bf16 [n], g / m / v f32 [n], coef the f32 clip coefficient (a float) or None,
    sc = adamw_scalars(...).  Returns {"m", "v", "p": (want, bound, delta)} float64 [n]."""
    u, DU = U_F32, DIV_SQRT_U
    cf = 1.0 if coef is None else float(coef)
    gg = cf * g.double()
    bm, bv = sc["b1"] * m.double(), sc["b2"] * v.double()
    t_m = sc["omb1"] * gg
    t_v = sc["omb2"] * gg * gg
    mn, vn = bm + t_m, bv + t_v
    delta_m = SLACK * u * (bm.abs() + 2 * t_m.abs())
    delta_v = SLACK * u * (bv.abs() + 4 * t_v)
    dm, dv = _round_bound(mn, delta_m, True), _round_bound(vn, delta_v, True)
    z = torch.zeros_like(mn)
    mh = mn / sc["bc1"]
    dmh = dm / sc["bc1"] + DU * mh.abs()
    vh = vn / sc["bc2"]
    dvh = dv / sc["bc2"] + DU * vh
    s = vh.sqrt()
    ds = torch.where(vh > 0, SLACK * s * dvh / (2 * vh.clamp_min(1e-300)) + DU * s, z)
    den = s + sc["eps"]
    dden = ds + u * den
    num = sc["lr"] * mh
    dnum = sc["lr"] * dmh + u * num.abs()
    q = num / den
    dq = (dnum + q.abs() * dden) / (den - dden) + DU * q.abs()
    lw = sc["lr"] * sc["wd"]
    decay = 1.0 - lw
    ddecay = u * (lw + decay) if lw != 0.0 else 0.0
    pd = p.double() * decay
    pn = pd - q
    r_prod = u * pd.abs() if decay != 1.0 else z
    r_diff = torch.where((q == 0) & (dq == 0), z, u * pn.abs())
    delta_p = SLACK * (dq + p.double().abs() * ddecay + r_prod + r_diff)
    return {"m": (mn, dm, delta_m), "v": (vn, dv, delta_v), "p": (pn, _round_bound(pn, delta_p, False), delta_p)}


def _loguniform(n, lo, hi, gen, device):
    return torch.pow(10.0, lo + (hi - lo) * torch.rand(n, device=device, generator=gen, dtype=torch.float64))


def _sign(n, gen, device):
    return torch.where(torch.rand(n, device=device, generator=gen) < 0.5, -1.0, 1.0).double()


def adamw_zero_stretch(n):
    """[lo, hi) of the elements whose gradient and moments are exactly 0 (none at n < 4)"""
    lo = n // 3
    return lo, lo + min(17, n // 4)


def adamw_gradient(n, gen, device):
    """f32 [n]: log-uniform in [1e-12, 1e4] with random sign (no f32 subnormal anywhere in the step), exact zeros on the zero stretch"""
    g = (_loguniform(n, -12, 4, gen, device) * _sign(n, gen, device)).float()
    lo, hi = adamw_zero_stretch(n)
    g[lo:hi] = 0
    return g


def adamw_state(n, random_moments, gen, device):
    """(p bf16 [n] log-uniform 1e-4 .. 1 with random sign, m f32 [n], v f32 [n]): zero moments, or m spanning 1e-8 .. 1e2 with random sign
    and v 1e-16 .. 1e4, zero on the zero stretch"""
    p = (_loguniform(n, -4, 0, gen, device) * _sign(n, gen, device)).to(torch.bfloat16)
    if random_moments:
        m = (_loguniform(n, -8, 2, gen, device) * _sign(n, gen, device)).float()
        v = _loguniform(n, -16, 4, gen, device).float()
        lo, hi = adamw_zero_stretch(n)
        m[lo:hi] = 0
        v[lo:hi] = 0
    else:
        m, v = torch.zeros(n, device=device), torch.zeros(n, device=device)
    return p, m, v


def adamw_condition(n, g, m, v, random_moments):
    """the coverage conditions of the generated AdamW operands"""
    lo, hi = adamw_zero_stretch(n)
    inside = torch.zeros(n, dtype=torch.bool, device=g.device)
    inside[lo:hi] = True
    assert hi - lo == (0 if n < 4 else min(17, n // 4))
    assert bool((g[inside] == 0).all()) and bool((m[inside] == 0).all()) and bool((v[inside] == 0).all()), "the zero stretch is not zero"
    ga = g[~inside].double().abs()
    assert bool((ga >= 0.99e-12).all()) and bool((ga <= 1.01e4).all()), "a gradient outside [1e-12, 1e4]"
    if random_moments:
        assert bool((m[~inside].double().abs() >= 0.99e-8).all()) and bool((v[~inside].double() >= 0.99e-16).all()), "a moment below its range"
    else:
        assert not bool(m.any()) and not bool(v.any())


# ---------------------------------------------------------------------------------------------------------------- checking flat vectors
def check_flat(rep, got, exp, what="", width=256):
    """got [n] against exp = (want, bound, delta) [n] through Report: element i is row i // width, column i % width of the message"""
    n = got.numel()
    pad = -n % width
    g = torch.nn.functional.pad(got.double().reshape(-1), (0, pad)).view(-1, width)
    want, bound, delta = (torch.nn.functional.pad(t.reshape(-1), (0, pad)).view(-1, width) for t in exp)
    rows = torch.arange(g.shape[0], device=g.device)
    return rep.check(g, want, bound, delta, sample=torch.zeros_like(rows), token=rows, what=what, unit=1)
