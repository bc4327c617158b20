"""float64 references of the training backward's row and element kernels (csrc/train.hip) and the bounds their outputs are held to, element
by element, with the checker of tests/ew_ref.py (Report / check_rows: the message names the launch, the sample, the row and the columns).
No GPU-only code here: tests/test_train_ref_cpu.py proves the bounds on f32 stand-ins of the kernels' arithmetic on the host,
tests/test_train_fp64_gpu.py holds the kernels to them.

Every function returns (want, bound, delta) in float64.  `want` is the exact operator on the operands the kernel read (bf16 / f32 -> float64
is exact), `delta` the f32 part of the bound -- the roundings of the kernel's own order of operations, counted below -- and `bound` adds the
output's single rounding: 1/2 ulp_bf16(|want| + delta) for bf16 outputs, U_F32 |want| for f32 outputs that are rounded once more; f32
partial sums ARE the f32 accumulators, so their bound is delta alone.  u = U_F32 = 2^-24.  A sum of n terms through any fixed tree of depth k
carries at most k u sum|terms| (first order); S = TRAIN_SLACK covers the second-order terms.

  Row sums.  Both forms of ln_mod_bwd reduce a row of D values: the wave-per-row kernel chains 8 ceil(D / 512) elements per lane (the
    first add is exact), wave_sum adds 6 levels, / D one rounding: 8 ceil(D/512) + 6.  The workgroup form chains 8 elements per thread (7),
    wave_sum_lane63 6 levels, block_sums' 8-slot LDS sum 7 (slots of waves that do not exist hold 0: exact adds), * fl(1 / D) two: 22.
    sum_depth(D) = max(8 ceil(D/512) + 7, 23) covers both (ew_ref.ln_mean_err's D/64 + 6 is the forward kernel's count and does not cover the
    LDS sum at D = 256, so the count is restated here; LN_MEAN_SLACK, LN_RSQRT_ULPS and const_rows are ew_ref's).
  ln_mod_bwd.  K = sum_depth(D).  mean: E_mu = S K u sum|x| / D; a constant row c is exact in the wave form (D c and D c / D are exact) and in
    the workgroup form whenever 2 |D fl(1/D) - 1| <= u (then fl(D c fl(1/D)) = c for every bf16 c: true for every D the model or the tests
    use), else E_mu = (|D fl(1/D) - 1| + u) |c| (const_mean_err).  rstd as ew_ref.ln_expect: e_r = (K + 4) u / 2 + E_mu^2 / (2 (var + eps))
    + LN_RSQRT_ULPS u.  xhat = (x - mu~) rstd~: E_xh = rstd (E_mu + |x - mu| (e_r + 2 u)); constant rows: rstd = 1 / sqrt(eps), xhat = 0,
    E_xh = 0 exactly.  g = dy fl(1 + m): 2 u |g|.  mean(g): E_mg = (K + 2) u sum|g| / D.  mean(g xhat): E_mgx = (sum |g| E_xh + (K + 2) u
    sum |g| (|xhat| + E_xh)) / D.  t = g - mg - xhat mgx (two subtractions and a product, each relative to at most |g| + |mg| + |xhat mgx|):
    E_t = 2 u |g| + E_mg + |xhat| E_mgx + E_xh (|mgx| + E_mgx) + 2 u (|g| + |mg| + |xhat mgx|).  dX = dXin + rstd~ t~:
    delta = S rstd (E_t + (|t| + E_t) (e_r + u)) + u |want| (the add of dXin, or of 0: then an over-estimate by u); bf16 output.
    partial[b][w][0] = sum_rows dy xhat~ (fma chain over the n live rows of the group, a dead row of a half-live step adds fma(0, 0, a)
    exactly): delta = sum |dy| E_xh + n u sum |dy| (|xhat| + E_xh).  partial[b][w][1] = sum_rows dy: (n - 1) u sum|dy| -- exact for
    R = 1.  f32 accumulators: bound = delta.
  gate_bwd.  dT = fmaf(gate, dX, G): u |want| (gate = None and G = None: a copy, delta = 0); bf16.  partial = fma chain over the n rows:
    n u sum |dX T|; bound = delta.
  reduce_rows.  Wave w of 16 adds rows w, w + 16, ..: 8 accumulators of at most ceil(np / 128) adds each, one of them the tail's, a 3-level
    tree, then the 16-slot LDS sum: at most ceil(np / 16) + 4 + 16 = A(np) roundings.  out = alpha t (+ old): delta = |alpha| A u sum|terms|
    (+ u |alpha t| for the product under accumulate), bound = delta + u |want|.
  softmax_pad.  a = x sl2 - mx with sl2 = fl(scale log2 e) (host, 2 u relative), E_a = u (|x sl2| + |mx|) + 3 u |a|; e = exp2(a):
    r = ln 2 E_a + SM_EXP2_ULPS u relative; the sum: chain 8 ceil(Ct / 512) + 6 levels = Ks; 1 / sum and the product 2 u:
    delta = P (r_j + sum_k P_k r_k + (Ks + 2) u) + SM_TAIL (exp2 flushes below 2^-126); bf16.  Padding rows / columns up to (Rt, Ct) are
    +0 bit-exactly, columns Ct .. ld keep the sentinel.
  softmax_bwd.  On the bf16 P the kernel reads: dot = fma chain + tree: E_dot = Ks u sum |P dP|; dS = scale P (dP - dot):
    delta = |scale P| (E_dot + u (|dP| + |dot|)) + 2 u |want|; bf16; same padding rules.
  act_bwd.  dA act'(pre) with act' evaluated in f32 from terms that cancel (1 + tanh, 1 - tanh^2, 1 + erf, 1 - sigmoid): the error is relative to
    the terms' magnitudes M(x), not to act'.  GELU-tanh: M = 1 + |x| c (1 + 3 a x^2); GELU-erf: M = 1 + |x| phi(x); SiLU: M = sig (1 + |x|).
    delta = |dA| (U_ACT M + ACT_TAIL (1 + |x|)) (gemm_ref's allowances for the same f32 functions; the tail: exp over- / underflow gives +-0
    where the exact value is a denormal); bf16, or f32 with + u |want|.
  qkv_split_bwd.  dn = RoPE^T dy: E_dn = 2 u (|dy_j c_j| + |dy_j' s|); ss = sum x^2 over 128: 8-chain + 4 shuffle levels: 12 u; r =
    rsqrt(ss / 128 + eps): e_r = 7 u + LN_RSQRT_ULPS u; dot = sum dn w x: E_dot = sum |w x| E_dn + 14 u sum |dn w x|; k = r^3 / 128 dot:
    E_k = |k| (3 e_r + 4 u) + r^3 / 128 E_dot; o = r w dn - x k: delta = S (|r w dn| (e_r + 3 u) + r |w| E_dn + |x| E_k + u |x k|) +
    u |want|; bf16.  dv is a copy: exact.  Columns 3 H 128 .. ldd of d0 / d1 keep the sentinel.
  skinny_bwd.  partial[chunk][b][k] = fma chain over the chunk's n rows: n u sum |dy W|, bound = delta; the reduced result adds
    reduce_rows' A(nchunk) u sum |partial| and its output rounding.
  kd_loss.  K = 8 ceil(D/512) + 7.  u_ = x - mean: E_m = S K u sum|x| / D (constant rows 0); sd = sqrt(sum u_^2 / (D - 1)):
    e_sd = ((K + 3) u + D E_m^2 / sum u_^2) / 2 + KD_SQRT_ULPS u; c = 1 / (fl(1e-7) + sd): e_c = e_sd + 2 u; k = c fl(1 / T): e_k = e_c + 2 u;
    z = u_ k: E_z = |k| (E_m + u |u_|) + |z| (e_k + u).  lse = mx + logf(sum expf(z - mx)): E_lse = sum_j sm_j (E_z_j + u |z_j - mx|) +
    (K + KD_EXP_ULPS) u + KD_LOG_ULPS u |log sum| + u |lse|.  lp = z - lse: E_lp = E_z + E_lse + u (|lp| + |z|), lq likewise; p = expf(lp):
    e_p = E_lp + KD_EXP_ULPS u; d = lp - lq: E_d = E_lp + E_lq + u |d|; row loss = sum p d: delta = sum p (E_d + |d| e_p) + K u sum p |d|,
    f32: + u |want|.  Gradient: dsh = p (d - rl) / T: E_dsh = p (E_d + E_rl + u |d - rl|) / T + |dsh| (e_p + 3 u); md = mean dsh:
    E_md = (sum E_dsh + K u sum |dsh|) / D; sdu = sum dsh u_: E_sdu = sum (E_dsh |u_| + |dsh| (E_m + u |u_|)) + K u sum |dsh u_|;
    kk = c^2 sdu / ((D - 1) sd): E_kk = |kk| (2 e_c + e_sd + 4 u) + c^2 / ((D - 1) sd) E_sdu -- and kk = 0, E_kk = 0 on a row with sd = 0,
    the kernel's documented convention (autograd gives NaN there); o = ls (c (dsh - md) - kk u_): delta = S |ls| (c (E_dsh + E_md +
    u |dsh - md|) + |c (dsh - md)| (e_c + u) + |u_| E_kk + |kk| (E_m + 2 u |u_|) + u |inner|) + u |want|; bf16.
  conv5x5_wgrad / plane_dot / sum_all.  Per-thread fma (add) chain, wave_sum 6, four wave sums 3, then reduce_rows:
    (chain + 9 + A(np)) u sum |terms| (+ u for the square of sum_all's squares mode), + u |want|.
  clip_coef.  norm = sqrtf(sumsq): CLIP_SQRT_ULPS u; coef = fminf(1, max / (norm + fl(1e-6))): (CLIP_SQRT_ULPS + 2 + CLIP_DIV_ULPS) u
    relative, exactly 1 where max / (norm + 1e-6) exceeds 1 by more than that.
  transpose: a copy, bit-exact; the destination outside the [C, R] tiles keeps the sentinel.

Constants that cannot be counted from the code (next to each the largest share of its kernel's f32 allowance that any launch of
tests/test_train_fp64_gpu.py used on MI355X: max over elements of (|err| - rounding part)+ / delta; see MEASURED below)."""
import math

import torch

from tests.ew_ref import LN_MEAN_SLACK, LN_RSQRT_ULPS, SIN_EXP_ULPS, const_rows, f32
from tests.gemm_ref import (ACT_GELU_ERF, ACT_GELU_TANH, ACT_SILU, ACT_TAIL, U_ACT, U_F32, _round_bound, dact_f64)

u = U_F32
# second-order terms of every first-order count above (ew_ref.LN_MEAN_SLACK: 1 + 2^-10)
TRAIN_SLACK = LN_MEAN_SLACK
# exp2 of softmax_pad (v_exp_f32: 1 ulp; 2 allowed, as ew_ref.SIN_EXP_ULPS for expf).  Measured: 0.067 of softmax_pad's allowance
SM_EXP2_ULPS = SIN_EXP_ULPS
SM_TAIL = 2.0 ** -126
# kd_loss: expf as ew_ref (2 ulps), logf 1 ulp = 2 u on gfx950 (2 ulps allowed), sqrtf correctly rounded (1 allowed).  Measured: 0.092 of
# kd_loss's allowance (row loss and gradient together); U_ACT / ACT_TAIL of gemm_ref in act_bwd: 0.031 (bf16), 0.252 (f32)
KD_EXP_ULPS = SIN_EXP_ULPS
KD_LOG_ULPS = 4.0
KD_SQRT_ULPS = 1.0
# clip_coef: sqrtf as above, the f32 division 1 ulp (2.5 allowed: the bound of a division that is not correctly rounded).  Measured: 0.249
CLIP_SQRT_ULPS = 1.0
CLIP_DIV_ULPS = 2.5

# MEASURED (MI355X, tests/test_train_fp64_gpu.py, profiles/train_fp64_gputest.log): worst share of the f32 allowance per kernel; no constant
# above had to be raised.  ln_mod_bwd / gate_bwd: set by elements whose f32 value lands next to a bf16 midpoint, where the last fma's own
# rounding (u |want|) is most of the allowance; skinny_bwd: a last chunk of ONE row (N = 257, chunk = 256) is a single rounded product
# against an allowance of exactly one rounding.
MEASURED = {"ln_mod_bwd wg": 0.488, "ln_mod_bwd wave": 0.488, "gate_bwd wg": 0.693, "gate_bwd wave": 0.693, "reduce_rows": 0.125,
            "softmax_pad": 0.067, "softmax_bwd": 0.048, "act_bwd bf16": 0.031, "act_bwd f32": 0.252, "qkv_split_bwd": 0.066,
            "skinny_bwd": 0.982, "kd_loss": 0.092, "conv5x5_wgrad": 0.000, "plane_dot": 0.002, "sum_all": 0.009, "clip_coef": 0.249}

# the whole-tensor rel-L2 thresholds of tests/test_train_gpu.py, kept here only to show what they miss (tests/test_train_ref_cpu.py)
OLD_LN_BWD_DX_REL_L2 = 1e-2
OLD_LN_BWD_PARTIAL_REL_L2 = 5e-3
OLD_GATE_BWD_REL_L2 = 5e-3
OLD_SOFTMAX_REL_L2 = 5e-3
OLD_ACT_BWD_REL_L2 = 5e-3
OLD_QKV_BWD_REL_L2 = 5e-3
OLD_SKINNY_BWD_REL_L2 = 1e-5
OLD_KD_GRAD_REL_L2 = 1e-2
OLD_PROJ_REL_L2 = 2e-2


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def sum_depth(D):
    """f32 roundings of a row sum / D in either form of ln_mod_bwd (module docstring)"""
    return max(8 * ((D + 511) // 512) + 7, 23)


def reduce_depth(n):
    """A(np) of reduce_rows_kernel"""
    return (n + 15) // 16 + 4 + 16


def const_mean_err(D):
    """relative error of the mean of a constant row (0 whenever fl(D c fl(1 / D)) = c for every bf16 c)"""
    d = abs(D * f32(1.0 / D) - 1.0)
    return 0.0 if 2 * d <= u else d + u


def group_rows(S, R):
    """[nw] live rows of every row group"""
    nw = (S + R - 1) // R
    return [min(S, (w + 1) * R) - w * R for w in range(nw)]


def _groups(t, R):
    """[B, S, D] -> [B, nw, R, D], zero rows behind S"""
    B, S, D = t.shape
    nw = (S + R - 1) // R
    p = torch.zeros((B, nw * R, D), dtype=t.dtype, device=t.device)
    p[:, :S] = t
    return p.view(B, nw, R, D)


# ---------------------------------------------------------------------------------------------------------------- ln_mod_bwd / gate_bwd
def ln_mod_bwd_expect(X, dY, m, dXin, *, R, mult_is_scale=True, eps=1e-6):
    """x2i_ln_mod_bwd_bf16 on X, dY (and dXin or None) bf16 [B, S, D] views, m f32 [B, D] (mult_is_scale) or [D]:
    ((want, bound, delta) of dX [B, S, D], (want, bound, delta) of partial [B, nw, 2, D])."""
    x, dy = X.double(), dY.double()
    B, S, D = x.shape
    K, SL = sum_depth(D), TRAIN_SLACK
    mu = x.sum(-1, keepdim=True) / D
    xc = x - mu
    var = (xc * xc).sum(-1, keepdim=True) / D
    epsf = f32(eps)
    rstd = torch.rsqrt(var + epsf)
    xh = xc * rstd
    const = const_rows(x)
    e_mu = torch.where(const, const_mean_err(D) * x[..., :1].abs(), SL * K * u * x.abs().sum(-1, keepdim=True) / D)
    e_r = 0.5 * (K + 4) * u + 0.5 * e_mu ** 2 / (var + epsf) + LN_RSQRT_ULPS * u
    e_xh = rstd * (e_mu + xc.abs() * (e_r + 2 * u))
    mul = (1.0 + m.double()).view(B, 1, D) if mult_is_scale else m.double().view(1, 1, D)
    g = dy * mul
    ag = g.abs()
    mg = g.sum(-1, keepdim=True) / D
    mgx = (g * xh).sum(-1, keepdim=True) / D
    t = g - mg - xh * mgx
    want = rstd * t
    if dXin is not None:
        want = want + dXin.double()
    e_mg = (K + 2) * u * ag.sum(-1, keepdim=True) / D
    e_mgx = ((ag * e_xh).sum(-1, keepdim=True) + (K + 2) * u * (ag * (xh.abs() + e_xh)).sum(-1, keepdim=True)) / D
    e_t = 2 * u * ag + e_mg + xh.abs() * e_mgx + e_xh * (mgx.abs() + e_mgx) + 2 * u * (ag + mg.abs() + (xh * mgx).abs())
    delta = SL * rstd * (e_t + (t.abs() + e_t) * (e_r + u)) + u * want.abs()
    dx = (want, _round_bound(want, delta, False), delta)
    n = torch.tensor(group_rows(S, R), dtype=torch.float64, device=x.device).view(1, -1, 1)
    gy, gx, ge = _groups(dy, R), _groups(xh, R), _groups(e_xh, R)
    p0 = (gy * gx).sum(2)
    d0 = (gy.abs() * ge).sum(2) + n * u * (gy.abs() * (gx.abs() + ge)).sum(2)
    p1 = gy.sum(2)
    d1 = (n - 1) * u * gy.abs().sum(2)
    pw, pd = torch.stack((p0, p1), 2), torch.stack((d0, d1), 2)
    return dx, (pw, pd, pd)


def gate_bwd_expect(dX, T, gate, G, *, R):
    """x2i_gate_bwd_bf16: dX (T, G or None) bf16 [B, S, D] views, gate f32 [B, D] or None: ((want, bound, delta) of dT, of partial [B, nw, D]
    or None without a gate)."""
    d = dX.double()
    B, S, D = d.shape
    want = d * gate.double().view(B, 1, D) if gate is not None else d.clone()
    if G is not None:
        want = want + G.double()
    delta = u * want.abs() if (gate is not None or G is not None) else torch.zeros_like(want)
    dt = (want, _round_bound(want, delta, False), delta)
    if gate is None:
        return dt, None
    n = torch.tensor(group_rows(S, R), dtype=torch.float64, device=d.device).view(1, -1, 1)
    prod = _groups(d * T.double(), R)
    pd = n * u * prod.abs().sum(2)
    return dt, (prod.sum(2), pd, pd)


# ---------------------------------------------------------------------------------------------------------------- reduce_rows and the sums
def reduce_rows_expect(inp, *, alpha=1.0, old=None, extra=None):
    """x2i_reduce_rows_f32 on inp f32 [nz, np, len] (a view of what the kernel read); old [nz, len]: the output before an accumulating
    launch; extra [nz, len]: error the terms themselves carry (first stage of a two-stage sum).  (want, bound, delta) [nz, len]."""
    t = inp.double()
    np_ = t.shape[1]
    a = f32(alpha)
    s = a * t.sum(1)
    delta = abs(a) * reduce_depth(np_) * u * t.abs().sum(1)
    if extra is not None:
        delta = delta + abs(a) * extra
    want = s
    if old is not None:
        want = old.double() + s
        delta = delta + u * s.abs()
    return want, delta + u * want.abs(), delta


def sum_all_expect(x, squares, nblocks=256):
    """ops.sum_all (no accumulate): (want, bound, delta) [1]"""
    t = x.double().reshape(-1)
    if squares:
        t = t * t
    chain = (t.numel() + nblocks * 256 - 1) // (nblocks * 256)
    delta = (chain + 9 + (1 if squares else 0) + reduce_depth(nblocks)) * u * t.abs().sum().view(1)
    want = t.sum().view(1)
    return want, delta + u * want.abs(), delta


def plane_dot_expect(x, dy, alpha=1.0, nchunk=64):
    """ops.plane_dot: x bf16 [B, C, S, H], dy bf16 [B, S, H]: (want, bound, delta) [C]"""
    B, C = x.shape[:2]
    p = x.double().reshape(B, C, -1) * dy.double().reshape(B, 1, -1)
    plane8 = p.shape[-1] // 8
    per = (plane8 + nchunk - 1) // nchunk
    chain = 8 * ((per + 255) // 256)
    a = f32(alpha)
    want = a * p.sum((0, 2))
    delta = abs(a) * (chain + 9 + reduce_depth(B * nchunk)) * u * p.abs().sum((0, 2))
    return want, delta + u * want.abs(), delta


def conv5x5_wgrad_expect(x, dy):
    """ops.conv5x5_wgrad: x bf16 [B, C, S, H], dy bf16 [B, S, H]: dw[c][ds][dh] = sum dy[b][s][h] x[b][c][s + ds - 2][h + dh - 2];
    (want, bound, delta) [C, 25]"""
    B, C, S, H = x.shape
    xp = torch.nn.functional.pad(x.double(), (2, 2, 2, 2))
    d = dy.double()[:, None]
    want = torch.zeros((C, 25), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(want)
    for ds in range(5):
        for dh in range(5):
            p = d * xp[:, :, ds:ds + S, dh:dh + H]
            want[:, ds * 5 + dh] = p.sum((0, 2, 3))
            mag[:, ds * 5 + dh] = p.abs().sum((0, 2, 3))
    chain = 16 * 8 * ((H // 8 + 255) // 256)
    delta = (chain + 9 + reduce_depth(B * ((S + 15) // 16))) * u * mag
    return want, delta + u * want.abs(), delta


def clip_coef_expect(sumsq, max_norm):
    """ops.clip_coef: sumsq f32 [1]: (want, bound, delta) [2] = (coef, norm); every rounding is in delta"""
    nrm = sumsq.double().view(1).sqrt()
    raw = f32(max_norm) / (nrm + f32(1e-6))
    r = (CLIP_SQRT_ULPS + 2 + CLIP_DIV_ULPS) * u
    dc = torch.where(raw * (1 - r) > 1.0, torch.zeros_like(raw), r * raw)
    want, delta = torch.cat((raw.clamp_max(1.0), nrm)), torch.cat((dc, CLIP_SQRT_ULPS * u * nrm))
    return want, delta, delta


# ---------------------------------------------------------------------------------------------------------------- softmax
def _sm_depth(Ct):
    return 8 * ((Ct // 8 + 63) // 64) + 6


def softmax_pad_expect(x, Cv, scale):
    """valid part of x2i_softmax_pad_bf16: x bf16 [rows, Ct] (the valid rows), columns < Cv: (want, bound, delta) [rows, Cv]"""
    Ct = x.shape[-1]
    sl2 = f32(f32(scale) * f32(1.4426950408889634))
    v = x.double()[:, :Cv]
    a = (v - v.amax(-1, keepdim=True)) * sl2
    P = torch.softmax(v * f32(scale), -1)
    e_a = u * ((v * sl2).abs() + (v.amax(-1, keepdim=True) * sl2).abs()) + 3 * u * a.abs()
    r = math.log(2.0) * e_a + SM_EXP2_ULPS * u
    delta = TRAIN_SLACK * P * (r + (P * r).sum(-1, keepdim=True) + (_sm_depth(Ct) + 2) * u) + SM_TAIL
    return P, _round_bound(P, delta, False), delta


def softmax_bwd_expect(P, dP, Cv, scale):
    """valid part of x2i_softmax_bwd_bf16: P, dP bf16 [rows, Ct] as the kernel read them: (want, bound, delta) [rows, Cv]"""
    Ct = P.shape[-1]
    p, g = P.double()[:, :Cv], dP.double()[:, :Cv]
    sc = f32(scale)
    dot = (p * g).sum(-1, keepdim=True)
    e_dot = _sm_depth(Ct) * u * (p * g).abs().sum(-1, keepdim=True)
    want = sc * p * (g - dot)
    delta = TRAIN_SLACK * (sc * p).abs() * (e_dot + u * (g.abs() + dot.abs())) + 2 * u * want.abs()
    return want, _round_bound(want, delta, False), delta


def check_softmax_layout(name, buf, nz, Rt, Rv, Ct, Cv, ld):
    """buf bf16 [nz, Rt, ld] after softmax_pad_ / softmax_bwd_: rows >= Rv and columns Cv .. Ct hold +0 bit-exactly, columns Ct .. ld the
    sentinel"""
    from tests.gemm_ref import sentinel_bits
    bits = buf.view(torch.int16).view(nz, Rt, ld)
    for what, z in (("padding row", bits[:, Rv:, :Ct]), ("padding column", bits[:, :Rv, Cv:Ct])):
        if bool((z != 0).any()):
            i = [int(v) for v in torch.nonzero(z != 0)[0]]
            off = (Rv, 0) if what == "padding row" else (0, Cv)
            raise AssertionError(f"{name}: {what} not +0: sample {i[0]}, row {i[1] + off[0]}, cols {i[2] + off[1]}..: bits "
                                 f"{int(z[tuple(i)]) & 0xFFFF:#06x}, {int((z != 0).sum())} elements")
    ok = sentinel_bits(buf.view(nz, Rt, ld)[:, :, Ct:])
    if not bool(ok.all()):
        i = [int(v) for v in torch.nonzero(~ok)[0]]
        raise AssertionError(f"{name}: written beyond Ct: sample {i[0]}, row {i[1]}, cols {Ct + i[2]}..")


# ---------------------------------------------------------------------------------------------------------------- act_bwd
def act_bwd_expect(dA, pre, act, out_f32=False):
    """x2i_act_bwd: dA (before the launch), pre [rows, cols] bf16 or f32: (want, bound, delta)"""
    d, x = dA.double(), pre.double()
    want = d * dact_f64(x, act)
    ax = x.abs()
    if act == ACT_GELU_TANH:
        M = 1.0 + ax * math.sqrt(2.0 / math.pi) * (1.0 + 3 * 0.044715 * x * x)
    elif act == ACT_GELU_ERF:
        M = 1.0 + ax * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    else:
        assert act == ACT_SILU, act
        M = torch.sigmoid(x) * (1.0 + ax)
    delta = d.abs() * (U_ACT * M + ACT_TAIL * (1.0 + ax))
    return want, _round_bound(want, delta, out_f32), delta


# ---------------------------------------------------------------------------------------------------------------- qkv_split_bwd
def qkv_split_bwd_rows(rows, dy, nw, c, s, *, H, eps=1e-6):
    """dq or dk rows of x2i_qkv_split_bwd_bf16: rows bf16 [m, H 128] (the saved pre-norm q or k section), dy [m, H, 128] (dQ / dK at the rows'
    tokens), nw bf16 [128], c / s float64 [m, 128] (the interleaved tables as the kernel reads them): (want, bound, delta) [m, H 128]"""
    m = rows.shape[0]
    x = rows.double().view(m, H, 128)
    g = dy.double().view(m, H, 128)
    w = nw.double().view(1, 1, 128)
    c, s = c.view(m, 1, 128), s.view(m, 1, 128)
    ge, go = g[..., 0::2], g[..., 1::2]
    dn = torch.empty_like(g)
    dn[..., 0::2] = ge * c[..., 0::2] + go * s[..., 1::2]
    dn[..., 1::2] = -ge * s[..., 0::2] + go * c[..., 1::2]
    e_dn = torch.empty_like(g)
    e_dn[..., 0::2] = 2 * u * ((ge * c[..., 0::2]).abs() + (go * s[..., 1::2]).abs())
    e_dn[..., 1::2] = 2 * u * ((ge * s[..., 0::2]).abs() + (go * c[..., 1::2]).abs())
    ss = (x * x).sum(-1, keepdim=True)
    r = torch.rsqrt(ss / 128 + f32(eps))
    e_r = 7 * u + LN_RSQRT_ULPS * u
    dot = (dn * w * x).sum(-1, keepdim=True)
    e_dot = ((w * x).abs() * e_dn).sum(-1, keepdim=True) + 14 * u * (dn * w * x).abs().sum(-1, keepdim=True)
    k = r ** 3 / 128 * dot
    e_k = k.abs() * (3 * e_r + 4 * u) + r ** 3 / 128 * e_dot
    want = r * w * dn - x * k
    delta = TRAIN_SLACK * ((r * w * dn).abs() * (e_r + 3 * u) + r * w.abs() * e_dn + x.abs() * e_k + u * (x * k).abs()) + u * want.abs()
    want, delta = want.reshape(m, H * 128), delta.reshape(m, H * 128)
    return want, _round_bound(want, delta, False), delta


# ---------------------------------------------------------------------------------------------------------------- skinny_bwd
def skinny_bwd_expect(dy, W, chunk):
    """x2i_skinny_linear_bwd: dy f32 [B, N], W bf16 [N, K]: ((want, bound, delta) of partial [nchunk, B, K], of the reduced [B, K])"""
    B, N = dy.shape
    Wd, d = W.double(), dy.double()
    nchunk = (N + chunk - 1) // chunk
    pw, pd = [], []
    for i in range(nchunk):
        lo, hi = i * chunk, min(N, (i + 1) * chunk)
        pw.append(d[:, lo:hi] @ Wd[lo:hi])
        pd.append((hi - lo) * u * (d[:, lo:hi].abs() @ Wd[lo:hi].abs()))
    pw, pd = torch.stack(pw), torch.stack(pd)
    K = W.shape[1]
    want, bound, delta = reduce_rows_expect(pw.view(1, nchunk, B * K), extra=pd.sum(0).view(1, B * K))
    delta = delta + reduce_depth(nchunk) * u * pd.sum(0).view(1, B * K)          # (the partials the kernel summed are within pd of pw)
    return (pw, pd, pd), (want.view(B, K), (delta + u * want.abs()).view(B, K), delta.view(B, K))


# ---------------------------------------------------------------------------------------------------------------- kd_loss
def _kd_side(x, inv_t, K):
    """z = normalize(x) / T and its log-softmax with their f32 allowances, x float64 [rows, D]"""
    D = x.shape[-1]
    m = x.sum(-1, keepdim=True) / D
    c0 = const_rows(x)
    e_m = torch.where(c0, torch.zeros_like(m), TRAIN_SLACK * K * u * x.abs().sum(-1, keepdim=True) / D)
    uu = x - m
    q = (uu * uu).sum(-1, keepdim=True)
    sd = torch.sqrt(q / (D - 1))
    e_sd = torch.where(q > 0, 0.5 * ((K + 3) * u + D * e_m ** 2 / q.clamp_min(1e-300)) + KD_SQRT_ULPS * u, torch.zeros_like(q))
    c = 1.0 / (f32(1e-7) + sd)
    e_c = e_sd + 2 * u
    k = c * inv_t
    e_k = e_c + 2 * u
    z = uu * k
    e_z = k * (e_m + u * uu.abs()) + z.abs() * (e_k + u)
    mx = z.amax(-1, keepdim=True)
    sm = torch.softmax(z, -1)
    lse = torch.logsumexp(z, -1, keepdim=True)
    e_lse = (sm * (e_z + u * (z - mx).abs())).sum(-1, keepdim=True) + (K + KD_EXP_ULPS) * u + KD_LOG_ULPS * u * (lse - mx).abs() + u * lse.abs()
    lp = z - lse
    e_lp = e_z + e_lse + u * (lp.abs() + z.abs())
    return dict(uu=uu, sd=sd, c=c, e_m=e_m, e_sd=e_sd, e_c=e_c, lp=lp, e_lp=e_lp)


def kd_loss_expect(teacher, student, temperature, loss_scale):
    """x2i_kd_loss_bf16 on teacher / student bf16 [rows, D] (x2i_amd/distill.py: normalize with the unbiased std and 1e-7 +, softmax of
    z / T, KL(teacher || student) per row): ((want, bound, delta) of row_loss [rows], of grad [rows, D] = d(loss_scale row_loss) / d student).
    A row with zero student std: the normalisation's second term is 0 (the kernel's convention)."""
    t, s = teacher.double(), student.double()
    D = t.shape[-1]
    K = 8 * ((D + 511) // 512) + 7
    inv_t = f32(1.0 / f32(temperature))
    ls = f32(loss_scale)
    T_, S_ = _kd_side(t, inv_t, K), _kd_side(s, inv_t, K)
    lp, lq = S_["lp"], T_["lp"]
    p = lp.exp()
    e_p = S_["e_lp"] + KD_EXP_ULPS * u
    d = lp - lq
    e_d = S_["e_lp"] + T_["e_lp"] + u * d.abs()
    rl = (p * d).sum(-1, keepdim=True)
    e_rl = (p * (e_d + d.abs() * e_p)).sum(-1, keepdim=True) + K * u * (p * d.abs()).sum(-1, keepdim=True)
    e_rl = TRAIN_SLACK * e_rl
    loss = (rl.view(-1), (e_rl + u * rl.abs()).view(-1), e_rl.view(-1))
    dsh = p * (d - rl) * inv_t
    e_dsh = p * (e_d + e_rl + u * (d - rl).abs()) * inv_t + dsh.abs() * (e_p + 3 * u)
    md = dsh.sum(-1, keepdim=True) / D
    e_md = (e_dsh.sum(-1, keepdim=True) + K * u * dsh.abs().sum(-1, keepdim=True)) / D
    uu, sd, c, e_m = S_["uu"], S_["sd"], S_["c"], S_["e_m"]
    sdu = (dsh * uu).sum(-1, keepdim=True)
    e_sdu = (e_dsh * uu.abs() + dsh.abs() * (e_m + u * uu.abs())).sum(-1, keepdim=True) + K * u * (dsh * uu).abs().sum(-1, keepdim=True)
    live = sd > 0
    den = ((D - 1) * sd).clamp_min(1e-300)
    kk = torch.where(live, c * c * sdu / den, torch.zeros_like(sd))
    e_kk = torch.where(live, kk.abs() * (2 * S_["e_c"] + S_["e_sd"] + 4 * u) + c * c / den * e_sdu, torch.zeros_like(sd))
    inner = c * (dsh - md) - kk * uu
    want = ls * inner
    delta = TRAIN_SLACK * abs(ls) * (c * (e_dsh + e_md + u * (dsh - md).abs()) + (c * (dsh - md)).abs() * (S_["e_c"] + u) + uu.abs() * e_kk +
                                     kk.abs() * (e_m + 2 * u * uu.abs()) + u * inner.abs()) + u * want.abs()
    return loss, (want, _round_bound(want, delta, False), delta)
