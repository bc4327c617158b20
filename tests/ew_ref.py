"""float64 reference of the row / element kernels of a bf16 denoise step (csrc/elementwise.hip: x2i_ln_modulate_bf16, x2i_skinny_linear,
x2i_gated_residual_bf16, x2i_qkv_split_bf16, x2i_timestep_sinusoid, x2i_euler_step_bf16) and a per-element checker that names the launch,
sample, row and columns of a failure.  No GPU-only code here: the CPU tests of the checker import it too.

Every kernel rounds each output once (include/x2i.h).  `want` is the exact value of the operator on the operands the kernel read (bf16 / f32
-> float64 is exact); the bound of an element is its f32 part `delta` plus the output's own rounding: 1/2 ulp_bf16(|want| + delta) for bf16,
U_F32 |want| for f32 outputs (gemm_ref._round_bound).  u = U_F32 = 2^-24 below.

  Modulated LayerNorm (ln_kernel / ln_rows_kernel, ln_mod1).  y = (x - mu) rstd (1 + sc) + sh, rstd = 1 / sqrt(var + eps), eps the f32 value.
    mean.  Each lane sums its D / 64 elements in a chain (D/64 - 1 roundings), wave_sum adds 6 butterfly levels, / D one more:
           |mu~ - mu| <= E_mu = LN_MEAN_SLACK (D/64 + 6) u sum|x| / D.  Rows whose D values are all equal are exact (k c has at most
           8 + log2 D <= 20 significant bits: every partial sum and D c / D are exact): E_mu = 0 there.
    var.   d = x - mu~ (1 rounding, 2 u on d^2), the fma chain and the tree (D/64 + 6 u), / D (u), + eps (u); sum (x - mu~)^2 =
           sum (x - mu)^2 + D (mu~ - mu)^2:  rstd~ = rstd (1 + e_r), |e_r| <= (D/64 + 10) u / 2 + E_mu^2 / (2 (var + eps)) + LN_RSQRT_ULPS u.
    output. fsub, fmul, fadd(1, sc), fma: 4 roundings, the last relative to |y|:
           delta = rstd |1 + sc| (E_mu + |x - mu| (e_r + 3 u)) + u |y|;  bf16 output.
  Skinny linear.  lin = bias + sum_k w a, a = act_in(x): lanes chain K / 64 fmas, wave_sum 6 levels, + bias: U_ACC (gemm_ref) relative to
    sum |w a| + |bias|, plus U_ACT sum |w a| + ACT_TAIL sum |w x| for act_in's f32 evaluation; act_out as gemm_ref._act_bound; accumulate:
    + u |y_old + v| (one add); f32 output.
  Gated residual.  fmaf(g, t, x): delta = u |x + g t|; bf16 output.   Euler.  fmaf(dt, e, x) or a product and a sum: u (|dt e| + |want|).
  qkv_split.  Q / K: gemm_ref.norm_rope_expect on the bf16 rows read (dx = 0: no bf16(lin) allowance here); V^T: v, exactly.
  Sinusoid.  f = expf(-logf(10000) k / half) (3 roundings of z = -ln(10000) k / half, exp as exp2 of z log2 e: SIN_Z_ULPS u |z| in the
    argument, SIN_EXP_ULPS u relative); a = t f: u.  |a~ - a| <= u |a| (SIN_Z_ULPS |z| + SIN_EXP_ULPS + 1); cosf / sinf add SIN_TRIG.
    delta = |a~ - a| + SIN_TRIG; f32 output, or with round_bf16 one bf16 rounding (either neighbour where want lies within delta of a
    midpoint -- what the bound allows).

Constants (the largest share of the f32 part any launch of tests/test_elementwise_fp64_gpu.py used on MI355X, next to each; the
statistic is max over elements of (|err| - rounding part)+ / delta, as gemm_ref.check_block's)."""
import math

import torch

from tests.gemm_ref import (ACT_NONE, ACT_SILU, ACT_TAIL, U_ACC, U_ACT, U_F32, _act_bound, _round_bound, act_f64, bf16_rne, check_untouched,
                            norm_rope_expect, poison_, sentinel_bits, ulp_bf16, write_mask)

__all__ = ["bf16_rne", "ulp_bf16", "poison_", "write_mask", "check_untouched", "sentinel_bits", "ACT_NONE", "ACT_SILU"]

# slack on the first-order worst case of the f32 mean (second-order terms).  Measured, mean + variance + rsqrtf + the u |y| of the last
# fma together: at most 0.935 of the LN allowance (ln_norm1 of the model; 0.859 in the unit launches) -- the share is set by elements whose
# f32 value lands next to a bf16 midpoint, where the fma's own rounding (u |y|) is most of the allowance
LN_MEAN_SLACK = 1.0 + 2.0 ** -10
# rsqrtf: 1 ulp on gfx950 (v_rsq_f32); 2 allowed
LN_RSQRT_ULPS = 2.0
# skinny: U_ACC (+ U_ACT with act_in) from gemm_ref.  Measured: at most 0.060 of it (K = 256 unit launches; 0.056 guidance embedder,
# 0.011 the full-depth modulation table, 0.007 ragged N at rpw = 16).  Gated residual: the one fmaf rounding, u |want|: 0.988 used.
# Euler: 0.194.  qkv_split (gemm_ref.U_NORM): 0.202.
# sinusoid: roundings of z = -logf(10000) * k / half (3) + the product of z with log2(e) inside expf (1) + 1 spare; expf 2 ulps; cosf / sinf
# 4 ulps of a value below 1 (absolute).  Measured: 0.222 of the allowance at the model's launches, 0.403 over t up to 10^4
SIN_Z_ULPS = 5.0
SIN_EXP_ULPS = 2.0
SIN_TRIG = 4.0 * U_F32
MAX_PERIOD = 10000.0

# the old whole-tensor checks, kept here only to show what they miss (tests/test_ew_ref_cpu.py)
OLD_LN_REL_L2 = 5e-3
OLD_SKINNY_REL_L2 = 1e-4
OLD_SIN_ABS = 2e-3


def f32(x):
    """the f32 value of a Python float, as a float"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- references
def const_rows(x):
    """[rows, 1] True where every value of the row x float64 [rows, D] is the same"""
    return x.amax(-1, keepdim=True) == x.amin(-1, keepdim=True)


def ln_mean_err(x):
    """E_mu [rows, 1] of x float64 [rows, D] (0 on constant rows)"""
    D = x.shape[-1]
    e = LN_MEAN_SLACK * (D / 64 + 6) * U_F32 * x.abs().sum(-1, keepdim=True) / D
    return torch.where(const_rows(x), torch.zeros_like(e), e)


def ln_expect(x, sh, sc, eps):
    """Modulated LayerNorm of the rows x [rows, D] (bf16 or float64 of bf16 values) with shift / scale [rows, D] or [D] (f32 values):
    (want, bound, delta) float64 [rows, D]."""
    x = x.double()
    sh, sc = sh.double(), sc.double()
    D = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / D         # (not mean(): on the GPU it multiplies by a rounded 1 / D, and a constant row must give mu = x)
    xc = x - mu
    var = (xc * xc).sum(-1, keepdim=True) / D
    epsf = f32(eps)
    rstd = torch.rsqrt(var + epsf)
    m = 1.0 + sc
    want = xc * rstd * m + sh
    e_mu = ln_mean_err(x)
    e_r = 0.5 * (D / 64 + 10) * U_F32 + 0.5 * e_mu ** 2 / (var + epsf) + LN_RSQRT_ULPS * U_F32
    delta = rstd * m.abs() * (e_mu + xc.abs() * (e_r + 3 * U_F32)) + U_F32 * want.abs()
    const = const_rows(x)                     # every operation exact: y = fma(0, 1 + sc, sh) = sh
    delta = torch.where(const, torch.zeros_like(delta), delta)
    want = torch.where(const, sh.expand_as(want), want)
    return want, _round_bound(want, delta, False), delta


def skinny_expect(X, W, bias=None, *, act_in=ACT_NONE, act_out=ACT_NONE, y_old=None):
    """x2i_skinny_linear for X [B, K] (f32 or bf16), W [N, K] bf16, bias [N] bf16 or None, y_old [B, N] f32 (accumulate) or None:
    (want, bound, delta) float64 [B, N]."""
    x = X.double()
    a = act_f64(x, act_in)
    Wd = W.double()
    lin = a @ Wd.T
    mag = a.abs() @ Wd.abs().T
    if bias is not None:
        lin += bias.double()
        mag += bias.double().abs()
    d = U_ACC * mag
    if act_in != ACT_NONE:
        d += U_ACT * mag + ACT_TAIL * (x.abs() @ Wd.abs().T)
    del mag, Wd
    v = act_f64(lin, act_out)
    d = _act_bound(lin, v, d, act_out)
    if y_old is not None:
        v = y_old.double() + v
        d = d + U_F32 * v.abs()
    return v, _round_bound(v, d, True), d


def gated_expect(x, t, g):
    """x2i_gated_residual_bf16: x [rows, D] bf16, t [rows, D] bf16, g [rows, D] or [D] f32"""
    want = x.double() + g.double() * t.double()
    d = U_F32 * want.abs()
    return want, _round_bound(want, d, False), d


def euler_expect(x, e, dt):
    """x2i_euler_step_bf16: x, e bf16 [n], dt the f32 value"""
    de = dt * e.double()
    want = x.double() + de
    d = U_F32 * (de.abs() + want.abs())
    return want, _round_bound(want, d, False), d


def sinusoid_expect(t, dim, round_bf16):
    """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) of t [B] f32: (want, bound, delta) float64 [B, dim]"""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64, device=t.device)
    z = -math.log(MAX_PERIOD) * k / half
    a = t.double()[:, None] * torch.exp(z)[None, :]
    want = torch.cat((torch.cos(a), torch.sin(a)), 1)
    da = U_F32 * a.abs() * (SIN_Z_ULPS * z.abs() + SIN_EXP_ULPS + 1.0)[None, :]
    d = torch.cat((da, da), 1) + SIN_TRIG
    return want, _round_bound(want, d, not round_bf16), d


def qkv_split_rows(rows, nw, c, s, *, H, eps=1e-6):
    """q or k of x2i_qkv_split_bf16 for bf16 rows [m, H 128] of one section, weights nw [128], c / s float64 [m, 128]: (want, bound, delta)
    float64 [m, H 128]"""
    m = rows.shape[0]
    x = rows.double().view(m, H, 128)
    o, b = norm_rope_expect(x, torch.zeros_like(x), nw, 1.0, f32(eps), c, s)
    return o.view(m, H * 128), _round_bound(o, b, False).view(m, H * 128), b.view(m, H * 128)


# ---------------------------------------------------------------------------------------------------------------- checker
def check_rows(name, got, want, bound, delta=None, *, sample, token, col0=0, unit=8):
    """Compare got [R, N] (any dtype) with want / bound float64 [R, N]; row i is token `token[i]` of sample `sample[i]` (int tensors [R]).
    Returns (None or a message naming the launch, the sample, the token and the `unit`-wide column range of the worst element and how many
    rows fail, worst share).  The share is |err| / bound, or with `delta` (|err| - rounding part)+ / delta: how much of the f32 allowance
    was used (entries with delta == 0 count as 0 when they are exact, as infinity when not)."""
    g = got.to(device=want.device, dtype=torch.float64)
    err = (g - want).abs()
    bad = ~(err <= bound)                     # (NaN fails)
    if delta is not None:
        over = (err - (bound - delta)).clamp_min(0)
        share = torch.where(over > 0, over / delta, torch.zeros_like(over))
    else:
        share = err / bound
    share = torch.where(torch.isfinite(share), share, torch.full_like(share, math.inf))
    worst = float(share.max()) if share.numel() else 0.0
    if not bool(bad.any()):
        return None, worst
    ratio = torch.where(bad, torch.where(torch.isfinite(err / bound), err / bound, torch.full_like(err, math.inf)), torch.zeros_like(err))
    i, n = (int(v) for v in torch.nonzero(ratio == ratio.max())[0])
    rows_bad = bad.any(1)
    nrows = int(rows_bad.sum())
    samples = sorted({int(v) for v in sample.to(rows_bad.device)[rows_bad].unique()})
    c0 = col0 + n - n % unit
    msg = (f"{name}: {nrows} rows over the bound (samples {samples[:8]}{'...' if len(samples) > 8 else ''}), {int(bad.sum())} elements; worst at "
           f"sample {int(sample[i])}, row (token) {int(token[i])}, cols {c0}..{c0 + unit - 1} (col {col0 + n}): got {float(g[i, n]):.9g} "
           f"want {float(want[i, n]):.9g} bound {float(bound[i, n]):.3e} (|err| / bound {float(ratio[i, n]):.3g})")
    return msg, worst


class Report:
    """Collects the checks of one launch; done() raises with the first failure and the number of failing rows of the whole launch, or
    returns the worst share."""

    def __init__(self, name):
        self.name, self.msgs, self.rows, self.worst = name, [], 0, 0.0

    def check(self, got, want, bound, delta=None, *, sample, token, col0=0, unit=8, what=""):
        msg, worst = check_rows(f"{self.name}{what}", got, want, bound, delta, sample=sample, token=token, col0=col0, unit=unit)
        self.worst = max(self.worst, worst)
        if msg:
            self.msgs.append(msg)
            self.rows += int(msg.split(": ", 1)[1].split(" rows", 1)[0])
        return msg

    def done(self):
        if self.msgs:
            raise AssertionError(f"{self.msgs[0]}  [{self.rows} failing rows in the launch]")
        return self.worst


def _idx(n, device):
    return torch.arange(n, device=device)


# ---------------------------------------------------------------------------------------------------------------- whole launches
def check_ln(rep, X3, Y3, S0, sh0, sc0, sh1, sc1, eps):
    """Every element of one x2i_ln_modulate_bf16 launch: X3 / Y3 [B, S, D] views (Y3 after the launch), shift / scale [B, >= D] views (the
    kernel reads their first D columns)."""
    B, S, D = X3.shape
    dev = X3.device
    for b in range(B):
        for lo, hi, sh, sc in ((0, S0, sh0, sc0), (S0, S, sh1, sc1)):
            if hi <= lo:
                continue
            want, bound, delta = ln_expect(X3[b, lo:hi], sh[b, :D], sc[b, :D], eps)
            tok = _idx(hi - lo, dev) + lo
            rep.check(Y3[b, lo:hi], want, bound, delta, sample=torch.full_like(tok, b), token=tok)
    return rep


def check_skinny(rep, X, W, bias, Y, *, act_in=ACT_NONE, act_out=ACT_NONE, y_old=None, rows=65536):
    """Every element of one x2i_skinny_linear launch: X [B, K], W [N, K], Y [B, N] (a view, after the launch), y_old [B, N] or None; the
    float64 reference in chunks of `rows` outputs."""
    B, N = Y.shape
    tok = torch.zeros(B, dtype=torch.long, device=X.device)
    smp = _idx(B, X.device)
    for n0 in range(0, N, rows):
        n1 = min(N, n0 + rows)
        want, bound, delta = skinny_expect(X, W[n0:n1], bias[n0:n1] if bias is not None else None, act_in=act_in, act_out=act_out,
                                           y_old=y_old[:, n0:n1] if y_old is not None else None)
        rep.check(Y[:, n0:n1], want, bound, delta, sample=smp, token=tok, col0=n0, unit=1)
    return rep


def check_gated(rep, X3_old, T3, G, X3):
    """x2i_gated_residual_bf16: X3_old (a copy from before the launch) / T3 / X3 [B, S, D], G [B, D]"""
    B, S, D = X3.shape
    for b in range(B):
        want, bound, delta = gated_expect(X3_old[b], T3[b], G[b])
        tok = _idx(S, X3.device)
        rep.check(X3[b], want, bound, delta, sample=torch.full_like(tok, b), token=tok)
    return rep


def qkv_split_rows_of(qkv0, qkv1, ld0, ld1, B, S, S0, H):
    """the bf16 [B, S, 3 H 128] rows x2i_qkv_split_bf16 reads: token s < S0 of sample b from qkv0 row b S0 + s, else qkv1 row b (S - S0) + s - S0"""
    C = 3 * H * 128
    parts = []
    if S0 > 0:
        parts.append(qkv0.as_strided((B, S0, C), (S0 * ld0, ld0, 1), qkv0.storage_offset()))
    if S0 < S:
        parts.append(qkv1.as_strided((B, S - S0, C), ((S - S0) * ld1, ld1, 1), qkv1.storage_offset()))
    return torch.cat(parts, 1)


def check_qkv_split(rep, rows, nq0, nk0, nq1, nk1, cos, sin, Q, K, VT, *, S, S0, H, eps=1e-6):
    """Every Q / K / V^T element of one x2i_qkv_split_bf16 launch: rows bf16 [B, S, 3 H 128] (qkv_split_rows_of), cos / sin f32 [S, 128]"""
    B = rows.shape[0]
    HD = H * 128
    dev = rows.device
    for b in range(B):
        for lo, hi, nq, nk in ((0, S0, nq0, nk0), (S0, S, nq1, nk1)):
            if hi <= lo:
                continue
            tok = _idx(hi - lo, dev) + lo
            smp = torch.full_like(tok, b)
            c, s = cos[lo:hi].double(), sin[lo:hi].double()
            for sec, nw, out in ((0, nq, Q), (1, nk, K)):
                want, bound, delta = qkv_split_rows(rows[b, lo:hi, sec * HD:(sec + 1) * HD], nw, c, s, H=H, eps=eps)
                got = out[b, :, lo:hi, :].permute(1, 0, 2).reshape(hi - lo, HD)
                rep.check(got, want, bound, delta, sample=smp, token=tok, unit=128, what=f" {'QK'[sec]}")
        v = rows[b, :, 2 * HD:].double()
        got = VT[b, :, :, :S].permute(2, 0, 1).reshape(S, HD)
        tok = _idx(S, dev)
        zero = torch.zeros_like(v)
        rep.check(got, v, zero, zero, sample=torch.full_like(tok, b), token=tok, unit=128, what=" V^T")
    return rep


def vt_zero_end(S):
    """x2i_qkv_split_bf16 writes zeros into V^T positions [S, vt_zero_end(S)) (its 64-token transpose tiles) and nothing beyond"""
    return 64 * ((S + 63) // 64)


def check_qkv_split_padding(name, Q, K, VT, S):
    """Q / K rows >= S keep the sentinel; V^T positions [S, vt_zero_end(S)) hold +0, the ones beyond keep the sentinel (include/x2i.h)"""
    for n, t in (("Q", Q), ("K", K)):
        ok = sentinel_bits(t[:, :, S:])
        if not bool(ok.all()):
            b, h, r, _ = (int(v) for v in torch.nonzero(~ok)[0])
            raise AssertionError(f"{name}: {n} padding row written: sample {b}, head {h}, row {S + r} (S = {S})")
    e = vt_zero_end(S)
    z = VT[..., S:e].view(torch.int16)
    if not bool((z == 0).all()):
        b, h, d, j = (int(v) for v in torch.nonzero(z != 0)[0])
        raise AssertionError(f"{name}: V^T position {S + j} (in [S, {e}) = zeros) holds bits {int(z[b, h, d, j]) & 0xFFFF:#06x}: sample {b}, "
                             f"head {h}, dim {d} (S = {S})")
    ok = sentinel_bits(VT[..., e:])
    if not bool(ok.all()):
        b, h, d, j = (int(v) for v in torch.nonzero(~ok)[0])
        raise AssertionError(f"{name}: V^T padding position {e + j} written (beyond the zeroed [S, {e})): sample {b}, head {h}, dim {d} (S = {S})")


# ---------------------------------------------------------------------------------------------------------------- operands
LN_KINDS = ("random", "large_mean", "outlier", "const", "mod_edge")
SK_KINDS = ("random", "cancel")


def ln_rows(R, D, kind, gen, device):
    """bf16 [R, D] LayerNorm inputs of one kind, generated on `device`:
    random      N(0.5, 2^2)
    large_mean  256 + 2 {-1, 0, 1}: a spread of one bf16 ulp around a large mean (the f32 mean's error and a one-pass variance matter)
    outlier     N(0, 1) with 4 channels per row at +-2^11 .. 2^13 (FLUX's large residual-stream values)
    const       rows r % 3 == 0 constant, r % 3 == 1 constant but for two elements one bf16 ulp off (eps dominates the variance), else random
    mod_edge    as random (the modulation vectors carry this kind's edge: mod_vectors)"""
    if kind in ("random", "mod_edge"):
        return (0.5 + 2.0 * torch.randn((R, D), device=device, generator=gen)).to(torch.bfloat16)
    if kind == "large_mean":
        return (256.0 + 2.0 * torch.randint(-1, 2, (R, D), device=device, generator=gen)).to(torch.bfloat16)
    if kind == "outlier":
        x = torch.randn((R, D), device=device, generator=gen)
        ch = torch.randint(0, D, (R, 4), device=device, generator=gen)
        mag = torch.exp2(11.0 + 2.0 * torch.rand((R, 4), device=device, generator=gen))
        sign = torch.where(torch.rand((R, 4), device=device, generator=gen) < 0.5, -1.0, 1.0)
        x.scatter_(1, ch, mag * sign)
        return x.to(torch.bfloat16)
    assert kind == "const", kind
    x = (0.5 + 2.0 * torch.randn((R, D), device=device, generator=gen)).to(torch.bfloat16).double()
    c = (torch.randn((R, 1), device=device, generator=gen) * 3).to(torch.bfloat16).double()
    r = torch.arange(R, device=device)[:, None]
    near = c.expand(R, D).clone()
    near[:, :2] += ulp_bf16(c) * torch.tensor([1.0, -1.0], device=device)
    x = torch.where(r % 3 == 0, c.expand(R, D), torch.where(r % 3 == 1, near, x))
    return x.to(torch.bfloat16)


def mod_vectors(n, kind, gen, device):
    """f32 [n] modulation storage (shift and scale vectors are views into it): 0.5 N(0, 1); `mod_edge`: one third scale-like values near -1
    (1 + sc cancels to 2^-12 .. 2^-6), one third large shifts (+-64 .. 512), the rest 0.5 N(0, 1), interleaved in blocks of 8"""
    v = 0.5 * torch.randn(n, device=device, generator=gen)
    if kind != "mod_edge":
        return v
    blk = (torch.arange(n, device=device) // 8) % 3
    near = -1.0 + torch.exp2(-12.0 + 6.0 * torch.rand(n, device=device, generator=gen)) * torch.sign(torch.randn(n, device=device, generator=gen))
    big = torch.exp2(6.0 + 3.0 * torch.rand(n, device=device, generator=gen)) * torch.sign(torch.randn(n, device=device, generator=gen))
    return torch.where(blk == 0, near, torch.where(blk == 1, big, v))
