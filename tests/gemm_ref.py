"""float64 reference of the bf16 GEMM epilogues (include/x2i.h: x2i_gemm_bf16, x2i_gemm_qkv_bf16) and a per-element checker, for the GEMM
kernels' tests.  No GPU-only code here: the CPU tests of the checker import it too.

The kernels accumulate A W^T in f32 and round every output ONCE, after the whole epilogue (include/x2i.h; csrc/gemm_device.h):
    v = act(acc + bias);  v = fmaf(gate, v, res) (one rounding);  C = bf16(v) or f32 v;  C2 = bf16(act2(v))
    fused QKV: x = bf16(acc + bias); q / k: y = x * rsqrt(mean(x^2) + eps) * w * q_scale, interleaved-pair RoPE, one bf16 rounding; v: x.
So every output element has its own bound, far sharper than any rel-L2 over a tile:

  f32 part.  |v - want| <= delta, with  delta = U_ACC * |gate| * (sum_k |a_mk w_nk| + |b_n|)  [+ the epilogue terms below].  bf16 -> f64 is
             exact and so are the products: `want` is the exact value of the epilogue on the operands the kernel read.  sum |a w| goes
             through an f32 GEMM: only the bound needs it.
  epilogue.  act:      |act'(lin)| delta (+ delta^2: |act''| < 1 for GELU / SiLU) + U_ACT |act(lin)| + ACT_TAIL |lin|  (+ U_ERF |lin| / 2, GELU-erf)
             residual: |gate| delta + U_F32 (|res| + |gate act(lin)|)     (the one rounding of fmaf)
  output.    bf16:     |out - want| <= delta + 1/2 ulp_bf16(|want| + delta)   (the one round-to-nearest; a second rounding, or truncation, costs
                       up to another half ulp and fails wherever it lands away from the first)
             f32:      |out - want| <= delta + U_F32 |want|
  QKV.       x = bf16(lin) is exact in the kernel unless lin lies within delta of a bf16 rounding midpoint: there x may be either neighbour.
             Exactly that one-ulp change of x (dx) is allowed, propagated through the norm (sum x^2 -> rsqrt, mean-value bound) and the
             rotation, plus U_NORM relative to the rotation's terms for the f32 arithmetic of norm_rope8; then half a bf16 ulp.

Constants (worst measured error / bound over the GPU tests, tests/test_gemm_fp64_gpu.py and tests/test_encoder_gemm_fp64_gpu.py, next to each)."""
import math

import torch

U_F32 = 2.0 ** -24
# f32 accumulation of the K sum, relative to sum |a w|.  An f32 fmaf chain on CDNA measures ~1.5e-7 at K <= 1024 and 3.5e-7 at K = 4096
# (2^-22.5 .. 2^-21.4); these bf16 MFMA kernels at K up to 15360 start from 2^-20 (9.5e-7).  Measured: at most 0.323 of the whole f32
# allowance used (to_out pair, gated residual, K = 3072: 3.1e-7 sum |a w|); the other plain launches 0.062 (x_embedder) .. 0.185
# (single-block proj_out, K = 15360), over every kernel form.
# The encoder and decoder modules' launches (tests/test_encoder_gemm_fp64_gpu.py; profiles/encoder_gemm_fp64_gputest.log), worst share of
# the whole f32 allowance per launch family, forms 128 and 256: plain and biased projections (qkv, gu / wi / fc1 without activation, pe,
# kv_proj, K | V slabs by ldc / c_offset, a_offset) 0.118 (SigLIP pe, K = 640); residual in place (out=X, res=X) 0.117 (SigLIP fc2,
# K = 4352; T5 wo at K = 10240: 0.087); residual with its own ldr 0.100 (Qwen2 7B o_proj); f32 gate with the residual in place
# (InternViT layer scale) 0.218; batched with c_offset (Whisper conv1, InternViT pe, the Qwen2 slab) 0.088; overlapping A rows (Whisper
# conv2, lda = 2 D, K = 3 D) 0.065; a weight per item (VAE attention: h, k, V^T as W) 0.038; out_f32 (projector head) 0.203; out2 / act2
# 0.061.  K = 18944 (Qwen2 7B down_proj), beyond the 15360 above: 0.088 into the slab, 0.095 plain: no larger a share than at
# K = 3584 (0.100), so 2^-20 holds there with the same margin.
U_ACC = 2.0 ** -20
# v_exp_f32 / v_rcp_f32 / erff in gelu_tanh_f, gelu_erf_f, silu_f: a few f32 ulps of the result; 32 ulps allowed.  Measured together with
# U_ACC: the GELU-tanh launches use at most 0.157 of the allowance (proj_mlp); not measured apart.  GELU-erf, SiLU and ReLU, measured with
# U_ACC as well, per activation over the toy grid of tests/test_encoder_gemm_fp64_gpu.py (every epilogue form on the 128, 256 and generic
# kernels; the f32 output shows most, a bf16 output's rounding hides the rest): GELU-erf 0.077, SiLU 0.086, ReLU 0.084 (no activation:
# 0.059, GELU-tanh 0.070); and in the modules' launches: GELU-erf 0.098 (InternViT fc1; Whisper fc1 0.073, its convs 0.065, the Qwen2.5-VL
# merger at M = 25 0.059, mlp1 at K = 4096 0.081, the projector 0.060), ReLU 0.045 (Whisper projection), GELU-tanh 0.069 (SigLIP fc1).
U_ACT = 2.0 ** -19
# gelu_erf_f is 0.5 x (1 + erff(x / sqrt 2)) as written (csrc/x2i_common.h), and for x < 0 the sum 1 + erf cancels: what is a few ulps of erf
# (|erf| < 1: ulps of 2^-24) is an ABSOLUTE error of the sum, however small the sum is, so the result carries 0.5 |x| times it -- relative to
# GELU(x) that grows without limit as x falls (at x = -4 the result is 1.3e-4 and an erf error of 2^-24 moves it by 1.2e-7, 1e-3 of it; torch's
# own f32 GELU has the same form and the same error).  U_ACT |act(x)| cannot hold there, so GELU-erf alone gets the term U_ERF 0.5 |x|, from
# the arithmetic and not from a run: erff within 4 ulps of its result (4 * 2^-24 = 2^-22), the rounding of x / sqrt 2 (erf' z <= 0.43: under
# 2^-25) and of the sum (half an ulp of a value in [1, 2): 2^-24; exact by Sterbenz where erf <= -1/2) -- under 2^-21 together.  The tanh
# GELU and SiLU are x / (1 + exp2(..)): no cancellation, their error stays relative.  Without this term the f32 stand-in of
# tests/test_gemm_ref_cpu.py itself fails (70 x its bound where 1 + erf is 0 in f32 and GELU is -1.2e-7); with it the stand-in uses 0.114
# of the allowance and the kernels the shares above.
U_ERF = 2.0 ** -21
# where exp2 over- / underflows (GELU far below 0) the kernel returns +-0 for a result below 2^-100 |x|
ACT_TAIL = 2.0 ** -100
# f32 arithmetic of the QKV norm / rotation, relative to |y_e c| + |y_o s|: sum of 128 squares (fma chain + shuffle tree, <= 12 u), the
# fma with 1/128 and eps (1 u), rsqrtf (1 ulp + half the argument's error), w * q_scale, x * r, * w, the products and the fma (4 u):
# under 16 u = 2^-20.  Measured together with U_ACC: the fused QKV launches use at most 0.157 of the allowance (double-block pair; heads
# with an x at a rounding midpoint, which may use their whole one-ulp allowance, left out of the statistic).
U_NORM = 2.0 ** -20

TILE = 256
SENTINEL16 = 0x7F7F             # bf16 bits of 3.39e38
SENTINEL32 = 0x7F7F7F7F         # f32 bits of 3.39e38

# the old style of check, kept here only to show what it misses (tests/test_gemm_ref_cpu.py): rel-L2 on a few sampled rows
OLD_SAMPLED_BOUND = 1e-2

ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU, ACT_RELU = 0, 1, 2, 3, 4


# ---------------------------------------------------------------------------------------------------------------- float64 helpers
def ulp_bf16(x):
    """ulp of bf16 at |x| (float64; 2^-133 below the smallest normal).  Built from the exponent bits: exact on every device (torch.ldexp
    goes through pow(2, e), which on the GPU need not be exact -- and a bound half an f64 ulp short rejects a correct tie)."""
    e = (x.double().abs().clamp_min(2.0 ** -126).view(torch.int64) >> 52) & 0x7FF
    return ((e - 7) << 52).view(torch.float64)


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), exactly in float64 (torch's double -> bf16 goes through f32: two roundings)."""
    u = ulp_bf16(x)
    return torch.round(x / u) * u


def act_f64(x, act):
    if act == ACT_GELU_TANH:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if act == ACT_GELU_ERF:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    if act == ACT_RELU:
        return x.clamp_min(0.0)
    assert act == ACT_NONE, act
    return x


def dact_f64(x, act):
    if act == ACT_GELU_TANH:
        c = math.sqrt(2.0 / math.pi)
        t = torch.tanh(c * (x + 0.044715 * x ** 3))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * x * x)
    if act == ACT_GELU_ERF:
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == ACT_SILU:
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    return torch.ones_like(x)


def _act_bound(x, y, d, act):
    """bound on |act_f32(x~) - act(x)| for |x~ - x| <= d, y = act(x)"""
    if act in (ACT_NONE, ACT_RELU):           # (ReLU is fmaxf(v, 0): exact, |max(a, 0) - max(b, 0)| <= |a - b|, no U_ACT term)
        return d
    b = (dact_f64(x, act).abs() + d) * d + U_ACT * y.abs() + ACT_TAIL * x.abs()
    if act == ACT_GELU_ERF:                   # (the one activation whose f32 form cancels: see U_ERF)
        b = b + U_ERF * 0.5 * x.abs()
    return b


def _round_bound(want, d, f32):
    return d + (U_F32 * want.abs() if f32 else 0.5 * ulp_bf16(want.abs() + d))


# ---------------------------------------------------------------------------------------------------------------- references
def linear_f64(A, W, bias):
    """lin = A W^T + b in float64 and mag = |A| |W|^T + |b| (f32 GEMM) for A [m, K], W [N, K] bf16 on one device."""
    lin = A.double() @ W.double().T
    mag = (A.float().abs() @ W.float().abs().T).double()
    if bias is not None:
        lin += bias.double()
        mag += bias.double().abs()
    return lin, mag


def epilogue_expect(lin, d, *, act=ACT_NONE, gate=None, res=None, act2=None, out_f32=False):
    """The epilogue of x2i_gemm_bf16 from the linear part on: lin float64 [m, N] (biases included) and d, the bound on the kernel's f32 value
    of it.  Returns what gemm_expect returns.  (The e4m3 GEMM's expectation, tests/fp8_ref.py, starts here with its own lin and d.)"""
    v = act_f64(lin, act)
    d = _act_bound(lin, v, d, act)
    if res is not None:                       # (the gate applies with a residual only)
        g = gate.double() if gate is not None else torch.ones_like(v[0])
        gv = v * g
        r = res.double()
        d = d * g.abs() + U_F32 * (r.abs() + gv.abs())
        v = r + gv
    out = (v, _round_bound(v, d, out_f32), d)
    if act2 is None:
        return out
    v2 = act_f64(v, act2)
    d2 = _act_bound(v, v2, d, act2)
    return out, (v2, _round_bound(v2, d2, False), d2)


def gemm_expect(A, W, bias=None, *, act=ACT_NONE, gate=None, res=None, act2=None, out_f32=False, bias2=None):
    """Expected outputs of x2i_gemm_bf16 for the rows A [m, K] of one batch item: W [N, K], bias [N] (bf16 or None), gate [N] f32 or None,
    res [m, N] bf16 or None, bias2 [N] f32 or None (x2i_gemm_args.bias2 of this item: added in front of the activation; its magnitude joins
    the U_ACC term like the bias's).  Returns (want, bound, delta) float64 [m, N] for C (delta: the f32 part of the bound), and (want2, bound2, delta2) for
    C2 = act2(v) when act2 is not None."""
    lin, mag = linear_f64(A, W, bias)
    if bias2 is not None:
        lin += bias2.double()
        mag += bias2.double().abs()
    d = U_ACC * mag
    del mag
    return epilogue_expect(lin, d, act=act, gate=gate, res=res, act2=act2, out_f32=out_f32)


def rope_rows(cos, sin, tok):
    """(c, s) float64 [m, 128] at joint tokens `tok` [m] from the interleaved tables cos / sin f32 [S, 128], or, sin None, from the pair-form
    table cos f32 [S, 64, 2] (ops.rope_pairs)."""
    if sin is None:
        p = cos.view(cos.shape[0], 64, 2)[tok].double()
        return p[..., 0].repeat_interleave(2, -1), p[..., 1].repeat_interleave(2, -1)
    return cos[tok].double(), sin[tok].double()


def norm_rope_expect(x, dx, nw, scale, epsf, c, s):
    """RMSNorm * w * scale, then interleaved-pair RoPE, of bf16 values x float64 [m, H, 128] (dx [m, H, 128]: the allowance on x, 0 where x
    is exact), c / s float64 [m, 128]: (want, f32 part of the bound) float64 [m, H, 128] -- norm_rope8 / rms_rsqrt128 (csrc/x2i_common.h),
    shared by the fused QKV epilogues and x2i_qkv_split_bf16."""
    w = nw.double() * scale
    ss = (x * x).sum(-1, keepdim=True)
    r = torch.rsqrt(ss / 128.0 + epsf)
    dss = (dx * (2 * x.abs() + dx)).sum(-1, keepdim=True)
    rmax = torch.rsqrt((ss - dss).clamp_min(0.0) / 128.0 + epsf)
    dr = 0.5 * rmax ** 3 * dss / 128.0
    y = x * r * w
    dy = w.abs() * (r * dx + (x.abs() + dx) * dr)
    cc, ss_ = c[:, None, :], s[:, None, :]
    ye, yo, dye, dyo = y[..., 0::2], y[..., 1::2], dy[..., 0::2], dy[..., 1::2]
    ce, co, se, so = cc[..., 0::2], cc[..., 1::2], ss_[..., 0::2], ss_[..., 1::2]
    o = torch.empty_like(y)
    b = torch.empty_like(y)
    o[..., 0::2] = ye * ce - yo * se
    o[..., 1::2] = yo * co + ye * so
    b[..., 0::2] = dye * ce.abs() + dyo * se.abs() + U_NORM * ((ye * ce).abs() + (yo * se).abs())
    b[..., 1::2] = dyo * co.abs() + dye * so.abs() + U_NORM * ((yo * co).abs() + (ye * so).abs())
    return o, b


def qkv_expect(A, W, bias, norm_q, norm_k, c, s, *, H, q_scale=1.0, eps=1e-6):
    """Expected Q / K / V rows of x2i_gemm_qkv_bf16 for A [m, K]: (want, bound) float64 [m, 3 H 128] in GEMM-column order (q | k | v sections,
    head-major, 128 dims each) and delta, the part of the bound that is not the output's own rounding.  c, s: float64 [m, 128] RoPE rows of the
    rows' tokens (rope_rows)."""
    lin, mag = linear_f64(A, W, bias)
    d = U_ACC * mag
    del mag
    return qkv_epilogue_expect(lin, d, norm_q, norm_k, c, s, H=H, q_scale=q_scale, eps=eps)


def qkv_epilogue_expect(lin, d, norm_q, norm_k, c, s, *, H, q_scale=1.0, eps=1e-6):
    """The fused QKV epilogue from the linear part on (lin, d as for epilogue_expect): what qkv_expect returns."""
    m, HD = lin.shape[0], H * 128
    want = torch.empty_like(lin)
    bound = torch.empty_like(lin)
    # v: x = bf16(lin), moved
    want[:, 2 * HD:] = lin[:, 2 * HD:]
    bound[:, 2 * HD:] = _round_bound(lin[:, 2 * HD:], d[:, 2 * HD:], False)
    delta = d.clone()
    qs = float(torch.tensor(q_scale if q_scale not in (0.0, 1.0) else 1.0, dtype=torch.float32))
    epsf = float(torch.tensor(eps, dtype=torch.float32))
    for sec, nw, scale in ((0, norm_q, qs), (1, norm_k, 1.0)):
        sl = slice(sec * HD, (sec + 1) * HD)
        lo, hi = bf16_rne(lin[:, sl] - d[:, sl]), bf16_rne(lin[:, sl] + d[:, sl])
        x = bf16_rne(lin[:, sl]).view(m, H, 128)
        dx = (hi - lo).view(m, H, 128)
        o, b = norm_rope_expect(x, dx, nw, scale, epsf, c, s)
        want[:, sl] = o.view(m, HD)
        bound[:, sl] = _round_bound(o, b, False).view(m, HD)
        # (for the statistic of check_block only: heads with an x at a rounding midpoint may use their whole dx allowance -- left out of it)
        delta[:, sl] = torch.where((dx > 0).any(-1, keepdim=True), torch.full_like(b, math.nan), b).view(m, HD)
    return want, bound, delta


# ---------------------------------------------------------------------------------------------------------------- checker
def check_block(name, got, want, bound, *, row0=0, where=None, delta=None):
    """Compare got [m, N] (any dtype) with want / bound float64 [m, N] element by element; rows are rows row0.. of one batch item (row0 %
    256 == 0).  Returns (None or failure message, worst |err| / bound, per-tile rel-L2 [tile rows, tile cols], failing tiles [(tr, tc, count)]).
    `where(m, n)` names an element (default: its (m, n)).  With `delta` (the f32 part of the bound) the second value is instead the worst
    (|err| - rounding part)+ / delta: how much of the f32 allowance (U_ACC, U_ACT, U_NORM) the kernel used -- the number the constants carry
    (NaN entries of delta are left out)."""
    assert row0 % TILE == 0
    m, N = want.shape
    g = got.to(device=want.device, dtype=torch.float64)
    err = (g - want).abs()
    ratio = err / bound
    bad = ~(err <= bound)                     # (NaN fails)
    tr, tc = (m + TILE - 1) // TILE, (N + TILE - 1) // TILE
    pad = lambda t: torch.nn.functional.pad(t, (0, tc * TILE - N, 0, tr * TILE - m)).view(tr, TILE, tc, TILE)
    num = pad(torch.where(torch.isfinite(err), err, torch.full_like(err, 1e300)) ** 2).sum((1, 3))
    den = pad(want * want).sum((1, 3))
    tile_rel = (num / den.clamp_min(1e-300)).sqrt()
    finite_ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    worst = float(finite_ratio.max()) if ratio.numel() else 0.0
    if delta is not None and ratio.numel():
        worst = float(((err - (bound - delta)).clamp_min(0) / delta).nan_to_num(nan=0.0, posinf=math.inf).max())
    if not bool(bad.any()):
        return None, worst, tile_rel, []
    counts = pad(bad.double()).sum((1, 3))
    tiles = [(int(a) + row0 // TILE, int(b_), int(counts[a, b_])) for a, b_ in torch.nonzero(counts)]
    fm, fn = (int(v) for v in torch.nonzero(finite_ratio == finite_ratio.max())[0])
    t_r, t_c = (row0 + fm) // TILE, fn // TILE
    n_in = int(counts[fm // TILE, fn // TILE])
    w = where(row0 + fm, fn) if where else f"(m={row0 + fm}, n={fn})"
    msg = (f"{name}: tile ({t_r}, {t_c}) [rows {t_r * TILE}..{t_r * TILE + TILE - 1}, cols {t_c * TILE}..{t_c * TILE + TILE - 1}]: "
           f"{n_in} elements over the bound; worst {w}: got {float(g[fm, fn]):.9g} want {float(want[fm, fn]):.9g} "
           f"bound {float(bound[fm, fn]):.3e} (|err| / bound {float(ratio[fm, fn]):.3g}); {len(tiles)} failing tiles in these rows")
    return msg, worst, tile_rel, tiles


class Report:
    """Collects the blocks of one launch: check(...) per block, then done() asserts with the first failing block's message and the total
    number of failing tiles, or returns the worst share of the f32 allowance used (check_block)."""

    def __init__(self, name):
        self.name, self.msgs, self.tiles, self.worst, self.worst_tile = name, [], 0, 0.0, 0.0

    def check(self, got, want, bound, delta=None, *, item=0, row0=0, where=None):
        msg, worst, tile_rel, tiles = check_block(f"{self.name}, item {item}", got, want, bound, row0=row0, where=where, delta=delta)
        self.worst = max(self.worst, worst)
        self.worst_tile = max(self.worst_tile, float(tile_rel.max()) if tile_rel.numel() else 0.0)
        if msg:
            self.msgs.append(msg)
            self.tiles += len(tiles)
        return msg

    def done(self):
        if self.msgs:
            raise AssertionError(f"{self.msgs[0]}  [{self.tiles} failing tiles in the launch]")
        return self.worst


# ---------------------------------------------------------------------------------------------------------------- token map, sentinel
def tokens_of(rows, z, tok_off, rows_per_sample):
    """(sample, joint token) of GEMM rows `rows` (a tensor) of batch item z of a fused QKV launch (include/x2i.h: x2i_qkv_desc)."""
    return z + torch.div(rows, rows_per_sample, rounding_mode="floor"), tok_off + rows % rows_per_sample


def vt_pos(t, perm):
    """Position of token t along a V^T row (csrc/x2i_common.h: x2i_vt_pos)."""
    if not perm:
        return t
    return (t & ~31) | (((t >> 2) & 3) << 3) | (((t >> 4) & 1) << 2) | (t & 3)


def qkv_got(Q, K, VT, b, s, vt_perm):
    """The kernel's outputs at samples b / tokens s [m]: [m, 3 H 128] in GEMM-column order."""
    m = b.shape[0]
    H = Q.shape[1]
    q = Q[b, :, s, :].reshape(m, H * 128)
    k = K[b, :, s, :].reshape(m, H * 128)
    v = VT[b, :, :, vt_pos(s, vt_perm)].reshape(m, H * 128)
    return torch.cat((q, k, v), 1)


def describe_qkv(H, b_of, s_of):
    """where(m, n) for a QKV check: sample, head, section, token, dim"""
    def where(m, n):
        sec, h, dd = n // (H * 128), (n % (H * 128)) // 128, n % 128
        return f"sample {int(b_of(m))}, head {h}, section {'qkv'[sec]}, token {int(s_of(m))}, dim {dd} (row m={m}, col n={n})"
    return where


def poison_(t):
    """fill t with the sentinel bit pattern (bf16: 0x7F7F, f32: 0x7F7F7F7F)"""
    if t.dtype == torch.float32:
        t.view(torch.int32).fill_(SENTINEL32)
    else:
        t.view(torch.int16).fill_(SENTINEL16)
    return t


def sentinel_bits(t):
    return (t.view(torch.int32) == SENTINEL32) if t.dtype == torch.float32 else (t.view(torch.int16) == SENTINEL16)


def write_mask(buf, views):
    """bool mask over the flat storage `buf` of the elements in `views`: [(shape, stride, storage offset)]"""
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    for shape, stride, off in views:
        mask.as_strided(shape, stride, off).fill_(True)
    return mask


def check_untouched(name, buf, mask, row_len=None):
    """Assert that every element of the flat storage `buf` outside `mask` still holds the sentinel.  row_len: names the first offender as
    (row, col) of a [*, row_len] view."""
    keep = sentinel_bits(buf.view(-1)) | mask
    if bool(keep.all()):
        return
    bad = torch.nonzero(~keep).view(-1)
    i = int(bad[0])
    at = f"element {i}" + (f" (row {i // row_len}, col {i % row_len})" if row_len else "")
    raise AssertionError(f"{name}: {bad.numel()} elements outside the launch's write set were written; first at {at}")


def check_qkv_padding(name, Q, K, VT, S, vt_perm):
    """Q / K rows >= S and the V^T positions that hold no token < S keep the sentinel."""
    for n, t in (("Q", Q), ("K", K)):
        ok = sentinel_bits(t[:, :, S:])
        if not bool(ok.all()):
            b, h, r, _ = (int(v) for v in torch.nonzero(~ok)[0])
            raise AssertionError(f"{name}: {n} padding row written: sample {b}, head {h}, row {S + r} (S = {S})")
    Spad = VT.shape[-1]
    used = torch.zeros(Spad, dtype=torch.bool, device=VT.device)
    used[vt_pos(torch.arange(S, device=VT.device), vt_perm)] = True
    ok = sentinel_bits(VT[..., ~used])
    if not bool(ok.all()):
        b, h, d, j = (int(v) for v in torch.nonzero(~ok)[0])
        raise AssertionError(f"{name}: V^T padding column written: sample {b}, head {h}, dim {d}, position "
                             f"{int(torch.nonzero(~used)[j])} (S = {S})")


# ---------------------------------------------------------------------------------------------------------------- operands
KINDS = ("random", "cancel", "tagged")


def tag_scales(M, K, z=0, device="cpu"):
    """`tagged` operand scales [M, K]: 2^(e_row + e_blk) with e_row = (7 (m + 3 z) mod 13) - 6 per row and e_blk = (5 kb mod 11) - 5 per
    64-wide K block kb: neighbouring rows / K-tiles / items differ by powers of two, so a row or K-tile that is read twice, missed or read
    from the wrong place changes the element that received it by a visible multiple of its share."""
    er = ((torch.arange(M, device=device) + 3 * z) * 7 % 13 - 6).double()
    eb = (torch.arange((K + 63) // 64, device=device) * 5 % 11 - 5).double().repeat_interleave(64)[:K]
    return torch.exp2(er[:, None] + eb[None, :])


def tag_scales_flat(n, lda, z=0, device="cpu"):
    """`tagged` scales [n] for the flat STORAGE of an operand whose rows overlap in memory (row stride lda < K: a strided convolution's
    A): storage element e lies in storage row e // lda, column e % lda, and gets 2^(e_row + e_blk) as in tag_scales -- per storage row and
    per 64-wide column block.  A kernel row m spans the storage rows m, m + 1, ..: each lda-wide stretch of its K carries another row
    exponent, so a stretch read from the neighbouring row, or the whole operand read densely (lda = K), changes the sum visibly."""
    e = torch.arange(n, device=device)
    er = ((torch.div(e, lda, rounding_mode="floor") + 3 * z) * 7 % 13 - 6).double()
    eb = (torch.div(e % lda, 64, rounding_mode="floor") * 5 % 11 - 5).double()
    return torch.exp2(er + eb)


def lin_scale(K):
    """rough std of lin for A ~ N(0, 1), W ~ 0.02 N(0, 1), bias ~ 0.5 N(0, 1)"""
    return math.sqrt(0.0004 * K + 0.25)


# ---------------------------------------------------------------------------------------------------------------- whole launches
ROWS = 4096     # rows per float64 block (a multiple of TILE): one [4096, 15360] float64 block is 0.5 GB


def check_gemm(rep, A, W, bias, C, *, act=ACT_NONE, gate=None, res=None, C2=None, act2=ACT_NONE, out_f32=False, rows=ROWS):
    """Every element of one x2i_gemm_bf16 problem: A [batch, M, K] (a view: the items may share their rows, a_batch_stride = 0, and the rows
    may overlap in memory, lda < K -- the reference reads what the kernel reads), W [N, K] or, a weight per item (w_batch_stride != 0),
    [batch, N, K]; C / res (the residual as it was BEFORE the launch: a clone where it shares the output's storage) / C2 [batch, M, N]
    (views), gate [batch, N] or None.  Adds to Report `rep`; returns it."""
    batch, M, _ = A.shape
    assert W.dim() == 2 or (W.dim() == 3 and W.shape[0] == batch), (tuple(W.shape), batch)
    for z in range(batch):
        Wz = W[z] if W.dim() == 3 else W
        for r0 in range(0, M, rows):
            r1 = min(M, r0 + rows)
            e = gemm_expect(A[z, r0:r1], Wz, bias, act=act, gate=gate[z] if gate is not None else None,
                            res=res[z, r0:r1] if res is not None else None, act2=act2 if C2 is not None else None, out_f32=out_f32)
            (want, bound, d), e2 = (e if C2 is not None else (e, None))
            rep.check(C[z, r0:r1], want, bound, d, item=z, row0=r0)
            del want, bound, d
            if e2 is not None:
                rep.check(C2[z, r0:r1], *e2, item=z, row0=r0, where=lambda m, n: f"C2 (m={m}, n={n})")
    return rep


def check_qkv(rep, A, W, bias, norm_q, norm_k, cos, sin, Q, K, VT, *, H, tok_off, rows_per_sample, q_scale=1.0, eps=1e-6, vt_perm=False,
              rows=ROWS):
    """Every element of one x2i_gemm_qkv_bf16 problem: A [batch, M, K] (view); Q, K [B, H, Spad, 128], VT [B, H, 128, Spad]; cos / sin as the
    kernel read them (sin None: pair form)."""
    batch, M, _ = A.shape
    dev = Q.device
    for z in range(batch):
        for r0 in range(0, M, rows):
            r1 = min(M, r0 + rows)
            idx = torch.arange(r0, r1, device=dev)
            b, s = tokens_of(idx, z, tok_off, rows_per_sample)
            c, sn = rope_rows(cos, sin, s.to(cos.device))
            want, bound, d = qkv_expect(A[z, r0:r1], W, bias, norm_q, norm_k, c.to(A.device), sn.to(A.device), H=H, q_scale=q_scale, eps=eps)
            got = qkv_got(Q, K, VT, b, s, vt_perm)
            bo = lambda m: z + m // rows_per_sample
            so = lambda m: tok_off + m % rows_per_sample
            rep.check(got, want, bound, d, item=z, row0=r0, where=describe_qkv(H, bo, so))
            del want, bound, d, got
    return rep
