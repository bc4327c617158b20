"""float64 reference of the e4m3 path (include/x2i.h "fp8 path": x2i_gemm_fp8, x2i_gemm_qkv_fp8, x2i_quantize_rows_fp8, x2i_ln_modulate_fp8,
x2i_attention_e4m3out) and a per-element checker, built on tests/gemm_ref.py and tests/ew_ref.py.  No GPU-only code here: the CPU tests of the
checker import it too.

  operands.  An e4m3 value is m 2^-9 (subnormal) or (8 + m) 2^(e - 10): the product of two is an integer multiple of 2^-18 below 2^18, and a
             sum of K <= 2^11 of them has at most 47 significant bits.  acc = sum_k a8 w8 is EXACT in float64, in any order.
  GEMM.      the kernels (gemm256_fp8.hip, gemm256p_epi.h) compute  x = fma(acc~ * (w_scale[n] * alpha), a_scale[z][m], bias[n]):
                 lin   = a_scale w_scale alpha acc + bias
                 delta = |a_scale w_scale alpha| U_ACC8 mag + 3 U_F32 |a_scale w_scale alpha acc| + U_F32 |lin|,   mag = sum_k |a8 w8|
             (the roundings of w_scale * alpha, of acc * that, and of the fma).  From (lin, delta) on the epilogue is the bf16 GEMM's:
             gemm_ref.epilogue_expect / qkv_epilogue_expect.
  e4m3 out.  C = e4m3_rne(clamp(v * out_inv_scale, +-448)) of the f32 epilogue value v~, |v~ - v| <= delta.  Rounding and clamping are
             monotone, so the decoded output lies in the closed interval
                 [e4m3_rne_sat((v - delta) oinv (1 -+ U_F32)), e4m3_rne_sat((v + delta) oinv (1 +- U_F32))]
             (no U_F32 when oinv == 1: the product is exact or skipped).  Where the two ends agree the output must be that value, bit for
             value.  An exact tie of v oinv is always two-valued while delta > 0: the direction of ties is checked where the arithmetic
             is exact -- x2i_quantize_rows_fp8 (quantize_expect, bit for bit).
  LN.        ew_ref.ln_expect gives (want, delta) of the f32 value y~.  row_scale: |rs - max|want| / 448| <= max_row(delta) / 448 + 2 U_F32
             rs (the rounded constant 1 / 448 and the product); an all-zero row has rs == 1.  Codes: the interval rule with inv = 1 / rs
             from the kernel's OWN stored scale, 3 U_F32 (2 for the reciprocal, 1 for the product).  The largest code of a row is +-448.
  attention. the f32 result o of an element satisfies bf16(o) = O, the bf16 launch of the same variant: o lies within half a bf16 ulp
             of O, and the output in [e4m3_rne_sat(lo oinv), e4m3_rne_sat(hi oinv)], lo, hi = O -+ ulp_bf16(O) / 2, one U_F32 for the product.

Sentinel of byte outputs: 0x7F, a NaN code that a saturating kernel never produces (decode gives NaN, and NaN fails every check)."""
import math

import torch

from tests import ew_ref as E
from tests import gemm_ref as G
from tests.gemm_ref import U_F32

# accumulation error of a chain of v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales) over the K-tiles, relative to mag = sum_k |a8 w8|.
# gemm_ref.U_ACC = 2^-20 does NOT hold for this instruction.  Measured on MI355X with unit scales, no bias and bf16 output, worst
# (|err| - 1/2 ulp_bf16)+ / mag over all elements (tests/test_fp8_fp64_gpu.py prints it for every plain_unit launch):
#   `cancel` launches   6.3e-6 (K = 128) 2.6e-6 (256) 1.5e-6 (384) 2.9e-6 (4136 x 3856 x 512) 7.0e-7 (5928 x 3856 x 2048)
#   `tagged` launches   8.8e-6 (K = 128) 1.1e-5 (256) 6.4e-6 (384) 1.2e-5 (4136 x 3856 x 512)
#   `random` launches   4.1e-5 (K = 128) 3.6e-5 (256) 2.4e-5 (384) 8.7e-5 (4136 x 3856 x 512) 5.2e-5 (5928 x 3856 x 2048)
#   tools/fp8_acc_probe.py, other seeds: N(0, 16^2) codes alone 1.1e-5 (K = 128) .. 3.0e-6 (K = 2048); `random` 9.3e-5 at 4136 x 3856 x 512, the worst seen
# The excess over 2^-20 is the same in every 256^2 tile (per-tile worst within a factor of ten of each other, none clean), bit for bit the
# same in the one-tile, persistent and stream-K forms, and present at every shape, at a single K-tile too: a property of the instruction,
# not of a kernel.  It goes with the largest product of a K-tile, not with K: relative to max |a| max |w| of the element's row and column
# it is 4e-5 .. 3e-4 for every kind, and the `random` kind's +-448 codes, whose products stand far above the rest of the sum, show it most
# (N(0, 16^2) codes with +-448 sprinkled in and nothing else: 3.0e-5; with subnormal codes or zeros instead: as without).  This is what an
# adder that aligns the 128 products of one instruction to the largest and drops the bits below a fixed width would give; the instruction's
# documentation does not say (tools/fp8_acc_probe.py, profiles/fp8_acc_probe.log).
# The bound has to hold for every kind, so it is taken from the largest ratio of any launch (the `cancel` launches alone, 6.3e-6, would
# give 2^-16, which the `random` launches exceed): the smallest power of two at or above 2 x 9.3e-5.
U_ACC8 = 2.0 ** -12
E4M3_MAX = 448.0
SENTINEL8 = 0x7F
FP8 = torch.float8_e4m3fn
KINDS = ("random", "cancel", "tagged")
TINY = 2.0 ** -20        # below every distance between two e4m3 values (>= 2^-9) and between a value and a midpoint (>= 2^-10)

# the old style of check (tests/test_fp8_gpu.py), kept here only to show what it misses (tests/test_fp8_ref_cpu.py)
OLD_GEMM_REL_L2 = 4e-3
OLD_CODE_MISMATCH = 2e-3
OLD_E4M3_REL_L2 = 4e-2
OLD_SCALE_RTOL = 1e-4
OLD_LN_CODES_REL_L2 = 3e-2


def f32(x):
    """the f32 value of a Python float, as a float"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- e4m3 in float64
def _decode_table():
    t = []
    for c in range(256):
        s, e, m = (-1.0 if c & 0x80 else 1.0), (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            t.append(math.nan)
        elif e == 0:
            t.append(s * m * 2.0 ** -9)
        else:
            t.append(s * (8 + m) * 2.0 ** (e - 10))
    return torch.tensor(t, dtype=torch.float64)


DECODE = _decode_table()
_tables = {}


def as_codes(t):
    """uint8 view of an e4m3 (or already uint8) tensor"""
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def decode(t):
    """e4m3 codes -> float64 (0x7F / 0xFF: NaN)"""
    c = as_codes(t)
    key = str(c.device)
    if key not in _tables:
        _tables[key] = DECODE.to(c.device)
    return _tables[key][c.long()]


def ulp_e4m3(x):
    """spacing of e4m3 at |x|: 2^(max(floor(log2 |x|), -6) - 3) (float64), from the exponent bits as gemm_ref.ulp_bf16"""
    e = (x.double().abs().clamp_min(2.0 ** -6).view(torch.int64) >> 52) & 0x7FF
    return ((e - 3) << 52).view(torch.float64)


def e4m3_rne_sat(x, codes=False):
    """float64 -> clamp to +-448, then the nearest e4m3 value, ties to even (x / ulp is exact: a power of two).  codes=True: the uint8 codes
    (the sign of x is kept on a zero result, as the hardware conversion and torch keep it).  x finite."""
    x = x.double()
    xc = x.clamp(-E4M3_MAX, E4M3_MAX)
    u = ulp_e4m3(xc)
    r = torch.round(xc / u) * u
    if not codes:
        return r
    a = r.abs()
    e = ((a.clamp_min(2.0 ** -6).view(torch.int64) >> 52) & 0x7FF) - 1023 + 7          # exponent field of a normal result
    p2 = ((e - 7 + 1023) << 52).view(torch.float64)
    normal = a >= 2.0 ** -6
    m = torch.where(normal, (a / p2 - 1.0) * 8.0, a * 512.0).long()
    c = torch.where(normal, e << 3, torch.zeros_like(e)) | m | (torch.signbit(x).long() << 7)
    return c.to(torch.uint8)


def e4m3_interval(v, d, oinv=1.0, ulps=None):
    """(lo, hi) float64: the e4m3 values a kernel may store for an f32 value within d of v, scaled by oinv > 0 with `ulps` U_F32 of relative
    error on the product (default: 1, or 0 when oinv == 1)"""
    assert oinv is not None and (not isinstance(oinv, float) or oinv > 0)
    if ulps is None:
        ulps = 0.0 if isinstance(oinv, float) and oinv == 1.0 else 1.0
    lo, hi = (v - d) * oinv, (v + d) * oinv
    lo = lo - ulps * U_F32 * lo.abs()
    hi = hi + ulps * U_F32 * hi.abs()
    return e4m3_rne_sat(lo), e4m3_rne_sat(hi)


def interval_bound(lo, hi):
    """(want, bound) such that |g - want| <= bound iff lo <= g <= hi for e4m3 values g (a single-valued interval gets TINY, not 0: 0 / 0
    would poison the checker's statistics, and no two e4m3 values are that close)"""
    return 0.5 * (lo + hi), (0.5 * (hi - lo)).clamp_min(TINY)


def poison_(t):
    """fill t with the sentinel (byte outputs: 0x7F; bf16 / f32: gemm_ref.poison_)"""
    if t.element_size() == 1:
        as_codes(t).fill_(SENTINEL8)
        return t
    return G.poison_(t)


def sentinel_bits(t):
    return (as_codes(t) == SENTINEL8) if t.element_size() == 1 else G.sentinel_bits(t)


def check_untouched(name, buf, mask, row_len=None):
    """gemm_ref.check_untouched for a flat byte, bf16 or f32 storage"""
    if buf.element_size() != 1:
        return G.check_untouched(name, buf, mask, row_len)
    keep = sentinel_bits(buf.view(-1)) | mask
    if bool(keep.all()):
        return
    bad = torch.nonzero(~keep).view(-1)
    i = int(bad[0])
    at = f"element {i}" + (f" (row {i // row_len}, col {i % row_len})" if row_len else "")
    raise AssertionError(f"{name}: {bad.numel()} bytes outside the launch's write set were written; first at {at}")


# ---------------------------------------------------------------------------------------------------------------- GEMM expectation
def deq_linear(A8, W8, bias=None, *, a_scale=None, w_scale=None, alpha=1.0, bias2=None, u_acc=None):
    """(lin, delta, acc_part) float64 [m, N] of the dequantised product of A8 [m, K], W8 [N, K] (e4m3 or uint8), a_scale [m] / w_scale [N]
    f32 or None, bias [N] bf16 or None; acc_part = |a_scale w_scale alpha| mag, the factor of U_ACC8 in delta."""
    u_acc = U_ACC8 if u_acc is None else u_acc
    a, w = decode(A8), decode(W8)
    acc = a @ w.T
    mag = (a.abs().float() @ w.abs().float().T).double()       # (for the bound only)
    del a, w
    s = torch.full((1, 1), f32(alpha), dtype=torch.float64, device=acc.device)
    if w_scale is not None:
        s = s * w_scale.double()[None, :]
    if a_scale is not None:
        s = s * a_scale.double()[:, None]
    lin0 = s * acc
    lin = lin0.clone()
    d = torch.zeros_like(lin)
    if bias is not None:
        lin += bias.double()
    if bias2 is not None:
        lin += bias2.double()
        if bias is not None:
            d += U_F32 * (bias.double() + bias2.double()).abs()       # (their f32 sum)
    part = s.abs() * mag
    d += u_acc * part + 3 * U_F32 * lin0.abs() + U_F32 * lin.abs()
    return lin, d, part


def gemm8_expect(A8, W8, bias=None, *, a_scale=None, w_scale=None, alpha=1.0, act=G.ACT_NONE, gate=None, res=None, out_fp8=False,
                 out_inv_scale=1.0, u_acc=None):
    """Expected output of x2i_gemm_fp8 for the rows A8 [m, K] of one batch item.  bf16 output: (want, bound, delta) as gemm_ref.gemm_expect;
    out_fp8: (lo, hi), the interval of the decoded output."""
    lin, d, _ = deq_linear(A8, W8, bias, a_scale=a_scale, w_scale=w_scale, alpha=alpha, u_acc=u_acc)
    want, bound, delta = G.epilogue_expect(lin, d, act=act, gate=gate, res=res)
    if not out_fp8:
        return want, bound, delta
    return e4m3_interval(want, delta, f32(out_inv_scale))


def qkv8_expect(A8, W8, bias, norm_q, norm_k, c, s, *, H, a_scale=None, w_scale=None, alpha=1.0, q_scale=1.0, eps=1e-6):
    """Expected Q / K / V rows of x2i_gemm_qkv_fp8: as gemm_ref.qkv_expect"""
    lin, d, _ = deq_linear(A8, W8, bias, a_scale=a_scale, w_scale=w_scale, alpha=alpha)
    return G.qkv_epilogue_expect(lin, d, norm_q, norm_k, c, s, H=H, q_scale=q_scale, eps=eps)


# ---------------------------------------------------------------------------------------------------------------- checker
class Report(G.Report):
    """gemm_ref.Report with e4m3 blocks: check8 compares decoded codes with an interval; `two` / `n` count the two-valued intervals
    (information only)."""

    def __init__(self, name):
        super().__init__(name)
        self.two, self.n = 0, 0

    def check8(self, got8, lo, hi, *, item=0, row0=0, where=None):
        want, bound = interval_bound(lo, hi)
        msg, _, _, tiles = G.check_block(f"{self.name} (e4m3), item {item}", decode(got8), want, bound, row0=row0, where=where)
        self.two += int((lo != hi).sum())
        self.n += lo.numel()
        if msg:
            self.msgs.append(msg)
            self.tiles += len(tiles)
        return msg

    def two_share(self):
        return self.two / max(self.n, 1)


def check_gemm8(rep, A8, W8, bias, C, *, a_scale=None, w_scale=None, alpha=1.0, act=G.ACT_NONE, gate=None, res=None, out_fp8=False,
                out_inv_scale=1.0, rows=G.ROWS, u_acc=None):
    """Every element of one x2i_gemm_fp8 problem: A8 [batch, M, K], C / res (as it was BEFORE the launch) [batch, M, N] (views), a_scale
    [batch, M] or None, gate [batch, N] or None.  Adds to Report `rep`; returns it."""
    batch, M, _ = A8.shape
    for z in range(batch):
        for r0 in range(0, M, rows):
            r1 = min(M, r0 + rows)
            e = gemm8_expect(A8[z, r0:r1], W8, bias, a_scale=a_scale[z, r0:r1] if a_scale is not None else None, w_scale=w_scale, alpha=alpha,
                             act=act, gate=gate[z] if gate is not None else None, res=res[z, r0:r1] if res is not None else None,
                             out_fp8=out_fp8, out_inv_scale=out_inv_scale, u_acc=u_acc)
            if out_fp8:
                rep.check8(C[z, r0:r1], *e, item=z, row0=r0)
            else:
                rep.check(C[z, r0:r1], *e, item=z, row0=r0)
            del e
    return rep


def acc_share(A8, W8, C, rows=G.ROWS):
    """The U_ACC8 measurement of one launch with unit scales, no bias, bf16 output C [M, N]: worst (|err| - 1/2 ulp_bf16)+ / mag"""
    worst = 0.0
    for r0 in range(0, A8.shape[0], rows):
        a, w = decode(A8[r0:r0 + rows]), decode(W8)
        acc = a @ w.T
        mag = a.abs() @ w.abs().T
        err = (C[r0:r0 + rows].double() - acc).abs()
        over = (err - 0.5 * G.ulp_bf16(C[r0:r0 + rows].double())).clamp_min(0)     # (got's own ulp: the rounding the kernel did)
        worst = max(worst, float((over / mag.clamp_min(2.0 ** -18)).max()))
    return worst


def check_qkv8(rep, A8, W8, bias, norm_q, norm_k, cos, sin, Q, K, VT, *, H, tok_off, rows_per_sample, a_scale=None, w_scale=None, alpha=1.0,
               q_scale=1.0, eps=1e-6, vt_perm=False, rows=G.ROWS):
    """Every element of one x2i_gemm_qkv_fp8 problem, as gemm_ref.check_qkv: A8 [batch, M, K] (view), a_scale [batch, M] or None"""
    batch, M, _ = A8.shape
    dev = Q.device
    for z in range(batch):
        for r0 in range(0, M, rows):
            r1 = min(M, r0 + rows)
            idx = torch.arange(r0, r1, device=dev)
            b, s = G.tokens_of(idx, z, tok_off, rows_per_sample)
            c, sn = G.rope_rows(cos, sin, s.to(cos.device))
            want, bound, d = qkv8_expect(A8[z, r0:r1], W8, bias, norm_q, norm_k, c.to(dev), sn.to(dev), H=H,
                                         a_scale=a_scale[z, r0:r1] if a_scale is not None else None, w_scale=w_scale, alpha=alpha, q_scale=q_scale,
                                         eps=eps)
            got = G.qkv_got(Q, K, VT, b, s, vt_perm)
            bo = lambda m, z=z: z + m // rows_per_sample
            so = lambda m: tok_off + m % rows_per_sample
            rep.check(got, want, bound, d, item=z, row0=r0, where=G.describe_qkv(H, bo, so))
            del want, bound, d, got
    return rep


# ---------------------------------------------------------------------------------------------------------------- quantise, LayerNorm
def quantize_expect(x, static_inv_scale=None):
    """x2i_quantize_rows_fp8 of x bf16 [rows, cols] (CPU f32 arithmetic is IEEE, as the kernel's): (codes uint8, scales f32 or None), exact"""
    xf = x.float().cpu()
    if static_inv_scale is None:
        amax = xf.abs().amax(1)
        s = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
        inv = 1.0 / s
    else:
        s, inv = None, torch.full((xf.shape[0],), static_inv_scale, dtype=torch.float32)
    return e4m3_rne_sat((xf * inv[:, None]).double(), codes=True), s


class RowReport(E.Report):
    """ew_ref.Report of one x2i_ln_modulate_fp8 launch: `worst` stays the share of the LN allowance the bf16 Y used, `rs_worst` is the worst
    |err| / bound of a row scale, `two` / `n` count the two-valued code intervals (information only)."""

    def __init__(self, name):
        super().__init__(name)
        self.two, self.n, self.rs_worst = 0, 0, 0.0

    def check_apart(self, *a, **k):
        """check() that leaves `worst` alone; returns the block's own worst |err| / bound"""
        keep, self.worst = self.worst, 0.0
        self.check(*a, **k)
        keep, self.worst = self.worst, keep
        return keep

    def two_share(self):
        return self.two / max(self.n, 1)


def check_ln8(rep, X3, Y3, Y8, rs, S0, sh0, sc0, sh1, sc1, eps):
    """Every output of one x2i_ln_modulate_fp8 launch: X3 [B, S, D], Y3 [B, S, D] bf16 or None, Y8 [B, S, D] codes, rs f32 [B S] (all after
    the launch), shift / scale [B, >= D] views.  Adds to RowReport `rep`."""
    B, S, D = X3.shape
    dev = X3.device
    for b in range(B):
        for lo_, hi_, sh, sc in ((0, S0, sh0, sc0), (S0, S, sh1, sc1)):
            if hi_ <= lo_:
                continue
            want, bound, delta = E.ln_expect(X3[b, lo_:hi_], sh[b, :D], sc[b, :D], eps)
            tok = torch.arange(lo_, hi_, device=dev)
            smp = torch.full_like(tok, b)
            if Y3 is not None:
                rep.check(Y3[b, lo_:hi_], want, bound, delta, sample=smp, token=tok, what=" Y")
            r = rs[b * S + lo_:b * S + hi_].double()[:, None]
            amax, dmax = want.abs().amax(-1, keepdim=True), delta.amax(-1, keepdim=True)
            zero = (amax == 0) & (dmax == 0)
            rs_want = torch.where(zero, torch.ones_like(amax), amax / E4M3_MAX)
            rs_bound = torch.where(zero, torch.zeros_like(amax), dmax / E4M3_MAX + 2 * U_F32 * r)
            rep.rs_worst = max(rep.rs_worst, rep.check_apart(r, rs_want, rs_bound.clamp_min(2.0 ** -200), sample=smp, token=tok, unit=1,
                                                             what=" row_scale"))
            ok = torch.isfinite(r) & (r > 0)
            inv = 1.0 / torch.where(ok, r, torch.full_like(r, math.nan))
            lo, hi = e4m3_interval(want, delta, inv, ulps=3.0)
            w8, b8 = interval_bound(lo, hi)
            g = decode(Y8[b, lo_:hi_])
            rep.check_apart(g, w8, b8, sample=smp, token=tok, what=" e4m3")
            rep.two += int((lo != hi).sum())
            rep.n += lo.numel()
            top = g.abs().amax(-1, keepdim=True)
            top_want = torch.where(zero, torch.zeros_like(amax), torch.full_like(amax, E4M3_MAX))
            rep.check_apart(top, top_want, torch.full_like(amax, TINY), sample=smp, token=tok, unit=1, what=" largest code of the row")
    return rep


def attn8_interval(O, oinv):
    """(lo, hi) of x2i_attention_e4m3out's decoded output from O, the bf16 launch of the same variant"""
    o = O.double()
    h = 0.5 * G.ulp_bf16(o)
    # (below a power of two the spacing halves: the values that round to O from below lie within a quarter of ulp_bf16(O) there -- the
    # half-ulp used here is the wider, still valid, interval)
    return e4m3_interval(o, h, f32(oinv), ulps=0.0 if f32(oinv) == 1.0 else 1.0)


# ---------------------------------------------------------------------------------------------------------------- operands
def _randn(shape, gen, device):
    return torch.randn(shape, generator=gen, device=device)


def _rand(shape, gen, device):
    return torch.rand(shape, generator=gen, device=device)


def random_codes(shape, gen, device, std=16.0, sprinkle=True):
    """e4m3 codes of N(0, std^2), made here (never by the quantise kernel), never 0x7F / 0xFF; with `sprinkle`, 1/64 subnormal codes, 1/64 +-0
    and 1/512 +-448"""
    c = e4m3_rne_sat((_randn(shape, gen, device) * std).double(), codes=True)
    if sprinkle:
        r = _rand(shape, gen, device)
        sign = (_rand(shape, gen, device) < 0.5).to(torch.uint8) << 7
        sub = (1 + (_rand(shape, gen, device) * 7).long().clamp(0, 6)).to(torch.uint8)
        c = torch.where(r < 1 / 64, sub | sign, c)
        c = torch.where((r >= 1 / 64) & (r < 2 / 64), sign, c)
        c = torch.where((r >= 2 / 64) & (r < 2 / 64 + 1 / 512), sign | 0x7E, c)
    assert not bool(((c & 0x7F) == 0x7F).any())
    return c


def k_tags(K, device):
    """`tagged` exponent offsets [K] within +-3: (3 kt mod 5) - 2 per 128-byte K-tile kt plus (kg mod 3) - 1 per 16-byte group kg of the tile"""
    k = torch.arange(K, device=device)
    return (3 * (k // 128)) % 5 - 2 + ((k % 128) // 16) % 3 - 1


def operands(M, N, K, kind, gen, device, batch=1):
    """(A8 uint8 [batch, M, K], W8 uint8 [N, K]) of one kind:
    random   N(0, 16^2) quantised, with subnormal codes, +-0 and +-448 sprinkled in
    cancel   a[2i+1] = -a[2i], w[2i+1] = w[2i], except on 1/64 of the pairs, where a[2i+1] is one mantissa step off: |lin| << mag, and the
             accumulation error shows above the output rounding
    tagged   exponent fields of A moved by k_tags (within [1, 14]: base exponents clamped to [4, 11]); the row / column / item tags go into
             the scales (tag_scales8)"""
    assert K % 128 == 0 and kind in KINDS
    A = random_codes((batch, M, K), gen, device, sprinkle=kind == "random")
    W = random_codes((N, K), gen, device, sprinkle=kind == "random")
    if kind == "cancel":
        ae = A[..., 0::2]
        off = _rand(ae.shape, gen, device) < 1 / 64
        odd = torch.where(off & ((ae & 0x7F) != 0x7E), ae ^ 0x81, ae ^ 0x80)
        A = torch.stack((ae, odd), -1).view(batch, M, K)
        W = W[:, 0::2].repeat_interleave(2, 1)
    elif kind == "tagged":
        e = ((A >> 3) & 15).long().clamp(4, 11) + k_tags(K, device)
        A = (A & 0x87) | (e << 3).to(torch.uint8)
    assert not bool(((A & 0x7F) == 0x7F).any())
    return A.contiguous(), W.contiguous()


def tag_scales8(M, N, batch, device, base_a=1.0, base_w=1.0):
    """`tagged` scales: a_scale [batch, M] = base_a 2^((3 (m + 2 z) mod 7) - 3) (1 + (m mod 5) / 8), w_scale [N] = base_w 2^((5 n mod 7) - 3)
    (1 + (n mod 3) / 8): neighbouring rows, rows 16 apart, columns and batch items all differ, by at least 1/8"""
    m = torch.arange(M, device=device)[None, :]
    z = torch.arange(batch, device=device)[:, None]
    n = torch.arange(N, device=device)
    a = base_a * torch.exp2(((3 * (m + 2 * z)) % 7 - 3).double()) * (1 + (m % 5).double() / 8)
    w = base_w * torch.exp2(((5 * n) % 7 - 3).double()) * (1 + (n % 3).double() / 8)
    return a.float().contiguous(), w.float().contiguous()


def random_scales(M, N, batch, gen, device, base_a=1.0, base_w=1.0):
    """a_scale [batch, M], w_scale [N]: base times 2^U(-1, 1)"""
    a = base_a * torch.exp2(2 * _rand((batch, M), gen, device) - 1)
    w = base_w * torch.exp2(2 * _rand((N,), gen, device) - 1)
    return a.float().contiguous(), w.float().contiguous()


def unit_bases(K):
    """(base_a, base_w) that bring lin of N(0, 16^2) codes to a standard deviation of about 2"""
    return 1 / 16, 2 / (16 * math.sqrt(K))
