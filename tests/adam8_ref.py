"""float64 reference of one block-wise 8-bit AdamW step (csrc/optim8.hip: x2i_adamw8_blockwise_bf16; the format is DESIGN.md section 4) and
a per-element checker that names the parameter, the block and the element of a failure.  No GPU-only code here: tests/test_adam8_ref_cpu.py
imports it too.  It also holds Adam8F64, the format as a float64 optimizer (no f32, no bf16), for the toy problem that shows what the format
costs against plain AdamW and why a positive second moment never takes the zero code.

`expect` computes from the state the kernel READ -- codes, absmax, bf16 p, f32 g, the clip coefficient and the f32 scalars -- in block form
([blocks, 256] with a validity mask): the exact m*, v*, p*, the two absmax* and the normalised values x* = m* / absmax_m*, v* / absmax_v*,
each with the bound on what the kernel's f32 evaluation may differ by.  u = U_F32 = 2^-24; every operation the kernel spells out (__fmul_rn,
fmaf, __fdiv_rn, __fsqrt_rn) is correctly rounded: relative error <= u.  SLACK = 1 + 2^-10 covers the second-order terms.

  scalars.  The kernel receives f32 lr, b1, b2, eps, wd, bc1 = f32(1 - beta1^step), bc2 and forms omb1 = 1 - b1, omb2 = 1 - b2 (exact for
       b >= 1/2, Sterbenz) and decay = 1 - f32(lr wd) in f32; `scalars` restates these operations in f32, so they are inputs here, not errors.
  m.   gg = cf g (u);  t = omb1 gg (u): |t~ - t| <= 2u |t|;  d = map_s[c] absmax (u);  m = fma(b1, d, t) (u |m|):
       dm = SLACK u (|b1 d| + 2 |t| + |m*|).
  v.   t = (omb2 gg) gg: gg enters twice (2u) and two products (2u);  d = map_u[c] absmax (u);  v = fma(b2, d, t):
       dv = SLACK u (|b2 d| + 4 t + v*).
  absmax.  max |m~| and max v~ over the block's valid elements, exact operations on the m~, v~: within the largest dm (dv) of the block.
  x.   r = 1 / absmax~ (DIV_U), x~ = m~ r (u):  m~ / a~ - m* / a* = (m~ - m*) / a~ + m* (1 / a~ - 1 / a*), so
       dx = SLACK ((dm + |x*| dabsmax) / (absmax* - dabsmax) + (DIV_U + u) |x*|);  absmax* = 0 gives x = 0 exactly (the zero entry).
  code.  The kernel's code is the rank of x~ among its f32 midpoints 0.5f * (map[k] + map[k + 1]): one rounded sum, the halving exact,
       |mid~ - mid| <= u |mid|.  Index k is accepted if its cell [mid[k - 1], mid[k]] (exact midpoints, each end moved outwards by u |mid|;
       the outer cells unbounded) meets [x* - dx, x* + dx]: a tie, or a value within dx of a midpoint, may go either way.  For v* > 0 the zero
       index is never accepted, and index 1 (the smallest positive entry) is accepted wherever index 0 would have been.
  p.   mh = m / bc1 (DIV_U): dmh = dm / bc1 + DIV_U |mh|;  vh = v / bc2: dvh = dv / bc2 + DIV_U vh;  s = sqrt(vh): ds = SLACK s dvh / (2 vh)
       + DIV_U s (v is a sum of non-negative terms: dvh / vh is a few u);  den = s + eps: dden = ds + u den;  num = lr mh: dnum = lr dmh +
       u |num|;  q = num / den: dq = (dnum + |q| dden) / (den - dden) + DIV_U |q|;  p = fma(p_old, decay, -q): dp = SLACK (dq + u |p*|).
       p is bf16, rounded once: the bound is dp + 1/2 ulp_bf16(|p*| + dp), so either neighbour passes where p* lies within dp of a bf16
       midpoint (gemm_ref._round_bound, as ew_ref does for bf16 outputs).

Constants: DIV_U.  __fdiv_rn / __fsqrt_rn are correctly rounded (u); 4u is allowed, as ew_ref allows 2 ulps where 1 is documented.  Nothing
here is tuned to the kernel's output.  Measured share of the f32 part of p's bound used, max over the launches of tests/test_adam8_gpu.py on
MI355X ((|err| - rounding part)+ / dp, as ew_ref's statistic): see P_SHARE_MEASURED below."""
import math

import numpy as np
import torch

from tests.gemm_ref import U_F32, _round_bound

BLOCK = 256
MIN_8BIT_SIZE = 4096
SLACK = 1.0 + 2.0 ** -10
DIV_U = 4.0 * U_F32
# largest share of dp any launch of tests/test_adam8_gpu.py used on MI355X (printed by the tests; not an input to any bound)
P_SHARE_MEASURED = 0.365   # the grid-stride launch (8196 blocks, 2.1 M elements); 0.040 at most in the other launches
ZERO_SIGNED, ZERO_UNSIGNED = 127, 0


def f32(x):
    """the f32 value of a Python float, as a float"""
    return float(np.float32(x))


def dynamic_map_f64(signed):
    """The code map restated from the format's definition (numpy float64, sorted): x2i_amd.optim.dynamic_map must equal its f32 rounding."""
    vals = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i if signed else 2 ** (i + 1)
        e = np.linspace(0.1, 1.0, k + 1)
        mid = (e[:-1] + e[1:]) / 2 * 10.0 ** (i - 6)
        vals += list(mid) + (list(-mid) if signed else [])
    return np.sort(np.array(vals, dtype=np.float64))


def maps(device="cpu"):
    """(signed, unsigned) maps: float64 tensors holding the f32 entries the kernel reads"""
    return tuple(torch.from_numpy(dynamic_map_f64(s).astype(np.float32).astype(np.float64)).to(device) for s in (True, False))


def scalars(*, lr, beta1, beta2, eps, weight_decay, step):
    """the f32 values the kernel computes with, as Python floats (ops.adamw8_ passes 1 - beta^step evaluated in double, rounded to f32)"""
    F = np.float32
    lr_, b1, b2, wd = F(lr), F(beta1), F(beta2), F(weight_decay)
    return dict(lr=float(lr_), b1=float(b1), b2=float(b2), eps=f32(eps), omb1=float(F(1) - b1), omb2=float(F(1) - b2),
                decay=float(F(1) - lr_ * wd), bc1=f32(1.0 - beta1 ** step), bc2=f32(1.0 - beta2 ** step))


def to_blocks(tensors):
    """[blocks, 256] form of a list of per-parameter tensors (flattened; each starts a new block, positions behind a ragged end hold 0).
    Returns (values, valid mask)."""
    vals, valid = [], []
    for t in tensors:
        t = t.reshape(-1)
        pad = -t.numel() % BLOCK
        vals.append(torch.nn.functional.pad(t, (0, pad)).view(-1, BLOCK))
        valid.append(torch.nn.functional.pad(torch.ones_like(t, dtype=torch.bool), (0, pad)).view(-1, BLOCK))
    return torch.cat(vals), torch.cat(valid)


def table_rows_of(sizes):
    """[(parameter index, first element, count)] for the blocks of parameters with `sizes` elements, in order"""
    return [(i, e, min(BLOCK, n - e)) for i, n in enumerate(sizes) for e in range(0, n, BLOCK)]


def expect(code_m, code_v, absmax_m, absmax_v, p, g, valid, coef, sc, map_s, map_u):
    """One step from the state the kernel read.  code_* uint8 / int [B, 256], absmax_* f32 [B], p bf16 [B, 256], g f32 [B, 256], valid bool
    [B, 256], coef the f32 clip coefficient (a float) or None, sc = scalars(...), maps float64 [256].  Returns a dict of float64 tensors:
    m, v, p, xm, xv [B, 256] and am, av [B], with d<name> the bound on the kernel's f32 evaluation of each (p: the f32 part; bp: with the
    bf16 rounding)."""
    u = U_F32
    cf = 1.0 if coef is None else float(coef)
    z = torch.zeros_like(g, dtype=torch.float64)
    gg = cf * g.double()
    d_m = map_s[code_m.long()] * absmax_m.double()[:, None]
    d_v = map_u[code_v.long()] * absmax_v.double()[:, None]
    t_m = sc["omb1"] * gg
    t_v = sc["omb2"] * gg * gg
    m = torch.where(valid, sc["b1"] * d_m + t_m, z)
    v = torch.where(valid, sc["b2"] * d_v + t_v, z)
    dm = torch.where(valid, SLACK * u * ((sc["b1"] * d_m).abs() + 2 * t_m.abs() + m.abs()), z)
    dv = torch.where(valid, SLACK * u * ((sc["b2"] * d_v).abs() + 4 * t_v + v), z)
    am, av = m.abs().amax(1), v.amax(1)
    dam, dav = dm.amax(1), dv.amax(1)

    def norm(val, dval, a, da):
        a_, da_ = a[:, None], da[:, None]
        x = torch.where(a_ > 0, val / a_.clamp_min(1e-300), z)
        room = a_ - da_
        dx = SLACK * ((dval + x.abs() * da_) / room.clamp_min(1e-300) + (DIV_U + u) * x.abs())
        dx = torch.where(a_ > 0, torch.where(room > 0, dx, torch.full_like(dx, math.inf)), z)
        return x, dx

    xm, dxm = norm(m, dm, am, dam)
    xv, dxv = norm(v, dv, av, dav)
    mh = m / sc["bc1"]
    dmh = dm / sc["bc1"] + DIV_U * mh.abs()
    vh = v / sc["bc2"]
    dvh = dv / sc["bc2"] + DIV_U * vh
    s = vh.sqrt()
    ds = torch.where(vh > 0, SLACK * s * dvh / (2 * vh.clamp_min(1e-300)) + DIV_U * s, z)
    den = s + sc["eps"]
    dden = ds + u * den
    num = sc["lr"] * mh
    dnum = sc["lr"] * dmh + u * num.abs()
    q = num / den
    dq = (dnum + q.abs() * dden) / (den - dden) + DIV_U * q.abs()
    pn = torch.where(valid, p.double() * sc["decay"] - q, z)
    dp = torch.where(valid, SLACK * (dq + u * pn.abs()), z)
    return dict(m=m, v=v, dm=dm, dv=dv, am=am, av=av, dam=dam, dav=dav, xm=xm, xv=xv, dxm=dxm, dxv=dxv, p=pn, dp=dp,
                bp=_round_bound(pn, dp, False), valid=valid)


def code_ok(code, x, dx, qmap, positive=None):
    """bool [B, 256]: is index `code` an acceptable nearest entry of qmap for a value within dx of x?  positive: bool mask of the elements
    under the positive-v rule (index 0 refused, index 1 accepted where 0 would have been)."""
    mid = (qmap[1:] + qmap[:-1]) / 2
    inf = torch.full((1,), math.inf, dtype=torch.float64, device=qmap.device)
    lo = torch.cat((-inf, mid - U_F32 * mid.abs()))
    hi = torch.cat((mid + U_F32 * mid.abs(), inf))

    def meets(k):
        return (lo[k] <= x + dx) & (hi[k] >= x - dx)

    k = code.long()
    ok = meets(k)
    if positive is not None:
        ok = torch.where(positive, (k != 0) & (ok | ((k == 1) & meets(torch.zeros_like(k)))), ok)
    return ok


def check_step(name, exp, got_p, got_cm, got_cv, got_am, got_av, map_s, map_u, where=None):
    """Compare what the kernel left -- p bf16 / codes [B, 256], absmax f32 [B] -- with `exp` = expect(...).  Raises AssertionError naming the
    parameter, block and element of the first failure of each kind (where[b] = (parameter name, block index within it)); returns the largest
    share of p's f32 allowance used."""
    valid = exp["valid"]
    msgs = []

    def at(b, e=None):
        par, blk = where[b] if where is not None else ("?", b)
        return f"parameter {par}, block {blk} (launch block {b})" + (f", element {e} (parameter element {blk * BLOCK + e})" if e is not None else "")

    for what, got, want, bound in (("absmax_m", got_am, exp["am"], exp["dam"]), ("absmax_v", got_av, exp["av"], exp["dav"])):
        err = (got.double() - want).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            b = int(torch.nonzero(bad)[0])
            msgs.append(f"{name}: {what} of {int(bad.sum())} blocks over the bound; first: {at(b)}: got {float(got[b]):.9g} want "
                        f"{float(want[b]):.9g} bound {float(bound[b]):.3e}")
    err = (got_p.double() - exp["p"]).abs()
    bad = valid & ~(err <= exp["bp"])
    over = (err - (exp["bp"] - exp["dp"])).clamp_min(0)
    share = torch.where(valid & (over > 0), over / exp["dp"], torch.zeros_like(over))
    share = torch.where(torch.isfinite(share), share, torch.full_like(share, math.inf))
    if bool(bad.any()):
        b, e = (int(i) for i in torch.nonzero(bad)[0])
        msgs.append(f"{name}: p of {int(bad.sum())} elements over the bound; first: {at(b, e)}: got {float(got_p[b, e]):.9g} want "
                    f"{float(exp['p'][b, e]):.9g} bound {float(exp['bp'][b, e]):.3e}")
    for what, got, x, dx, qmap, pos in (("code_m", got_cm, exp["xm"], exp["dxm"], map_s, None),
                                        ("code_v", got_cv, exp["xv"], exp["dxv"], map_u, exp["v"] > 0)):
        bad = valid & ~code_ok(got, x, dx, qmap, pos)
        if bool(bad.any()):
            b, e = (int(i) for i in torch.nonzero(bad)[0])
            msgs.append(f"{name}: {what} of {int(bad.sum())} elements is not a nearest entry; first: {at(b, e)}: got index {int(got[b, e])} "
                        f"(entry {float(qmap[int(got[b, e])]):.6g}) for x = {float(x[b, e]):.9g} +- {float(dx[b, e]):.2e}"
                        + (" (v > 0: the zero index is never accepted)" if pos is not None and bool(pos[b, e]) and int(got[b, e]) == 0 else ""))
    if msgs:
        raise AssertionError("; ".join(msgs))
    return float(share.max()) if share.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- the format in float64
def quantise(x, qmap, positive_rule=False):
    """index of the entry of qmap (float64, sorted) nearest to x; ties to the lower entry.  positive_rule: x > 0 never gives index 0."""
    k = torch.bucketize(x, (qmap[1:] + qmap[:-1]) / 2)
    return torch.where((x > 0) & (k == 0), torch.ones_like(k), k) if positive_rule else k


class Adam8F64:
    """The format as an optimizer in float64 on one flat vector of n elements (n a multiple of 256): nothing rounds but the quantisation."""

    def __init__(self, n, positive_rule=True):
        self.map_s, self.map_u = maps()
        self.cm = torch.full((n // BLOCK, BLOCK), ZERO_SIGNED)
        self.cv = torch.full((n // BLOCK, BLOCK), ZERO_UNSIGNED)
        self.am = torch.zeros(n // BLOCK, dtype=torch.float64)
        self.av = torch.zeros(n // BLOCK, dtype=torch.float64)
        self.rule, self.t = positive_rule, 0

    def step(self, p, g, lr, b1, b2, eps, wd):
        self.t += 1
        g = g.view(-1, BLOCK)
        m = b1 * self.map_s[self.cm] * self.am[:, None] + (1 - b1) * g
        v = b2 * self.map_u[self.cv] * self.av[:, None] + (1 - b2) * g * g
        p = p * (1 - lr * wd) - (lr * (m / (1 - b1 ** self.t)) / ((v / (1 - b2 ** self.t)).sqrt() + eps)).view(-1)
        self.am, self.av = m.abs().amax(1), v.amax(1)
        z = torch.zeros_like(m)
        self.cm = quantise(torch.where(self.am[:, None] > 0, m / self.am[:, None].clamp_min(1e-300), z), self.map_s)
        self.cv = quantise(torch.where(self.av[:, None] > 0, v / self.av[:, None].clamp_min(1e-300), z), self.map_u, self.rule)
        return p


def adamw_f64(p, g, m, v, t, lr, b1, b2, eps, wd):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p * (1 - lr * wd) - lr * (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps), m, v


def toy_distance(positive_rule, *, seed=0, n=4096, lo=-1.5, hi=1.5, lr=1e-3, wd=1e-2, steps=200, b1=0.9, b2=0.999, eps=1e-8):
    """Noisy gradients of a quadratic, g = scale (p - target + 0.3 noise) with per-element scales logspace(lo, hi) permuted, so that every
    block holds the whole spread: ||p8 - p32|| / ||p32|| after `steps` steps of Adam8F64 against float64 AdamW on the same noise."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # 4096-element operations: a thread pool costs thirty times what it saves
    try:
        return _toy_distance(positive_rule, seed, n, lo, hi, lr, wd, steps, b1, b2, eps)
    finally:
        torch.set_num_threads(threads)


def _toy_distance(positive_rule, seed, n, lo, hi, lr, wd, steps, b1, b2, eps):
    gen = torch.Generator().manual_seed(seed)
    target = torch.randn(n, dtype=torch.float64, generator=gen)
    scale = torch.logspace(lo, hi, n, dtype=torch.float64)[torch.randperm(n, generator=gen)]
    p8 = torch.zeros(n, dtype=torch.float64)
    p32, m, v = p8.clone(), p8.clone(), p8.clone()
    opt = Adam8F64(n, positive_rule)
    for t in range(1, steps + 1):
        noise = 0.3 * torch.randn(n, dtype=torch.float64, generator=gen)
        p8 = opt.step(p8, (p8 - target + noise) * scale, lr, b1, b2, eps, wd)
        p32, m, v = adamw_f64(p32, (p32 - target + noise) * scale, m, v, t, lr, b1, b2, eps, wd)
    return float((p8 - p32).norm() / p32.norm())
