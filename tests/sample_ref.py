"""The float64 reference of sampled token selection (include/ext/sample/x2i_sample.h), Philox4x32-10 in numpy, the allowance of a draw with
its derivation, the verdict, and the inputs and cases of tests/test_sample_gpu.py (a helper; it holds no tests).

THE ALLOWANCE.  The kernel gives token n the integer mass m_n = round(fl(exp(fl(s_n - s_max))) * 2^34) and adds integers, exactly; the
reference gives it w_n = exp(s_n - s_max) in float64.  Per token:
  * d = fl(s_n - s_max) is off by at most 2^-24 |d| (one f32 rounding), which moves exp(d) by the relative 2^-24 |d|.  A weight below 2^-35
    rounds to no unit at all, which is every |d| above 35 ln 2 = 24.3; so |d| <= 25 wherever the relative error matters:  25 * 2^-24
  * the f32 exp is within one ulp:                                                                                            2^-23
  * the product with 2^34 is exact and the rounding to an integer moves it by at most half a unit:                           2^-35 absolute
so |m_n 2^-34 - w_n| <= R w_n + 2^-35 with R = 25 * 2^-24 + 2^-23 = 1.61e-6, and a sum over any subset of `count` tokens is within
R * (its true value) + count * 2^-35.  A draw compares C_n / Z_fix with u, numerator and denominator sums of that kind over at most the kept
tokens, and Z >= 1 because the largest score (weight exactly 1) is always kept; the quotient of two values each within the relative
e = R + count * 2^-35 is within 2 e (1 + e).  Hence
  eps(count) = 2.001 * (R + count * 2^-35)
in units of Z: 3.3e-6 for up to 1024 kept tokens, 1.2e-5 for all 151 936.  diag's Z is the integer sum rounded once more to f32 (2^-24),
inside eps.

THE TOP-P CUT compares M, the mass of the `above` survivors strictly above a value, with top_p * Zk, Zk the mass of all `surv` survivors
(Zk >= 1), both integer sums of the kind above and the comparison itself exact.  With f = M / Zk the kernel decides as the reference does
unless |f - top_p| <= f R + above 2^-35 + top_p (R + surv 2^-35) to first order, so the margin a case must leave is
  eps_cut(f, above, surv) = 2.001 * (R (f + top_p) + (above + top_p surv) * 2^-35)
which is at most 2 eps(surv), and is NOT a constant: the largest value has nothing above it, its M is the integer 0 whatever was rounded, and
it is kept under any top_p > 0 (the library's "keep at least one"); top_p = 1e-6 lies below eps(surv) itself and is still no matter of
rounding.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MASS_BITS = 34
R = 25 * 2.0 ** -24 + 2.0 ** -23


def eps(count):
    return 2.001 * (R + count * 2.0 ** -(MASS_BITS + 1))


def eps_cut(f, above, surv, top_p):
    return 2.001 * (R * (f + top_p) + (above + top_p * surv) * 2.0 ** -(MASS_BITS + 1))


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words -> 4 words (python ints)"""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK, p1 >> 32, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, offset, col, b, word=0):
    """The kernel's u for sample b: word 0 of Philox under key (seed lo, seed hi), counter (lo32(c), hi32(c), b, 0), c = offset + col"""
    seed, c = int(seed) & (2 ** 64 - 1), (int(offset) + int(col)) & (2 ** 64 - 1)
    x = philox4x32_10((c & MASK, c >> 32, b, 0), (seed & MASK, seed >> 32))[word]
    return np.float32((x >> 8) * 2.0 ** -24)


class Selection:
    """keep bool [V], Z, lo / hi float64 [V] (a kept token's interval in units of Z), s f32 [V], survivors (of top-k), margin (the top-p
    cut's least distance to a mass fraction beyond that fraction's eps_cut, inf where top-p is off), s_min (the smallest kept value)"""


def select(p, temperature=1.0, top_k=0, top_p=1.0, topk_strict=False, topp_inclusive=False, top_p_exact=False):
    """The selection in float64 from f32 scores p.  The three flags are PLANTED FAULTS or test devices: `>` for `>=` at the top-k threshold,
    `<=` for `<` at top-p, and a top_p taken as float64 instead of being rounded to f32 first."""
    p = np.asarray(p, np.float32)
    V = p.size
    s = (p / np.float32(temperature)).astype(np.float32) + np.float32(0)       # (-0 becomes +0)
    s64 = s.astype(np.float64)
    w = np.exp(s64 - s64.max())
    keep = np.ones(V, bool)
    if top_k > 0:
        k = min(int(top_k), V)
        thr = np.partition(s, V - k)[V - k]
        keep = s > thr if topk_strict else s >= thr
    r = Selection()
    r.survivors, r.margin = int(keep.sum()), np.inf
    tp = float(top_p) if top_p_exact else float(np.float32(top_p))
    if tp < 1 and r.survivors:
        idx = np.flatnonzero(keep)
        order = idx[np.argsort(-s[idx], kind="stable")]
        so, wo = s[order], w[order]
        csum = np.cumsum(wo)
        first = np.r_[True, so[1:] != so[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(so.size), 0))
        frac = np.where(start > 0, csum[np.maximum(start - 1, 0)], 0.0) / csum[-1]     # the mass strictly above, over the survivors'
        kp = frac <= tp if topp_inclusive else frac < tp
        r.margin = float(np.min(np.abs(frac - tp) - eps_cut(frac, start, so.size, tp)))       # positive: no fraction is within its allowance of the cut
        keep = np.zeros(V, bool)
        keep[order[kp]] = True
    wk = np.where(keep, w, 0.0)
    r.keep, r.s, r.Z = keep, s, float(wk.sum())
    r.hi = np.cumsum(wk) / r.Z
    r.lo = r.hi - wk / r.Z
    r.count = int(keep.sum())
    r.s_min = s[keep].min()
    return r


def draw(ref, u, descending=False):
    """The token an exact draw gives (descending: the planted fault that walks the kept set from the top index down)"""
    kept = np.flatnonzero(ref.keep)
    w = (ref.hi - ref.lo)[kept]
    if descending:
        kept, w = kept[::-1], w[::-1]
    hit = np.flatnonzero(np.cumsum(w) > float(u))
    return int(kept[hit[0]] if hit.size else kept.max())


def admitted(ref, u, e=None):
    """The tokens the verdict admits for u: kept, lo - eps <= u < hi + eps"""
    e = eps(ref.count) if e is None else e
    u = float(u)
    return np.flatnonzero(ref.keep & (ref.lo - e <= u) & (u < ref.hi + e))


def share(ref, n, u):
    """How much of eps token n needs for u (0: inside its exact interval)"""
    return max(ref.lo[n] - float(u), float(u) - ref.hi[n], 0.0) / eps(ref.count)


def verdict(ref, n, u, diag_count, diag_Z):
    """-> the list of what is wrong with a draw of token n for u (empty: it passes)"""
    e, bad = eps(ref.count), []
    n = int(n)
    if not (0 <= n < ref.keep.size and ref.keep[n]):
        return ["token %d is not kept" % n]
    if not (ref.lo[n] - e <= float(u) < ref.hi[n] + e):
        bad.append("token %d: u=%.9g is outside [%.9g, %.9g) by more than eps=%.3g" % (n, u, ref.lo[n], ref.hi[n], e))
    if int(diag_count) != ref.count:
        bad.append("kept count %d, the reference keeps %d" % (diag_count, ref.count))
    if not abs(float(diag_Z) - ref.Z) <= e * ref.Z:
        bad.append("Z %.9g, the reference has %.9g (eps %.3g)" % (diag_Z, ref.Z, e))
    return bad


# ---- the inputs and cases of the GPU test ----------------------------------------------------------------------------------------------
KINDS = ("normal", "spike", "flat", "two", "tie", "ramp", "lastmax")
VS, BS, KS, PS, TS = (1, 17, 1000, 4099, 151936), (1, 3, 8), (0, 1, 2, 50, "V+5"), (1.0, 0.8, 1e-6), (0.1, 0.7, 1.0, 5.0)
U_FIXED = (0.0, 1 - 2.0 ** -24, 0.2512345, 0.5003219, 0.7390851, 0.9004711)
# (seed, offset, col) of the Philox draws; the second one's offset + col crosses 2^32, the third wraps 2^64
PHILOX = ((11, 0, 5), (2 ** 63 + 12345, 2 ** 32 - 3, 7), (0xDEADBEEFCAFEF00D, 2 ** 64 - 2, 6))


def scores(kind, V, seed, top_k=0):
    """One row of f32 scores.  top_k: where the `tie` kind plants its tie (the k-th and the (k+1)-th largest are made equal)"""
    g = np.random.default_rng(seed)
    if kind == "normal":
        return (2 * g.standard_normal(V)).astype(np.float32)
    if kind == "spike":                                     # all mass in one token: exp(-60) is below the fixed point's unit
        p = np.full(V, -30, np.float32) - g.random(V).astype(np.float32)
        p[V // 3] = 30
        return p
    if kind == "flat":
        return np.full(V, 1.25, np.float32)
    if kind == "two":
        p = np.full(V, -1.0, np.float32)
        p[::7] = 2.0
        return p
    if kind == "tie":
        p = (2 * g.standard_normal(V)).astype(np.float32)
        k = top_k if 0 < top_k < V else 2
        if V > k:
            order = np.argsort(-p, kind="stable")
            p[order[k]] = p[order[k - 1]]
        return p
    if kind == "ramp":                                      # at temperature 0.1 a step of 0.5 per token: no unit of mass after 49 tokens
        return (-0.05 * np.arange(V)).astype(np.float32)
    if kind == "lastmax":
        p = (2 * g.standard_normal(V)).astype(np.float32)
        p[V - 1] = p.max() + 1
        return p
    raise ValueError(kind)


def _case(V, B, kind, top_k, top_p, T, seed):
    return dict(V=V, B=B, kind=kind, top_k=V + 5 if top_k == "V+5" else top_k, top_p=top_p, temperature=T, seed=seed,
                id="%s-V%d-B%d-k%s-p%g-T%g" % (kind, V, B, top_k, top_p, T))


def cases():
    """About a hundred cases: every value of every axis, every kind at every V, three of each.  The ramp is always at temperature 0.1 (what it
    is for).  Where the reference finds a coverage condition unmet -- a kept tail of vanishing masses, which admits many tokens at u = 0 or
    at u = 1 - 2^-24, or a top-p cut too near a mass fraction -- a case without top-p gets top_p = 0.8, then another seed, then a lower
    temperature.  That is decided by the reference alone, here, once."""
    global _CASES
    if _CASES is None:
        _CASES = []
        for i in range(len(VS) * len(KINDS) * 3):
            q, r = divmod(i, 3)
            V, kind = VS[q // len(KINDS)], KINDS[q % len(KINDS)]
            k, pp, T, B = KS[(q + 2 * r) % 5], PS[(q + r) % 3], TS[(q + r) % 4], BS[(q + r) % 3]
            if V == VS[-1]:
                B = 8 if kind == "normal" and r == 0 else 3 if kind == "ramp" and r == 1 else 1       # (the reference's float64 sort of the long rows is the test's time)
            if kind == "ramp":
                T = 0.1
            for attempt in range(8):
                c = _case(V, B, kind, k, pp, T, 1000 + 17 * i + attempt)
                if not coverage(c):
                    break
                if pp == 1.0:
                    pp = 0.8
                elif attempt >= 3 and T > TS[0]:        # (a dense row leaves no margin at the cut: a peakier one)
                    T = TS[TS.index(T) - 1]
            _CASES.append(c)
        for V in VS[-2:]:       # the whole row kept, nearly all of it below one unit of mass (more than 1024 kept: the band may admit several)
            _CASES.append(_case(V, 1, "ramp", 0, 1.0, 0.1, 5000 + V))
    return _CASES


_CASES = None


def rows(case):
    """The B rows of a case's scores, f32 [B, V]"""
    return np.stack([scores(case["kind"], case["V"], case["seed"] + 1000 * b, case["top_k"]) for b in range(case["B"])])


def us(case, b):
    """The draws of sample b of a case: [(u f32, None or (seed, offset, col))]"""
    return [(np.float32(u), None) for u in U_FIXED] + [(uniform(s + case["seed"], o, c, b), (s + case["seed"], o, c)) for s, o, c in PHILOX]


_REFS = {}


def reference(case, b):
    """The Selection of sample b of a case: computed once, shared, never changed"""
    key = (case["id"], case["seed"], b)
    if key not in _REFS:
        _REFS[key] = select(rows(case)[b], case["temperature"], case["top_k"], case["top_p"])
    return _REFS[key]


def coverage(case):
    """-> the list of what a case lacks (empty: it may run): the top-p margin, and that 99 % of the draws admit exactly one token where at
    most 1024 are kept"""
    bad = []
    for b in range(case["B"]):
        ref = reference(case, b)
        if not ref.margin > 0:
            bad.append("sample %d: the top-p cut is within eps_cut of a mass fraction (by %.3g)" % (b, ref.margin))
        if ref.count <= 1024:
            n = [admitted(ref, u).size for u, _ in us(case, b)]
            if sum(x == 1 for x in n) < 0.99 * len(n):
                bad.append("sample %d: draws admit %s tokens" % (b, n))
    return bad
