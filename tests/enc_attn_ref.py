"""The online softmax of the encoder, resampler and decode attention kernels, restated for the tests (no tests here, and no GPU-only code:
tests/test_enc_attn_ref_cpu.py and tests/test_encoder_attention_fp64_gpu.py both import it).

  x2i_amd/csrc/encoder_attention.hip + encoder_attention_tile.inc   RELBIAS, CAUSAL, CAUSAL_PLAIN, CAUSAL_EXT (wave-wide defer test), SEGMENT (per row)
  resampler_attn_kernel (resampler.hip)                             per row, NP = 2 / 4 key parts merged through LDS
  decode_attention_kernel + decode_attention_combine_kernel         256-key chunks under their true maximum, merged by the combine

All of them keep a running maximum while no row grew by more than THR = 8 in the exp2 domain, and multiply l and O by
alpha = exp2(m_run - m_new) only when it moves.  The suite's random inputs (scores of std ~3.2 in the exp2 domain) almost never make it
move after a row's first tile (three existing cases do, by accident of their seeds), so a kernel that rescales wrongly passed nearly every test.  This module holds

  Head / problem_*   one (sample, head) of a launch as the kernel sees it: float64 and f32 scores in the exp2 domain for every row a wave
                     holds (dead rows too: they vote in the wave-wide test), the counted-key mask, and the walk of every 32-row wave as key
                     blocks per key part
  walk               the walk model: which rows take alpha != 1 with l_run > 0 (a *genuine* rescale) at which step, each step's growth
                     mx - m_run, and the merge weights of the parts.  With emulate=True the same walk in the kernel's arithmetic (f32 scores
                     and sums, bf16 P, one output rounding) with fault switches: the CPU restatement
  coverage / meets   what a set of inputs exercises; the GPU cases assert it before they launch
  plant_* / build_*  the input kinds spike, ramp, last, dead (and a masked twin) on top of each mode's attention_inputs
  reference          float64 O, and the per-element allowance |O - ref| <= TOL_ROW |ref| + 2^-8 A + F32 A
"""
import math

import torch

from tests import qwen_ref as QR
from tests import qwen_vision_ref as VR
from tests import t5_ref as TR
from tests.t5_ref import TOL_ROW

THR = 8.0                 # the kernels' defer threshold (exp2 domain)
NEG_BIG = -1.0e30         # a masked score (encoder_common.h)
M_FLOOR = -1.0e15         # where the running maximum starts outside RELBIAS
LOG2E = 1.4426950408889634
KVB, WAVE, CHUNK = 64, 32, 256
BAND = (7.0, 9.0)         # no step's growth may lie here: the kernel's f32 scores and the float64 model could take different branches
U32 = 2.0 ** -24          # unit roundoff of f32
U_P = 2.0 ** -8           # one rounding of p to bf16: half an ulp is at most 2^-8 of the value (8 significand bits)
STRENGTH = 30.0           # a planted spike's score above an ordinary one, exp2 domain
RAMP = 5.5                # the ramp's step per walk step, exp2 domain: below THR, twice it above BAND
FAULTS = ("no_o_rescale", "one_dblock", "alpha_lane0", "wave_rule", "drop_merge_weight", "off_3pct")


# ---------------------------------------------------------------------------------------------------------------- one head of a launch
class Head:
    """One (sample b, query head h).  rows: everything a wave of the launch holds, in 32-row groups.
      s2, s2f   [R, Kn] scores in the exp2 domain, float64 and in the kernel's f32 order (product, one multiply or fma)
      mask      [R, Kn] bool, key j counts for row i
      V         [Kn, d] float64 (bf16 values)
      sched     [(r0, r1, parts)]: the rows r0..r1-1 of one wave and its key parts, a part being the (k0, k1) key blocks it walks in order
      rule      "wave" or "row": who decides that the running maximum stays
      m0        where the running maximum starts; merge: the parts are merged (resampler LDS merge, decode combine) from m_merge0
      live      [R] bool: the row is stored, at output row `out_row`
      sabs      [R] max over the counted keys of sum_i |q_i k_ji| scale2 + |bias|: the magnitude the f32 score error scales with"""

    def __init__(self, b, h, q, k, v, scale2, mask, sched, rule, m0, live, out_row, bias2=None, merge=False, m_merge0=M_FLOOR, relbias=False):
        f = torch.float64
        q, k, v = q.to(f), k.to(f), v.to(f)
        q = torch.where(live[:, None], q, torch.nan_to_num(q, nan=0.0))     # (the resampler's rows >= NQ may hold anything; they vote nowhere)
        self.b, self.h, self.rule, self.m0, self.merge, self.m_merge0 = b, h, rule, m0, merge, m_merge0
        self.mask, self.V, self.sched, self.live, self.out_row = mask, v, sched, live, out_row
        self.s2 = q @ k.t() * scale2
        sf = q.float() @ k.float().t()
        if relbias:   # fma(s, log2 e, table * log2 e), the table scaled in f32 on its way into LDS
            self.s2 = self.s2 + bias2
            self.s2f = sf * torch.tensor(LOG2E, dtype=torch.float32) + (bias2 / LOG2E).float() * torch.tensor(LOG2E, dtype=torch.float32)
        else:
            self.s2f = sf * torch.tensor(scale2, dtype=torch.float32)
        mag = q.abs() @ k.abs().t() * scale2 + (bias2.abs() if bias2 is not None else 0.0)
        self.sabs = torch.where(mask, mag, torch.zeros_like(mag)).max(1).values if mask.shape[1] else torch.zeros(q.shape[0], dtype=f)
        self.n = mask.sum(1)
        self.dk = q.shape[1]


def _ceil(a, b):
    return (a + b - 1) // b * b


def _tiles(t0, t1, n):
    """the key blocks of the tiles t0..t1 (inclusive), cut at n keys"""
    return [(t * KVB, min((t + 1) * KVB, n)) for t in range(t0, t1 + 1) if t * KVB < n]


def problem_relbias(Q, K, V, table, S, R):
    """t5_ops.attention_relbias: every wave computes every tile; the rows >= S of the last wave read Q row min(q, Spad - 1)"""
    B, H, Spad, dk = Q.shape
    Rn = _ceil(S, WAVE)
    i = torch.arange(Rn)
    idx = (torch.arange(S)[None, :] - i[:, None]).clamp(-R, R) + R
    mask = torch.ones((Rn, S), dtype=torch.bool)
    sched = [(r, r + WAVE, [_tiles(0, (S - 1) // KVB, S)]) for r in range(0, Rn, WAVE)]
    return [Head(b, h, Q[b, h, i.clamp(max=Spad - 1)], K[b, h, :S], V[b, h, :S], LOG2E, mask, sched, "wave", NEG_BIG, i < S, i,
                 bias2=table[h].double()[idx] * LOG2E, relbias=True) for b in range(B) for h in range(H)]


def problem_causal(Q, K, V, S, scale, k_lo=None, k_hi=None, row0=None):
    """qwen_ops.attention / clip_ops.attention_causal (row0 None) and qwen_extend_ops.attention (rows row0 .. S - 1, k_hi = S): key j counts
    for row i iff k_lo <= j <= min(i, k_hi - 1).  A dead row of the extension takes the Q of the nearest live row and masks by its own index"""
    B, Hq, Spad, dk = Q.shape
    rep = Hq // K.shape[1]
    first = 0 if row0 is None else row0 // WAVE * WAVE
    i = torch.arange(first, _ceil(S, WAVE))
    j = torch.arange(S)
    heads = []
    for b in range(B):
        lo = 0 if k_lo is None else min(max(int(k_lo[b]), 0), S)
        hi = S if k_hi is None else min(max(int(k_hi[b]), 0), S)
        qidx = i.clamp(max=Spad - 1) if row0 is None else i.clamp(row0, S - 1)
        mask = (j[None, :] >= lo) & (j[None, :] <= torch.minimum(i, torch.tensor(hi - 1))[:, None])
        sched = []
        for q0 in range(first, _ceil(S, WAVE), WAVE):
            on = q0 < S and q0 + 31 >= lo and hi > lo and (row0 is None or q0 + 31 >= row0)
            sched.append((q0 - first, q0 - first + WAVE, [_tiles(lo // KVB, min(q0 // KVB, (hi - 1) // KVB), S)] if on else []))
        live = (i < S) & (i >= (row0 or 0))
        for h in range(Hq):
            heads.append(Head(b, h, Q[b, h, qidx], K[b, h // rep, :S], V[b, h // rep, :S], scale * LOG2E, mask, sched, "wave", M_FLOOR, live,
                              i - (row0 or 0)))
    return heads


def problem_segment(Q, K, V, S, dk, scale, row_lo=None, row_hi=None):
    """vit_ops.attention: a key range per query row, the defer test per row; a wave walks the tiles of the union of its rows' ranges"""
    B, H, Spad, _ = Q.shape
    Rn = _ceil(S, WAVE)
    i = torch.arange(Rn)
    j = torch.arange(S)
    heads = []
    for b in range(B):
        lo = torch.zeros(S, dtype=torch.long) if row_lo is None else torch.as_tensor(row_lo[b], dtype=torch.long).clamp(0, S)
        hi = torch.full((S,), S, dtype=torch.long) if row_hi is None else torch.as_tensor(row_hi[b], dtype=torch.long).clamp(0, S)
        lo, hi = lo[i.clamp(max=S - 1)], hi[i.clamp(max=S - 1)]
        mask = (j[None, :] >= lo[:, None]) & (j[None, :] < hi[:, None])
        sched = []
        for q0 in range(0, Rn, WAVE):
            ne = hi[q0:q0 + WAVE] > lo[q0:q0 + WAVE]
            if bool(ne.any()):
                ulo, uhi = int(lo[q0:q0 + WAVE][ne].min()), int(hi[q0:q0 + WAVE][ne].max())
                sched.append((q0, q0 + WAVE, [_tiles(ulo // KVB, (uhi - 1) // KVB, S)]))
            else:
                sched.append((q0, q0 + WAVE, []))
        for h in range(H):
            heads.append(Head(b, h, Q[b, h, i.clamp(max=Spad - 1), :dk], K[b, h, :S, :dk], V[b, h, :S, :dk], scale * LOG2E, mask, sched, "row",
                              M_FLOOR, i < S, i))
    return heads


def resampler_parts(NQ, nk):
    """the key blocks of each of the NP key parts over the 128-key steps (resampler.hip): NP = 2 a whole 64-key tile, NP = 4 a 32-key sub-tile"""
    NP = 2 if NQ > 32 else 4
    nkw = 64 if NP == 2 else 32
    parts = []
    for kp in range(NP):
        off = kp * 64 if NP == 2 else (kp >> 1) * 64 + (kp & 1) * 32
        parts.append([(n * 128 + off, min(n * 128 + off + nkw, nk)) for n in range((nk + 127) // 128) if n * 128 + off < nk])
    return parts


def problem_resampler(Q, K, V, counts, scale, NQ, L):
    """resampler_ops.attention: Q [H, NQpad, 128] shared by the samples, keys j < clamp(n_keys[b], 0, L); per row; merged parts"""
    B, H = K.shape[:2]
    NQpad = _ceil(NQ, WAVE)
    i = torch.arange(NQpad)
    heads = []
    for b in range(B):
        nk = L if counts is None else min(max(int(counts[b]), 0), L)
        mask = torch.ones((NQpad, nk), dtype=torch.bool)
        sched = [(r, r + WAVE, resampler_parts(NQ, nk)) for r in range(0, NQpad, WAVE)]
        for h in range(H):
            heads.append(Head(b, h, Q[h, :NQpad], K[b, h, :nk], V[b, h, :nk], scale * LOG2E, mask, sched, "row", M_FLOOR, i < NQ, i, merge=True))
    return heads


def problem_decode(Qd, K, V, k_lo, k_hi, scale):
    """qwen_decode_ops.attention: one row per query head; a 256-key chunk is one block under its true maximum; the combine merges the chunks"""
    B, Hq, dk = Qd.shape
    cap = K.shape[2]
    rep = Hq // K.shape[1]
    heads = []
    for b in range(B):
        lo, hi = min(max(int(k_lo[b]), 0), cap), min(max(int(k_hi[b]), 0), cap)
        n = max(hi - lo, 0)
        parts = [[(max(lo, c * CHUNK) - lo, min(hi, (c + 1) * CHUNK) - lo)] for c in range(lo // CHUNK, (hi - 1) // CHUNK + 1)] if n else []
        for h in range(Hq):
            heads.append(Head(b, h, Qd[b, h][None], K[b, h // rep, lo:lo + n], V[b, h // rep, lo:lo + n], scale * LOG2E,
                              torch.ones((1, n), dtype=torch.bool), [(0, 1, parts)], "row", NEG_BIG, torch.ones(1, dtype=torch.bool),
                              torch.zeros(1, dtype=torch.long), merge=True, m_merge0=NEG_BIG))
    return heads


# ---------------------------------------------------------------------------------------------------------------- the walk
def walk(hd, emulate=False, fault=None):
    """-> (steps, merges, O [R, d]).  The model (emulate=False) is float64 throughout and reads nothing but the reference's scores; its O is
    the softmax itself.  emulate=True is the kernel's arithmetic: f32 scores, p = exp2(s - m) summed unrounded in f32, P rounded to bf16
    before P V, f32 accumulators, the deferred walk, the merge in part order, one rounding of O.  fault: one of FAULTS.
      steps   dict(wave, part, k0, last, growth [n], genuine [n], before [n] (l_run > 0 on entry), moved)  per (wave, part, key block)
      merges  dict(wave, weights [NP, n], genuine [NP, n])"""
    f = torch.float32 if emulate else torch.float64
    s_all = hd.s2f if emulate else hd.s2
    V = hd.V.to(f)
    R, d = s_all.shape[0], V.shape[1]
    rule = "wave" if fault == "wave_rule" else hd.rule
    O = torch.zeros((R, d), dtype=f)
    steps, merges = [], []
    neg = torch.tensor(NEG_BIG, dtype=f)
    for wv, (r0, r1, parts) in enumerate(hd.sched):
        n = r1 - r0
        recs = []
        for pi, blocks in enumerate(parts):
            m = torch.full((n,), hd.m0, dtype=f)
            l = torch.zeros(n, dtype=f)
            acc = torch.zeros((n, d), dtype=f)
            for bi, (k0, k1) in enumerate(blocks):
                sm = torch.where(hd.mask[r0:r1, k0:k1], s_all[r0:r1, k0:k1], neg)
                mx = sm.max(1).values
                m_new = torch.maximum(m, mx)
                keep = (m_new - m) <= THR
                if rule == "wave":
                    if bool(keep.all()):
                        m_new = m
                else:
                    m_new = torch.where(keep, m, m_new)
                alpha = torch.exp2(m - m_new)
                moved = not bool((m_new == m).all())
                steps.append(dict(wave=wv, part=pi, k0=k0, last=bi == len(blocks) - 1, growth=(mx - m).double(), genuine=(m_new != m) & (l > 0),
                                  before=l > 0, moved=moved))
                p = torch.exp2(sm - m_new[:, None])
                if fault == "alpha_lane0":
                    alpha = alpha[:1].expand(n)
                l = l * alpha + p.sum(1)
                if moved:
                    if fault == "one_dblock":
                        acc[:, :32] *= alpha[:, None]
                    elif fault != "no_o_rescale":
                        acc = acc * alpha[:, None]
                acc = acc + (p.bfloat16().to(f) if emulate else p) @ V[k0:k1]
                m = m_new
            recs.append((m, l, acc))
        if not recs:
            continue
        if hd.merge:
            m_all = torch.full((n,), hd.m_merge0, dtype=f)
            for m, _, _ in recs:
                m_all = torch.maximum(m_all, m)
            w = torch.stack([torch.exp2(m - m_all) for m, _, _ in recs])
            merges.append(dict(wave=wv, weights=w.double(), genuine=(w != 1) & torch.stack([l > 0 for _, l, _ in recs])))
            if fault == "drop_merge_weight":
                w = w.clone()
                w[0] = 1.0
            l = torch.zeros(n, dtype=f)
            acc = torch.zeros((n, d), dtype=f)
            for pi, (_, lp, ap) in enumerate(recs):
                l = l + lp * w[pi]
                acc = acc + ap * w[pi][:, None]
        else:
            _, l, acc = recs[0]
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        O[r0:r1] = acc * inv[:, None]
    if emulate:
        O = O.bfloat16().to(f)
    if fault == "off_3pct":
        live = torch.nonzero(hd.live)[:, 0]
        flat = int(O[live].abs().argmax())
        O[live[flat // d], flat % d] *= 1.03
    return steps, merges, O


def coverage(heads):
    """What the inputs exercise, over every head, from the walk model alone.  Row-steps and genuine rescales count live rows; the band check
    counts every row a wave holds, because a dead row votes in the wave-wide test.
      row_steps   (row, step) pairs that follow the row's first live block       genuine    those with alpha != 1
      mixed       steps where some live rows with l > 0 rescale and others keep alpha = 1
      deferred    row-steps kept at the old maximum although the row grew by a value in (4, 7)
      last        genuine rescales at the last block of a wave's walk            twice      rows with two or more genuine rescales
      dead        genuine rescales in waves that also hold dead rows             merge      merge weights != 1 on a part with l > 0
      wide        those merge weights below 2^-8: one part dominates by more than the defer threshold
      band        growths inside BAND, any row                                   max_growth the largest growth of a row that had l > 0"""
    c = dict(row_steps=0, genuine=0, mixed=0, deferred=0, last=0, twice=0, dead=0, merge=0, wide=0, band=0, max_growth=0.0)
    for hd in heads:
        per_row = torch.zeros(hd.live.shape[0], dtype=torch.long)
        steps, merges, _ = walk(hd)
        for s in steps:
            r0, r1, _ = hd.sched[s["wave"]]
            live = hd.live[r0:r1]
            g, gen, bef = s["growth"], s["genuine"] & live, s["before"] & live
            c["row_steps"] += int(bef.sum())
            c["genuine"] += int(gen.sum())
            c["mixed"] += int(bool(gen.any()) and bool((bef & ~gen).any()))
            c["deferred"] += int((bef & ~gen & (g > 4) & (g < 7)).sum())
            c["last"] += int(gen.sum()) if s["last"] else 0
            c["dead"] += int(gen.sum()) if not bool(live.all()) else 0
            c["band"] += int(((g >= BAND[0]) & (g <= BAND[1])).sum())
            if bool(s["before"].any()):
                c["max_growth"] = max(c["max_growth"], float(g[s["before"]].max()))
            per_row[r0:r1] += gen.long()
        c["twice"] += int((per_row >= 2).sum())
        for mg in merges:
            r0, r1, _ = hd.sched[mg["wave"]]
            c["merge"] += int((mg["genuine"] & hd.live[r0:r1][None, :]).sum())
            c["wide"] += int((mg["genuine"] & (mg["weights"] < 2.0 ** -THR) & hd.live[r0:r1][None, :]).sum())
    return c


def meets(kind, cov):
    """The coverage condition of an input kind (the issue's): at least one genuine rescale (of a step, or of the merge where the kernel has
    no other), nothing inside BAND, and what the kind is for"""
    ok = cov["genuine"] + cov["merge"] >= 1 and cov["band"] == 0
    if kind == "spike":
        ok = ok and (cov["mixed"] >= 1 or cov["wide"] >= 1)
    elif kind == "ramp":
        ok = ok and (cov["deferred"] >= 1 or cov["row_steps"] == 0 and cov["merge"] >= 1)     # (decode: a chunk is one block; the ramp is its combine's)
    elif kind == "last":
        ok = ok and (cov["last"] >= 1 or cov["wide"] >= 1)
    elif kind == "dead":
        ok = ok and cov["dead"] >= 1
    return ok


# ---------------------------------------------------------------------------------------------------------------- reference and allowance
def reference(heads, shape):
    """-> (ref, allow), float64 of `shape` [B, H, rows, d]: the masked softmax times V per live row, and the per-element allowance

        |O - ref| <= TOL_ROW |ref| + 2^-8 A + F32 A,     A = sum_j softmax_j |v_j|

    TOL_ROW |ref|: the one rounding of O to bf16 (half an ulp, 2 % margin; tests/t5_ref.py).  2^-8 A: every p_j is rounded to bf16 before
    P V, half an ulp each (at most 2^-8 p_j), while l sums the unrounded p_j, so the roundings do not cancel in O = sum p_j v_j / l.
    F32 A covers the f32 arithmetic, worst case and linear in the roundings (nothing in it is fitted):
      * a score is dk exact products summed in f32, one multiply by scale2 (or one fma with the bias), then s - m: an absolute error of at
        most u ((dk + 2) sabs + 2 sabs), u = 2^-24, sabs = max_j (sum_i |q_i k_ji| scale2 + |bias|) >= |s|, |m|
      * exp2 turns an absolute error e into a relative one of e ln 2, and v_exp_f32 adds 1 ulp = 2 u:   rho = u (ln 2 (dk + 4) sabs + 2) on p_j
      * a relative error rho on every p_j moves sum p_j v_j / sum p_j by at most 2 rho A
      * the sums over n counted keys: l and each O accumulator take at most n additions of positive / signed terms, n u A each, and each
        of the walk's at most n / 32 + 1 rescales and the merge two more roundings: (2 n + 4 (n / 32 + 1) + 4) u A <= (2.2 n + 8) u A
    F32 = u (2 ln 2 (dk + 4) sabs + 2.2 n + 12).  At dk = 128, sabs ~ 25, n = 300 that is 3e-4, a tenth of the bf16 terms: the allowance is
    the two bf16 roundings, and an f32 summation order cannot decide a case.
    Measured, on the CPU restatement (walk(emulate=True)) over every case of the GPU module, not on a kernel: the worst share of the allowance
    used is 0.755 (a three-key row); of F32 A alone the restatement's f32 arithmetic cannot be told apart from the bf16 roundings, which is
    why no constant in it is a measured one."""
    ref = torch.zeros(shape, dtype=torch.float64)
    allow = torch.zeros(shape, dtype=torch.float64)
    for hd in heads:
        rows = torch.nonzero(hd.live)[:, 0]
        s = torch.where(hd.mask[rows], hd.s2[rows], torch.tensor(float("-inf"), dtype=torch.float64))
        some = hd.mask[rows].any(1)
        p = torch.zeros_like(s)
        if s.shape[1]:
            p[some] = torch.softmax(s[some] * math.log(2.0), -1)
        o, a = p @ hd.V, p @ hd.V.abs()
        f32 = U32 * (2 * math.log(2.0) * (hd.dk + 4) * hd.sabs[rows] + 2.2 * hd.n[rows].double() + 12)
        ref[hd.b, hd.h, hd.out_row[rows]] = o
        allow[hd.b, hd.h, hd.out_row[rows]] = TOL_ROW * o.abs() + (U_P + f32[:, None]) * a
    return ref, allow


def shares(out, ref, allow):
    """|out - ref| / allow per element; an element whose allowance is 0 (a zero row) must be met exactly"""
    err = (out.detach().double().cpu() - ref).abs()
    sh = err / allow.clamp_min(1e-300)
    return torch.where(allow > 0, sh, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))


def check_elements(name, out, ref, allow):
    """Assert every element of out [B, H, rows, d] inside its allowance; returns the worst share used"""
    sh = shares(out, ref, allow)
    bad = ~(sh <= 1.0)       # (NaN fails too)
    if bool(bad.any()):
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("%s: element %s is %r, float64 says %r: %.2f of its allowance %.3e; %d of %d elements over"
                             % (name, i, float(out[i]), float(ref[i]), float(sh[i]), float(allow[i]), int(bad.sum()), bad.numel()))
    return float(sh.max()) if sh.numel() else 0.0


def emulate(heads, shape, fault=None, only=None):
    """The CPU restatement over every head -> bf16-valued float64 `shape`.  only: the index of the one head that carries the fault"""
    out = torch.zeros(shape, dtype=torch.float64)
    for n, hd in enumerate(heads):
        _, _, O = walk(hd, emulate=True, fault=fault if only is None or only == n else None)
        rows = torch.nonzero(hd.live)[:, 0]
        out[hd.b, hd.h, hd.out_row[rows]] = O[rows].double()
    return out


# ---------------------------------------------------------------------------------------------------------------- the input kinds
def directions(shape, dk, seed):
    """one unit direction per key/value head, zero beyond dk: [..., 1, width]"""
    u = torch.zeros(shape)
    u[..., :dk] = torch.randn(shape[:-1] + (dk,), generator=torch.Generator().manual_seed(seed))
    return u / u.norm(dim=-1, keepdim=True)


def _without(T, u, n, gain=1.0):
    """rows < n of T with their component along u removed (so that a planted score is the planted product and nothing else), times gain"""
    t = T[..., :n, :].float()
    return gain * (t - (t * u).sum(-1, keepdim=True) * u)


def plant_spikes(Q, K, u, rep, n_q, n_k, scale2, rows, keys):
    """In place, bf16 Q [.., Hq, >= n_q, w] and K [.., Hkv, >= n_k, w]: u projected out of the rows < n_q / < n_k, then the query rows `rows`
    shifted by a u and key `key` by mult a u for (key, mult) in keys, a^2 scale2 = STRENGTH: those rows score mult STRENGTH above an ordinary
    score against that key, every other (row, key) pair scores what its other components give.  The queries' own components are halved
    (scores of std ~1.6 in the exp2 domain): at the full 3.2 an ordinary row's tile maxima land inside BAND once in about two thousand
    row-steps, which a case of several heads cannot avoid, and at half of it they do not"""
    a = (STRENGTH / scale2) ** 0.5
    uq = u.repeat_interleave(rep, dim=-3)
    q, k = _without(Q, uq, n_q, 0.5), _without(K, u, n_k)
    q[..., rows, :] += a * uq
    for key, mult in keys:
        k[..., key, :] += mult * a * u[..., 0, :]
    Q[..., :n_q, :], K[..., :n_k, :] = q.bfloat16(), k.bfloat16()


def plant_ramp(Q, K, u, rep, n_q, n_k, scale2, sub, step):
    """In place: the queries' own components damped to a tenth (scores of std ~0.3: the maximum of a full tile and the few counted scores of
    a diagonal tile then differ by about 1, so that a growth is the ramp's, RAMP or 2 RAMP, and stays clear of BAND), every query shifted by
    a u and key j by (j // sub) a u with a^2 scale2 = step: the scores of each `sub` keys sit `step` above those of the `sub` before"""
    a = (step / scale2) ** 0.5
    uq = u.repeat_interleave(rep, dim=-3)
    q, k = _without(Q, uq, n_q, 0.1) + a * uq, _without(K, u, n_k)
    k += (torch.arange(n_k) // sub).float()[:, None] * a * u
    Q[..., :n_q, :], K[..., :n_k, :] = q.bfloat16(), k.bfloat16()


def with_spike_at(K, u, key, scale2, mult=1.0):
    """a copy of K with key `key` shifted as plant_spikes shifts a spike's key (the masked twin: a key that counts for no spiked row)"""
    K2 = K.clone()
    K2[..., key, :] = (K[..., key, :].float() + mult * (STRENGTH / scale2) ** 0.5 * u[..., 0, :]).bfloat16()
    return K2


def subset(rows, residues=(5, 17)):
    """the rows whose index mod 32 is one of `residues`: a part of every wave, so that a moving wave has rows that keep alpha = 1"""
    rows = torch.as_tensor(rows)
    keep = torch.zeros_like(rows, dtype=torch.bool)
    for r in residues:
        keep |= rows % WAVE == r
    return rows[keep]


def built_at(make, seed):
    """make(seed) -> (inputs, heads); -> (inputs, heads, coverage).  One draw, from the case's own seed: whether it meets the kind's coverage
    condition is asserted by the tests (CPU: every case; GPU: each case before it launches)"""
    inp, heads = make(seed)
    return inp, heads, coverage(heads)


# ---- T5 (RELBIAS).  (dk, S, R): the three widths, and R = 4, where every (wave, tile) pair beyond +-4 takes the uniform bias
T5_CASES = [(32, 200, 128), (64, 300, 128), (128, 260, 128), (64, 200, 4)]


def build_t5(kind, dk, S, R, seed=0, B=1, H=2):
    T = (S + KVB - 1) // KVB

    def make(sd):
        Q, K, V, table = TR.attention_inputs(B, H, S, dk, R, seed=sd)
        u = directions((B, H, 1, dk), dk, sd + 1)
        if kind == "ramp":     # (the bias table damped as the queries are: its entries differ from tile to tile as the scores do)
            plant_ramp(Q, K, u, 1, S, S, LOG2E, KVB, RAMP)
            table = 0.1 * table
        elif kind == "last":   # the ragged last tile
            plant_spikes(Q, K, u, 1, S, S, LOG2E, subset(torch.arange(S)), [(S - 1, 1.0)])
        else:                  # a late tile for a part of every wave, and the last tile for a part of those
            plant_spikes(Q, K, u, 1, S, S, LOG2E, subset(torch.arange(S)), [((T - 2) * KVB + 13, 1.0), ((T - 1) * KVB + 3, 2.0)])
        return dict(Q=Q, K=K, V=V, table=table, S=S, R=R, u=u, twice=kind == "spike"), problem_relbias(Q, K, V, table, S, R)
    return built_at(make, 1000 * S + dk + R + seed)


# ---- CLIP and Qwen2 (CAUSAL_PLAIN, CAUSAL).  (B, Hq, Hkv, S, dk, k_lo, k_hi)
QWEN_CASES = [(1, 7, 1, 300, 64, None, None), (1, 4, 2, 300, 128, None, None), (1, 2, 1, 300, 128, [70], [290]), (2, 4, 2, 200, 128, [70, 0], [200, 150])]
CLIP_CASES = [(1, 2, 300)]


def causal_keys(kind, S, lo, hi):
    """(rows, keys, twice) of one sample of a causal case with the range [lo, hi).  The walk of a row goes from tile lo / 64 to the tile of
    min(S, hi) - 1 or its own diagonal.  spike -- key 13 of a tile past the first (the third from the end where there are that many) for the
    rows past it, and key 13 of the next tile at twice the strength (twice: there is such a tile, and rows that walk both); last -- a key of
    the tile that holds min(S, hi) - 1, the diagonal tile of the rows that count it.  With lo > 0 the rows from lo on are aligned and key
    lo itself carries a third of a spike: the first counted key of the first walked tile then owns those rows (10 above an ordinary score)
    until the spike proper, which still grows by 2/3 STRENGTH, and a lower mask that is off by one loses it"""
    top = min(S, hi)
    t0, T = lo // KVB, (top - 1) // KVB
    first = [(lo, 1.0 / 3)] if lo > 0 else []
    if kind == "last":
        key = max(T * KVB + 2, lo + 1)
        return subset(torch.arange(lo if lo > 0 else key, S)), first + [(key, 1.0)], False
    t1 = max(T - 2, t0 + 1)
    k1 = min(t1 * KVB + 13, top - 1)
    keys = first + [(k1, 1.0)] + ([(min((t1 + 1) * KVB + 13, top - 1), 2.0)] if t1 + 1 <= T else [])
    return subset(torch.arange(lo if lo > 0 else k1, S)), keys, t1 + 1 <= T


def plant_causal(kind, Q, K, u, rep, S, scale2, k_lo, k_hi, row_min=0):
    """plant_spikes per sample, each with the keys of its own range -> whether some sample has rows with two spikes"""
    twice = False
    for b in range(Q.shape[0]):
        rows, keys, tw = causal_keys(kind, S, 0 if k_lo is None else int(k_lo[b]), S if k_hi is None else int(k_hi[b]))
        plant_spikes(Q[b:b + 1], K[b:b + 1], u[b:b + 1], rep, S, S, scale2, rows[rows >= row_min], keys)
        twice = twice or tw
    return twice


def build_causal(kind, B, Hq, Hkv, S, dk, k_lo, k_hi, seed=0):
    scale = dk ** -0.5

    def make(sd):
        Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=sd)
        u = directions((B, Hkv, 1, dk), dk, sd + 1)
        twice = False
        if kind == "ramp":
            plant_ramp(Q, K, u, Hq // Hkv, S, S, scale * LOG2E, KVB, RAMP)
        else:
            twice = plant_causal(kind, Q, K, u, Hq // Hkv, S, scale * LOG2E, k_lo, k_hi) and kind == "spike"
        return dict(Q=Q, K=K, V=V, S=S, k_lo=k_lo, k_hi=k_hi, scale=scale, u=u, twice=twice), problem_causal(Q, K, V, S, scale, k_lo, k_hi)
    return built_at(make, 1000 * S + dk + Hq + seed)


# ---- the Qwen2 prompt extension (CAUSAL_EXT).  (B, Hq, Hkv, dk, cap, row0, n, k_lo): row0 inside a wave (rows 64..69 of the wave 64..95 are
# dead, and so are 291..319 of the last one)
EXT_CASES = [(1, 4, 2, 128, 320, 70, 221, None), (2, 7, 1, 64, 320, 70, 221, [0, 40])]


def build_ext(kind, B, Hq, Hkv, dk, cap, row0, n, k_lo, seed=0):
    S, scale = row0 + n, dk ** -0.5

    def make(sd):
        Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=sd, Spad=cap)
        u = directions((B, Hkv, 1, dk), dk, sd + 1)
        twice = False
        if kind == "ramp":
            plant_ramp(Q, K, u, Hq // Hkv, S, S, scale * LOG2E, KVB, RAMP)
        elif kind == "dead":
            # the wave 64..95: tiles 0 and 1; the spike at key 66 of tile 1 is seen by the live rows 72 and 81 and 90 (not by row0, whose Q the dead
            # rows 64..69 take), and the wave that holds S - 1 gets it through its own rows
            w0 = row0 // WAVE * WAVE
            plant_spikes(Q, K, u, Hq // Hkv, S, S, scale * LOG2E, torch.tensor([row0 + 2, row0 + 11, row0 + 20, S - 3]),
                         [(w0 + 2, 1.0), ((S - 1) // KVB * KVB + 1, 2.0)])
        else:
            twice = plant_causal(kind, Q, K, u, Hq // Hkv, S, scale * LOG2E, k_lo, None, row_min=row0) and kind == "spike"
        Q[:, :, :row0] = 0
        return dict(Q=Q, K=K, V=V, row0=row0, n=n, k_lo=k_lo, scale=scale, u=u, twice=twice), problem_causal(Q, K, V, S, scale, k_lo, None, row0=row0)
    return built_at(make, 1000 * row0 + n + dk + seed)


# ---- the vision towers (SEGMENT).  (H, S, dk, segments): one segment of five tiles at each width; frames; windows with boundaries inside tiles
WINDOWS = [64, 16, 16, 4, 48, 36, 48, 36]
VIT_CASES = [(2, 300, 64, [300]), (1, 300, 80, [300]), (1, 300, 128, [300]), (2, 268, 80, [100, 84, 84]), (2, 268, 80, WINDOWS)]


def build_vit(kind, H, S, dk, segs, seed=0, spare=None):
    """spike: in every segment of at least 48 rows, one key for a part of the segment's rows: 20 before the segment's end, which is past the
    segment's first tile; a long segment has it in its middle and a second, twice as strong, in its last tile.  ramp: 64 keys per step, or
    16 where no segment spans three tiles (windows: a 48-key window that crosses a tile edge then grows by RAMP, 2 RAMP or 3 RAMP there).
    spare: the index of a segment that gets no spike (the bit-identity test: its rows must not notice)"""
    scale = dk ** -0.5
    lo, hi = VR.segment_ranges(segs)

    def make(sd):
        Q, K, V = VR.attention_inputs(1, H, S, dk, seed=sd)
        u = directions((1, H, 1, Q.shape[-1]), dk, sd + 1)
        if kind == "ramp":
            plant_ramp(Q, K, u, 1, S, S, scale * LOG2E, KVB if max(segs) >= 128 else 16, RAMP)
        else:
            rows, keys, start = [], [], 0
            for si, n in enumerate(segs):
                if n >= 48 and si != spare:
                    rows.append(subset(torch.arange(start, start + n)))
                    if kind == "last":
                        keys.append((start + n - 1, 1.0))
                    elif n >= 200:
                        keys += [(start + n // 2, 1.0), (start + n - 3, 2.0)]
                    else:
                        keys.append((start + n - 20, 1.0))
                start += n
            plant_spikes(Q, K, u, 1, S, S, scale * LOG2E, torch.cat(rows), keys)
        return dict(Q=Q, K=K, V=V, S=S, dk=dk, lo=[lo], hi=[hi], scale=scale, u=u, twice=kind == "spike" and max(segs) >= 200), \
            problem_segment(Q, K, V, S, dk, scale, [lo], [hi])
    return built_at(make, 1000 * S + dk + H + len(segs) + seed)


# ---- the resampler.  (H, NQ, L, Lpad, n_keys, part): NP = 2 and NP = 4, the spike in each key part in turn, ragged n_keys
RESAMPLER_CASES = [(2, 64, 320, 320, [320], 0), (2, 64, 320, 320, [300], 1), (1, 33, 320, 320, [320], 1), (1, 64, 1024, 1024, [1000], 1),
                   (1, 8, 320, 320, [320], 0), (1, 8, 320, 320, [290], 1), (1, 8, 320, 320, [320], 2), (1, 8, 1024, 1024, [1001], 3)]


def build_resampler(kind, H, NQ, L, Lpad, counts, part, seed=0):
    scale, B = 128 ** -0.5, len(counts)
    NQpad = _ceil(NQ, WAVE)
    NP = 2 if NQ > 32 else 4
    nk = min(counts)

    def make(sd):
        twice = False
        g = torch.Generator().manual_seed(sd)
        Q = torch.full((H, NQpad, 128), float("nan"))
        Q[:, :NQ] = 1.5 * torch.randn((H, NQ, 128), generator=g)
        K, V = 1.5 * torch.randn((B, H, Lpad, 128), generator=g), torch.randn((B, H, Lpad, 128), generator=g)
        Q, K, V = Q.bfloat16(), K.bfloat16(), V.bfloat16()
        u = directions((H, 1, 128), 128, sd + 1)
        if kind == "ramp":     # a part's next block lies 128 keys on: RAMP per step inside a part, and the parts RAMP / NP apart for the merge
            plant_ramp(Q, K, u, 1, NQ, nk, scale * LOG2E, 128 // NP, RAMP / NP)
        else:
            blocks = resampler_parts(NQ, nk)[part]
            k0, k1 = blocks[-1] if kind == "last" else blocks[len(blocks) // 2]
            keys = [(min(k0 + 3, k1 - 1), 1.0)] + ([(blocks[-1][0], 2.0)] if kind == "spike" and len(blocks) > 2 else [])
            twice = len(keys) > 1
            plant_spikes(Q, K, u, 1, NQ, nk, scale * LOG2E, subset(torch.arange(NQ), (5, 17) if NQ > 8 else (5,)), keys)
        for b in range(B):     # what lies at and beyond a sample's key count is finite noise that no row may see
            K[b, :, counts[b]:], V[b, :, counts[b]:] = 100.0, -100.0
        return dict(Q=Q, K=K, V=V, counts=counts, NQ=NQ, L=L, Lpad=Lpad, scale=scale, u=u, twice=twice), problem_resampler(Q, K, V, counts, scale, NQ, L)
    return built_at(make, 1000 * L + 10 * NQ + H + part + seed)


# ---- decode.  (Hq, Hkv, dk, cap, k_lo, k_hi, chunk): the spike in the first, a middle and the last chunk of the range; ranges that cut chunks
DECODE_CASES = [(4, 2, 128, 768, [0], [768], 0), (14, 2, 64, 768, [5], [700], 1), (4, 2, 128, 768, [0], [768], 2), (16, 2, 128, 576, [200], [530], 2),
                (4, 2, 128, 576, [200], [530], 0)]


def build_decode(kind, Hq, Hkv, dk, cap, k_lo, k_hi, chunk, seed=0):
    scale, B = dk ** -0.5, len(k_lo)

    def make(sd):
        g = torch.Generator().manual_seed(sd)
        Qd = (1.5 * torch.randn((B, Hq, dk), generator=g)).bfloat16()
        K = (1.5 * torch.randn((B, Hkv, cap, dk), generator=g)).bfloat16()
        V = torch.randn((B, Hkv, cap, dk), generator=g).bfloat16()
        u = directions((B, Hkv, 1, dk), dk, sd + 1)
        Q4 = Qd[:, :, None, :].clone()      # [B, Hq, 1, dk]: one query row per head
        if kind == "ramp":
            plant_ramp(Q4, K, u, Hq // Hkv, 1, cap, scale * LOG2E, CHUNK, RAMP)
        else:               # every other head of a group is aligned, so that a group holds both kinds of row
            a = (STRENGTH / (scale * LOG2E)) ** 0.5
            uq = u.repeat_interleave(Hq // Hkv, dim=1)
            q, k = _without(Q4, uq, 1, 0.5), _without(K, u, cap)
            q[:, ::2] += a * uq[:, ::2]
            k[:, :, min(max(chunk * CHUNK + 77, k_lo[0]), k_hi[0] - 1)] += a * u[:, :, 0]
            Q4, K = q.bfloat16(), k.bfloat16()
        Qd = Q4[:, :, 0].contiguous()
        return dict(Qd=Qd, K=K, V=V, k_lo=k_lo, k_hi=k_hi, scale=scale, u=u), problem_decode(Qd, K, V, k_lo, k_hi, scale)
    return built_at(make, cap + Hq + 10 * chunk + seed)


# ---- SEGMENT with overlapping ranges: rows < 150 count the keys [0, 200), rows >= 150 the keys [40, 300).  The wave 128..159 holds rows of both,
# and tile 2 holds key 150, which both count.  With `spiked`, the rows >= 150 at 24 and 29 mod 32 (152 and 157 there) are aligned with that key; K is the same either way,
# so the rows < 150 -- their Q, their keys -- are the same problem in both and their result must be bit for bit the same
OVERLAP = (2, 300, 80, 150, (0, 200), (40, 300))


def build_vit_overlap(spiked, seed=0):
    H, S, dk, cut, ra, rb = OVERLAP
    scale = dk ** -0.5
    lo, hi = [ra[0]] * cut + [rb[0]] * (S - cut), [ra[1]] * cut + [rb[1]] * (S - cut)
    Q, K, V = VR.attention_inputs(1, H, S, dk, seed=4242 + seed)
    u = directions((1, H, 1, Q.shape[-1]), dk, 4243 + seed)
    rows = subset(torch.arange(cut, S), (24, 29)) if spiked else torch.zeros(0, dtype=torch.long)
    plant_spikes(Q, K, u, 1, S, S, scale * LOG2E, rows, [(cut, 1.0)])
    heads = problem_segment(Q, K, V, S, dk, scale, [lo], [hi])
    return dict(Q=Q, K=K, V=V, S=S, dk=dk, lo=[lo], hi=[hi], scale=scale, cut=cut), heads, coverage(heads)


# ---------------------------------------------------------------------------------------------------------------- every case of the GPU module
def _clip(kind, B, H, S, seed=0):
    return build_causal(kind, B, H, H, S, 64, None, None, seed)


ENTRIES = {   # entry point -> (builder, cases, kinds)
    "t5": (build_t5, T5_CASES, ("spike", "ramp", "last")),
    "clip": (_clip, CLIP_CASES, ("spike", "ramp", "last")),
    "qwen": (build_causal, QWEN_CASES, ("spike", "ramp", "last")),
    "extend": (build_ext, EXT_CASES, ("spike", "ramp", "last", "dead")),
    "vit": (build_vit, VIT_CASES, ("spike", "ramp", "last")),
    "resampler": (build_resampler, RESAMPLER_CASES, ("spike", "ramp", "last")),
    "decode": (build_decode, DECODE_CASES, ("spike", "ramp")),
}


def cases_of(entry):
    """[(kind, case)] and their test ids"""
    _, cases, kinds = ENTRIES[entry]
    pairs = [(k, c) for c in cases for k in kinds]
    return pairs, ["%s-%s" % (k, "_".join(str(v).replace(" ", "") for v in c)) for k, c in pairs]


def build(entry, kind, case):
    """-> (inputs (CPU tensors and the launch's parameters), heads, coverage)"""
    return ENTRIES[entry][0](kind, *case)


def out_shape(heads):
    """[B, H, stored rows, d] of the launch the heads belong to"""
    return (max(h.b for h in heads) + 1, max(h.h for h in heads) + 1, max(int(h.out_row[h.live].max()) for h in heads) + 1, heads[0].V.shape[1])
