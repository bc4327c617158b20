"""float64 references of the ControlNeXt backward launches (csrc/conv_bwd.hip: x2i_groupnorm_nhwc_bwd_bf16, x2i_linear_wgrad_f32,
x2i_conv_stem_wgrad_bf16, x2i_conv_wgrad_bf16; driven by x2i_amd/lightcontrol_train.py: ControlNeXtTrainer._backward_net) and the bounds their
outputs are held to, element by element.  No GPU-only code here: tests/test_cnx_bwd_ref_cpu.py proves the bounds on f32 stand-ins of the
kernels' arithmetic and shows which planted faults the old whole-tensor norms let through; tests/test_cnx_bwd_fp64_gpu.py holds the kernels to
them.  Built on tests/gemm_ref.py, tests/ew_ref.py, tests/conv_ref.py and tests/train_ref.py.

`want` is the exact float64 value of the operator on the operands the kernel read (bf16 / f32 -> float64 is exact); every allowance is an
operation count read off the code, times u = 2^-24 on the float64 magnitude sums.  A sum through any fixed tree whose longest path has k
additions carries at most k u sum|terms| (first order); S = GN_SLACK (1 + 2^-10) covers the second-order terms.  A = train_ref.reduce_depth
is the depth of x2i_reduce_rows_f32.

  GroupNorm backward (gn_bwd_stats_kernel, gn_bwd_dz_kernel, gn_bwd_finish_kernel, gn_bwd_dx_kernel, two reduce_rows).
    plan.   gn_plan restated (gn_bwd_plan): n = min(ceil(1024 / B), ceil(HW / 64)) chunks asked for, chunk = ceil(HW / n) pixels,
            nchunk = ceil(HW / chunk), rows = 256 / (C / 8) pixel rows per block, T = ceil(chunk / rows) pixels per thread.
    chain.  Every per-channel sum of a sample: T adds (fmas) in a thread, the block's `rows`-term sum (gn_block_store), reduce_rows over the
            chunks: Dc = T + rows + A(nchunk).  A group sum adds its cg = C / G channels: D = Dc + cg.
    stats.  S1 = sum z, S2 = sum z^2 (one pass), z = x + pre_add one f32 add: one more rounding in S1, two in S2 with a pre_add.
            E_m = (D1 + 2) u sum|z| / n and E_v = (D2 + 2) u Q + 2 |m| E_m + E_m^2 + u m^2 + u (Q + m^2), Q = var + m^2: the forms of
            conv_ref.gn_stat_errors with this chain (n~ = (float) HW cg and the division: the + 2).  E_r, r_hi from conv_ref.gn_rstd.  E_v
            carries the one-pass cancellation ~ kappa u: under large_mean or pre_add_dominant the bound is wide and says so (stat_share).
    xhat.   ((x + pa) - m~) r~: d(xhat) = S (|z - m| E_r + r_hi (E_m + u |z| [with a pre_add] + u |z - m|) + u |xhat|).
    lin.    fma(w, xhat, b): d(lin) = |w| d(xhat) + u |lin|.
    act'.   none: 1.  SiLU: s = 1 / (1 + expf(-lin)), s (1 + lin (1 - s)): |silu''| <= 1/2, so 1/2 d(lin), plus the f32 evaluation relative
            to the terms' magnitude s (1 + |lin|): U_ACT (expf 2 ulps, the add, the division, 1 - s, two products, the add: under 32 u) and
            ACT_TAIL (expf overflow) as train_ref.act_bwd_expect.  dz = dy act': one more rounding u |dz| (exact for none and ReLU).
            ReLU: the step.  An element with |lin| <= d(lin) is UNDECIDED: the kernel may take dz = 0 or dz = dy, both values of dx at that
            element are accepted, and sum |w dy| (1, |xhat| + d(xhat)) / n over a group's undecided elements joins E_A and E_Q (the
            corresponding sums join dw, db, dpre).  That is a cap, not a measurement: at most UNDECIDED_CAP = 1e-3 of a launch's elements
            may be undecided (check_gn_bwd fails beyond it), and the operands are chosen so that the reference alone stays inside it.
    A, Q.   A = mean_g(w dz), Q = mean_g(w dz xhat): the per-channel chains Dc, then the finish kernel's fma chain over cg channels, and
            a / n~: DA = Dc + cg + 2.  E_A = (S (DA u sum|w dz| + sum |w| d(dz)) + undecided) / n,
            E_Q = (S (DA u sum|w dz xhat| + sum |w| (d(dz) (|xhat| + d(xhat)) + |dz| d(xhat))) + undecided) / n.
    dx.     t = w dz - A - xhat Q: two products, two subtractions, each relative to at most |w dz| + |A| + |xhat Q|:
            d(t) = |w| d(dz) + E_A + |xhat| E_Q + d(xhat) (|Q| + E_Q) + 3 u (|w dz| + |A| + |xhat Q|);
            delta = S (r_hi d(t) + |t| E_r + E_r d(t)) + u |r t|; with dx_in one add: + u |want|; one bf16 rounding.
            Under in_relu an element with x <= 0 has allowance 0: it equals dx_in bit for bit, or is +0 without one.
    dpre.   The closed form r (w S0_c - HW A - Q sxh), sxh = (S1_c - HW m) r, S0_c = sum_p dz, S1_c = sum_p z of channel c:
            E_S0 = Dc u sum|dz| + sum d(dz) (+ undecided), E_S1 = (Dc + pre) u sum|z|,
            E_sxh = r_hi (E_S1 + HW E_m + u HW |m| + u |S1_c - HW m|) + |S1_c - HW m| E_r + u |sxh|  -- the cancellation of S1_c - HW m: the
            term u HW |m| |Q| r of the result;  d(t') = |w| E_S0 + HW E_A + |Q| E_sxh + E_Q (|sxh| + E_sxh) + 3 u (|w S0| + HW |A| + |Q sxh|);
            delta = S (r_hi d(t') + |t'| E_r + E_r d(t')) + u |want|.  f32: bound = delta.
    dw, db. Per sample the chains Dc of sum dz xhat and sum dz (with the propagated d(dz), d(xhat) of every term and the undecided sums), then
            the B samples in order: B u sum; accumulating: + u |prev + sum|.  f32: bound = delta.
  linear_wgrad.  dw[n][k] = sum_b dy[b][n] act(x[b][k]): a B-term fma chain behind s = 0, (B + 1) u sum_b |dy act(x)|; SiLU x / (1 + expf(-x))
    per term: U_ACT |dy silu(x)| + ACT_TAIL |dy x|; accumulating + u |prev + sum|.  db[n] = sum_b dy: B u sum|dy| (+ u |prev + sum|).
  conv_stem_wgrad.  stem_plan restated (stem_plan): nblk blocks of chunk output pixels; a thread chains ceil(chunk / 4) fmas, 3 adds join the
    four `sub` partials, reduce_rows over nblk, one more add when accumulating: (ceil(chunk / 4) + 3 + A(nblk)) u sum|x dy| (+ u |want|);
    db the same chain on sum|dy|.  OH = (H + 1) / 2: an odd H's last output row reads one real input row and the padding.
  conv_wgrad.  (32 + steps + nsplit) u sum|x dy| + u |want| (wgrad_bound): the 32 products of an MFMA step, the steps of a split, the
    splits -- moved here unchanged from tests/test_controlnext_train_gpu.py.  `tagged` operands (wgrad_operands): conv_ref.conv_tags' powers
    of two on x, a per-pixel, per-64-channel, per-sample power of two on dy (dy_tags).

Largest share of the allowance used on MI355X (tests/test_cnx_bwd_fp64_gpu.py, profiles/cnx_bwd_fp64_gputest.log): see MEASURED."""
import math

import torch

from tests.conv_ref import GN_SLACK, conv_tags, gn_rstd, gn_stats, where_gn
from tests.gemm_ref import (ACT_NONE, ACT_RELU, ACT_SILU, ACT_TAIL, U_ACT, U_F32, Report, _round_bound, act_f64, dact_f64, ulp_bf16)
from tests.train_ref import reduce_depth

u = U_F32
UNDECIDED_CAP = 1e-3
MIN_RELU_BIAS = 0.125           # |b| >= 1/8 where ReLU meets the `const` kind: a constant group has lin = b exactly

# the whole-tensor assertions of tests/test_controlnext_train_gpu.py, kept here only to show what they miss (tests/test_cnx_bwd_ref_cpu.py)
OLD_GN_DX_REL_L2 = 6e-3
OLD_GN_DWDB_REL_L2 = 1e-4
OLD_GN_DPRE_SCALE = 1e-4
OLD_STEM_DB_RTOL, OLD_STEM_DB_ATOL = 1e-5, 1e-3

# MEASURED (MI355X, tests/test_cnx_bwd_fp64_gpu.py, profiles/cnx_bwd_fp64_gputest.log): worst share of the allowance per kernel and output
# over every case and operand kind (dx: (|err| - rounding part)+ / delta; the f32 outputs: |err| / bound).  No count had to be changed and no
# kernel was outside its bound.  groupnorm_bwd dx peaks on pre_add_dominant (0.230; random 0.026, outlier 0.096, const 0.037, large_mean
# 0.015).  linear_wgrad at B = 2 is a two-term chain whose last rounding (u |prev + sum| when accumulating) is most of the allowance, as
# train_ref's skinny_bwd.  The f32 stand-ins of tests/test_cnx_bwd_ref_cpu.py: groupnorm_bwd dx 0.066, dw 0.372, db 0.120, dpre 0.011;
# linear_wgrad 0.940; conv_stem_wgrad 0.325.  The statistics' part of the dx allowance in half an output ulp (median over a launch's elements,
# largest over the launches): random 0.37, outlier 0.52, and from 1e3 up on large_mean, const and pre_add_dominant with one channel per
# group: there the one-pass variance leaves the bound wide, and the check is of finiteness, the mask, the sentinels and the other kinds.
MEASURED = {"groupnorm_bwd dx": 0.230, "groupnorm_bwd dw": 0.049, "groupnorm_bwd db": 0.017, "groupnorm_bwd dpre": 0.010,
            "linear_wgrad dw": 0.849, "linear_wgrad db": 0.680, "conv_stem_wgrad dw": 0.317, "conv_stem_wgrad db": 0.020,
            "conv_wgrad dw": 0.137, "conv_wgrad db": 0.027, "dgrad_2x2s2 gemm": 0.021}


def old_stem_gamma(P):
    """the allowance of test_conv_stem_wgrad_against_float64, in units of u"""
    return P / 1024 / 4 + 1024 + 8


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- plans
def gn_bwd_plan(B, HW, C, G):
    """gn_plan of csrc/conv_bwd.hip: dict chunk, nchunk, rows, T (pixels per thread), Dc, ws (x2i_groupnorm_bwd_workspace_floats)"""
    assert C % 8 == 0 and C % G == 0 and 256 % (C // 8) == 0 and C <= 1024, (C, G)
    rows = 256 // (C // 8)
    n = max(1, min(-(-1024 // B), -(-HW // 64)))
    chunk = -(-HW // n)
    nchunk = -(-HW // chunk)
    T = -(-chunk // rows)
    return dict(chunk=chunk, nchunk=nchunk, rows=rows, T=T, Dc=T + rows + reduce_depth(nchunk), ws=B * nchunk * 2 * C + 4 * B * C + 4 * B * G)


def stem_plan(B, H, W, Cout):
    """stem_plan of csrc/conv_bwd.hip: dict OH, OW, P, chunk, nblk, depth, ws (x2i_conv_stem_wgrad_workspace_floats)"""
    OH, OW = (H + 1) // 2, (W + 1) // 2
    P = B * OH * OW
    n = max(1, min(1024, -(-P // 256)))
    chunk = -(-P // n)
    nblk = -(-P // chunk)
    return dict(OH=OH, OW=OW, P=P, chunk=chunk, nblk=nblk, depth=-(-chunk // 4) + 3 + reduce_depth(nblk), ws=nblk * Cout * 28)


def _wgrad_bound_terms(B, OH, OW, Cin, Cout, k):
    """Accumulation length of x2i_conv_wgrad_bf16 per output element: the 32-product MFMA steps of one split, then the splits' partials."""
    from x2i_amd import ops
    n = ops.conv_wgrad_workspace_floats(B, OH, OW, Cin, Cout, k, k)
    nsplit = n // (Cout * Cin * k * k + Cout)
    steps = math.ceil(math.ceil(B * OH * OW / 32) / nsplit)
    return steps, nsplit


def wgrad_bound(want, absum, steps, nsplit):
    return (32 + steps + nsplit) * u * absum + u * want.abs() + 1e-30


# ---------------------------------------------------------------------------------------------------------------- GroupNorm backward
def gn_bwd_stat_errors(st, D, has_pre_add):
    """(E_m, E_v) [G]: conv_ref.gn_stat_errors with the backward's own chain D"""
    d1, d2 = D + (1 if has_pre_add else 0), D + (2 if has_pre_add else 0)
    m, var = st["mean"], st["var"]
    Q = var + m * m
    e_m = (d1 + 2) * u * st["absmean"]
    e_v = (d2 + 2) * u * Q + 2 * m.abs() * e_m + e_m * e_m + u * m * m + u * (Q + m * m)
    return e_m, e_v


def _gn_bwd_item(x, dy, w, b, pa, G, eps, act, pl):
    """one sample: x, dy bf16 [HW, C], pa f32 [C] or None -> dict of float64 tensors (module docstring)"""
    HW, C = x.shape
    cg = C // G
    n = HW * cg
    has_pre = pa is not None
    st = gn_stats(x, pa, G)
    Dc = pl["Dc"]
    e_m, e_v = gn_bwd_stat_errors(st, Dc + cg, has_pre)
    r, r_hi, e_r = gn_rstd(st["var"], e_v, eps)
    ch = lambda t: t.repeat_interleave(cg)
    grp = lambda t: t.reshape(HW, G, cg).sum((0, 2))
    m, r, r_hi, e_r, e_m = ch(st["mean"]), ch(r), ch(r_hi), ch(e_r), ch(e_m)
    wd, bd, g = w.double(), b.double(), dy.double()
    z = x.double() + (pa.double() if has_pre else 0.0)
    zc = z - m
    xh = zc * r
    axh = xh.abs()
    d_xh = GN_SLACK * (zc.abs() * e_r + r_hi * (e_m + (u * z.abs() if has_pre else 0.0) + u * zc.abs()) + u * axh)
    lin = wd * xh + bd
    d_lin = wd.abs() * d_xh + u * lin.abs()
    und = torch.zeros_like(lin, dtype=torch.bool)
    if act == ACT_NONE:
        fac, d_dz = torch.ones_like(lin), torch.zeros_like(lin)
    elif act == ACT_RELU:
        fac, d_dz = (lin > 0).double(), torch.zeros_like(lin)
        und = (lin.abs() <= d_lin) & (g != 0)
    else:
        assert act == ACT_SILU, act
        fac = dact_f64(lin, ACT_SILU)
        d_fac = GN_SLACK * 0.5 * d_lin + (U_ACT * torch.sigmoid(lin) + ACT_TAIL) * (1.0 + lin.abs())
        d_dz = g.abs() * d_fac + u * (g * fac).abs()
    dz = g * fac
    dz_alt = torch.where(und, g * (1.0 - fac), dz)
    wdz = wd * dz
    uw = torch.where(und, (wd * g).abs(), torch.zeros_like(lin))          # what an undecided element may move a group sum by
    ug = torch.where(und, g.abs(), torch.zeros_like(lin))
    DA = Dc + cg + 2
    A = grp(wdz) / n
    e_A = (GN_SLACK * (DA * u * grp(wdz.abs()) + grp(wd.abs() * d_dz)) + grp(uw)) / n
    p_dzxh = d_dz * (axh + d_xh) + dz.abs() * d_xh                        # error of one term dz xhat
    Q = grp(wdz * xh) / n
    e_Q = (GN_SLACK * (DA * u * grp((wdz * xh).abs()) + grp(wd.abs() * p_dzxh)) + grp(uw * (axh + d_xh))) / n
    Ac, Qc, e_Ac, e_Qc = ch(A), ch(Q), ch(e_A), ch(e_Q)
    mag = wdz.abs() + Ac.abs() + (xh * Qc).abs()
    t = wdz - Ac - xh * Qc
    d_t = wd.abs() * d_dz + e_Ac + axh * e_Qc + d_xh * (Qc.abs() + e_Qc) + 3 * u * mag
    dx = r * t
    d_dx = GN_SLACK * (r_hi * d_t + t.abs() * e_r + e_r * d_t) + u * dx.abs()
    dx_alt = r * (wd * dz_alt - Ac - xh * Qc)
    stat = t.abs() * e_r + r_hi * (Qc.abs() * (zc.abs() * e_r + r_hi * e_m) + e_Ac + axh * e_Qc)
    # per-channel sums of this sample
    S0, S1dz = dz.sum(0), (dz * xh).sum(0)
    e_S0 = Dc * u * dz.abs().sum(0) + d_dz.sum(0) + ug.sum(0)
    e_S1dz = Dc * u * (dz * xh).abs().sum(0) + p_dzxh.sum(0) + (ug * (axh + d_xh)).sum(0)
    out = dict(dx=dx, d_dx=d_dx, dx_alt=dx_alt, und=und, stat=stat, S0=S0, S1dz=S1dz, e_S0=e_S0, e_S1dz=e_S1dz, kappa=st["kappa"])
    if has_pre:
        S1 = z.sum(0)
        e_S1 = (Dc + 1) * u * z.abs().sum(0)
        dif = S1 - HW * m
        sxh = dif * r
        e_sxh = r_hi * (e_S1 + HW * e_m + u * HW * m.abs() + u * dif.abs()) + dif.abs() * e_r + u * sxh.abs()
        mag2 = (wd * S0).abs() + HW * Ac.abs() + (Qc * sxh).abs()
        t2 = wd * S0 - HW * Ac - Qc * sxh
        d_t2 = wd.abs() * e_S0 + HW * e_Ac + Qc.abs() * e_sxh + e_Qc * (sxh.abs() + e_sxh) + 3 * u * mag2
        out["dpre"] = r * t2
        out["d_dpre"] = GN_SLACK * (r_hi * d_t2 + t2.abs() * e_r + e_r * d_t2) + u * out["dpre"].abs()
    return out


def gn_bwd_expect(x, dy, w, b, G, eps, *, act=ACT_NONE, pre_add=None, dx_in=None, in_relu=False, prev_dw=None, prev_db=None, with_dw=True):
    """x2i_groupnorm_nhwc_bwd_bf16 on x, dy (dx_in) bf16 [B, HW, C], w, b bf16 [C], pre_add f32 [B, C]: dict
    dx (want, alt, bound, delta, exact) [B, HW, C] -- alt: the other accepted value of an undecided element (= want elsewhere), exact: the
    elements that must equal dx_in (or +0) bit for bit; dw, db (want, bound) [C] (prev_*: the contents before an accumulating launch);
    dpre (want, bound) [B, C] with a pre_add; undecided (count), stat_share (median over the elements of the statistics' part of the
    allowance over half an output ulp), kappa (largest finite)."""
    B, HW, C = x.shape
    pl = gn_bwd_plan(B, HW, C, G)
    items = [_gn_bwd_item(x[z], dy[z], w, b, None if pre_add is None else pre_add[z], G, eps, act, pl) for z in range(B)]
    st = lambda k: torch.stack([it[k] for it in items])
    want, alt, delta, und = st("dx"), st("dx_alt"), st("d_dx"), st("und")
    exact = torch.zeros_like(und)
    if in_relu:
        exact = ~(x.double() > 0)
        zero = torch.zeros_like(want)
        want, alt, delta = torch.where(exact, zero, want), torch.where(exact, zero, alt), torch.where(exact, zero, delta)
    half_ulp = 0.5 * ulp_bf16(want + (dx_in.double() if dx_in is not None else 0.0))
    live = ~exact
    share = (st("stat") / half_ulp)[live]
    if dx_in is not None:
        want, alt = want + dx_in.double(), alt + dx_in.double()
        delta = torch.where(exact, delta, delta + u * torch.maximum(want.abs(), alt.abs()))
    out = dict(dx=(want, alt, _round_bound(want, delta, False), delta, exact), undecided=int(und.sum()), numel=und.numel(),
               stat_share=float(share.median()) if share.numel() else 0.0)
    k = st("kappa")
    out["kappa"] = float(k[torch.isfinite(k)].max()) if bool(torch.isfinite(k).any()) else 0.0
    if with_dw:
        for name, key, ekey, prev in (("dw", "S1dz", "e_S1dz", prev_dw), ("db", "S0", "e_S0", prev_db)):
            s = st(key)
            wv = s.sum(0)
            d = st(ekey).sum(0) + B * u * (s.abs() + st(ekey)).sum(0)
            if prev is not None:
                wv = wv + prev.double()
                d = d + u * wv.abs()
            out[name] = (wv, d)
    if pre_add is not None:
        out["dpre"] = (st("dpre"), st("d_dpre"))
    return out


def _where_vec(C, G, name):
    cg = C // G

    def where(i):
        return f"{name}: sample {i // C}, channel {i % C}, group {(i % C) // cg}"
    return where


def check_vec(name, got, want, bound, where):
    """f32 entries against want / bound (any shape, flattened): raises naming the worst entry through where(flat index); returns the worst
    |err| / bound (an entry with bound 0 must be exact; NaN fails)."""
    g = got.to(device=want.device, dtype=torch.float64).reshape(-1)
    w_, b_ = want.reshape(-1), bound.reshape(-1)
    err = (g - w_).abs()
    bad = ~(err <= b_)
    share = torch.where(b_ > 0, err / b_, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    share = torch.where(torch.isfinite(share), share, torch.full_like(share, math.inf))
    if bool(bad.any()):
        i = int(torch.nonzero(bad & (share == share[bad].max()))[0])
        raise AssertionError(f"{name}: {int(bad.sum())} entries over the bound; worst {where(i)}: got {float(g[i]):.9g} want {float(w_[i]):.9g} "
                             f"bound {float(b_[i]):.3e} (|err| / bound {float(share[i]):.3g})")
    return float(share.max()) if share.numel() else 0.0


def check_gn_bwd(name, exp, dx, G, *, dx_in=None, dw=None, db=None, dpre=None, W=None):
    """Hold one launch's outputs to gn_bwd_expect's dict `exp`: dx bf16 [B, HW, C] element by element (the message names the sample, pixel,
    channel and group), the exact elements bit for bit, dw / db / dpre entry by entry; the undecided cap.  Returns {output: worst share}."""
    want, alt, bound, delta, exact = exp["dx"]
    B, HW, C = want.shape
    cg = C // G
    if exp["undecided"] > UNDECIDED_CAP * exp["numel"]:
        raise AssertionError(f"{name}: {exp['undecided']} of {exp['numel']} elements undecided under ReLU (cap {UNDECIDED_CAP:g}): "
                             "the operands do not suit this case")
    if bool(exact.any()):
        ref = dx_in if dx_in is not None else torch.zeros_like(dx)
        same = (dx.view(torch.int16) == ref.to(dx.device).view(torch.int16)) | ~exact.to(dx.device)
        if dx_in is not None:                                             # (0 + -0 is +0)
            same |= (dx == 0) & (ref.to(dx.device) == 0) & (dx.view(torch.int16) == 0)
        if not bool(same.all()):
            z, p, c = (int(v) for v in torch.nonzero(~same)[0])
            raise AssertionError(f"{name}: dx where x <= 0 under in_relu must be {'dx_in' if dx_in is not None else '+0'} bit for bit: "
                                 f"{where_gn(W, cg, z)(p, c)}: got {float(dx[z, p, c])!r}, {int((~same).sum())} elements")
    rep = Report(name + " dx")
    g64 = dx.to(device=want.device, dtype=torch.float64)
    sel = torch.where((g64 - alt).abs() < (g64 - want).abs(), alt, want)
    for z in range(B):
        rep.check(dx[z], sel[z], bound[z], delta[z], item=z, where=where_gn(W, cg, z))
    shares = dict(dx=rep.done())
    for key, got in (("dw", dw), ("db", db), ("dpre", dpre)):
        if got is not None:
            shares[key] = check_vec(f"{name} {key}", got, exp[key][0], exp[key][1], _where_vec(C, G, key))
    return shares


def gn_bwd_affine(C, gen, device="cpu", relu_const=False):
    """conv_ref.gn_affine's (w, b) bf16 [C].  relu_const (the ReLU cases): 1/8 <= |b| <= 0.275 and 0.75 <= w <= 1.25.  A constant group has
    lin = b exactly (const); the large_mean kind has xhat in {0, +-1.22} with d(xhat) up to 0.77 (0.63 |xhat|) at kappa = 24577 and the
    chain of 108 additions of the trainer's embedding norms (2 x 4096 x 128, G = 2), so the step stays decided where |b| < 0.45 w."""
    w = 1.0 + 0.2 * torch.randn(C, device=device, generator=gen)
    b = 0.3 * torch.randn(C, device=device, generator=gen)
    if relu_const:
        w = w.clamp(0.75, 1.25)
        b = torch.where(b < 0, -1.0, 1.0) * (MIN_RELU_BIAS + 0.15 * torch.rand(C, device=device, generator=gen))
    return w.to(torch.bfloat16), b.to(torch.bfloat16)


def dy_tagged(B, HW, C, gen, device="cpu"):
    """`tagged` dy bf16 [B, HW, C]: N(0, 1) times a power of two that differs between neighbouring pixels, 8-channel pieces and samples"""
    ar = lambda n: torch.arange(n, device=device)
    e = (ar(B) % 3 - 1)[:, None, None] + (ar(HW) * 3 % 7 - 3)[None, :, None] + (ar(C // 8) * 2 % 5 - 2).repeat_interleave(8)[None, None, :]
    return (torch.randn((B, HW, C), device=device, generator=gen) * torch.exp2(e.float())).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- linear_wgrad
def linear_wgrad_expect(dy, x, act_in=ACT_NONE, prev_w=None, prev_b=None):
    """x2i_linear_wgrad_f32 on dy f32 [B, N], x f32 [B, K]: ((want, bound) of dw [N, K], (want, bound) of db [N])"""
    B = dy.shape[0]
    g, a = dy.double(), act_f64(x.double(), act_in)
    want, mag = g.T @ a, g.abs().T @ a.abs()
    d = (B + 1) * u * mag
    if act_in == ACT_SILU:
        d = d + U_ACT * mag + ACT_TAIL * (g.abs().T @ x.double().abs())
    wb, db_ = g.sum(0), B * u * g.abs().sum(0)
    if prev_w is not None:
        want = want + prev_w.double()
        d = d + u * want.abs()
    if prev_b is not None:
        wb = wb + prev_b.double()
        db_ = db_ + u * wb.abs()
    return (want, d), (wb, db_)


def where_linear(K):
    return lambda i: f"dw[n={i // K}][k={i % K}] (output feature {i // K}, input feature {i % K})"


# ---------------------------------------------------------------------------------------------------------------- conv_stem_wgrad
def stem_wgrad_expect(x, dy, prev_w=None, prev_b=None):
    """x2i_conv_stem_wgrad_bf16 on x bf16 [B, H, W, 3], dy bf16 [B, OH, OW, Cout] (NHWC): ((want, bound) of dw [Cout, 3, 3, 3], of db [Cout])"""
    B, H, W, _ = x.shape
    Cout = dy.shape[-1]
    pl = stem_plan(B, H, W, Cout)
    assert tuple(dy.shape[1:3]) == (pl["OH"], pl["OW"]), (tuple(dy.shape), pl)
    xn, gn = x.cpu().double().permute(0, 3, 1, 2), dy.cpu().double().permute(0, 3, 1, 2)       # (float64 convolutions: on the host, as the old test)
    want = torch.nn.grad.conv2d_weight(xn, (Cout, 3, 3, 3), gn, stride=2, padding=1)
    mag = torch.nn.grad.conv2d_weight(xn.abs(), (Cout, 3, 3, 3), gn.abs(), stride=2, padding=1)
    d = pl["depth"] * u * mag
    wb, db_ = gn.sum((0, 2, 3)), pl["depth"] * u * gn.abs().sum((0, 2, 3))
    if prev_w is not None:
        want = want + prev_w.cpu().double()
        d = d + u * want.abs()
    if prev_b is not None:
        wb = wb + prev_b.cpu().double()
        db_ = db_ + u * wb.abs()
    return (want, d), (wb, db_)


def where_wgrad(Cin, KH, KW):
    def where(i):
        co, rest = divmod(i, Cin * KH * KW)
        ci, tap = divmod(rest, KH * KW)
        return f"dw[co={co}][ci={ci}][ky={tap // KW}][kx={tap % KW}]"
    return where


def dy_tags(B, OH, OW, Cout, device="cpu"):
    """`tagged` scales of a weight gradient's dy [B, OH, OW, Cout]: a power of two per output row, column, 64-channel slice and sample"""
    ar = lambda n: torch.arange(n, device=device)
    e = (ar(B) * 2 % 3 - 1)[:, None, None, None] + (ar(OH) * 3 % 5 - 2)[None, :, None, None] + (ar(OW) * 2 % 7 - 3)[None, None, :, None] + \
        (ar((Cout + 63) // 64) % 3 - 1).repeat_interleave(64)[:Cout][None, None, None, :]
    return torch.exp2(e.double())


def wgrad_operands(kind, B, H, W, Cin, OH, OW, Cout, KH, KW, gen, device="cpu"):
    """(x bf16 [B, H, W, Cin], dy bf16 [B, OH, OW, Cout]): `random` N(0, 1), or `tagged`: random times conv_tags (x) and dy_tags (dy), so a
    tap, channel tile, split or sample read twice, missed or taken from the neighbour moves the receiving element by a visible multiple"""
    x = torch.randn((B, H, W, Cin), device=device, generator=gen)
    dy = torch.randn((B, OH, OW, Cout), device=device, generator=gen)
    if kind == "tagged":
        x = x * conv_tags(B, H, W, Cin, KH, KW, device)[0].float()
        dy = dy * dy_tags(B, OH, OW, Cout, device).float()
    else:
        assert kind == "random", kind
    return x.to(torch.bfloat16), dy.to(torch.bfloat16)


def conv_wgrad_expect(x, dy, KH, KW, stride, pad, steps, nsplit, prev_w=None, prev_b=None):
    """x2i_conv_wgrad_bf16 on x bf16 [B, H, W, Cin], dy bf16 [B, OH, OW, Cout] (NHWC views): ((want, bound) of dw, of db), wgrad_bound"""
    Cin, Cout = x.shape[-1], dy.shape[-1]
    xn, gn = x.cpu().double().permute(0, 3, 1, 2), dy.cpu().double().permute(0, 3, 1, 2)
    want = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, KH, KW), gn, stride=stride, padding=pad)
    mag = torch.nn.grad.conv2d_weight(xn.abs(), (Cout, Cin, KH, KW), gn.abs(), stride=stride, padding=pad)
    wb, mb = gn.sum((0, 2, 3)), gn.abs().sum((0, 2, 3))
    dw_b, db_b = wgrad_bound(want, mag, steps, nsplit), wgrad_bound(wb, mb, steps, nsplit)
    if prev_w is not None:
        want = want + prev_w.cpu().double()
        dw_b = dw_b + u * want.abs()
    if prev_b is not None:
        wb = wb + prev_b.cpu().double()
        db_b = db_b + u * wb.abs()
    return (want, dw_b), (wb, db_b)


# ---------------------------------------------------------------------------------------------------------------- GroupNorm backward cases
# (B, HW, C, G): what each reaches is in tests/test_cnx_bwd_fp64_gpu.py
GN_BWD_SHAPES = [(2, 560, 64, 2), (2, 560, 128, 4), (2, 560, 256, 8), (1, 1, 8, 1), (3, 63, 8, 8), (3, 64, 8, 2), (3, 65, 8, 1),
                 (1, 130, 512, 32), (2, 70, 1024, 512), (2, 70, 1024, 1024), (1, 7300, 64, 2), (5, 300, 128, 8)]
# (C, G, eps, act, pre_add, in_relu): every combination ControlNeXtTrainer runs (tests/test_controlnext_train_gpu.py: GN_CASES)
TRAINER_GN_CASES = [(64, 2, 1e-5, ACT_RELU, False, False), (128, 2, 1e-5, ACT_RELU, False, False), (128, 4, 1e-6, ACT_SILU, False, False),
                    (128, 4, 1e-6, ACT_SILU, True, False), (128, 8, 1e-6, ACT_SILU, False, False), (256, 8, 1e-6, ACT_SILU, True, False),
                    (256, 8, 1e-5, ACT_NONE, False, False), (256, 8, 1e-5, ACT_NONE, False, True)]
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_SILU: "silu"}
# the ReLU launches of the recorded step (128 x 128 hint, B = 2: embedding.7, .4, .1), as tests/test_cnx_bwd_fp64_gpu.py replays them
RECORDED_RELU_CASES = [dict(shape=(2, 4096, C, 2), act=ACT_RELU, eps=1e-5, in_relu=False, pre=False, dx_in="none", dw="acc") for C in (128, 64)]
RELU_SHAPES = [(2, 560, 64, 2), (2, 560, 128, 4), (2, 560, 256, 8), (1, 130, 512, 32), (1, 7300, 64, 2), (5, 300, 128, 8)]


def gn_bwd_cases():
    """[dict shape, act, eps, in_relu, pre, dx_in ('none' / 'sep' / 'alias'), dw ('none' / 'plain' / 'acc')].  Per shape three cases, one
    per option (in_relu; pre_add + dpre; dx_in), the activation rotating with the shape so that every activation meets every option and
    every option every rows-per-block value; dx separate from dx_in and dx aliasing it once per shape; dw / db None, plain and accumulated
    onto random contents.  Then the trainer's eight combinations at its own geometry (accumulating, dx_in separate; norm1 of down_res.1
    aliases)."""
    cases = []
    for i, shape in enumerate(GN_BWD_SHAPES):
        # ReLU only where every operand kind leaves the step decided (the undecided cap): not at 256 rows per block, where the chain of
        # 279 additions at kappa = 24577 (large_mean) leaves no digit of the variance, nor at G >= 512, where the two off-constant elements
        # of every nearly constant group (const) are 3e-3 of the launch
        acts = (ACT_NONE, ACT_RELU, ACT_SILU) if shape in RELU_SHAPES else (ACT_NONE, ACT_SILU)
        for j, (in_relu, pre, dx_in, dw) in enumerate([(True, False, "none", "plain"), (False, True, "sep", "acc"), (False, False, "alias", "none")]):
            act = acts[(i + j) % len(acts)]
            cases.append(dict(shape=shape, act=act, eps=1e-6 if act == ACT_SILU else 1e-5, in_relu=in_relu, pre=pre, dx_in=dx_in, dw=dw))
    for k, (C, G, eps, act, pre, in_relu) in enumerate(TRAINER_GN_CASES):
        cases.append(dict(shape=(2, 560, C, G), act=act, eps=eps, in_relu=in_relu, pre=pre, dx_in="alias" if k == 2 else "sep", dw="acc"))
    return cases


def case_id(c):
    B, HW, C, G = c["shape"]
    return (f"{B}x{HW}x{C}g{G}-{ACT_NAME[c['act']]}" + ("-in_relu" if c["in_relu"] else "") + ("-pre" if c["pre"] else "") +
            f"-dxin_{c['dx_in']}-dw_{c['dw']}")


def gn_bwd_operands(c, kind, dy_kind, seed, device="cpu"):
    """dict x, dy, w, b, pre_add (None where the kind has none), dx_in, prev_dw, prev_db for case c on operand kind `kind` of
    conv_ref.GN_KINDS.  in_relu: x went through a ReLU (exact zeros).  ReLU cases draw |b| >= MIN_RELU_BIAS."""
    from tests.conv_ref import gn_input
    B, HW, C, G = c["shape"]
    gen = torch.Generator(device=device).manual_seed(seed)
    x, pa = gn_input(kind, B, HW, C, G, gen, device)
    if c["in_relu"]:
        x = torch.relu(x.float()).to(torch.bfloat16)
    w, b = gn_bwd_affine(C, gen, device, relu_const=c["act"] == ACT_RELU)
    rn = lambda *s: torch.randn(s, device=device, generator=gen)
    dy = dy_tagged(B, HW, C, gen, device) if dy_kind == "tagged" else rn(B, HW, C).to(torch.bfloat16)
    o = dict(x=x, dy=dy, w=w, b=b, pre_add=pa if c["pre"] else None, dx_in=None, prev_dw=None, prev_db=None)
    if c["dx_in"] != "none":
        o["dx_in"] = rn(B, HW, C).to(torch.bfloat16)
    if c["dw"] == "acc":
        o["prev_dw"], o["prev_db"] = 3.0 * rn(C), 3.0 * rn(C)
    return o


def gn_bwd_expect_case(c, o):
    return gn_bwd_expect(o["x"], o["dy"], o["w"], o["b"], c["shape"][3], c["eps"], act=c["act"], pre_add=o["pre_add"], dx_in=o["dx_in"],
                         in_relu=c["in_relu"], prev_dw=o["prev_dw"], prev_db=o["prev_db"], with_dw=c["dw"] != "none")
