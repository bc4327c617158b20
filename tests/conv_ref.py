"""float64 reference of the convolution and GroupNorm kernels (include/x2i.h: x2i_conv2d_nhwc_bf16 with x2i_conv_desc.moments,
x2i_conv3x3_narrow_bf16, x2i_conv3x3_image_bf16, x2i_conv_stem_bf16, x2i_groupnorm_nhwc*_bf16, x2i_groupnorm_moments_f32,
x2i_groupnorm_nhwc_from_moments*_bf16) and a per-element checker that names the launch, sample, output pixel, channel and group of a failure.
No GPU-only code here: the CPU tests of the checker (tests/test_conv_ref_cpu.py) import it too.  Built on tests/gemm_ref.py and tests/ew_ref.py.

`want` is the exact float64 value of the documented operator on the operands the kernel read (packed weights, stored moments, bf16
activations; bf16 / f32 -> float64 is exact).  u = U_F32 = 2^-24 below.

  Implicit-GEMM conv.  gather() builds the bf16 matrix A [rows, KH KW Cin] of a block of output rows of one batch item from the descriptor's
    DOCUMENTED meaning (virtual image = the input, nearest-upsampled along H (up = 1, 2) and W (up = 1); tap (ky, kx) of output pixel (oy, ox)
    sits at virtual (oy stride + ky - pad, ox stride + kx - pad_w); outside the virtual image: zero), then gemm_ref.gemm_expect: U_ACC sum|a w|
    holds for any order of the K sum.  bias2 joins the bias; ReLU is exact; the plain residual is one f32 add (gemm_expect's gate = 1 form).
  Epilogue moments.  Entry [z][c][0 / 1], c % 4 == 0: sum / sum of squares of the STORED bf16 outputs of channels c .. c + 3 over the item's M
    pixels; the other entries exactly 0 (with moments_accumulate: every entry plus its previous contents, the other three thus unchanged).
    The code sums in f32: a lane's rows of a row block through v_dot2c_f32_bf16 (exact products; two products and the running sum per
    instruction: 2 roundings allowed) -- RB / 16 rows x 2 instructions; the DPP row sum (4 levels); mom_block_sum over the row blocks (chain
    cnt / 4 + 3 per accumulator, 2 tree levels, groups - 1 through LDS), once (<= 128 row blocks) or twice (64 slabs, then the slabs); one
    more add when accumulating.  Any summation order has |err| <= depth u sum|terms| with depth the most additions a term passes through:
        bound(sum) = depth u sum|y| + u |prev|,   bound(sum of squares) = depth u sum y^2 + u |prev|          -- PER ENTRY.
    (+ 2^-126 per summed element: v_dot2c may flush a denormal operand.)
  Narrow / image / stem convs.  want, then sum|a w| (+ |bias|) times U_ACC (MFMA kernels, K = 9 Cin) or STEM_DEPTH u (the stem's f32 chain of
    27 products behind the bias: 27 additions + 1 for an unfused product), then one bf16 rounding.
  GroupNorm (gn_partial_kernel, gn_finish_kernel, gn_apply_kernel; ONE pass).  z = x + pre_add; n = HW cpg; S1 = sum z, S2 = sum z^2.
    chain.  A thread adds 4 channels of ceil(per / ppi) pixels (per = ceil(HW / 256) pixels per slab, ppi = 2048 / C pixels per iteration);
            then ppi threads' sums, cpg / 4 chunk halves, and in the finish 8 slabs per accumulator, 2 tree levels, 8 parts:
            D = 4 ceil(per / ppi) + ppi + cpg / 4 + 18.  With pre_add, z is a rounded f32 sum: one more rounding in S1, two in S2.
    mean.   m~ = S1~ / n~ (n~ = (float) HW (float) cpg: one rounding each):  E_m = (D1 + 2) u sum|z| / n.
    var.    v~ = max(S2~ / n~ - m~ m~, 0).  With Q = S2 / n = var + m^2 = kappa var:
            E_v = (D2 + 2) u Q + 2 |m| E_m + E_m^2 + u m^2 + u (Q + m^2)   -- the one-pass cancellation: E_v / var ~ 3 (D + 4) u kappa.
            The clamp cannot increase the error (var >= 0).  + eps: u (v + E_v + eps) more = E_v'.
    rstd.   r = 1 / sqrt(var + eps) (eps the f32 value).  With r_hi = 1 / sqrt(max(var - E_v', 0) + eps) >= r, r~:
            E_r = r_hi^3 E_v' / 2 + GN_RSQRT_ULPS u r_hi   (mean value theorem at the smallest argument; a constant group, var = 0, has
            r = 1 / sqrt(eps) and a finite bound: r_hi <= 1 / sqrt(eps))
    apply.  sc = r w; sh = fma(pre_add - m, sc, b); lin = fma(x, sc, sh):
            d = |w| (|z - m| E_r + E_m r_hi) + u (|x sc| + 2 |(pre_add - m) sc| + |sh| + |lin|),  times GN_SLACK for the second-order terms;
            act through gemm_ref._act_bound; post_add: + u |y + post| (one add); one bf16 rounding.
  x2i_groupnorm_moments_f32.  Per channel, f32 [B][C][2]: chain ceil(per / ppi) + ppi + 256 (the finish adds the 256 slabs one by one).
  From moments.  The moments are an OPERAND: a = sum_c (S1_c + HW v_c), q = sum_c (S2_c + 2 v_c S1_c + HW v_c^2) in float64 ARE the
    statistics (m = a / n, var = max(q / n - m^2, 0)).  f32: fma (1 rounding) for the first, 3 roundings for the second, a chain of cpg:
    E_m = (cpg + 3) u sum_c A_c / n, A_c = |S1_c| + HW |v_c|;  E_v = (cpg + 5) u sum_c Q_c / n + 2 |m| E_m + E_m^2 + u m^2 + u (|q / n| + m^2),
    Q_c = |S2_c| + 2 |v_c S1_c| + HW v_c^2 -- which carries the cancellation of the pre_add-dominant case.  rstd and apply as above.

Constants: every allowance below is an operation count read off the code; the f32 stand-ins of tests/test_conv_ref_cpu.py stay inside every
one of them (asserted there).  Largest share used on MI355X (tests/test_conv_fp64_gpu.py, profiles/conv_fp64_gputest.log; |err| beyond the
output's own rounding over the f32 allowance, or |err| / bound per moments entry), over every kernel form and the models' replayed launches:
U_ACC: conv outputs 0.14 (gemm256c in either K order, eight-wave 256^2), 0.17 (gemm512c in either K order, 128^2), narrow 0.02, image 0.07;
STEM_DEPTH 0.03; MOM_* per entry 0.11 (gemm256c, eight-wave), 0.09 (gemm512c), 0.12 (128^2), 0.03 (image conv); gn_moments_chain 0.20;
GN_* direct 0.03 - 0.07 per operand kind, from per-channel moments 0.08 - 0.18, from channel-quad moments 0.13 - 0.23.  None was changed."""
import math

import torch

from tests.ew_ref import f32
from tests.gemm_ref import (ACT_NONE, ACT_RELU, ACT_SILU, ROWS, U_ACC, U_F32, Report, _act_bound, _round_bound, act_f64, bf16_rne,
                            check_block, check_untouched, gemm_expect, poison_, sentinel_bits, tag_scales, ulp_bf16, write_mask)

__all__ = ["ACT_NONE", "ACT_RELU", "ACT_SILU", "Report", "bf16_rne", "check_block", "check_untouched", "poison_", "sentinel_bits", "tag_scales",
           "ulp_bf16", "write_mask", "ROWS"]

# conv outputs: gemm_ref.U_ACC (2^-20 sum|a w|)
# roundings per v_dot2c_f32_bf16 (two products + the accumulator)
MOM_DOT2_ROUNDINGS = 2
MOM_SLABS = 64                  # csrc/gemm.hip
MOM_DIRECT_BLOCKS = 128         # up to this many row blocks the finishing kernel adds them itself
MOM_FLUSH = 2.0 ** -126         # per summed element
# x2i_conv_stem_bf16: a = bias; a += w[k] * in[k], k = 0 .. 26
STEM_DEPTH = 28
# rsqrtf: 1 ulp on gfx950 (v_rsq_f32); 2 allowed (as ew_ref.LN_RSQRT_ULPS)
GN_RSQRT_ULPS = 2.0
# second-order terms of the GroupNorm apply bound
GN_SLACK = 1.0 + 2.0 ** -10
GN_SLABS = 256                  # csrc/controlnext.hip

# the old whole-tensor checks, kept here only to show what they miss (tests/test_conv_ref_cpu.py)
OLD_CONV_REL_L2 = 1e-2
OLD_GN_REL_L2 = 5e-3
OLD_MOM_MAXNORM = 2e-5


# ---------------------------------------------------------------------------------------------------------------- conv geometry
class Geom:
    """x2i_conv_desc as documented (include/x2i.h).  pad_w None: as pad; out_w / out_h None: computed."""

    def __init__(self, H, W, Cin, KH, KW, stride, pad, *, up=0, pad_w=None, out_w=None, out_h=None):
        self.H, self.W, self.Cin, self.KH, self.KW, self.stride, self.pad, self.up = H, W, Cin, KH, KW, stride, pad, int(up)
        self.pad_w = pad if pad_w is None else pad_w
        self.uh, self.uw = (2 if self.up else 1), (2 if self.up == 1 else 1)
        self.OH = (H * self.uh + 2 * pad - KH) // stride + 1 if not out_h else out_h
        self.OW = (W * self.uw + 2 * self.pad_w - KW) // stride + 1 if not out_w else out_w
        self.M, self.K = self.OH * self.OW, KH * KW * Cin


def gather(x, g, r0, r1):
    """A bf16 [r1 - r0, KH KW Cin] ((ky, kx, ci) order) of output rows r0 .. r1 - 1 (row = oy OW + ox) of ONE batch item x [H, W, Cin]"""
    dev = x.device
    m = torch.arange(r0, r1, device=dev)
    oy, ox = torch.div(m, g.OW, rounding_mode="floor"), m % g.OW
    vy = oy[:, None] * g.stride + torch.arange(g.KH, device=dev)[None, :] - g.pad          # [rows, KH], virtual (upsampled) coordinates
    vx = ox[:, None] * g.stride + torch.arange(g.KW, device=dev)[None, :] - g.pad_w        # [rows, KW]
    oky, okx = (vy >= 0) & (vy < g.H * g.uh), (vx >= 0) & (vx < g.W * g.uw)
    sy = torch.div(vy.clamp(0, g.H * g.uh - 1), g.uh, rounding_mode="floor")
    sx = torch.div(vx.clamp(0, g.W * g.uw - 1), g.uw, rounding_mode="floor")
    A = x[sy[:, :, None], sx[:, None, :]]                                                  # [rows, KH, KW, Cin]
    A = A * (oky[:, :, None] & okx[:, None, :])[..., None].to(A.dtype)
    return A.reshape(r1 - r0, g.K)


def strided(store, shape, stride, off):
    """view of the flat tensor `store` with `off` counted from ITS first element (as_strided counts from the storage's)"""
    return store.as_strided(shape, stride, store.storage_offset() + off)


def item_view(store, g, z, a_offset=0, a_batch_stride=None):
    """batch item z of the input as the descriptor addresses it: [H, W, Cin] at a_offset + z a_batch_stride of the flat storage"""
    bs = g.H * g.W * g.Cin if a_batch_stride is None else a_batch_stride
    return strided(store.view(-1), (g.H, g.W, g.Cin), (g.W * g.Cin, g.Cin, 1), a_offset + z * bs)


def out_geometry(g, N, B, *, c_offset=0, c_batch_stride=None, ldc=None, out_row_pitch=0):
    """(shape, stride, offset) of the launch's write set [B, OH, OW, N] in the flat output storage"""
    ldc = N if ldc is None else ldc
    pitch = out_row_pitch if out_row_pitch else g.OW * ldc
    cbs = g.OH * g.OW * N if c_batch_stride is None else c_batch_stride
    return (B, g.OH, g.OW, N), (cbs, pitch, ldc, 1), c_offset


def where_pixel(OW, z, what=""):
    return lambda m, n: f"{what}sample {z}, output pixel (oy={m // OW}, ox={m % OW}), channel {n} (row m={m})"


def check_conv(rep, x_store, w, bias, out_store, g, N, B, *, act=ACT_NONE, bias2=None, res_store=None, res_offset=0, res_batch_stride=None,
               ldr=None, w_group=0, a_offset=0, a_batch_stride=None, c_offset=0, c_batch_stride=None, ldc=None, out_row_pitch=0, rows=ROWS):
    """Every output element of one x2i_conv2d_nhwc_bf16 launch.  x_store / out_store / res_store: flat storages (res_store: as it was BEFORE
    the launch -- a clone when it aliases the output); w [N, K] or, grouped, [groups, N, K]; bias [N] / [groups, N] or None; bias2 f32 [B, N]."""
    shape, stride, off = out_geometry(g, N, B, c_offset=c_offset, c_batch_stride=c_batch_stride, ldc=ldc, out_row_pitch=out_row_pitch)
    out4 = strided(out_store.view(-1), shape, stride, off)
    ldr = N if ldr is None else ldr
    rbs = g.M * N if res_batch_stride is None else res_batch_stride
    for z in range(B):
        xz = item_view(x_store, g, z, a_offset, a_batch_stride)
        wz = w[z // w_group] if w_group else w
        bz = None if bias is None else (bias[z // w_group] if w_group else bias)
        got = out4[z].reshape(g.M, N)
        resz = None if res_store is None else strided(res_store.view(-1), (g.M, N), (ldr, 1), res_offset + z * rbs)
        for r0 in range(0, g.M, rows):
            r1 = min(g.M, r0 + rows)
            A = gather(xz, g, r0, r1)
            want, bound, d = gemm_expect(A, wz, bz, act=act, res=None if resz is None else resz[r0:r1],
                                         bias2=None if bias2 is None else bias2[z])
            rep.check(got[r0:r1], want, bound, d, item=z, row0=r0, where=where_pixel(g.OW, z))
            del A, want, bound, d
    return rep


# ---------------------------------------------------------------------------------------------------------------- epilogue moments
def reduce_depth(rows, N):
    """most additions a term passes through in mom_block_sum (csrc/gemm.hip) over `rows` rows of N / 2 floats"""
    lanes = max(1, N // 8)
    groups = max(1, 256 // lanes)
    cnt = (rows + groups - 1) // groups
    return cnt // 4 + 3 + 2 + (groups - 1)


def moments_depth(M, N, row_block=128, accumulate=False, lane_rows=None, blocks=None):
    """depth of the whole moments accumulation of a conv launch whose kernel writes one partial row per `row_block` output rows (64: the
    128^2 kernel; 128: the 256^2, persistent and 512 x 128 kernels)"""
    lane = MOM_DOT2_ROUNDINGS * 2 * (row_block // 16) if lane_rows is None else lane_rows
    blocks = ((M + 2 * row_block - 1) // (2 * row_block)) * 2 if blocks is None else blocks
    if blocks <= MOM_DIRECT_BLOCKS:
        red = reduce_depth(blocks, N)
    else:
        red = reduce_depth((blocks + MOM_SLABS - 1) // MOM_SLABS, N) + reduce_depth(MOM_SLABS, N)
    return lane + 4 + red + (1 if accumulate else 0)


def image_moments_depth(H, W, N):
    """x2i_conv3x3_image_bf16 (csrc/vae_encode.hip): a lane's quad (3 adds, fma chain) over at most min(H, 128) rows, the DPP row, 3 waves,
    then the convs' reduce kernels over at most 2 ceil(H W / 128) partial rows"""
    return moments_depth(H * W, N, lane_rows=4 + min(H, 128) + 3, blocks=(H * W + 127) // 128 * 2)


def moments_expect(Y, depth, prev=None, rows=65536):
    """Expected x2i_conv_desc.moments of the STORED outputs Y [B, M, N] (bf16 view): (want, bound) float64 [B, N, 2]; prev [B, N, 2] f32: the
    contents before a moments_accumulate launch."""
    B, M, N = Y.shape
    want = torch.zeros((B, N, 2), dtype=torch.float64, device=Y.device)
    bound = torch.zeros_like(want)
    for z in range(B):
        s1 = torch.zeros(N // 4, dtype=torch.float64, device=Y.device)
        s2, sa = torch.zeros_like(s1), torch.zeros_like(s1)
        for r0 in range(0, M, rows):
            q = Y[z, r0:r0 + rows].double().reshape(-1, N // 4, 4)
            s1 += q.sum((0, 2))
            s2 += (q * q).sum((0, 2))
            sa += q.abs().sum((0, 2))
        want[z, 0::4, 0], want[z, 0::4, 1] = s1, s2
        bound[z, 0::4, 0] = depth * U_F32 * sa + 4 * M * MOM_FLUSH
        bound[z, 0::4, 1] = depth * U_F32 * s2 + 4 * M * MOM_FLUSH
    if prev is not None:
        p = prev.double()
        pq = torch.zeros_like(p)
        pq[:, 0::4] = p[:, 0::4]
        bound = bound + U_F32 * pq.abs()
        want = want + p
    return want, bound


def check_entries(name, got, want, bound, names):
    """got vs want / bound [B, C, 2] (per-channel f32 results): (None or a message naming sample, channel and component, worst |err| / bound
    over the entries with a bound > 0; an entry with bound 0 must be exact)."""
    g = got.to(device=want.device, dtype=torch.float64)
    err = (g - want).abs()
    bad = ~(err <= bound)
    share = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    share = torch.where(torch.isfinite(share), share, torch.full_like(share, math.inf))
    worst = float(share.max()) if share.numel() else 0.0
    if not bool(bad.any()):
        return None, worst
    b, c, k = (int(v) for v in torch.nonzero(share == share.max())[0])
    return (f"{name}: {int(bad.sum())} entries over the bound; worst at sample {b}, channel {c}, {names[k]}: got {float(g[b, c, k]):.9g} want "
            f"{float(want[b, c, k]):.9g} bound {float(bound[b, c, k]):.3e} (|err| / bound {float(share[b, c, k]):.3g})"), worst


def assert_entries(name, got, want, bound, names=("sum", "sum of squares")):
    msg, worst = check_entries(name, got, want, bound, names)
    if msg:
        raise AssertionError(msg)
    return worst


# ---------------------------------------------------------------------------------------------------------------- the other convs
def small_conv_expect(A, W, bias, uacc):
    """want / bound / delta of out = bf16(A W^T + bias) with |f32 error| <= uacc (sum|a w| + |bias|); A [m, K], W [N, K] of any float type"""
    Ad, Wd = A.double(), W.double()
    lin, mag = Ad @ Wd.T, Ad.abs() @ Wd.abs().T
    if bias is not None:
        lin, mag = lin + bias.double(), mag + bias.double().abs()
    d = uacc * mag
    return lin, _round_bound(lin, d, False), d


def check_narrow(rep, x, w, bias, y, Cout, rows=ROWS):
    """x2i_conv3x3_narrow_bf16: x [B, H, W, Cin], w [Cout, 9 Cin], y [B, H, W, ldy] (after the launch, poisoned before): channels < Cout
    against float64, channels Cout .. 3 exactly +0, channels from 4 on still the sentinel."""
    B, H, W, Cin = x.shape
    g = Geom(H, W, Cin, 3, 3, 1, 1)
    for z in range(B):
        got = y[z].reshape(g.M, -1)
        for r0 in range(0, g.M, rows):
            r1 = min(g.M, r0 + rows)
            want, bound, d = small_conv_expect(gather(x[z], g, r0, r1), w, bias, U_ACC)
            rep.check(got[r0:r1, :Cout], want, bound, d, item=z, row0=r0, where=where_pixel(W, z))
        zb = got[:, Cout:4].contiguous().view(torch.int16)
        if not bool((zb == 0).all()):
            m, c = (int(v) for v in torch.nonzero(zb != 0)[0])
            raise AssertionError(f"{rep.name}: channel {Cout + c} of sample {z}, pixel (oy={m // W}, ox={m % W}) is not +0 "
                                 f"(bits {int(zb[m, c]) & 0xFFFF:#06x})")
        ok = sentinel_bits(got[:, 4:])
        if not bool(ok.all()):
            m, c = (int(v) for v in torch.nonzero(~ok)[0])
            raise AssertionError(f"{rep.name}: channel {4 + c} (behind the four the kernel owns) of sample {z}, pixel (oy={m // W}, ox={m % W}) written")
    return rep


def check_image(rep, x_nchw, w, bias, y, rows=ROWS):
    """x2i_conv3x3_image_bf16: x [B, Cin, H, W] NCHW, w [Cout, Cin, 3, 3] (the nn.Conv2d weight as it is), y [B, H, W, Cout]"""
    B, Cin, H, W = x_nchw.shape
    Cout = w.shape[0]
    g = Geom(H, W, Cin, 3, 3, 1, 1)
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    for z in range(B):
        xz = x_nchw[z].permute(1, 2, 0)
        got = y[z].reshape(g.M, Cout)
        for r0 in range(0, g.M, rows):
            r1 = min(g.M, r0 + rows)
            want, bound, d = small_conv_expect(gather(xz, g, r0, r1), wp, bias, U_ACC)
            rep.check(got[r0:r1], want, bound, d, item=z, row0=r0, where=where_pixel(W, z))
    return rep


def check_stem(rep, x, w, bias, y, rows=ROWS):
    """x2i_conv_stem_bf16: x [B, H, W, 3] bf16, w f32 [Cout, 3, 3, 3] (ky, kx, ci), bias f32 [Cout], y [B, H / 2, W / 2, Cout]"""
    B, H, W, _ = x.shape
    Cout = w.shape[0]
    g = Geom(H, W, 3, 3, 3, 2, 1)
    for z in range(B):
        got = y[z].reshape(g.M, Cout)
        for r0 in range(0, g.M, rows):
            r1 = min(g.M, r0 + rows)
            want, bound, d = small_conv_expect(gather(x[z], g, r0, r1), w.reshape(Cout, 27), bias, STEM_DEPTH * U_F32)
            rep.check(got[r0:r1], want, bound, d, item=z, row0=r0, where=where_pixel(g.OW, z))
    return rep


# ---------------------------------------------------------------------------------------------------------------- GroupNorm
def gn_chain(HW, C, G):
    """D of the docstring: the most additions an element passes through in the statistics of x2i_groupnorm_nhwc_bf16"""
    cpp = C // 8
    ppi = 256 // cpp
    per = (HW + GN_SLABS - 1) // GN_SLABS
    return 4 * ((per + ppi - 1) // ppi) + ppi + max(1, (C // G) // 4) + 18


def gn_moments_chain(HW, C):
    ppi = 256 // (C // 8)
    per = (HW + GN_SLABS - 1) // GN_SLABS
    return (per + ppi - 1) // ppi + ppi + GN_SLABS


def _group_sums(t, G):
    """[HW or 1, C] -> [G]: sum over pixels and the channels of each group"""
    return t.reshape(t.shape[0], G, -1).sum((0, 2))


def gn_stats(x, pre_add, G, rows=65536):
    """Two-pass float64 statistics of z = x + pre_add over the groups of ONE item x [HW, C] (bf16): dict of [G] tensors mean, var, absmean
    (sum|z| / n), kappa = (mean^2 + var) / var (inf for a constant group), n."""
    HW, C = x.shape
    n = HW * (C // G)
    pa = torch.zeros(C, dtype=torch.float64, device=x.device) if pre_add is None else pre_add.double()
    s = torch.zeros(G, dtype=torch.float64, device=x.device)
    sa = torch.zeros_like(s)
    for r0 in range(0, HW, rows):
        z = x[r0:r0 + rows].double() + pa
        s += _group_sums(z, G)
        sa += _group_sums(z.abs(), G)
    mean = s / n
    mc = mean.repeat_interleave(C // G)
    v = torch.zeros_like(s)
    for r0 in range(0, HW, rows):
        zc = x[r0:r0 + rows].double() + pa - mc
        v += _group_sums(zc * zc, G)
    var = v / n
    kappa = torch.where(var > 0, (mean * mean + var) / var.clamp_min(1e-300), torch.full_like(var, math.inf))
    return dict(mean=mean, var=var, absmean=sa / n, kappa=kappa, n=n)


def gn_stat_errors(st, HW, C, G, has_pre_add):
    """(E_m, E_v) [G] of the one-pass f32 statistics (docstring)"""
    D = gn_chain(HW, C, G)
    d1, d2 = D + (1 if has_pre_add else 0), D + (2 if has_pre_add else 0)
    m, var = st["mean"], st["var"]
    Q = var + m * m
    e_m = (d1 + 2) * U_F32 * st["absmean"]
    e_v = (d2 + 2) * U_F32 * Q + 2 * m.abs() * e_m + e_m * e_m + U_F32 * m * m + U_F32 * (Q + m * m)
    return e_m, e_v


def moments_stats(mom, pre_add, HW, G):
    """The statistics x2i_groupnorm_nhwc_from_moments_bf16 derives from the moments GIVEN (mom [C, 2] f32 of one item, per channel or per
    quad; pre_add [C] f32 or None), in float64, and the errors of their f32 evaluation: dict mean, var, kappa, e_m, e_v [G]."""
    C = mom.shape[0]
    cpg = C // G
    n = HW * cpg
    s1, s2 = mom[:, 0].double(), mom[:, 1].double()
    v = torch.zeros_like(s1) if pre_add is None else pre_add.double()
    cs1, cs2 = s1 + HW * v, s2 + 2 * v * s1 + HW * v * v
    A, Qc = s1.abs() + HW * v.abs(), s2.abs() + 2 * (v * s1).abs() + HW * v * v
    grp = lambda t: t.reshape(G, cpg).sum(1)
    a, q = grp(cs1), grp(cs2)
    m = a / n
    var = (q / n - m * m).clamp_min(0.0)
    e_m = (cpg + 3) * U_F32 * grp(A) / n
    e_v = (cpg + 5) * U_F32 * grp(Qc) / n + 2 * m.abs() * e_m + e_m * e_m + U_F32 * m * m + U_F32 * ((q / n).abs() + m * m)
    kappa = torch.where(var > 0, (m * m + var) / var.clamp_min(1e-300), torch.full_like(var, math.inf))
    return dict(mean=m, var=var, kappa=kappa, e_m=e_m, e_v=e_v, n=n)


def gn_rstd(var, e_v, eps):
    """(r, r_hi, E_r) [G]"""
    epsf = f32(eps)
    r = torch.rsqrt(var + epsf)
    e_v1 = e_v + U_F32 * (var + e_v + epsf)
    r_hi = torch.rsqrt((var - e_v1).clamp_min(0.0) + epsf)
    return r, r_hi, 0.5 * r_hi ** 3 * e_v1 + GN_RSQRT_ULPS * U_F32 * r_hi


def gn_apply_expect(x, pre_add, w, b, mean, var, e_m, e_v, eps, act, post, G):
    """(want, bound, delta) float64 [rows, C] of rows x [rows, C] (bf16) of one item, given its group statistics [G] and their errors"""
    C = x.shape[1]
    cpg = C // G
    r, r_hi, e_r = gn_rstd(var, e_v, eps)
    ch = lambda t: t.repeat_interleave(cpg)
    m, r, r_hi, e_r, e_mc = ch(mean), ch(r), ch(r_hi), ch(e_r), ch(e_m)
    pa = torch.zeros(C, dtype=torch.float64, device=x.device) if pre_add is None else pre_add.double()
    xd, wd, bd = x.double(), w.double(), b.double()
    sc = r * wd
    sh = (pa - m) * sc + bd
    lin = xd * sc + sh
    zc = (xd + pa - m).abs()
    d = wd.abs() * (zc * e_r + e_mc * r_hi) + U_F32 * ((xd * sc).abs() + 2 * ((pa - m) * sc).abs() + sh.abs() + lin.abs())
    d = GN_SLACK * d
    y = act_f64(lin, act)
    d = _act_bound(lin, y, d, act)
    if post is not None:
        y = y + post.double()
        d = d + U_F32 * y.abs()
    return y, _round_bound(y, d, False), d


def where_gn(W, cpg, z):
    def where(m, n):
        pix = f"pixel {m}" if not W else f"pixel (oy={m // W}, ox={m % W})"
        return f"sample {z}, {pix}, channel {n}, group {n // cpg}"
    return where


def check_groupnorm(rep, x, y, w, b, G, eps, *, act=ACT_NONE, pre_add=None, post=None, moments=None, w_group=0, W=None, rows=ROWS):
    """Every element of one GroupNorm launch: x / y / post [B, HW, C] (post as it was before the launch), w / b [C] or, grouped,
    [groups, C]; pre_add f32 [B, C]; moments f32 [B, C, 2]: the from-moments entry point (its statistics are the float64 function of them).
    Returns {"kappa": the largest finite kappa, "stat_share": the largest (statistics part of the bound) / (half an output ulp)}."""
    B, HW, C = x.shape
    cpg = C // G
    info = dict(kappa=0.0)
    for z in range(B):
        pa = None if pre_add is None else pre_add[z]
        if moments is None:
            st = gn_stats(x[z], pa, G)
            e_m, e_v = gn_stat_errors(st, HW, C, G, pa is not None)
        else:
            st = moments_stats(moments[z], pa, HW, G)
            e_m, e_v = st["e_m"], st["e_v"]
        k = st["kappa"]
        if bool(torch.isfinite(k).any()):
            info["kappa"] = max(info["kappa"], float(k[torch.isfinite(k)].max()))
        wz, bz = (w[z // w_group], b[z // w_group]) if w_group else (w, b)
        for r0 in range(0, HW, rows):
            r1 = min(HW, r0 + rows)
            want, bound, d = gn_apply_expect(x[z, r0:r1], pa, wz, bz, st["mean"], st["var"], e_m, e_v, eps, act,
                                             None if post is None else post[z, r0:r1], G)
            rep.check(y[z, r0:r1], want, bound, d, item=z, row0=r0, where=where_gn(W, cpg, z))
    return info


def gn_moments_expect(x, rows=65536):
    """x2i_groupnorm_moments_f32 of x [B, HW, C]: (want, bound) float64 [B, C, 2]"""
    B, HW, C = x.shape
    want = torch.zeros((B, C, 2), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(want)
    for z in range(B):
        for r0 in range(0, HW, rows):
            t = x[z, r0:r0 + rows].double()
            want[z, :, 0] += t.sum(0)
            want[z, :, 1] += (t * t).sum(0)
            mag[z, :, 0] += t.abs().sum(0)
            mag[z, :, 1] += (t * t).sum(0)
    return want, gn_moments_chain(HW, C) * U_F32 * mag


# ---------------------------------------------------------------------------------------------------------------- operands
CONV_KINDS = ("random", "cancel", "tagged")
GN_KINDS = ("random", "large_mean", "outlier", "const", "pre_add_dominant")
LARGE_MEAN_KAPPA = 24577.0      # kappa of every group of the large_mean kind: 1 + 2048^2 / (256 * 2 / 3) = 1 + 512^2 / (16 * 2 / 3) (gn_input)


def conv_tags(B, H, W, Cin, KH, KW, device="cpu"):
    """`tagged` scales: (input [B, H, W, Cin], weight taps [KH KW Cin]) powers of two that differ between neighbouring input rows, columns,
    64-channel slices, filter taps and batch items, so a tap, slice or item read twice, missed or taken from the neighbour changes the
    receiving element by a visible multiple of its share."""
    ar = lambda n: torch.arange(n, device=device)
    ey, ex = (ar(H) * 2 % 5 - 2).double(), (ar(W) * 3 % 7 - 3).double()
    es = (ar((Cin + 63) // 64) * 2 % 3 - 1).double().repeat_interleave(64)[:Cin]
    ez = (ar(B) % 3 - 1).double()
    xs = torch.exp2(ez[:, None, None, None] + ey[None, :, None, None] + ex[None, None, :, None] + es[None, None, None, :])
    et = (ar(KH * KW) * 4 % 9 - 4).double().repeat_interleave(Cin)
    return xs, torch.exp2(et)


def conv_operands(kind, B, H, W, Cin, N, KH, KW, gen, device="cpu", groups=0):
    """(x bf16 [B, H, W, Cin], w bf16 [N, K] or [groups, N, K], bias bf16 [N] or [groups, N]) of one kind:
    random   x ~ N(0, 1), w ~ N(0, 1 / K), bias ~ 0.5 N(0, 1)
    cancel   x ~ 4 + N(0, 1) and every weight row with zero mean over K: inside the image the mean cancels (|lin| << sum|a w|), at a padded
             border it does not -- a wrong padding tap shows as a multiple of the output
    tagged   random times conv_tags"""
    K = KH * KW * Cin
    rn = lambda *s: torch.randn(s, device=device, generator=gen)
    x = rn(B, H, W, Cin)
    wshape = (groups, N, K) if groups else (N, K)
    w = rn(*wshape) / math.sqrt(K)
    bias = 0.5 * rn(*wshape[:-1])
    if kind == "cancel":
        x = x + 4.0
        w = w - w.mean(-1, keepdim=True)
    elif kind == "tagged":
        xs, ws = conv_tags(B, H, W, Cin, KH, KW, device)
        x, w = x * xs.float(), w * ws.float()
    else:
        assert kind == "random", kind
    return x.to(torch.bfloat16), w.to(torch.bfloat16), bias.to(torch.bfloat16)


def gn_input(kind, B, HW, C, G, gen, device="cpu"):
    """(x bf16 [B, HW, C], pre_add f32 [B, C] or None) of one kind:
    random            N(0.5, 2^2), pre_add 0.5 N(0, 1)
    large_mean        values one bf16 ulp around a large mean: even groups 2048 + 16 {-1, 0, 1} (var = 512 / 3), odd groups 512 + 4 {-1, 0, 1}
                      (var = 32 / 3): kappa = LARGE_MEAN_KAPPA = 24577 in both; no pre_add
    outlier           N(0, 1) with one pixel per 512 at +-2^8 .. 2^10 in 4 channels; pre_add 0.5 N(0, 1)
    const             groups g % 3 == 0 constant, g % 3 == 1 constant but for two elements one bf16 ulp off, the others random; no pre_add
    pre_add_dominant  x ~ N(0, 1), pre_add = +-(256 .. 1024): |v| >> |x|, the cancelling case of the moments form"""
    rn = lambda *s: torch.randn(s, device=device, generator=gen)
    cpg = C // G
    if kind == "random":
        return (0.5 + 2.0 * rn(B, HW, C)).to(torch.bfloat16), 0.5 * rn(B, C)
    if kind == "large_mean":
        t = torch.randint(-1, 2, (B, HW, C), device=device, generator=gen).float()
        grp = (torch.arange(C, device=device) // cpg) % 2
        x = torch.where(grp == 0, 2048.0 + 16.0 * t, 512.0 + 4.0 * t)
        return x.to(torch.bfloat16), None
    if kind == "outlier":
        x = rn(B, HW, C)
        npx = max(1, HW // 512)
        px = torch.randint(0, HW, (B, npx), device=device, generator=gen)
        chn = torch.randint(0, C, (B, npx, 4), device=device, generator=gen)
        mag = torch.exp2(8.0 + 2.0 * torch.rand((B, npx, 4), device=device, generator=gen))
        mag = mag * torch.where(torch.rand((B, npx, 4), device=device, generator=gen) < 0.5, -1.0, 1.0)
        for bb in range(B):
            x[bb, px[bb][:, None].expand(npx, 4), chn[bb]] = mag[bb]
        return x.to(torch.bfloat16), 0.5 * rn(B, C)
    if kind == "const":
        x = (0.5 + 2.0 * rn(B, HW, C)).to(torch.bfloat16).double()
        c = (3.0 * rn(B, 1, G)).to(torch.bfloat16).double().repeat_interleave(cpg, -1)       # one constant per (item, group)
        near = c.expand(B, HW, C).clone()
        near[:, 0, :] += ulp_bf16(c[:, 0, :]) * (torch.arange(C, device=device) % cpg == 0)
        if HW > 1:
            near[:, HW - 1, :] -= ulp_bf16(c[:, 0, :]) * (torch.arange(C, device=device) % cpg == cpg - 1)
        g3 = (torch.arange(C, device=device) // cpg) % 3
        x = torch.where(g3 == 0, c.expand(B, HW, C), torch.where(g3 == 1, near, x))
        return x.to(torch.bfloat16), None
    assert kind == "pre_add_dominant", kind
    v = torch.exp2(8.0 + 2.0 * torch.rand((B, C), device=device, generator=gen))
    v = v * torch.where(torch.rand((B, C), device=device, generator=gen) < 0.5, -1.0, 1.0)
    return rn(B, HW, C).to(torch.bfloat16), v


def gn_affine(C, gen, device="cpu", groups=0):
    shape = (groups, C) if groups else (C,)
    w = (1.0 + 0.2 * torch.randn(shape, device=device, generator=gen)).to(torch.bfloat16)
    b = (0.3 * torch.randn(shape, device=device, generator=gen)).to(torch.bfloat16)
    return w, b
