"""float64 reference of the projector's layer-fusion launches (include/x2i.h: x2i_proj_conv5x5_bf16, x2i_proj_conv5x5_pack,
x2i_proj_conv5x5_packed_bf16, x2i_proj_layer_mean_bf16, x2i_seq_mean_f32) and a per-element checker that names the launch, the kernel form,
the sample, the output row and column of a failure and the row / column block of that form it falls in.  No GPU-only code here: the CPU
tests of the checker (tests/test_proj_ref_cpu.py) import it too.  Built on tests/gemm_ref.py, tests/ew_ref.py and tests/conv_ref.py.

`want` is the exact float64 value of the documented operator on the operands the kernel read (bf16 / f32 -> float64 is exact).
u = U_F32 = 2^-24 below; any summation in f32 has |err| <= depth u sum|terms|, depth the most roundings a term passes through.

  conv5x5.  y[b][s][h] = bias + sum_c sum_di sum_dj bf16(w[c][di][dj]) x[b][c][s + di - 2][h + dj - 2], zero outside the (S, H) plane: the taps
    are rounded to bf16 (RNE) by both kernels (csrc/projector.hip: the packed taps; csrc/proj_conv_mfma.hip: conv5x5_pack_kernel), the bias
    stays f32, products of two bf16 values are exact in f32.  conv5x5_sums builds it from 25 shifted float64 adds per layer, which also yields
    A = sum|x w|.  Allowance on the f32 value: depth u (A + |bias|) (+ MOM_FLUSH per summed element), then ONE bf16 rounding.
      VALU form (conv5x5_kernel<1 / 2>): an output's accumulator is one chain through every sub-step that feeds it: 5 input rows (one per
        kernel row) x 8 ceil(C / 8) layers (the layers past C are zero taps on zero-filled rows: counted all the same) x 3 v_dot2 (two exact
        products and the running sum per instruction: conv_ref.MOM_DOT2_ROUNDINGS), then the bias add:
        depth = VALU_DOT2_PER_ROW x 5 x 8 ceil(C / 8) x MOM_DOT2_ROUNDINGS + VALU_BIAS_ADDS.
      MFMA forms (conv5x5_mfma_kernel<2, 2>, conv5x5_mfma_pipe_kernel, conv5x5_mfma_rb2_kernel): each of the five per-kernel-row accumulators
        is a chain of C v_mfma_f32_16x16x32_bf16; one MFMA adds 32 products, 5 of them non-zero (a Toeplitz row holds the five taps; adding an
        exact zero rounds nothing), and the accumulator, in an order the hardware does not document: any order of 6 terms has at most 5
        additions on a term's way.  Then the epilogue's left-to-right sum bias + P_0 + ... + P_4: depth = MFMA_NONZERO x C + MFMA_EPILOGUE_ADDS.
  pack.  table[c][ds][n + 16 g][j] = bf16(w[c][ds][8 g + j - n - 6]), +0 outside the five taps: every entry compared bit for bit.
  layer_mean.  y = (1 / C) sum_c scale[c] x[c] (scale 1 without the pointer): C multiply-adds, fused or not (LM_MADD_ROUNDINGS each), the
    rounded 1 / C and the multiply by it (LM_SCALE_ROUNDINGS), one bf16 rounding.
  seq_mean.  y = (sum_s x[s]) / S in f32: S adds and the divide; f32 out: bound = (S + SEQ_DIVIDE) u sum|x| / S, no further rounding.

Constants: every allowance is an operation count read off the code (next to each constant); the f32 stand-ins of tests/test_proj_ref_cpu.py
stay inside every one of them (asserted there).  Largest share used on MI355X (tests/test_proj_fp64_gpu.py,
profiles/proj_fp64_gputest.log; |err| beyond the output's own rounding over the f32 allowance, for seq_mean |err| / bound):
conv5x5 VALU form: one stream 0.018 (edge operands, 510 tiles), two streams 0.003; MFMA forms: two-layer stages 0.013, pipelined 0.013, two row
blocks 0.108 (the self-chosen launch at n2 = 260, edge operands; 0.013 where conv5_variant forces it on the small shapes); layer_mean 0.054
(the grid-stride case, with scales); seq_mean 0.300.  The kernels' f32 sums are far more accurate than a worst-case chain: nearly every
error lies inside the output's own bf16 rounding.  None of the constants was changed."""
import torch

from tests.conv_ref import MOM_DOT2_ROUNDINGS, MOM_FLUSH
from tests.ew_ref import Report as RowReport
from tests.gemm_ref import (U_F32, Report, _round_bound, bf16_rne, check_untouched, poison_, sentinel_bits, ulp_bf16,  # noqa: F401
                            write_mask)

# ---------------------------------------------------------------------------------------------------------------- operation counts
# csrc/projector.hip, conv_substep: acc = dot2(p2, ., dot2(p1, ., dot2(p0, ., acc))) -- three v_dot2 per output, kernel row and layer
VALU_DOT2_PER_ROW = 3
# csrc/projector.hip: CL = 8 layers per sub-step; every sub-step runs all 8 (zero taps for the layers past C)
VALU_CL = 8
# csrc/projector.hip, the store in row(): pack_bf16x2(acc + bv, ...) -- one f32 add
VALU_BIAS_ADDS = 1
# csrc/proj_conv_mfma.hip, conv5x5_pack_kernel: dh = 8 g + j - n - 6 in 0 .. 4 -- five non-zero entries per Toeplitz row, so five non-zero
# products per accumulator element and MFMA
MFMA_NONZERO = 5
# csrc/proj_conv_mfma.hip, the epilogues: v = bv + acc[0] + row_shl<1>(acc[1]) + ... + row_shl<4>(acc[4]) -- five f32 adds, left to right
MFMA_EPILOGUE_ADDS = 5
# csrc/projector.hip, layer_mean_kernel: acc += sc * x -- product and sum (one rounding when contracted to an fma)
LM_MADD_ROUNDINGS = 2
# ... invC = 1.f / (float)C and acc * invC
LM_SCALE_ROUNDINGS = 2
# csrc/elementwise.hip, seq_mean_kernel: acc / (float)S
SEQ_DIVIDE = 1

# the old whole-tensor checks (tests/test_ops_gpu.py), kept here only to show what they miss (tests/test_proj_ref_cpu.py)
OLD_MFMA_REL_L2 = 3e-3          # against f32 F.conv2d on the bf16-rounded taps
OLD_VALU_REL_L2 = 5e-3          # against f32 F.conv2d on the unrounded taps
OLD_LAYER_MEAN_REL_L2 = 5e-3
OLD_SEQ_MEAN_REL_L2 = 1e-5
OLD_TABLE_ENTRIES = ((0, 0, 6), (1, 5, 3), (1, 0, 2), (2, 15, 7), (3, 15, 1), (0, 3, 0), (3, 0, 0))      # (g, n, j) per (layer, kernel row)

# kernel form -> (output rows, output columns) a workgroup owns
BLOCKS = {"valu1": (16, 512), "valu2": (32, 512), "mfma_pair": (12, 256), "mfma_pipe": (12, 256), "mfma_rb2": (24, 256)}
ROWS = 256                      # rows per float64 block


def _cdiv(a, b):
    return (a + b - 1) // b


def valu_form(B, S, H):
    """the kernel x2i_launch_proj_conv5x5 takes: two stacked row streams per block from 512 one-stream tiles on"""
    return "valu2" if _cdiv(H, 512) * _cdiv(S, 16) * B >= 512 else "valu1"


def mfma_tiles2(B, S, H):
    """n2 of x2i_launch_proj_conv5x5_packed: tiles of the two-row-block form"""
    return _cdiv(H, 256) * _cdiv(S, 24) * B


def mfma_form(variant, B, S, H):
    """the kernel x2i_launch_proj_conv5x5_packed takes under conv5_variant = variant"""
    n2 = mfma_tiles2(B, S, H)
    eff2 = n2 / (_cdiv(n2, 512) * 512)
    if variant == 1:
        return "mfma_pair"
    rb2 = variant == 3 or (variant == 0 and n2 >= 256 and (n2 <= 512 or eff2 >= 0.75))
    return "mfma_rb2" if rb2 else "mfma_pipe"


def conv5x5_depth(form, C):
    """roundings on the way of a term of one output's f32 sum (docstring)"""
    if form.startswith("valu"):
        return VALU_DOT2_PER_ROW * 5 * VALU_CL * _cdiv(C, VALU_CL) * MOM_DOT2_ROUNDINGS + VALU_BIAS_ADDS
    assert form.startswith("mfma"), form
    return MFMA_NONZERO * C + MFMA_EPILOGUE_ADDS


# ---------------------------------------------------------------------------------------------------------------- conv5x5
def conv5x5_sums(x, w, r0, r1):
    """(sum, sum of magnitudes) float64 [r1 - r0, H] of the 25 C products of output rows r0 .. r1 - 1 of ONE sample x [C, S, H] (bf16) with the
    taps w f32 [C, 25] rounded to bf16 -- without the bias.  25 shifted adds per layer."""
    C, S, H = x.shape
    rows = r1 - r0
    wd = w.reshape(C, 5, 5).to(torch.bfloat16).double()
    lo, hi = max(r0 - 2, 0), min(r1 + 2, S)
    xp = torch.zeros((C, rows + 4, H + 4), dtype=torch.float64, device=x.device)
    xp[:, lo - (r0 - 2):hi - (r0 - 2), 2:H + 2] = x[:, lo:hi].double()
    lin = torch.zeros((rows, H), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(lin)
    for di in range(5):
        for dj in range(5):
            t = xp[:, di:di + rows, dj:dj + H] * wd[:, di, dj, None, None]
            lin += t.sum(0)
            mag += t.abs().sum(0)
    return lin, mag


def conv5x5_bound(lin, mag, bias, form, C):
    """(want, bound, delta) from conv5x5_sums' pair: bias f32 [1] or None"""
    if bias is not None:
        bd = bias.double().reshape(())
        lin, mag = lin + bd, mag + bd.abs()
    d = conv5x5_depth(form, C) * U_F32 * mag + 25 * C * MOM_FLUSH
    return lin, _round_bound(lin, d, False), d


def conv5x5_expect(x, w, bias, form="mfma_pipe", r0=0, r1=None):
    """(want, bound, delta) float64 [r1 - r0, H] of output rows r0 .. r1 - 1 of one sample x [C, S, H] under kernel form `form`"""
    r1 = x.shape[1] if r1 is None else r1
    lin, mag = conv5x5_sums(x, w, r0, r1)
    return conv5x5_bound(lin, mag, bias, form, x.shape[0])


def where_conv(form, z):
    rb, cb = BLOCKS[form]

    def where(m, n):
        return (f"form {form}, sample {z}, output row {m}, column {n} (row block {m // rb}: rows {m // rb * rb}..{m // rb * rb + rb - 1}, row "
                f"{m % rb} of it; column block {n // cb}: columns {n // cb * cb}..{n // cb * cb + cb - 1})")
    return where


def check_written(name, y, form):
    """no element of the output y [B, S, H] may still hold the sentinel the buffer was poisoned with"""
    left = sentinel_bits(y)
    if bool(left.any()):
        z, s, h = (int(v) for v in torch.nonzero(left)[0])
        raise AssertionError(f"{name}: {int(left.sum())} output elements left unwritten (still the sentinel); first at {where_conv(form, z)(s, h)}")


class ConvRef:
    """The float64 sums of one operand set x [B, C, S, H], w [C, 25], computed once in row blocks and shared by every launch on it (any kernel
    form, with or without the bias)."""

    def __init__(self, x, w, rows=ROWS):
        self.B, self.C, self.S, self.H = x.shape
        self.blocks = [[(r0,) + conv5x5_sums(x[z], w, r0, min(self.S, r0 + rows)) for r0 in range(0, self.S, rows)] for z in range(self.B)]

    def check(self, name, y, form, bias):
        """every element of y [B, S, H] (a view into a poisoned buffer, after the launch): the worst share of the f32 allowance used"""
        assert tuple(y.shape) == (self.B, self.S, self.H)
        check_written(name, y, form)
        rep = Report(f"{name} [{form}]")
        for z in range(self.B):
            for r0, lin, mag in self.blocks[z]:
                want, bound, d = conv5x5_bound(lin, mag, bias, form, self.C)
                rep.check(y[z, r0:r0 + lin.shape[0]], want, bound, d, item=z, row0=r0, where=where_conv(form, z))
        return rep.done()


def check_conv5x5(name, x, w, bias, y, form):
    return ConvRef(x, w).check(name, y, form, bias)


# ---------------------------------------------------------------------------------------------------------------- the packed table
def pack_expect(w):
    """the exact table of x2i_proj_conv5x5_pack for w f32 [C, 25]: bf16 [C, 5, 64, 8]"""
    C = w.shape[0]
    wb = w.reshape(C, 5, 5).to(torch.bfloat16)
    lane = torch.arange(64, device=w.device)
    n, g = lane % 16, lane // 16
    dh = 8 * g[:, None] + torch.arange(8, device=w.device)[None, :] - n[:, None] - 6                # [64, 8]
    ok = (dh >= 0) & (dh <= 4)
    t = wb[:, :, dh.clamp(0, 4)]                                                                     # [C, 5, 64, 8]
    return torch.where(ok, t, torch.zeros((), dtype=torch.bfloat16, device=w.device))


def check_table(name, table, w):
    want = pack_expect(w)
    assert tuple(table.shape) == tuple(want.shape), (tuple(table.shape), tuple(want.shape))
    diff = table.view(torch.int16) != want.to(table.device).view(torch.int16)
    if bool(diff.any()):
        c, ds, lane, j = (int(v) for v in torch.nonzero(diff)[0])
        raise AssertionError(f"{name}: {int(diff.sum())} table entries differ; first at layer {c}, kernel row {ds}, lane {lane} (n={lane % 16}, "
                             f"g={lane // 16}), j={j} (tap {8 * (lane // 16) + j - lane % 16 - 6}): got {float(table[c, ds, lane, j])!r} want "
                             f"{float(want[c, ds, lane, j])!r}")


# ---------------------------------------------------------------------------------------------------------------- the means
def layer_mean_expect(x, scale):
    """x2i_proj_layer_mean_bf16 of ONE sample x [C, ...] (bf16), scale f32 [C] or None: (want, bound, delta) float64 [...]"""
    C = x.shape[0]
    t = x.double()
    if scale is not None:
        t = t * scale.double().view(C, *([1] * (x.dim() - 1)))
    want, mag = t.sum(0) / C, t.abs().sum(0) / C
    d = (LM_MADD_ROUNDINGS * C + LM_SCALE_ROUNDINGS) * U_F32 * mag
    return want, _round_bound(want, d, False), d


def check_layer_mean(name, x, scale, y):
    """every element of y [B, S, H] against x [B, C, S, H]: the worst share of the f32 allowance used; a failure names sample, row, the
    8-wide chunk and the column"""
    B, C, S, H = x.shape
    rep = RowReport(name)
    tok = torch.arange(S)
    for z in range(B):
        want, bound, d = layer_mean_expect(x[z], scale)
        rep.check(y[z], want, bound, d, sample=torch.full((S,), z), token=tok, unit=8)
    return rep.done()


def seq_mean_expect(x):
    """x2i_seq_mean_f32 of x f32 [B, S, N]: (want, bound) float64 [B, N]"""
    S = x.shape[1]
    t = x.double()
    want, mag = t.sum(1) / S, t.abs().sum(1) / S
    return want, (S + SEQ_DIVIDE) * U_F32 * mag


def check_seq_mean(name, x, y):
    """every element of y [B, N]: worst |err| / bound; a failure names the sample and the 256-wide block of columns"""
    B = x.shape[0]
    want, bound = seq_mean_expect(x)
    rep = RowReport(name)
    rep.check(y, want, bound, sample=torch.arange(B), token=torch.zeros(B, dtype=torch.long), unit=256)
    return rep.done()


# ---------------------------------------------------------------------------------------------------------------- operands
CONV_KINDS = ("random", "cancel", "edge", "tagged")


def layer_tags(C, device="cpu"):
    """`tagged` exponents: a different power of two for each of up to 64 layers (37 is coprime to 64), neighbours far apart"""
    return ((torch.arange(C, device=device) * 37) % 64 - 32).double()


def conv_operands(kind, B, C, S, H, gen, device="cpu"):
    """(x bf16 [B, C, S, H], w f32 [C, 25], bias f32 [1]) of one kind:
    random   x ~ 3 N(0, 1), w ~ N(0, 1 / (25 C)), bias ~ N(0, 1)
    cancel   x ~ 4 + N(0, 1), every layer's 25 taps with zero mean, a small bias: inside the plane |want| << sum|x w| -- the bound is absolute
             there, not hidden behind the output's own rounding; at the zero-padded border the mean does not cancel
    edge     |x| in 64 [0.5, 1) in rows {0, 1, S - 2, S - 1} and columns {0, 1, H - 2, H - 1} of every layer, in [0.5, 1) / 64 elsewhere: a row's
             end wrapped into the next row, or a padding row read from the neighbouring layer or sample, misses by far more than the bound
    tagged   random with layer c of x times 2^e_c and of w times 2^-e_c, e_c all different: a layer met with another layer's taps is visible"""
    rn = lambda *s: torch.randn(s, device=device, generator=gen)
    x = 3.0 * rn(B, C, S, H)
    w = rn(C, 25) / (25 * C) ** 0.5
    bias = rn(1)
    if kind == "cancel":
        x = x / 3.0 + 4.0
        w = w - w.mean(1, keepdim=True)
        bias = bias * 0.01
    elif kind == "edge":
        s, h = torch.arange(S, device=device), torch.arange(H, device=device)
        border = ((s < 2) | (s >= S - 2))[:, None] | ((h < 2) | (h >= H - 2))[None, :]
        mag = torch.where(border, 64.0, 1.0 / 64.0)
        x = torch.sign(x) * (0.5 + 0.5 * torch.rand((B, C, S, H), device=device, generator=gen)) * mag
    elif kind == "tagged":
        e = layer_tags(C, device)
        x = x * torch.exp2(e).float().view(1, C, 1, 1)
        w = w * torch.exp2(-e).float().view(C, 1)
    else:
        assert kind == "random", kind
    return x.to(torch.bfloat16), w.contiguous(), bias
