"""The checker of tests/conv_ref.py is itself tested, without a GPU:

  * the reference is right: gather() plus a float64 matmul equals float64 F.conv2d on F.pad / F.interpolate / repeat_interleave inputs for
    every descriptor form (integer operands: both sides exact), the GroupNorm reference equals float64 F.group_norm;
  * f32 stand-ins, written in plain torch, of each kernel's documented algorithm pass on every operand kind -- the one-pass GroupNorm with
    its slab structure among them: the derived bounds admit a correct kernel;
  * every fault of the list below, put into a stand-in, is rejected at the right sample, pixel and channel -- and OLD_MISSES names the ones
    the old checks (rel-L2 1e-2 / 5e-3 over the tensor, moments normalised by their largest entry) let through."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests.gemm_ref import U_F32

BF = torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- the reference is right
def torch_conv_f64(x, w, g, *, pad_fix=None):
    """float64 F.conv2d of x [B, H, W, Cin] with w [N, K] ((ky, kx, ci) order) for geometry g, through F.pad / F.interpolate /
    repeat_interleave: [B, OH, OW, N]"""
    xin = x.double().permute(0, 3, 1, 2)
    if g.up == 1:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    elif g.up == 2:
        xin = xin.repeat_interleave(2, dim=2)
    Hv, Wv = xin.shape[2], xin.shape[3]
    bottom = (g.OH - 1) * g.stride + g.KH - g.pad - Hv
    right = (g.OW - 1) * g.stride + g.KW - g.pad_w - Wv
    xp = F.pad(xin, (g.pad_w, right, g.pad, bottom))
    wk = w.double().view(-1, g.KH, g.KW, g.Cin).permute(0, 3, 1, 2)
    return F.conv2d(xp, wk, stride=g.stride).permute(0, 2, 3, 1)


FORMS = {
    "3x3": dict(KH=3, KW=3, stride=1, pad=1),
    "up1": dict(KH=3, KW=3, stride=1, pad=1, up=1),
    "up2_phase0": dict(KH=3, KW=2, stride=1, pad=1, up=2, pad_w=1, out_w=10),
    "up2_phase1": dict(KH=3, KW=2, stride=1, pad=1, up=2, pad_w=0, out_w=10),
    "phase00": dict(KH=2, KW=2, stride=1, pad=1, pad_w=1, out_w=10, out_h=8),
    "phase11": dict(KH=2, KW=2, stride=1, pad=0, pad_w=0, out_w=10, out_h=8),
    "stride2": dict(KH=3, KW=3, stride=2, pad=1),
    "stride2_onesided": dict(KH=3, KW=3, stride=2, pad=0, out_w=5, out_h=4),
    "5x5": dict(KH=5, KW=5, stride=2, pad=2),
    "2x2_nopad": dict(KH=2, KW=2, stride=2, pad=0),
    "5x1": dict(KH=5, KW=1, stride=2, pad=2, pad_w=0),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_gather_equals_torch_conv(form):
    kw = dict(FORMS[form])
    H, W, Cin, N, B = 8, 10, 64, 8, 2
    g = R.Geom(H, W, Cin, kw.pop("KH"), kw.pop("KW"), kw.pop("stride"), kw.pop("pad"), **kw)
    x = torch.randint(-4, 5, (B, H, W, Cin), generator=gen(1)).to(BF)
    w = torch.randint(-3, 4, (N, g.K), generator=gen(2)).to(BF)
    ref = torch_conv_f64(x, w, g)
    assert tuple(ref.shape) == (B, g.OH, g.OW, N)
    for z in range(B):
        got = R.gather(x[z], g, 0, g.M).double() @ w.double().T
        assert torch.equal(got.view(g.OH, g.OW, N), ref[z]), form
        got = R.gather(x[z], g, 7, min(g.M, 19)).double() @ w.double().T           # a block in the middle
        assert torch.equal(got, ref[z].reshape(g.M, N)[7:min(g.M, 19)])


def test_gather_one_row_window_1x5():
    """the 1 x 5 edge launch of the composed 5 x 5 conv: a window of ONE input row per item (a_batch_stride = H W Cin), pad_w = 2, pad = 0"""
    H, W, Cin, N, B = 6, 12, 64, 8, 3
    x = torch.randint(-4, 5, (B, H, W, Cin), generator=gen(3)).to(BF)
    w = torch.randint(-3, 4, (N, 5 * Cin), generator=gen(4)).to(BF)
    g = R.Geom(1, W, Cin, 1, 5, 2, 0, pad_w=2)
    assert (g.OH, g.OW) == (1, 6)
    for row in (0, 3):
        ref = torch_conv_f64(x[:, row:row + 1].contiguous(), w, g)
        for z in range(B):
            xz = R.item_view(x, g, z, a_offset=row * W * Cin, a_batch_stride=H * W * Cin)
            assert torch.equal(R.gather(xz, g, 0, g.M).double() @ w.double().T, ref[z].reshape(g.M, N))


@pytest.mark.parametrize("G,C,act", [(2, 64, R.ACT_RELU), (32, 128, R.ACT_SILU), (8, 256, R.ACT_NONE)])
def test_groupnorm_reference_equals_torch(G, C, act):
    B, HW = 2, 77
    x, pa = R.gn_input("random", B, HW, C, G, gen(5))
    w, b = R.gn_affine(C, gen(6))
    post = torch.randn((B, HW, C), generator=gen(7)).to(BF)
    for z in range(B):
        st = R.gn_stats(x[z], pa[z], G)
        zero = torch.zeros_like(st["mean"])
        want, _, _ = R.gn_apply_expect(x[z], pa[z], w, b, st["mean"], st["var"], zero, zero, 1e-6, act, post[z], G)
        zz = (x[z].double() + pa[z].double()).T[None]                     # [1, C, HW]
        ref = F.group_norm(zz, G, w.double(), b.double(), eps=R.f32(1e-6))
        ref = {R.ACT_RELU: torch.relu, R.ACT_SILU: F.silu, R.ACT_NONE: lambda t: t}[act](ref)[0].T + post[z].double()
        assert float((want - ref).abs().max()) < 1e-12 * float(ref.abs().max())
        # the statistics from exact per-channel moments are the same statistics
        mom = torch.stack((x[z].double().sum(0), (x[z].double() ** 2).sum(0)), 1)
        ms = R.moments_stats(mom, pa[z], HW, G)
        assert float((ms["mean"] - st["mean"]).abs().max()) < 1e-12 and float((ms["var"] / st["var"] - 1).abs().max()) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- conv stand-in
def conv_acc_f32(x, w, g, *, pad_fault=None, up_fault=False):
    """f32 accumulators [B, OH, OW, N] of the documented conv through F.pad / F.unfold and an f32 matmul (no use of conv_ref.gather)"""
    xin = x.float().permute(0, 3, 1, 2)
    if g.up == 1:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    elif g.up == 2:
        if up_fault:            # columns doubled instead of rows; virtual rows >= H are then out of range
            xin = F.pad(xin.repeat_interleave(2, dim=3)[:, :, :, :g.W], (0, 0, 0, g.H))
        else:
            xin = xin.repeat_interleave(2, dim=2)
    Hv, Wv = xin.shape[2], xin.shape[3]
    bottom = (g.OH - 1) * g.stride + g.KH - g.pad - Hv
    right = (g.OW - 1) * g.stride + g.KW - g.pad_w - Wv
    xp = F.pad(xin, (g.pad_w, right, g.pad, bottom))
    if pad_fault:
        pad_fault(xp, xin)
    cols = F.unfold(xp, (g.KH, g.KW), stride=g.stride)                                   # [B, Cin KH KW, L], (ci, ky, kx) order
    B = x.shape[0]
    cols = cols.view(B, g.Cin, g.KH * g.KW, g.M).permute(0, 3, 2, 1).reshape(B, g.M, g.K)
    wz = w.float()
    acc = cols @ (wz.transpose(-1, -2) if wz.dim() == 3 else wz.T)
    return acc.view(B, g.OH, g.OW, -1)


def truncate_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def epilogue(acc, bias, *, bias2=None, act=R.ACT_NONE, res=None, mode="ok"):
    """v = act(acc + bias + bias2) + res, rounded ONCE (include/x2i.h); `mode` injects a fault"""
    v = acc
    if bias is not None:
        v = v + (bias.float()[:, None, None, :] if bias.dim() == 2 else bias.float())
    if bias2 is not None and mode != "bias2_behind_relu":
        v = v + bias2[:, None, None, :]
    if act == R.ACT_RELU:
        v = v.clamp_min(0.0)
    if bias2 is not None and mode == "bias2_behind_relu":
        v = v + bias2[:, None, None, :]
    if res is not None:
        v = (v.to(BF).float() if mode == "round_before_res" else v) + res.float()
    return truncate_bf16(v) if mode == "truncate" else v.to(BF)


def run_check(name, x, w, bias, out, g, N, B, **kw):
    rep = R.Report(name)
    R.check_conv(rep, x, w, bias, out, g, N, B, rows=256, **kw)
    return rep.done()


CONV_CASES = {
    "3x3": (dict(KH=3, KW=3, stride=1, pad=1), dict()),
    "3x3_relu_bias2": (dict(KH=3, KW=3, stride=1, pad=1), dict(act=R.ACT_RELU, bias2=True)),
    "3x3_res": (dict(KH=3, KW=3, stride=1, pad=1), dict(res=True)),
    "stride2": (dict(KH=3, KW=3, stride=2, pad=1), dict()),
    "5x5": (dict(KH=5, KW=5, stride=2, pad=2), dict(res=True)),
    "2x2": (dict(KH=2, KW=2, stride=2, pad=0), dict()),
    "up1": (dict(KH=3, KW=3, stride=1, pad=1, up=1), dict()),
    "up2": (dict(KH=3, KW=2, stride=1, pad=1, up=2, pad_w=1, out_w=16), dict()),
    "phase": (dict(KH=2, KW=2, stride=1, pad=0, pad_w=1, out_w=16, out_h=12), dict()),
}


def make_case(case, kind, seed, B=2, H=12, W=16, Cin=64, N=16):
    gk, ek = (dict(d) for d in CONV_CASES[case])
    g = R.Geom(H, W, Cin, gk.pop("KH"), gk.pop("KW"), gk.pop("stride"), gk.pop("pad"), **gk)
    gn = gen(seed)
    x, w, bias = R.conv_operands(kind, B, H, W, Cin, N, g.KH, g.KW, gn)
    extra = dict(act=ek.get("act", R.ACT_NONE))
    if ek.get("bias2"):
        extra["bias2"] = 0.5 * torch.randn((B, N), generator=gn)
    acc = conv_acc_f32(x, w, g)
    if ek.get("res"):
        lin = acc + bias.float()
        extra["res"] = (-lin if kind == "cancel" else lin.abs().mean() * torch.randn(lin.shape, generator=gn)).to(BF)
    return g, x, w, bias, acc, extra


@pytest.mark.parametrize("kind", R.CONV_KINDS)
@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv_standin_passes(case, kind):
    g, x, w, bias, acc, extra = make_case(case, kind, 11)
    B, N = x.shape[0], w.shape[0]
    out = epilogue(acc, bias, **extra)
    kw = dict(act=extra["act"], bias2=extra.get("bias2"))
    if "res" in extra:
        kw["res_store"] = extra["res"]
    share = run_check(f"{case} {kind}", x, w, bias, out, g, N, B, **kw)
    assert share <= 1.0


def test_conv_standin_passes_grouped_strided_and_in_place():
    """grouped weights (item b uses group b // w_group), the output in a wider pixel (ldc > N) of a larger tensor, the residual aliasing the
    output and a residual shared by all items (res_batch_stride = 0); the sentinel stays everywhere else"""
    B, H, W, Cin, N, wg = 4, 8, 8, 64, 16, 2
    g = R.Geom(H, W, Cin, 3, 3, 1, 1)
    x, w, bias = R.conv_operands("random", B, H, W, Cin, N, 3, 3, gen(12), groups=2)
    acc = torch.stack([conv_acc_f32(x[z:z + 1], w[z // wg], g)[0] for z in range(B)])
    bz = bias[torch.arange(B) // wg]
    ldc, cbs, coff = 2 * N + 8, g.M * (2 * N + 8) + 64, 8
    store = R.poison_(torch.empty(B * cbs + 64, dtype=BF))
    res = torch.randn((B, H, W, N), generator=gen(13)).to(BF)
    shape, stride, off = R.out_geometry(g, N, B, c_offset=coff, c_batch_stride=cbs, ldc=ldc)
    view = store.as_strided(shape, stride, off)
    view.copy_(res)                                   # the residual lives where the output goes
    before = store.clone()
    view.copy_(epilogue(acc, bz, res=res))
    run_check("grouped in place", x, w, bias, store, g, N, B, w_group=wg, c_offset=coff, c_batch_stride=cbs, ldc=ldc, res_store=before,
              res_offset=coff, res_batch_stride=cbs, ldr=ldc)
    R.check_untouched("grouped in place", store, R.write_mask(store, [(shape, stride, off)]), row_len=ldc)
    # one residual map for every item
    out = epilogue(acc, bz, res=res[:1])
    run_check("shared residual", x, w, bias, out, g, N, B, w_group=wg, res_store=res[0], res_batch_stride=0)
    # group off by one: the first item that changes group is rejected
    wrong = torch.stack([conv_acc_f32(x[z:z + 1], w[min(1, (z + 1) // wg)], g)[0] for z in range(B)])
    with pytest.raises(AssertionError, match=r"sample 1, output pixel"):
        run_check("group off by one", x, w, bias, epilogue(wrong, bz), g, N, B, w_group=wg)


# ---------------------------------------------------------------------------------------------------------------- conv faults
def _fault_corner(xp, xin):         # the top-left padding pixel holds its neighbour: tap (0, 0) of output pixel (0, 0) of sample 1 only
    xp[1, :, 0, 0] = xin[1, :, 0, 0]


def _fault_right(xp, xin):          # the right-hand padding column reads on in memory: the next row's first pixel
    xp[:, :, :xin.shape[2] - 1, -1] = xin[:, :, 1:, 0]


def _fault_next_item(xp, xin):      # the bottom padding row of sample 0 is the first row of sample 1
    xp[0, :, -1, 1:-1] = xin[1, :, 0, :]


def conv_fault_outputs(fault, kind="random"):
    """(geometry, operands, the faulty stand-in's output, checker kwargs, where the failure must be named, f32 reference for the old check)"""
    B, N = 2, 16
    if fault == "corner_tap_unmasked":
        g, x, w, bias, acc, ex = make_case("3x3", kind, 21, H=32, W=32)
        bad = conv_acc_f32(x, w, g, pad_fault=_fault_corner)
        return g, x, w, bias, epilogue(bad, bias), {}, r"sample 1, output pixel \(oy=0, ox=0\)", epilogue(acc, bias)
    if fault == "right_padding_ignored_out_w":
        g, x, w, bias, acc, ex = make_case("phase", kind, 22, H=32, W=32)
        g = R.Geom(32, 32, 64, 2, 2, 1, 0, pad_w=0, out_w=32, out_h=32)
        acc = conv_acc_f32(x, w, g)
        bad = conv_acc_f32(x, w, g, pad_fault=_fault_right)
        return g, x, w, bias, epilogue(bad, bias), {}, r"ox=31\)", epilogue(acc, bias)
    if fault == "stride2_last_column_off_by_one":
        g, x, w, bias, acc, ex = make_case("stride2", kind, 23, H=32, W=32)
        bad = acc.clone()
        bad[:, :, -1] = conv_acc_f32(torch.roll(x, -1, 2), w, g)[:, :, -1]
        return g, x, w, bias, epilogue(bad, bias), {}, r"ox=15\)", epilogue(acc, bias)
    if fault == "tap_into_next_item":
        g, x, w, bias, acc, ex = make_case("3x3", kind, 24, H=32, W=32)
        bad = conv_acc_f32(x, w, g, pad_fault=_fault_next_item)
        return g, x, w, bias, epilogue(bad, bias), {}, r"sample 0, output pixel \(oy=31,", epilogue(acc, bias)
    if fault == "channel_slice_twice":
        g, x, w, bias, acc, ex = make_case("3x3", kind, 25, Cin=128)
        x2 = x.clone()
        x2[..., 64:] = x[..., :64]
        return g, x, w, bias, epilogue(conv_acc_f32(x2, w, g), bias), {}, r"sample \d, output pixel", epilogue(acc, bias)
    if fault == "up2_doubles_columns":
        g, x, w, bias, acc, ex = make_case("up2", kind, 26)
        return g, x, w, bias, epilogue(conv_acc_f32(x, w, g, up_fault=True), bias), {}, r"sample \d, output pixel", epilogue(acc, bias)
    if fault in ("truncate", "round_before_res", "bias2_behind_relu"):
        case = {"truncate": "3x3", "round_before_res": "3x3_res", "bias2_behind_relu": "3x3_relu_bias2"}[fault]
        g, x, w, bias, acc, ex = make_case(case, kind, 27, H=32, W=32)
        kw = dict(act=ex["act"], bias2=ex.get("bias2"))
        if "res" in ex:
            kw["res_store"] = ex["res"]
        return g, x, w, bias, epilogue(acc, bias, mode=fault, **ex), kw, r"sample \d, output pixel", epilogue(acc, bias, **ex)
    raise AssertionError(fault)


CONV_FAULTS = ["corner_tap_unmasked", "right_padding_ignored_out_w", "stride2_last_column_off_by_one", "tap_into_next_item",
               "channel_slice_twice", "up2_doubles_columns", "truncate", "round_before_res", "bias2_behind_relu"]
# faults that the old checks let through (rel-L2 < 1e-2 against the correct f32 result over the whole tensor; 5e-3 for GroupNorm;
# moments |got - want| / max|want| < 2e-5)
OLD_MISSES = {"corner_tap_unmasked", "truncate", "round_before_res", "gn_bf16_mean"}


@pytest.mark.parametrize("fault", CONV_FAULTS)
def test_conv_fault_is_rejected(fault):
    g, x, w, bias, out, kw, where, good = conv_fault_outputs(fault)
    with pytest.raises(AssertionError, match=where):
        run_check(fault, x, w, bias, out, g, w.shape[0], x.shape[0], **kw)
    run_check(fault + " (no fault)", x, w, bias, good, g, w.shape[0], x.shape[0], **kw)
    old_passes = rel_l2(out, good) < R.OLD_CONV_REL_L2
    assert old_passes == (fault in OLD_MISSES), (fault, rel_l2(out, good))


@pytest.mark.parametrize("fault", ["corner_tap_unmasked", "tap_into_next_item", "channel_slice_twice", "stride2_last_column_off_by_one"])
def test_addressing_faults_are_rejected_on_tagged_operands_too(fault):
    """`tagged` operands: rows, columns, slices, taps and items differ by powers of two; the addressing faults are named at the same place"""
    g, x, w, bias, out, kw, where, good = conv_fault_outputs(fault, kind="tagged")
    with pytest.raises(AssertionError, match=where):
        run_check("tagged " + fault, x, w, bias, out, g, w.shape[0], x.shape[0], **kw)
    run_check("tagged " + fault + " (no fault)", x, w, bias, good, g, w.shape[0], x.shape[0], **kw)


def test_write_into_the_other_phase_is_rejected():
    """phase (0, 0) of a four-phase upsampling conv: ldc = 2 N, rows two output rows apart; a store into the other phase's column, and one
    into the channels behind N of a wide pixel, leave the write set"""
    B, H, W, Cin, N = 2, 8, 8, 64, 16
    g = R.Geom(H, W, Cin, 2, 2, 1, 1, pad_w=1, out_w=W, out_h=H)
    x, w, bias = R.conv_operands("random", B, H, W, Cin, N, 2, 2, gen(31))
    out = epilogue(conv_acc_f32(x, w, g), bias)
    geo = dict(c_offset=0, c_batch_stride=4 * H * W * N, ldc=2 * N, out_row_pitch=4 * W * N)
    shape, stride, off = R.out_geometry(g, N, B, **geo)
    store = R.poison_(torch.empty(B * 4 * H * W * N, dtype=BF))
    store.as_strided(shape, stride, off).copy_(out)
    run_check("phase", x, w, bias, store, g, N, B, **geo)
    R.check_untouched("phase", store, R.write_mask(store, [(shape, stride, off)]), row_len=2 * N)
    bad = store.clone()
    bad[3 * 2 * N + N + 5] = 1.0                      # pixel 3's neighbour column (phase px = 1), channel 5
    with pytest.raises(AssertionError, match=r"row 3, col 21"):
        R.check_untouched("phase", bad, R.write_mask(bad, [(shape, stride, off)]), row_len=2 * N)


# ---------------------------------------------------------------------------------------------------------------- moments
def moments_standin(y, *, row_block=128, prev=None, fault=None, v32=None):
    """f32 channel-quad moments of the stored outputs y [B, M, N] (bf16): per-row-block sums, then the blocks in order"""
    B, M, N = y.shape
    src = (v32 if fault == "f32_values" else y.float()).view(B, M, N // 4, 4)
    mom = torch.zeros((B, N, 2))
    Mu = M - M % row_block if fault == "no_ragged_block" else M
    s1, s2 = torch.zeros((B, N // 4)), torch.zeros((B, N // 4))
    for r0 in range(0, Mu, row_block):
        blk = src[:, r0:r0 + row_block]
        s1 = s1 + blk.sum((1, 3))
        s2 = s2 + (blk * blk).sum((1, 3))
    slot = 1 if fault == "slot_c_plus_1" else 0
    mom[:, slot::4, 0], mom[:, slot::4, 1] = s1, s2
    if prev is not None and fault != "accumulate_overwrites":
        mom = mom + prev
    return mom


def _moments_case(kind, seed=41, M_side=(25, 36)):
    H, W = M_side
    g, x, w, bias, acc, ex = make_case("3x3", kind, seed, H=H, W=W, N=32)
    v32 = acc + bias.float()
    return v32.view(2, H * W, 32), v32.to(BF).view(2, H * W, 32)


@pytest.mark.parametrize("kind", R.CONV_KINDS)
def test_moments_standin_passes(kind):
    v32, y = _moments_case(kind)
    B, M, N = y.shape
    for rb in (64, 128):
        want, bound = R.moments_expect(y, R.moments_depth(M, N, rb))
        assert R.assert_entries(f"moments {kind}", moments_standin(y, row_block=rb), want, bound) <= 1.0
    prev = moments_standin(y) * 3.0
    want, bound = R.moments_expect(y, R.moments_depth(M, N, 128, accumulate=True), prev=prev)
    assert R.assert_entries("accumulate", moments_standin(y, prev=prev), want, bound) <= 1.0


def _old_moments_check(got, want):
    return float((got.double() - want).abs().max() / want.abs().max()) < R.OLD_MOM_MAXNORM


@pytest.mark.parametrize("fault,where", [("no_ragged_block", r"sample \d, channel \d+, sum"), ("f32_values", r"sample \d, channel \d+, sum"),
                                         ("slot_c_plus_1", r"sample \d, channel \d+, sum"), ("accumulate_overwrites", r"sample \d, channel")])
def test_moments_fault_is_rejected(fault, where):
    v32, y = _moments_case("random")
    B, M, N = y.shape
    prev = moments_standin(y) * 3.0 if fault == "accumulate_overwrites" else None
    want, bound = R.moments_expect(y, R.moments_depth(M, N, 128, accumulate=prev is not None), prev=prev)
    got = moments_standin(y, fault=fault, v32=v32, prev=prev)
    with pytest.raises(AssertionError, match=where):
        R.assert_entries(fault, got, want, bound)
    assert _old_moments_check(got, want) == (fault in OLD_MISSES), fault


def test_moments_small_quad_is_checked_per_entry():
    """one quad with small outputs next to large ones: its sum is wrong by half, which the max-normalised check cannot see"""
    v32, y = _moments_case("random")
    y = y.clone()
    y[:, :, 4:8] = (y[:, :, 4:8].float() * 2.0 ** -16).to(BF)
    B, M, N = y.shape
    want, bound = R.moments_expect(y, R.moments_depth(M, N, 128))
    got = moments_standin(y)
    R.assert_entries("small quad", got, want, bound)
    got[0, 4] *= 0.5
    assert _old_moments_check(got, want)
    with pytest.raises(AssertionError, match=r"sample 0, channel 4, sum"):
        R.assert_entries("small quad", got, want, bound)


# ---------------------------------------------------------------------------------------------------------------- the other convs
def test_narrow_image_and_stem_standins_and_faults():
    B, H, W, Cin, Cout, ldy = 2, 9, 21, 32, 3, 8
    g = R.Geom(H, W, Cin, 3, 3, 1, 1)
    x, w, bias = R.conv_operands("random", B, H, W, Cin, Cout, 3, 3, gen(51))
    y = R.poison_(torch.empty((B, H, W, ldy), dtype=BF))
    y[..., :Cout] = epilogue(conv_acc_f32(x, w, g), bias)
    y[..., Cout:4] = 0.0
    R.check_narrow(R.Report("narrow"), x, w, bias, y, Cout).done()
    bad = y.clone()
    bad[1, 2, 3, 3] = -0.0
    with pytest.raises(AssertionError, match=r"channel 3 of sample 1, pixel \(oy=2, ox=3\) is not \+0"):
        R.check_narrow(R.Report("narrow"), x, w, bias, bad, Cout)
    bad = y.clone()
    bad[0, 1, 1, 4] = 0.0
    with pytest.raises(AssertionError, match=r"channel 4 .* of sample 0, pixel \(oy=1, ox=1\) written"):
        R.check_narrow(R.Report("narrow"), x, w, bias, bad, Cout)
    # image stem: NCHW input, the nn.Conv2d weight as it is
    xi = torch.randn((B, 3, H, W), generator=gen(52)).to(BF)
    wi = (torch.randn((16, 3, 3, 3), generator=gen(53)) / 5).to(BF)
    bi = torch.randn(16, generator=gen(54)).to(BF)
    yi = (F.conv2d(xi.float(), wi.float(), bi.float(), padding=1)).permute(0, 2, 3, 1).to(BF)
    R.check_image(R.Report("image"), xi, wi, bi, yi).done()
    want, bound = R.moments_expect(yi.view(B, H * W, 16), R.image_moments_depth(H, W, 16))          # its moments: the convs' layout
    assert R.assert_entries("image moments", moments_standin(yi.view(B, H * W, 16)), want, bound) <= 1.0
    with pytest.raises(AssertionError, match=r"sample 1, output pixel \(oy=8, ox=20\), channel 7"):
        yb = yi.clone()
        yb[1, 8, 20, 7] = (yb[1, 8, 20, 7].float() * (1 + 2.0 ** -7)).to(BF)          # one bf16 ulp
        R.check_image(R.Report("image"), xi, wi, bi, yb).done()
    # ControlNeXt stem: f32 weights, stride 2
    xs = torch.randn((B, 10, 14, 3), generator=gen(55)).to(BF)
    ws, bs = torch.randn((16, 3, 3, 3), generator=gen(56)) / 5, torch.randn(16, generator=gen(57))
    ys = F.conv2d(xs.float().permute(0, 3, 1, 2), ws.permute(0, 3, 1, 2), bs, stride=2, padding=1).permute(0, 2, 3, 1).to(BF)
    R.check_stem(R.Report("stem"), xs, ws, bs, ys).done()


# ---------------------------------------------------------------------------------------------------------------- GroupNorm stand-ins
def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def gn_sums_standin(z, G):
    """one-pass f32 (S1, S2) [B, G] of z [B, HW, C] f32 with the kernels' slab structure: 256 slabs of ceil(HW / 256) pixels, per slab the
    pixels one after the other per channel, the channels of a group, then the slabs one after the other"""
    B, HW, C = z.shape
    per = (HW + R.GN_SLABS - 1) // R.GN_SLABS
    zp = F.pad(z, (0, 0, 0, per * R.GN_SLABS - HW)).view(B, R.GN_SLABS, per, C)
    s, q = torch.zeros((B, R.GN_SLABS, C)), torch.zeros((B, R.GN_SLABS, C))
    for p in range(per):
        s = s + zp[:, :, p]
        q = fma32(zp[:, :, p], zp[:, :, p], q)
    s, q = s.view(B, R.GN_SLABS, G, -1).sum(-1), q.view(B, R.GN_SLABS, G, -1).sum(-1)
    a, b = torch.zeros((B, G)), torch.zeros((B, G))
    for sl in range(R.GN_SLABS):
        a, b = a + s[:, sl], b + q[:, sl]
    return a, b


def gn_apply_standin(x, y_stats, w, b, G, act, pre_add, post, fault=None):
    B, HW, C = x.shape
    cpg = C // G
    m, r = (t.repeat_interleave(cpg, -1) for t in y_stats)                        # [B, C]
    if fault == "group_boundary_shift":                                            # channel c takes the statistics of channel c + 4's group
        m, r = (torch.cat((t[:, 4:], t[:, -4:]), 1) for t in (m, r))
    pa = torch.zeros((B, C)) if pre_add is None else pre_add
    sc = r * w.float()
    sh = fma32(pa - m, sc, b.float().expand_as(sc))
    v = fma32(x.float(), sc[:, None, :], sh[:, None, :].expand(B, HW, C))
    if post is not None and fault == "post_before_act":
        v = v + post.float()
    v = {R.ACT_NONE: lambda t: t, R.ACT_RELU: torch.relu, R.ACT_SILU: lambda t: (t.double() * torch.sigmoid(t.double())).float()}[act](v)
    if post is not None and fault != "post_before_act":
        v = v + post.float()
    return v.to(BF)


def gn_standin(x, w, b, G, eps, act=R.ACT_NONE, pre_add=None, post=None, fault=None):
    B, HW, C = x.shape
    z = x.float() if (pre_add is None or fault == "pre_add_not_in_stats") else x.float() + pre_add[:, None, :]
    a, q = gn_sums_standin(z, G)
    n = torch.tensor(float(HW), dtype=torch.float32) * torch.tensor(float(C // G), dtype=torch.float32)
    m = a / n
    var = (q / n - m * m).clamp_min(0.0)
    r = torch.rsqrt(var + torch.tensor(1e-5 if fault == "eps_1e-5" else eps, dtype=torch.float32))
    if fault == "bf16_mean":
        m = m.to(BF).float()
    if fault == "stats_of_previous_sample":
        m, r = torch.roll(m, 1, 0), torch.roll(r, 1, 0)
    return gn_apply_standin(x, (m, r), w, b, G, act, pre_add, post, fault)


def gn_from_moments_standin(x, mom, w, b, G, eps, act=R.ACT_NONE, pre_add=None, post=None):
    B, HW, C = x.shape
    n1 = torch.tensor(float(HW), dtype=torch.float32)
    v = torch.zeros((B, C)) if pre_add is None else pre_add
    s1, s2 = mom[..., 0], mom[..., 1]
    cs1 = fma32(n1.expand_as(v), v, s1)
    cs2 = fma32(n1 * v, v, fma32(2.0 * v, s1, s2))
    a, q = torch.zeros((B, G)), torch.zeros((B, G))
    for c in range(C // G):
        a, q = a + cs1.view(B, G, -1)[..., c], q + cs2.view(B, G, -1)[..., c]
    n = n1 * torch.tensor(float(C // G), dtype=torch.float32)
    m = a / n
    var = (q / n - m * m).clamp_min(0.0)
    return gn_apply_standin(x, (m, torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))), w, b, G, act, pre_add, post)


def gn_moments_standin(x):
    """x2i_groupnorm_moments_f32: per channel, slab by slab"""
    B, HW, C = x.shape
    per = (HW + R.GN_SLABS - 1) // R.GN_SLABS
    zp = F.pad(x.float(), (0, 0, 0, per * R.GN_SLABS - HW)).view(B, R.GN_SLABS, per, C)
    s, q = torch.zeros((B, R.GN_SLABS, C)), torch.zeros((B, R.GN_SLABS, C))
    for p in range(per):
        s, q = s + zp[:, :, p], fma32(zp[:, :, p], zp[:, :, p], q)
    a, b = torch.zeros((B, C)), torch.zeros((B, C))
    for sl in range(R.GN_SLABS):
        a, b = a + s[:, sl], b + q[:, sl]
    return torch.stack((a, b), -1)


GN_SHAPES = [(2, 2, 64, 32 * 40, R.ACT_RELU, 1e-5), (2, 32, 128, 700, R.ACT_SILU, 1e-6), (3, 8, 256, 255, R.ACT_NONE, 1e-5), (1, 32, 512, 1, R.ACT_SILU, 1e-6)]


@pytest.mark.parametrize("kind", R.GN_KINDS)
@pytest.mark.parametrize("B,G,C,HW,act,eps", GN_SHAPES)
def test_groupnorm_standin_passes(kind, B, G, C, HW, act, eps):
    x, pa = R.gn_input(kind, B, HW, C, G, gen(61))
    w, b = R.gn_affine(C, gen(62))
    post = torch.randn((B, HW, C), generator=gen(63)).to(BF) if C == 256 else None
    y = gn_standin(x, w, b, G, eps, act, pa, post)
    rep = R.Report(f"gn {kind}")
    info = R.check_groupnorm(rep, x, y, w, b, G, eps, act=act, pre_add=pa, post=post, rows=256)
    assert rep.done() <= 1.0
    if kind == "large_mean" and HW > 1:
        assert info["kappa"] >= 0.9 * R.LARGE_MEAN_KAPPA
    if kind == "const":
        assert bool(torch.isfinite(y.float()).all())
    # per-channel moments of x: against float64, and as the statistics operand of the from-moments form
    mom = gn_moments_standin(x)
    want, bound = R.gn_moments_expect(x)
    assert R.assert_entries(f"gn moments {kind}", mom, want, bound) <= 1.0
    y2 = gn_from_moments_standin(x, mom, w, b, G, eps, act, pa, post)
    rep = R.Report(f"gn from moments {kind}")
    R.check_groupnorm(rep, x, y2, w, b, G, eps, act=act, pre_add=pa, post=post, moments=mom, rows=256)
    assert rep.done() <= 1.0


def test_groupnorm_from_quad_moments_and_grouped_parameters():
    B, G, C, HW, wg = 4, 32, 128, 300, 2
    x, _ = R.gn_input("random", B, HW, C, G, gen(64))
    w, b = R.gn_affine(C, gen(65), groups=2)
    mom = moments_standin(x)                                  # the conv epilogue's layout: quad sums at c % 4 == 0, zeros elsewhere
    wz, bz = w[torch.arange(B) // wg], b[torch.arange(B) // wg]
    y = gn_from_moments_standin(x, mom, wz, bz, G, 1e-6, R.ACT_SILU)
    rep = R.Report("gn quad moments grouped")
    R.check_groupnorm(rep, x, y, w, b, G, 1e-6, act=R.ACT_SILU, moments=mom, w_group=wg)
    assert rep.done() <= 1.0
    wrong = gn_from_moments_standin(x, mom, w[(torch.arange(B) + 1) // wg % 2], b[(torch.arange(B) + 1) // wg % 2], G, 1e-6, R.ACT_SILU)
    rep = R.Report("gn group off by one")
    R.check_groupnorm(rep, x, wrong, w, b, G, 1e-6, act=R.ACT_SILU, moments=mom, w_group=wg)
    with pytest.raises(AssertionError, match=r"sample 1, pixel"):
        rep.done()


GN_FAULTS = {
    # fault: (kind, G, C, act, with post, the failure names)
    "bf16_mean": ("random", 32, 128, R.ACT_SILU, False, r"sample \d, pixel \d+, channel \d+, group \d+"),
    "group_boundary_shift": ("random", 32, 128, R.ACT_SILU, False, r"sample \d, pixel \d+, channel \d+, group \d+"),
    "pre_add_not_in_stats": ("random", 32, 128, R.ACT_SILU, False, r"sample \d, pixel"),
    "eps_1e-5": ("const", 32, 128, R.ACT_SILU, False, r"sample \d, pixel"),
    "stats_of_previous_sample": ("random", 32, 128, R.ACT_SILU, False, r"sample \d, pixel"),
    "post_before_act": ("random", 8, 256, R.ACT_RELU, True, r"sample \d, pixel"),
}


@pytest.mark.parametrize("fault", list(GN_FAULTS))
def test_groupnorm_fault_is_rejected(fault):
    kind, G, C, act, with_post, where = GN_FAULTS[fault]
    B, HW = 2, 600
    x, pa = R.gn_input(kind, B, HW, C, G, gen(71))
    if fault == "pre_add_not_in_stats":
        pa = pa * 0.05                   # a small time-embedding term: the statistics hardly move
    w, b = R.gn_affine(C, gen(72))
    post = torch.randn((B, HW, C), generator=gen(73)).to(BF) if with_post else None
    good = gn_standin(x, w, b, G, 1e-6, act, pa, post)
    bad = gn_standin(x, w, b, G, 1e-6, act, pa, post, fault=fault)
    rep = R.Report(fault)
    R.check_groupnorm(rep, x, good, w, b, G, 1e-6, act=act, pre_add=pa, post=post)
    rep.done()
    rep = R.Report(fault)
    R.check_groupnorm(rep, x, bad, w, b, G, 1e-6, act=act, pre_add=pa, post=post)
    with pytest.raises(AssertionError, match=where):
        rep.done()
    assert (rel_l2(bad, good) < R.OLD_GN_REL_L2) == ("gn_" + fault in OLD_MISSES), (fault, rel_l2(bad, good))


def test_variance_error_grows_with_kappa_as_derived():
    """E_v / var of the derived bound is proportional to kappa -- between D u kappa and (3 D + 16) u kappa: (D + 4) u Q from S2 and from the
    subtraction, 2 (D + 2) u m^2 from the mean -- and the one-pass stand-in stays inside it"""
    B, G, C, HW = 1, 2, 64, 4096
    for mean in (0.0, 8.0, 64.0, 512.0):
        x = (mean + torch.randn((B, HW, C), generator=gen(81))).to(BF)
        st = R.gn_stats(x[0], None, G)
        e_m, e_v = R.gn_stat_errors(st, HW, C, G, False)
        a, q = gn_sums_standin(x.float(), G)
        n = float(HW * C // G)
        m = a[0].double() / n
        var32 = (q[0].double() / n - m * m).clamp_min(0)
        assert bool(((var32 - st["var"]).abs() <= e_v).all()), (mean, var32, st["var"], e_v)
        D = R.gn_chain(HW, C, G)
        assert bool((e_v / st["var"] <= (3 * D + 16) * U_F32 * st["kappa"] * 1.01).all())
        assert bool((e_v / st["var"] >= D * U_F32 * st["kappa"]).all())
