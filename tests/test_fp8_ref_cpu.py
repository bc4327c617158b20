"""The e4m3 checker of tests/fp8_ref.py, without a GPU: its e4m3 arithmetic against torch's float8_e4m3fn, an f32 torch emulation of each
kernel (x2i_gemm_fp8 with its epilogues, x2i_ln_modulate_fp8, x2i_quantize_rows_fp8) that must pass, and planted faults that must fail with a
message naming the tile, row or element.  For every fault the old bounds of tests/test_fp8_gpu.py (whole-output rel-L2 < 4e-3, share of
differing codes < 2e-3, rtol 1e-4 on scales) are evaluated too and printed: several faults pass them.

Two remarks on what a fault can show.  (1) The old tests start their outputs as zeros: the "element left unwritten" fault is judged by the
old bound with a zero in that place, by the new check with the sentinel.  (2) While delta > 0 an exact tie of the f32 value is a two-valued
interval, so the direction of ties cannot be judged on a GEMM output; it is judged where the arithmetic is exact, on the quantise kernel's
`midpoints` row (scale exactly 1, every e4m3 midpoint as a bf16 element)."""
import math

import pytest
import torch

from tests import ew_ref as E
from tests import fp8_ref as R
from tests import gemm_ref as G
from tests.util import rel_l2

M, N, K, BATCH = 300, 520, 256, 3
FP8 = torch.float8_e4m3fn


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- e4m3 arithmetic
def test_decode_table_equals_torch_on_every_finite_code():
    c = torch.arange(256, dtype=torch.uint8)
    fin = (c & 0x7F) != 0x7F
    assert int(fin.sum()) == 254
    assert torch.equal(R.decode(c)[fin], c.view(FP8).double()[fin])
    assert bool(torch.isnan(R.decode(c)[~fin]).all())
    assert torch.equal(R.e4m3_rne_sat(R.decode(c)[fin], codes=True), c[fin])          # (codes round-trip, -0 included)


def test_ulp_e4m3():
    x = torch.tensor([0.0, 2.0 ** -9, 2.0 ** -7, 2.0 ** -6, 0.0234375, 1.0, 1.875, 2.0, 448.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 0.125, 0.125, 0.25, 32.0, 0.25], dtype=torch.float64)
    assert torch.equal(R.ulp_e4m3(x), want)


def torch_codes(x32):
    return x32.clamp(-448, 448).to(FP8).view(torch.uint8)


def test_rne_sat_equals_torch_on_codes_midpoints_their_neighbours_and_random_values():
    c = torch.arange(127, dtype=torch.uint8)                       # +0 .. 448
    v = R.decode(c)
    mid = 0.5 * (v[1:] + v[:-1])                                   # (exact in f32: one bit more than e4m3)
    m32 = mid.float()
    assert torch.equal(m32.double(), mid)
    up, dn = torch.nextafter(m32, torch.tensor(math.inf)), torch.nextafter(m32, torch.tensor(-math.inf))
    edge = torch.tensor([448.0, 464.0, 463.99997, 464.00003, 480.0, 1e4, 3e38, 2.0 ** -10, 2.0 ** -11, 1e-30])
    rnd = torch.cat((torch.randn(50000, generator=gen(1)) * 100, torch.randn(50000, generator=gen(2)) * 0.05))
    x = torch.cat((v.float(), m32, up, dn, edge, rnd))
    x = torch.cat((x, -x))
    assert torch.equal(R.e4m3_rne_sat(x.double(), codes=True), torch_codes(x))
    assert torch.equal(R.e4m3_rne_sat(x.double()), torch_codes(x).view(FP8).double())
    # ties go to even: every midpoint lands on the neighbour with an even mantissa
    assert bool((R.e4m3_rne_sat(mid, codes=True) & 1 == 0).all())


# ---------------------------------------------------------------------------------------------------------------- GEMM emulation
def fma32(a, b, c):
    """f32 fma of f32 tensors (through float64: a * b is exact there)"""
    return (a.double() * b.double() + c.double()).float()


def gelu32(x):
    """gelu_tanh_f (csrc/x2i_common.h): x / (1 + exp2(x (a + b x^2))), in f32"""
    return x / (1.0 + torch.exp2(x * (x * x * -0.10294324 - 2.3022082)))


def emu_gemm(A8, W8, bias, sa, sw, alpha, *, act=0, gate=None, res=None, out_fp8=False, oinv=1.0, acc_hook=None, pre_round=None,
             convert=None):
    """x2i_gemm_fp8 of one item in f32, spelled as the kernels spell it: the exact accumulator rounded to f32, acc * (w_scale * alpha), the
    fma with a_scale and bias, the activation, fmaf(gate, v, res), then bf16 or clamp + e4m3.  Hooks plant faults."""
    acc = R.decode(A8) @ R.decode(W8).T
    if acc_hook:
        acc = acc_hook(acc)
    acc = acc.float()
    swa = (sw if sw is not None else torch.ones(W8.shape[0])) * torch.tensor(alpha, dtype=torch.float32)
    s = sa if sa is not None else torch.ones(A8.shape[0])
    b = bias.float() if bias is not None else torch.zeros(W8.shape[0])
    x = fma32(acc * swa[None, :], s[:, None].expand_as(acc), b[None, :].expand_as(acc))
    if act == G.ACT_GELU_TANH:
        x = gelu32(x)
    if res is not None:
        x = fma32(gate[None, :].expand_as(x), x, res.float())
    if not out_fp8:
        return x.bfloat16()
    if oinv != 1.0:
        x = x * torch.tensor(oinv, dtype=torch.float32)
    if pre_round:
        x = pre_round(x)
    return convert(x) if convert else torch_codes(x)


@pytest.fixture(scope="module")
def prob():
    """operands of every kind at M, N, K = 300, 520, 256, batch 3, with tagged scales (a_scale [3, 300] differs between rows, rows 16 apart and
    items) and a bias"""
    out = {}
    ba, bw = R.unit_bases(K)
    for i, kind in enumerate(R.KINDS):
        g = gen(10 + i)
        A8, W8 = R.operands(M, N, K, kind, g, "cpu", batch=BATCH)
        sa, sw = R.tag_scales8(M, N, BATCH, "cpu", ba, bw)
        bias = (0.5 * torch.randn(N, generator=g)).bfloat16()
        out[kind] = dict(A8=A8, W8=W8, sa=sa, sw=sw, bias=bias, gate=torch.randn((BATCH, N), generator=g),
                         res=(2 * torch.randn((BATCH, M, N), generator=g)).bfloat16())
    return out


EPILOGUES = {"plain_unit": dict(scales=False, bias=False), "bias_scales": dict(), "gelu_bf16": dict(act=G.ACT_GELU_TANH),
             "gelu_e4m3_1": dict(act=G.ACT_GELU_TANH, out_fp8=True, oinv=1.0), "gelu_e4m3_075": dict(act=G.ACT_GELU_TANH, out_fp8=True, oinv=0.75),
             "gelu_e4m3_64": dict(act=G.ACT_GELU_TANH, out_fp8=True, oinv=64.0), "gated": dict(alpha=1.25, gated=True)}


def run(p, epi, fault=None, n=N):
    """Emulate one batched launch (with `fault` planted) and check it.  Returns (Report, got [batch, M, n], reference f32 [batch, M, n])."""
    e = dict(scales=True, bias=True, act=0, out_fp8=False, oinv=1.0, alpha=1.0, gated=False)
    e.update(EPILOGUES[epi])
    fault = fault or {}
    A8, W8 = p["A8"], p["W8"][:n]
    sa, sw = (p["sa"], p["sw"][:n]) if e["scales"] else (None, None)
    bias = p["bias"][:n] if e["bias"] else None
    gate, res = (p["gate"][:, :n], p["res"][:, :, :n]) if e["gated"] else (None, None)
    outs = []
    for z in range(BATCH):
        kw = dict(act=e["act"], gate=gate[z] if e["gated"] else None, res=res[z] if e["gated"] else None, out_fp8=e["out_fp8"], oinv=e["oinv"])
        A_used = fault["A"](A8[z]) if "A" in fault else A8[z]
        sa_used = None if sa is None else (fault["sa"](sa, z) if "sa" in fault else sa[z])
        alpha_used = fault.get("alpha", e["alpha"])
        kw.update({k: fault[k] for k in ("acc_hook", "pre_round", "convert") if k in fault and fault.get("item", z) == z})
        outs.append(emu_gemm(A_used, W8, bias, sa_used, sw, alpha_used, **kw))
    got = torch.stack(outs)
    if "out" in fault:
        fault["out"](got)
    rep = R.Report(f"emulation {epi}")
    R.check_gemm8(rep, A8, W8, bias, got, a_scale=sa, w_scale=sw, alpha=e["alpha"], act=e["act"], gate=gate, res=res, out_fp8=e["out_fp8"],
                  out_inv_scale=e["oinv"])
    # what the old test compares with: an f32 matmul of the dequantised operands, the epilogue in f32
    ref = []
    for z in range(BATCH):
        a = A8[z].view(FP8).float() * (sa[z][:, None] if sa is not None else 1.0)
        w = W8.view(FP8).float() * (sw[:, None] if sw is not None else 1.0)
        r = e["alpha"] * (a @ w.T) + (bias.float() if bias is not None else 0.0)
        r = gelu32(r) if e["act"] else r
        ref.append(res[z].float() + gate[z] * r if e["gated"] else r)
    return rep, got, torch.stack(ref), e


def old_bounds_pass(got, ref, e):
    """tests/test_fp8_gpu.py on this output (an unwritten element as that test's zero-filled output shows it)"""
    if e["out_fp8"]:
        g = got.clone()
        g[(g & 0x7F) == 0x7F] = 0
        want8 = (ref * e["oinv"]).clamp(-448, 448).to(FP8)
        mism = float((g != want8.view(torch.uint8)).float().mean())
        return mism < R.OLD_CODE_MISMATCH and rel_l2(g.view(FP8).float(), (ref * e["oinv"]).clamp(-448, 448)) < R.OLD_E4M3_REL_L2
    g = torch.where(G.sentinel_bits(got), torch.zeros_like(got), got)
    return rel_l2(g, ref) < R.OLD_GEMM_REL_L2


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("epi", list(EPILOGUES))
def test_emulated_gemm_passes(prob, kind, epi):
    rep, got, ref, e = run(prob[kind], epi)
    worst = rep.done()
    assert worst < 1.0
    assert old_bounds_pass(got, ref, e) or kind != "random"      # (`cancel` and `tagged` outputs are not what a whole-output norm suits)
    print(f"\n  {epi} {kind}: share of the f32 allowance {worst:.3f}, two-valued e4m3 intervals {rep.two_share():.4f}")


def test_cancel_kind_cancels(prob):
    a, w = R.decode(prob["cancel"]["A8"][0]), R.decode(prob["cancel"]["W8"])
    lin, mag = a @ w.T, a.abs() @ w.abs().T
    assert float((lin.abs() / mag).median()) < 2e-3
    t = R.k_tags(1024, "cpu")
    assert int(t.min()) == -3 and int(t.max()) == 3 and len({int(v) for v in t[::128]}) == 5


# ---------------------------------------------------------------------------------------------------------------- planted GEMM faults
def swap_k_groups(A):
    g = A.view(A.shape[0], -1, 16).clone()
    g[:, 0::2], g[:, 1::2] = A.view(A.shape[0], -1, 16)[:, 1::2], A.view(A.shape[0], -1, 16)[:, 0::2]
    return g.view(A.shape)


def ktile_hook(p, sign):
    """one K-tile (k 128..255) dropped (-1) or counted twice (+1) in the 256^2 tile (1, 2) of item 1"""
    def hook(acc):
        a, w = R.decode(p["A8"][1][256:, 128:]), R.decode(p["W8"][512:, 128:])
        acc = acc.clone()
        acc[256:, 512:] += sign * (a @ w.T)
        return acc
    return hook


def sa_one_row(sa, z):
    s = sa[z].clone()
    if z == 2:
        s[37] *= 1.125
    return s


def set_sentinel(got):
    if got.dtype == torch.uint8:
        got[2, M - 1, -1] = R.SENTINEL8
    else:
        got.view(torch.int16)[2, M - 1, -1] = G.SENTINEL16


def truncate(x):
    xc = x.double().clamp(-448, 448)
    u = R.ulp_e4m3(xc)
    return R.e4m3_rne_sat(torch.trunc(xc / u) * u, codes=True)


def no_clamp_once(x):
    c = torch_codes(x)
    i = int(torch.argmax(x))
    assert float(x.view(-1)[i]) > 480
    c.view(-1)[i] = 0x7F                        # e4m3(x) of an unclamped x >= 480: NaN
    return c


GEMM_FAULTS = {
    # name: (epilogue, kind, fault, what the message must name)
    "A k-groups permuted": ("bias_scales", "random", lambda p: dict(A=swap_k_groups), "tile (0, 0)"),
    "a_scale of row m + 16": ("bias_scales", "tagged", lambda p: dict(sa=lambda sa, z: torch.roll(sa[z], -16)), "item 0: tile ("),
    "a_scale of the previous item": ("bias_scales", "tagged", lambda p: dict(sa=lambda sa, z: sa[z - 1]), "item 0"),
    "a_scale of one row off by 1 + 1/8": ("bias_scales", "random", lambda p: dict(sa=sa_one_row), "item 2: tile (0, "),
    "alpha applied twice": ("gated", "random", lambda p: dict(alpha=1.25 * 1.25), "tile (0, 0)"),
    "one K-tile dropped in one tile": ("bias_scales", "random", lambda p: dict(acc_hook=ktile_hook(p, -1), item=1), "item 1: tile (1, 2)"),
    "one K-tile counted twice in one tile": ("bias_scales", "random", lambda p: dict(acc_hook=ktile_hook(p, 1), item=1), "item 1: tile (1, 2)"),
    "one element left at the sentinel": ("bias_scales", "random", lambda p: dict(out=set_sentinel), f"(m={M - 1}, n={N - 1})"),
    "one e4m3 element left at the sentinel": ("gelu_e4m3_1", "random", lambda p: dict(out=set_sentinel), f"(m={M - 1}, n={N - 1})"),
    "e4m3 output truncated": ("gelu_e4m3_075", "random", lambda p: dict(convert=truncate), "tile (0, 0)"),
    "clamp missing on one element": ("gelu_e4m3_64", "random", lambda p: dict(convert=no_clamp_once, item=1), "item 1: tile"),
    "bf16 rounding before the e4m3 rounding": ("gelu_e4m3_1", "random", lambda p: dict(pre_round=lambda x: x.bfloat16().float()), "tile ("),
}
# faults that the old whole-output bounds let through (asserted; the others are printed)
OLD_BOUNDS_MISS = {"a_scale of one row off by 1 + 1/8", "one element left at the sentinel", "one e4m3 element left at the sentinel",
                   "clamp missing on one element"}


@pytest.mark.parametrize("name", list(GEMM_FAULTS))
def test_planted_gemm_fault_fails_and_is_named(prob, name):
    epi, kind, make, names = GEMM_FAULTS[name]
    p = prob[kind]
    rep, got, ref, e = run(p, epi, make(p))
    with pytest.raises(AssertionError) as err:
        rep.done()
    msg = str(err.value)
    old = old_bounds_pass(got, ref, e)
    print(f"\n  {name}: old bounds {'PASS' if old else 'fail'}; new: {msg[:230]}")
    assert names in msg, msg
    if name in OLD_BOUNDS_MISS:
        assert old


# ---------------------------------------------------------------------------------------------------------------- fused QKV emulation
def emu_qkv(A8, W8, bias, sa, sw, nq, nk, cos, sin, Q, K, VT, *, z, H, tok_off, rps, q_scale, vt_perm, eps=1e-6):
    """x2i_gemm_qkv_fp8 of batch item z in f32: the dequantised accumulator (emu_gemm), x = bf16 of it, RMSNorm * w * q_scale and the
    interleaved-pair rotation as norm_rope8 spells them, written into Q / K / VT"""
    m = A8.shape[0]
    x = emu_gemm(A8, W8, bias, sa, sw, 1.0).float().view(m, 3, H, 128)
    b, s = G.tokens_of(torch.arange(m), z, tok_off, rps)
    c, sn = cos[s], sin[s]
    for sec, w, dst in ((0, nq.float() * torch.tensor(q_scale, dtype=torch.float32), Q), (1, nk.float(), K)):
        xs = x[:, sec]
        a = xs * torch.rsqrt((xs * xs).sum(-1, keepdim=True) / 128 + eps) * w
        o = torch.empty_like(a)
        o[..., 0::2] = (a[..., 0::2].double() * c[:, None, 0::2] - (a[..., 1::2] * sn[:, None, 0::2]).double()).float()
        o[..., 1::2] = (a[..., 1::2].double() * c[:, None, 1::2] + (a[..., 0::2] * sn[:, None, 1::2]).double()).float()
        dst[b, :, s, :] = o.bfloat16()
    VT[b, :, :, G.vt_pos(s, vt_perm)] = x[:, 2].bfloat16()


@pytest.mark.parametrize("fault", [None, "a_scale of row m + 16"])
@pytest.mark.parametrize("kind,vt_perm", [("random", False), ("tagged", True)])
def test_emulated_qkv_passes_and_a_row_scale_fault_is_named(kind, vt_perm, fault):
    """batched image rows: batch 2, Si = 300 behind 128 text tokens, H = 2, K = 256, q_scale = 0.1275"""
    H, Kq, batch, Si, tok_off, Spad = 2, 256, 2, 300, 128, 512
    g = gen(60)
    A8, W8 = R.operands(Si, 3 * H * 128, Kq, kind, g, "cpu", batch=batch)
    ba, bw = R.unit_bases(Kq)
    sa, sw = R.tag_scales8(Si, 3 * H * 128, batch, "cpu", ba, bw)
    bias = (0.5 * torch.randn(3 * H * 128, generator=g)).bfloat16()
    nq, nk = ((1 + 0.1 * torch.randn(128, generator=g)).bfloat16() for _ in range(2))
    ang = torch.randn((tok_off + Si, 64), generator=g) * 3
    cos, sin = torch.cos(ang).repeat_interleave(2, 1).contiguous(), torch.sin(ang).repeat_interleave(2, 1).contiguous()
    Q, K_, VT = (G.poison_(torch.empty(sh, dtype=torch.bfloat16)) for sh in ((batch, H, Spad, 128), (batch, H, Spad, 128), (batch, H, 128, Spad)))
    for z in range(batch):
        emu_qkv(A8[z], W8, bias, torch.roll(sa[z], -16) if fault and z == 1 else sa[z], sw, nq, nk, cos, sin, Q, K_, VT, z=z, H=H, tok_off=tok_off,
                rps=Si, q_scale=0.1275, vt_perm=vt_perm)
    rep = R.check_qkv8(R.Report(f"emulated qkv {kind}"), A8, W8, bias, nq, nk, cos, sin, Q, K_, VT, H=H, tok_off=tok_off, rows_per_sample=Si, a_scale=sa,
                       w_scale=sw, q_scale=0.1275, vt_perm=vt_perm)
    G.check_qkv_padding("emulated qkv", Q, K_, VT, tok_off + Si, vt_perm)
    assert bool(G.sentinel_bits(Q[:, :, :tok_off]).all())
    if fault is None:
        assert rep.done() < 1.0
        return
    with pytest.raises(AssertionError) as err:
        rep.done()
    assert "item 1" in str(err.value) and "sample 1, head" in str(err.value), str(err.value)
    print(f"\n  qkv, {fault}: {str(err.value)[:230]}")


# ---------------------------------------------------------------------------------------------------------------- quantise: ties
def midpoints_row():
    """bf16 row with amax exactly 448 (scale exactly 1) and every e4m3 midpoint of both signs (all bf16 values: at most 5 significant bits)"""
    v = R.decode(torch.arange(127, dtype=torch.uint8))
    mid = 0.5 * (v[1:] + v[:-1])
    row = torch.cat((torch.tensor([448.0], dtype=torch.float64), mid, -mid, torch.zeros(3, dtype=torch.float64)))
    assert row.numel() % 8 == 0 and torch.equal(row.bfloat16().double(), row)
    return row.bfloat16()


def test_quantize_expect_equals_torch_and_catches_ties_away_from_zero():
    x = (3 * torch.randn((400, 256), generator=gen(3))).bfloat16()
    x[0] = midpoints_row()
    x[1] = 0
    codes, s = R.quantize_expect(x)
    amax = x.float().abs().amax(1)
    want_s = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    assert torch.equal(s, want_s) and float(s[0]) == 1.0 and float(s[1]) == 1.0
    assert torch.equal(codes, (x.float() * (1.0 / want_s)[:, None]).clamp(-448, 448).to(FP8).view(torch.uint8))
    assert bool((codes[0, 1:253] & 1 == 0).all())                   # every tie went to the even code
    # the fault: ties rounded away from zero.  One row of 400: the exact ties are 252 / 102400 of the elements; half of them change, about 1e-3
    xs = (x.float() * (1.0 / want_s)[:, None]).double()              # (the kernel's f32 product; exact on row 0)
    u = R.ulp_e4m3(xs.clamp(-448, 448))
    away = codes.clone()                                            # (planted on the midpoints row only: ordinary rows hold exact ties too)
    away[0] = R.e4m3_rne_sat(torch.sign(xs[0]) * torch.floor(xs[0].abs().clamp(max=448) / u[0] + 0.5) * u[0], codes=True)
    share = float((away != codes).float().mean())
    assert 0 < share < R.OLD_CODE_MISMATCH                          # the old "share of differing codes" bound lets it through
    assert rel_l2(away.view(FP8).float(), codes.view(FP8).float()) < R.OLD_E4M3_REL_L2
    assert not torch.equal(away, codes)                             # the bit-exact comparison does not
    bad = torch.nonzero(away != codes)
    assert int((bad[:, 0] == 0).sum()) == 126                       # ... and names row 0, the midpoints row: every second tie
    print(f"\n  ties away from zero: {share:.2e} of the codes differ (old bound {R.OLD_CODE_MISMATCH}): old bounds PASS, new fails")


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def emu_ln(X3, S0, sh0, sc0, sh1, sc1, eps, fault=None):
    """x2i_ln_modulate_fp8 in f32 (ln_fp8_kernel's statements; the sums in float64, rounded): (Y bf16, codes, row scales)"""
    B, S, D = X3.shape
    x = X3.float()
    mean = (x.double().sum(-1, keepdim=True).float() / D)
    d = x - mean
    var = (d.double() * d.double()).sum(-1, keepdim=True).float() / D
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    side0 = (torch.arange(S) < S0)[None, :, None]
    if fault == "wrong stream at S0":
        side0 = (torch.arange(S) <= S0)[None, :, None]
    sh = torch.where(side0, sh0[:, None, :D], sh1[:, None, :D])
    sc = torch.where(side0, sc0[:, None, :D], sc1[:, None, :D])
    y = fma32(d * rstd, (1.0 + sc).expand_as(d), sh.expand_as(d))
    amax = (y[..., :512] if fault == "amax over 512 columns" else y).abs().amax(-1)
    rs = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
    inv = 1.0 / rs
    if fault == "neighbouring row's scale":
        inv = torch.roll(inv, -1, 1)
    return y.bfloat16(), torch_codes(y * inv[..., None]), rs.reshape(-1)


def ln_problem(D, kind, seed):
    B, S, S0 = 2, 9, 4
    g = gen(seed)
    X = E.ln_rows(B * S, D, kind, g, "cpu").view(B, S, D)
    mod = E.mod_vectors(B * 4 * D, kind, g, "cpu").view(B, 4 * D)
    if kind == "const":
        mod[0, :D] = 0                                               # sample 0, stream 0: a constant row with zero shift -> scale 1, zero codes
    return X, S0, (mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:3 * D], mod[:, 3 * D:])


@pytest.mark.parametrize("D", [520, 3072])
@pytest.mark.parametrize("kind", E.LN_KINDS)
def test_emulated_ln_passes(D, kind):
    X, S0, mods = ln_problem(D, kind, 40)
    Y, Y8, rs = emu_ln(X, S0, *mods, 1e-6)
    rep = R.check_ln8(R.RowReport(f"emulated ln {kind} D={D}"), X, Y, Y8, rs, S0, *mods, 1e-6)
    assert rep.done() < 1.0 and rep.rs_worst <= 1.0
    if kind == "const":
        assert float(rs[0]) == 1.0 and int(Y8[0, 0].max()) & 0x7F == 0                  # (row 0 of sample 0: constant, zero shift)
        assert float(R.decode(Y8[0, 6]).abs().max()) == 448.0                              # (a constant row with a shift: exact +-448)
    print(f"\n  ln {kind} D={D}: Y share {rep.worst:.3f}, row scale {rep.rs_worst:.3f}, two-valued {rep.two_share():.4f}")


@pytest.mark.parametrize("fault,names", [("wrong stream at S0", "row (token) 4"), ("neighbouring row's scale", "e4m3"),
                                         ("amax over 512 columns", "row_scale")])
def test_planted_ln_fault_fails_and_is_named(fault, names):
    D = 3072
    X, S0, mods = ln_problem(D, "random", 41)
    Y, Y8, rs = emu_ln(X, S0, *mods, 1e-6, fault)
    Yc, Y8c, rsc = emu_ln(X, S0, *mods, 1e-6)
    rep = R.check_ln8(R.RowReport(f"ln, {fault}"), X, Y, Y8, rs, S0, *mods, 1e-6)
    with pytest.raises(AssertionError) as err:
        rep.done()
    msg = str(err.value)
    old = bool(torch.allclose(rs, rsc, rtol=R.OLD_SCALE_RTOL)) and rel_l2(Y8.view(FP8).float() * rs.view(2, -1, 1),
                                                                         Y8c.view(FP8).float() * rsc.view(2, -1, 1)) < R.OLD_LN_CODES_REL_L2
    print(f"\n  {fault}: old bounds {'PASS' if old else 'fail'}; new: {msg[:230]}")
    assert names in msg and "sample" in msg, msg


# ---------------------------------------------------------------------------------------------------------------- attention interval, sentinels
def test_attention_interval_and_byte_sentinels():
    o = (torch.randn(20000, generator=gen(5)) * 2)
    O = o.bfloat16()
    for oinv in (1.0, 2000.0):
        lo, hi = R.attn8_interval(O, oinv)
        got = R.decode(torch_codes(o * oinv))
        assert bool(((lo <= got) & (got <= hi)).all())
        wrong = R.decode(truncate(o * oinv))
        assert not bool(((lo <= wrong) & (wrong <= hi)).all())
    buf = R.poison_(torch.empty(64, dtype=FP8))
    assert bool(R.sentinel_bits(buf).all()) and bool(torch.isnan(R.decode(buf)).all())
    mask = G.write_mask(buf.view(torch.uint8), [((2, 8), (16, 1), 4)])
    buf.view(torch.uint8).as_strided((2, 8), (16, 1), 4).fill_(0)
    R.check_untouched("bytes", buf.view(torch.uint8), mask, row_len=16)
    buf.view(torch.uint8)[13] = 0
    with pytest.raises(AssertionError, match="row 0, col 13"):
        R.check_untouched("bytes", buf.view(torch.uint8), mask, row_len=16)
