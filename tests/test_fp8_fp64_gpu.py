"""The e4m3 kernels against the float64 reference of tests/fp8_ref.py, element by element: x2i_gemm_fp8 in its three forms (one-tile 7256,
persistent 8256, stream-K 9256; read back through last_gemm_tile) with every epilogue, x2i_gemm_qkv_fp8, x2i_ln_modulate_fp8 in both forms,
x2i_quantize_rows_fp8 bit for bit, and x2i_attention_e4m3out.  Every output starts as the sentinel (0x7F bytes / 0x7F7F bf16), every element
is checked, and nothing outside a launch's write set may change.  Operands are made here as e4m3 codes (fp8_ref.operands): no GEMM test
depends on the quantise kernel.

Shapes are the smallest at which each form exists (plan_gemm_fp8 / streamk_for at 256 CUs: persistent from K = 384; stream-K with more than
256 tiles, K / 128 >= 16 and a remainder r with 2 r >= 256); tests/test_gemm_plan_cpu.py pins the same table without a GPU.  Each test
prints the worst share of the f32 allowance its launches used and, for e4m3 outputs, the share of two-valued intervals (information)."""
import math

import pytest
import torch

from tests import ew_ref as E
from tests import fp8_ref as R
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
ALL, TWO = R.KINDS, ("random", "cancel")

# id: (M, N, K, batch, option, value, form, kinds) -- the kernel form of every launch is asserted
GEMM_ROWS = {
    "one_ktile": (300, 520, 128, 1, None, None, 7256, ALL),
    "one_tile_k256": (300, 520, 256, 1, None, None, 7256, ALL),
    "one_tile_k384": (300, 520, 384, 1, "gemm_fp8_persist", 0, 7256, ALL),
    "persistent_k384": (300, 520, 384, 1, None, None, 8256, ALL),
    "batched_one_tile": (300, 520, 384, 3, "gemm_fp8_persist", 0, 7256, ALL),
    "batched_persistent": (300, 520, 384, 3, None, None, 8256, ALL),
    "second_tile_walk": (4136, 3856, 512, 1, None, None, 8256, ALL),          # 17 x 16 = 272 tiles: 16 workgroups walk a second tile
    "stream_k": (5928, 3856, 2048, 1, None, None, 9256, TWO),                 # 24 x 16 = 384 tiles, remainder 128, 16 K-tiles, ragged M and N
    "half_filled_round": (5928, 3856, 2048, 1, "gemm_streamk", 0, 8256, TWO),
}
# name: (scales and bias, act, out_fp8, out_inv_scale, alpha, gated)
EPILOGUES = {
    "plain_unit": (False, G.ACT_NONE, False, 1.0, 1.0, False),
    "bias_scales": (True, G.ACT_NONE, False, 1.0, 1.0, False),
    "gelu_bf16": (True, G.ACT_GELU_TANH, False, 1.0, 1.0, False),
    "gelu_e4m3_1": (True, G.ACT_GELU_TANH, True, 1.0, 1.0, False),
    "gelu_e4m3_075": (True, G.ACT_GELU_TANH, True, 0.75, 1.0, False),
    "gelu_e4m3_64": (True, G.ACT_GELU_TANH, True, 64.0, 1.0, False),          # clamps many elements
    "gated_residual": (True, G.ACT_NONE, False, 1.0, 1.25, True),
}
A_ROWS, A_OFF = 428, 128          # batched geometry: M image rows behind a 128-row offset in a [batch, 428, K] buffer
ACC = {}                          # (row id, kind) -> worst (|err| - rounding)+ / mag of the launch with unit scales: the U_ACC8 measurement


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture
def opt(ops):
    from x2i_amd import _lib
    saved = {}

    def set_(name, value):
        old = _lib.set_option(name, value)
        saved.setdefault(name, old)
    yield set_
    for k, v in saved.items():
        _lib.set_option(k, v)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


_operands = {}


def operands(M, N, K, batch, kind):
    """fp8_ref.operands, kept for the launches of one shape (the epilogues of a row share them)"""
    key = (M, N, K, batch)
    if _operands.get("key") != key:
        _operands.clear()
        _operands["key"] = key
    if kind not in _operands:
        _operands[kind] = R.operands(M, N, K, kind, gen(100 + R.KINDS.index(kind)), DEV, batch=batch)
    return _operands[kind]


def scales_for(kind, M, N, K, batch, g):
    ba, bw = R.unit_bases(K)
    return R.tag_scales8(M, N, batch, DEV, ba, bw) if kind == "tagged" else R.random_scales(M, N, batch, g, DEV, ba, bw)


def a_buffer(A8, batch):
    """A as the launch reads it: contiguous [M, K], or rows A_OFF.. of a [batch, A_ROWS, K] buffer (the other rows hold 448).  Returns
    (buffer, launch keywords)"""
    _, M, K = A8.shape
    if batch == 1:
        return A8[0].contiguous(), {}
    buf = torch.full((batch, A_ROWS, K), 0x7E, dtype=torch.uint8, device=DEV)
    buf[:, A_OFF:A_OFF + M] = A8
    return buf, dict(batch=batch, a_batch_stride=A_ROWS * K, lda=K, a_offset=A_OFF * K)


def gemm_n(N, out8):
    """N = 528 instead of 520 where out_fp8 needs N % 16 == 0"""
    return 528 if (out8 and N == 520) else N


def run_gemm(ops, row, epi, kind, seed):
    """One x2i_gemm_fp8 launch of GEMM_ROWS[row] with EPILOGUES[epi] on `kind` operands, checked.  Returns (form, Report)."""
    from x2i_amd import _lib
    M, N, K, batch = GEMM_ROWS[row][:4]
    scaled, act, out8, oinv, alpha, gated = EPILOGUES[epi]
    N, Nfull = gemm_n(N, out8), gemm_n(N, True)
    g = gen(seed)
    A8, W8 = operands(M, Nfull, K, batch, kind)
    W8 = W8[:N]
    sa, sw = scales_for(kind, M, N, K, batch, g) if scaled else (None, None)
    bias = (0.5 * torch.randn(N, device=DEV, generator=g)).bfloat16() if scaled else None
    Abuf, akw = a_buffer(A8, batch)
    ldc, c_off = N + 16, 32
    c_bs = M * ldc + 64 if batch > 1 else 0
    cbuf = R.poison_(torch.empty(c_off + (batch - 1) * c_bs + M * ldc + 48, device=DEV, dtype=torch.uint8 if out8 else torch.bfloat16))
    view = ((batch, M, N), (c_bs, ldc, 1), c_off)
    C3 = cbuf.as_strided(*view)
    kw = dict(akw, M=M, N=N, K=K, a_scale=sa, a_scale_batch_stride=M if (batch > 1 and sa is not None) else 0, w_scale=sw, alpha=alpha,
              c_batch_stride=c_bs, ldc=ldc, c_offset=c_off, act=act, out_fp8=out8, out_inv_scale=oinv)
    gate = res = None
    if gated:
        gate = torch.randn((batch, N), device=DEV, generator=g)
        C3.copy_((2.0 * torch.randn((batch, M, N), device=DEV, generator=g)).bfloat16())
        res = C3.clone()
        kw.update(res=cbuf, res_batch_stride=c_bs, ldr=ldc, res_offset=c_off, gate=gate, gate_batch_stride=N)
    ops.gemm_fp8(Abuf.view(FP8), W8.view(FP8), bias, out=cbuf.view(FP8) if out8 else cbuf, **kw)
    form = int(_lib.get_option("last_gemm_tile"))
    torch.cuda.synchronize()
    rep = R.Report(f"{row} {epi} {kind}")
    R.check_gemm8(rep, A8, W8, bias, C3, a_scale=sa, w_scale=sw, alpha=alpha, act=act, gate=gate, res=res, out_fp8=out8, out_inv_scale=oinv)
    R.check_untouched(f"{row} {epi} {kind}", cbuf, G.write_mask(cbuf, [view]), row_len=None)
    if epi == "plain_unit":
        ACC[row, kind] = max(R.acc_share(A8[z], W8, C3[z]) for z in range(batch))
    return form, rep


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("row", list(GEMM_ROWS))
def test_gemm_fp8_vs_fp64(ops, opt, row, epi):
    name, value, want_form, kinds = GEMM_ROWS[row][4:]
    if name:
        opt(name, value)
    line = []
    for kind in kinds:               # (back to back: a stream-K launch follows one of its own geometry on other inputs -- a stale slab or flag shows)
        form, rep = run_gemm(ops, row, epi, kind, seed=7 + R.KINDS.index(kind))
        assert form == want_form, (row, epi, kind, form, want_form)
        worst = rep.done()
        assert worst < 1.0
        line.append(f"{kind} two-valued intervals {rep.two_share():.4f}" if rep.n else f"{kind} {worst:.3f}")
    ops.streamk_check(sync=True)
    print(f"\n  {row} {epi}: form {want_form}; " + ("" if EPILOGUES[epi][2] else "share of the f32 allowance: ") + ", ".join(line)
          + (f"; accumulation error / mag: " + ", ".join(f"{k} {ACC[row, k]:.3e}" for k in kinds) + f" (U_ACC8 = {R.U_ACC8:.3e})"
             if epi == "plain_unit" else ""))


# ---------------------------------------------------------------------------------------------------------------- fused QKV
def run_qkv(ops, geom, K, kind, vt_perm, pair, H=2, M_big=None):
    from x2i_amd import _lib
    g = gen(31 + R.KINDS.index(kind))
    if geom == "batched":            # image rows of a [2, 428, K] activation behind a 128-token text offset
        batch, M, tok_off, rps, B, S = 2, 300, A_OFF, 300, 2, A_ROWS
    elif geom == "flat":             # the flattened single-block rows
        batch, M, tok_off, rps, B, S = 1, 2 * A_ROWS, 0, A_ROWS, 2, A_ROWS
    else:
        batch, M, tok_off, rps, B, S = 1, M_big, 0, M_big, 1, M_big
    N, Spad = 3 * H * 128, ops.pad128(S)
    A8, W8 = operands(M, N, K, batch, kind)
    sa, sw = scales_for(kind, M, N, K, batch, g)
    bias = (0.5 * torch.randn(N, device=DEV, generator=g)).bfloat16()
    nq, nk = ((1 + 0.1 * torch.randn(128, device=DEV, generator=g)).bfloat16() for _ in range(2))
    ang = torch.randn((S, 64), device=DEV, generator=g) * 3
    cos, sin = torch.cos(ang).repeat_interleave(2, 1).contiguous(), torch.sin(ang).repeat_interleave(2, 1).contiguous()
    if pair:
        cos, sin = ops.rope_pairs(cos, sin), None
    Abuf, akw = a_buffer(A8, batch)
    z = lambda *sh: G.poison_(torch.empty(sh, device=DEV, dtype=torch.bfloat16))
    Q, Kk, VT = z(B, H, Spad, 128), z(B, H, Spad, 128), z(B, H, 128, Spad)
    ops.gemm_qkv_fp8(Abuf.view(FP8), W8.view(FP8), bias, Q, Kk, VT, nq, nk, cos, sin, M=M, H=H, Spad=Spad, tok_off=tok_off, rows_per_sample=rps,
                     a_scale=sa, a_scale_batch_stride=M if batch > 1 else 0, w_scale=sw, q_scale=0.1275, vt_perm=vt_perm, **akw)
    form = int(_lib.get_option("last_gemm_tile"))
    torch.cuda.synchronize()
    name = f"qkv {geom} K={K} {kind} vt_perm={int(vt_perm)} pair={int(pair)}"
    rep = R.Report(name)
    R.check_qkv8(rep, A8, W8, bias, nq, nk, cos, sin, Q, Kk, VT, H=H, tok_off=tok_off, rows_per_sample=rps, a_scale=sa, w_scale=sw, q_scale=0.1275,
                 vt_perm=vt_perm)
    G.check_qkv_padding(name, Q, Kk, VT, S, vt_perm)
    if tok_off:                      # the text rows in front belong to another launch
        front = torch.arange(tok_off, device=DEV)
        assert bool(G.sentinel_bits(Q[:, :, :tok_off]).all()) and bool(G.sentinel_bits(Kk[:, :, :tok_off]).all()), f"{name}: rows below tok_off written"
        assert bool(G.sentinel_bits(VT[..., G.vt_pos(front, vt_perm)]).all()), f"{name}: V^T positions below tok_off written"
    return form, rep.done()


@pytest.mark.parametrize("geom", ["batched", "flat"])
@pytest.mark.parametrize("K,want_form", [(256, 7256), (384, 8256)])
def test_gemm_qkv_fp8_vs_fp64(ops, K, want_form, geom):
    worst = {}
    for kind in R.KINDS:
        for vt_perm, pair in ((False, False), (True, True), (True, False), (False, True)):
            form, w = run_qkv(ops, geom, K, kind, vt_perm, pair)
            assert form == want_form, (geom, K, kind, form)
            assert w < 1.0
            worst[kind] = max(worst.get(kind, 0.0), w)
    print(f"\n  qkv {geom} K={K}: form {want_form}; share of the f32 allowance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_gemm_qkv_fp8_stream_k_vs_fp64(ops):
    """H = 8, M = 8000, K = 2048: 32 x 12 = 384 tiles, a 128-tile remainder cut along K"""
    line = []
    for kind in TWO:
        form, w = run_qkv(ops, "big", 2048, kind, True, True, H=8, M_big=8000)
        assert form == 9256 and w < 1.0, (kind, form, w)
        line.append(f"{kind} {w:.3f}")
    ops.streamk_check(sync=True)
    print("\n  qkv stream-K: share of the f32 allowance: " + ", ".join(line))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_CASES = {"rows_form": (2, 2051, 3072, 510, 0), "per_row_same_inputs": (2, 2051, 3072, 510, 2), "per_row_37": (2, 37, 3072, 5, 0),
            "two_chunks_per_lane": (1, 9, 520, 0, 0), "d4096": (1, 5, 4096, 2, 0), "d64": (3, 6, 64, 3, 0)}


@pytest.mark.parametrize("kind", E.LN_KINDS)
@pytest.mark.parametrize("case", list(LN_CASES))
def test_ln_modulate_fp8_vs_fp64(ops, opt, case, kind):
    """With Y (dense outputs) and with Y = None into a strided Y8 (ldy8 = D + 16 behind an offset of 16 bytes) under the sentinel.  4102 rows
    at D = 3072 take the four-rows-per-wave kernel: a ragged last 16-row block, the stream and the sample boundary inside a wave's rows."""
    B, S, D, S0, fp8 = LN_CASES[case]
    opt("fp8", fp8)
    g = gen(50 + E.LN_KINDS.index(kind))
    X = E.ln_rows(B * S, D, kind, g, DEV).view(B, S, D)
    mod = E.mod_vectors(B * 4 * D, kind, g, DEV).view(B, 4 * D)
    if kind == "const":
        mod[0, :D] = 0               # sample 0, first stream: constant rows with zero shift -> scale exactly 1, zero codes
    mods = (mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:3 * D], mod[:, 3 * D:])
    line = []
    for with_y in (True, False):
        ld8, off8 = (D, 0) if with_y else (D + 16, 16)
        y8buf = R.poison_(torch.empty(off8 + B * S * ld8 + 8, device=DEV, dtype=torch.uint8))
        Y = G.poison_(torch.empty((B, S, D), device=DEV, dtype=torch.bfloat16)) if with_y else None
        rs = G.poison_(torch.empty(B * S + 4, device=DEV, dtype=torch.float32))
        ops.ln_modulate_fp8(X, Y, y8buf.view(FP8), rs, B, S, D, S0, *mods, 4 * D, ldy8=ld8, y8_offset=off8)
        torch.cuda.synchronize()
        view = ((B, S, D), (S * ld8, ld8, 1), off8)
        rep = R.check_ln8(R.RowReport(f"ln {case} {kind} {'with Y' if with_y else 'Y = None, strided Y8'}"), X, Y, y8buf.as_strided(*view), rs[:B * S],
                          S0, *mods, 1e-6)
        worst = rep.done()
        assert worst < 1.0 and rep.rs_worst <= 1.0
        R.check_untouched(f"ln {case} {kind} Y8", y8buf, G.write_mask(y8buf, [view]), row_len=ld8)
        assert bool(G.sentinel_bits(rs[B * S:]).all())
        if kind == "const" and S0 > 0:
            zero_rows = torch.arange(0, S0, 3, device=DEV)      # rows r % 3 == 0 of sample 0 are constant (ew_ref.ln_rows)
            assert bool((rs[zero_rows] == 1.0).all()) and bool(((y8buf.as_strided(*view)[0, zero_rows] & 0x7F) == 0).all())
        line.append(f"Y {worst:.3f}, row scale {rep.rs_worst:.3f}, two-valued {rep.two_share():.4f}")
    print(f"\n  ln {case} {kind}: " + " | ".join(line))


# ---------------------------------------------------------------------------------------------------------------- quantise
def special_rows(cols=256):
    """bf16 [5, cols]: every e4m3 midpoint of both signs with amax exactly 448 (scale exactly 1: the ties must go to even); values below 2^-6
    only; a row whose amax is the largest finite bf16; a zero row; -0 and tiny values"""
    v = R.decode(torch.arange(127, dtype=torch.uint8))
    mid = 0.5 * (v[1:] + v[:-1])
    rows = torch.zeros((5, cols), dtype=torch.float64)
    rows[0, :253] = torch.cat((torch.tensor([448.0], dtype=torch.float64), mid, -mid))
    g = torch.Generator().manual_seed(9)
    rows[1] = (torch.rand(cols, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -6
    rows[2] = torch.randn(cols, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(60, 121, (cols,), generator=g).double())
    rows[2, 5] = -float(torch.finfo(torch.bfloat16).max)
    rows[4, :4] = torch.tensor([-0.0, 1e-30, -1e-38, 2.0 ** -9])
    x = rows.bfloat16()
    assert torch.equal(x[0].double(), rows[0]) and float(x[1].abs().max()) < 2.0 ** -6
    return x


def test_quantize_rows_fp8_bit_exact_with_ties_subnormals_and_the_largest_bf16(ops):
    x = torch.cat((special_rows(), (3 * torch.randn((11, 256), generator=torch.Generator().manual_seed(4))).bfloat16()))
    want, want_s = R.quantize_expect(x)
    y, s = ops.quantize_rows_fp8(x.to(DEV))
    assert torch.equal(s.cpu(), want_s) and float(s[0]) == 1.0 and float(s[3]) == 1.0
    got = y.cpu().view(torch.uint8)
    bad = torch.nonzero(got != want)
    assert bad.numel() == 0, f"row {int(bad[0, 0])}, col {int(bad[0, 1])}: code {int(got[tuple(bad[0])]):#04x}, want {int(want[tuple(bad[0])]):#04x}"
    assert bool((got[0, 1:253] & 1 == 0).all())                  # the midpoints row: every tie on the even code
    for inv in (1.0, 200.0):                                     # the static form; with 1.0 row 1 gives subnormal codes only
        want2, _ = R.quantize_expect(x, static_inv_scale=inv)
        y2, s2 = ops.quantize_rows_fp8(x.to(DEV), static_inv_scale=inv)
        assert s2 is None
        got2 = y2.cpu().view(torch.uint8)
        bad = torch.nonzero(got2 != want2)
        assert bad.numel() == 0, f"static {inv}: row {int(bad[0, 0])}, col {int(bad[0, 1])}"
    sub, _ = R.quantize_expect(x[1:2], static_inv_scale=1.0)
    assert bool(((sub & 0x78) == 0).all()) and int((sub & 0x07).max()) > 0      # (the subnormal-only row is what it claims)


# ---------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("variant", [0, 9])
def test_attention_e4m3out_vs_the_bf16_launch_per_element(ops, opt, variant):
    """The e4m3 epilogue shares its arithmetic with the bf16 launch of the same variant: the f32 result o of an element rounds to the bf16
    output O, so the e4m3 output lies in fp8_ref.attn8_interval(O) -- per element, with the pad columns left at the sentinel."""
    opt("attn_variant", variant)
    B, H, S = 2, 4, 600
    Spad = ops.pad128(S)
    g = gen(3)
    Q = torch.randn((B, H, Spad, 128), device=DEV, generator=g).bfloat16()
    K = torch.randn((B, H, Spad, 128), device=DEV, generator=g).bfloat16()
    VT = (torch.randn((B, H, 128, Spad), device=DEV, generator=g) * 3).bfloat16()
    ld = H * 128 + 256               # strided destination, like the CAT buffer of the single blocks
    O = G.poison_(torch.empty((B, S, ld), device=DEV, dtype=torch.bfloat16))
    ops.attention(Q, K, VT, O, B, H, S, Spad, ld, S * ld, 1 / math.sqrt(128))
    assert bool(G.sentinel_bits(O[..., H * 128:]).all())
    tok = torch.arange(S, device=DEV)
    line = []
    for oinv in (1.0, 2000.0):
        O8 = R.poison_(torch.empty((B, S, ld), device=DEV, dtype=torch.uint8))
        ops.attention_e4m3out(Q, K, VT, O8.view(FP8), B, H, S, Spad, ld, S * ld, 1 / math.sqrt(128), out_inv_scale=oinv)
        torch.cuda.synchronize()
        assert bool(R.sentinel_bits(O8[..., H * 128:]).all()), "pad columns written"
        rep = R.RowReport(f"attention_e4m3out variant {variant} out_inv_scale {oinv}")
        for b in range(B):
            lo, hi = R.attn8_interval(O[b, :, :H * 128], oinv)
            rep.check_apart(R.decode(O8[b, :, :H * 128]), *R.interval_bound(lo, hi), sample=torch.full_like(tok, b), token=tok, unit=128)
            rep.two += int((lo != hi).sum())
            rep.n += lo.numel()
        rep.done()
        if oinv == 2000.0:
            assert float(R.decode(O8[..., :H * 128]).abs().max()) == 448.0
        line.append(f"out_inv_scale {oinv}: two-valued {rep.two_share():.4f}")
    print(f"\n  attention_e4m3out variant {variant}: " + ", ".join(line))
