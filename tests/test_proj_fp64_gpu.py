"""The projector's layer-fusion launches against the float64 reference of tests/proj_ref.py -- every output element of every launch, the
sentinel in the guard rows around the output and in every element the launch must leave alone.

(a) x2i_proj_conv5x5_bf16 (VALU form): the one-stream kernel on small and ragged shapes, one tile below the launch threshold (510 tiles), and
    the two-stream kernel (>= 512 tiles) with the last block's second stream holding one row, lying wholly past S, and exact.
(b) x2i_proj_conv5x5_pack + x2i_proj_conv5x5_packed_bf16 (MFMA forms) under conv5_variant 0 / 1 / 2 / 3, each variant against float64 on its
    own (and the variants bit-identical among themselves); one default-dispatch case that takes the two-row-block form by itself (n2 = 260);
    the whole packed table, bit for bit.
(c) x2i_proj_layer_mean_bf16 with and without scales, with a grid-stride case (more than 2048 x 256 chunks); x2i_seq_mean_f32 at N % 256 != 0.

Every conv case runs with a bias pointer into an output that is 4-byte (VALU) or 8-byte (MFMA) but not 16-byte aligned, and without one into a
16-byte aligned output.  The form named in a line of the log is the one the launcher takes for that shape (proj_ref.valu_form / mfma_form mirror
its dispatch; tests/test_proj_ref_cpu.py pins them at the threshold shapes).  The largest share of the f32 allowance used per launch and form
is kept in WORST and printed by the last test."""
import time

import pytest
import torch

from tests import proj_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
WORST = {}      # launch and kernel form -> worst share of the f32 allowance used, over everything this module ran


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture
def opt(ops):
    """Set library A/B switches for one test (restored afterwards)."""
    from x2i_amd import _lib
    saved = {}

    def set_(name, value):
        old = _lib.set_option(name, value)
        saved.setdefault(name, old)
    yield set_
    for k, v in saved.items():
        _lib.set_option(k, v)


def note(name, share):
    WORST[name] = max(WORST.get(name, 0.0), share)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def guarded(shape, off, dtype=BF, guard=None):
    """(buffer, view, mask): a poisoned flat buffer, the output view of `shape` `off` elements behind `guard` leading guard elements (two output
    rows by default), and the mask of the view's elements"""
    n = 1
    for s in shape:
        n *= s
    guard = 2 * shape[-1] if guard is None else guard
    buf = R.poison_(torch.empty(guard + off + n + guard + 8, device=DEV, dtype=dtype))
    view = buf[guard + off:guard + off + n].view(shape)
    stride = tuple(view.stride())
    return buf, view, R.write_mask(buf, [(tuple(shape), stride, guard + off)])


# ---------------------------------------------------------------------------------------------------------------- conv5x5
def run_valu(ops, ref, x, w, bias, off, name):
    B, C, S, H = x.shape
    buf, y, mask = guarded((B, S, H), off)
    assert y.data_ptr() % 16 == (2 * off) % 16
    ops.proj_conv5x5(x, w, bias, out=y)
    torch.cuda.synchronize()
    form = R.valu_form(B, S, H)
    share = ref.check(name, y, form, bias)
    R.check_untouched(name, buf, mask, row_len=H)
    note(f"conv5x5 {form}", share)
    return form, share


def run_mfma(ops, ref, x, table, bias, off, variant, name):
    B, C, S, H = x.shape
    buf, y, mask = guarded((B, S, H), off)
    assert y.data_ptr() % 16 == (2 * off) % 16
    ops.proj_conv5x5_packed(x, table, bias, out=y)
    torch.cuda.synchronize()
    form = R.mfma_form(variant, B, S, H)
    share = ref.check(name, y, form, bias)
    R.check_untouched(name, buf, mask, row_len=H)
    note(f"conv5x5 {form}", share)
    return form, share, y.clone()


def valu_case(ops, shape, kinds, seed):
    t0 = time.time()
    B, C, S, H = shape
    for kind in kinds:
        x, w, bias = R.conv_operands(kind, B, C, S, H, gen(seed), DEV)
        ref = R.ConvRef(x, w)
        form, s1 = run_valu(ops, ref, x, w, bias, 2, f"proj_conv5x5 {shape} {kind} bias, y + 4 bytes")
        _, s0 = run_valu(ops, ref, x, w, None, 0, f"proj_conv5x5 {shape} {kind} no bias")
        tiles = R._cdiv(H, 512) * R._cdiv(S, 16) * B
        print(f"\n  proj_conv5x5 {shape} {kind}: {tiles} one-stream tiles -> {form}; share of the f32 allowance {max(s0, s1):.3f}", end="")
        del x, ref
    print(f"\n  ({time.time() - t0:.1f} s)")


VALU_SMALL = [(1, 1, 1, 8), (1, 3, 6, 64), (2, 29, 40, 896), (1, 8, 16, 512), (1, 9, 17, 520), (1, 64, 5, 8)]
VALU_LARGE = [(2, 3, 1360, 1032),       # 510 tiles: one below the threshold, still one stream
              (2, 3, 1361, 1032),       # 516 tiles: two streams; the last block's second stream holds one row
              (2, 3, 1384, 1032),       # ... lies wholly past S
              (2, 3, 1376, 1032)]       # ... exact


@pytest.mark.parametrize("shape", VALU_SMALL, ids=str)
def test_valu_one_stream(ops, shape):
    assert R.valu_form(shape[0], shape[2], shape[3]) == "valu1"
    valu_case(ops, shape, R.CONV_KINDS, 100 + shape[2])


@pytest.mark.parametrize("kind", ["random", "edge"])
@pytest.mark.parametrize("shape", VALU_LARGE, ids=str)
def test_valu_launch_threshold_and_two_streams(ops, shape, kind):
    assert R.valu_form(shape[0], shape[2], shape[3]) == ("valu1" if shape[2] == 1360 else "valu2")
    valu_case(ops, shape, (kind,), 200 + shape[2])


MFMA_SHAPES = [(1, 1, 1, 8), (1, 2, 5, 64), (2, 4, 13, 264), (2, 5, 25, 520), (1, 2, 36, 256), (3, 37, 40, 512), (1, 3, 12, 2048),
               (1, 29, 24, 3584)]


@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=str)
def test_mfma_forms(ops, opt, shape):
    """every conv5_variant against float64 on its own; then the variants bit-identical"""
    t0 = time.time()
    B, C, S, H = shape
    for kind in R.CONV_KINDS:
        x, w, bias = R.conv_operands(kind, B, C, S, H, gen(300 + S), DEV)
        ref = R.ConvRef(x, w)
        table = ops.proj_conv5x5_pack(w)
        outs, line = [], []
        for variant in (0, 1, 2, 3):
            opt("conv5_variant", variant)
            form, s1, y1 = run_mfma(ops, ref, x, table, bias, 4, variant, f"proj_conv5x5_packed {shape} {kind} variant {variant} bias, y + 8 bytes")
            _, s0, y0 = run_mfma(ops, ref, x, table, None, 0, variant, f"proj_conv5x5_packed {shape} {kind} variant {variant} no bias")
            outs.append((y1, y0))
            line.append(f"{variant}:{form} {max(s0, s1):.3f}")
        opt("conv5_variant", 0)
        for variant in (1, 2, 3):
            assert torch.equal(outs[variant][0], outs[0][0]) and torch.equal(outs[variant][1], outs[0][1]), (kind, variant)
        print(f"\n  proj_conv5x5_packed {shape} {kind}: variant:form share  " + ", ".join(line), end="")
    print(f"\n  ({time.time() - t0:.1f} s)")


@pytest.mark.parametrize("kind", ["random", "edge"])
def test_mfma_default_dispatch_takes_the_two_row_block_form(ops, kind):
    """(1, 2, 1248, 1032): n2 = 5 x 52 = 260 >= 256 tiles of the two-row-block form, not a multiple of 8 (four dead workgroups)"""
    t0 = time.time()
    shape = B, C, S, H = 1, 2, 1248, 1032
    assert R.mfma_tiles2(B, S, H) == 260 and R.mfma_form(0, B, S, H) == "mfma_rb2"
    assert int(ops._lib.get_option("conv5_variant")) == 0
    x, w, bias = R.conv_operands(kind, B, C, S, H, gen(400), DEV)
    ref = R.ConvRef(x, w)
    table = ops.proj_conv5x5_pack(w)
    form, s1, _ = run_mfma(ops, ref, x, table, bias, 4, 0, f"proj_conv5x5_packed {shape} {kind} default dispatch bias, y + 8 bytes")
    _, s0, _ = run_mfma(ops, ref, x, table, None, 0, 0, f"proj_conv5x5_packed {shape} {kind} default dispatch no bias")
    print(f"\n  proj_conv5x5_packed {shape} {kind}: n2 = {R.mfma_tiles2(B, S, H)} -> {form} by default; share {max(s0, s1):.3f} ({time.time() - t0:.1f} s)")


@pytest.mark.parametrize("C", [1, 37])
def test_pack_table_every_entry(ops, C):
    w = torch.randn((C, 25), device=DEV, generator=gen(500 + C)) / (25 * C) ** 0.5
    # the table inside a guarded buffer: x2i_proj_conv5x5_pack may write C x 5 x 64 x 8 entries and nothing else
    buf, table, mask = guarded((C, 5, 64, 8), 0, guard=64)
    ops.check(ops._lib.load().x2i_proj_conv5x5_pack(ops._p(w), ops._p(table), C, ops._stream()), "proj_conv5x5_pack")
    torch.cuda.synchronize()
    R.check_table(f"proj_conv5x5_pack C={C}", table, w)
    R.check_untouched(f"proj_conv5x5_pack C={C}", buf, mask)
    assert torch.equal(ops.proj_conv5x5_pack(w), table)
    print(f"\n  proj_conv5x5_pack C={C}: {table.numel()} entries equal")


# ---------------------------------------------------------------------------------------------------------------- the means
@pytest.mark.parametrize("B,C,plane", [(2, 1, 8), (2, 25, 8), (2, 1, 8 * 257), (2, 25, 8 * 257), (1, 2, 8 * (2048 * 256 + 3))])
def test_layer_mean(ops, B, C, plane):
    """plane = 8 * 257: a second, partly filled block; the last case has 2048 * 256 + 3 chunks of 8: the grid-stride loop runs a second time"""
    t0 = time.time()
    x = (3.0 * torch.randn((B, C, 1, plane), device=DEV, generator=gen(600 + C))).to(BF)
    sc = torch.randn(C, device=DEV, generator=gen(601))
    shares = []
    for scale in (sc, None):
        buf, y, mask = guarded((B, 1, plane), 0, guard=64)
        ops.proj_layer_mean(x, scale, out=y)
        torch.cuda.synchronize()
        name = f"layer_mean {(B, C, plane)} {'scale' if scale is not None else 'no scale'}"
        shares.append(R.check_layer_mean(name, x, scale, y))
        R.check_untouched(name, buf, mask)
        note("layer_mean", shares[-1])
    print(f"\n  layer_mean {(B, C, plane)}: {R._cdiv(plane // 8, 256)} blocks of 256 chunks (grid <= 2048); share scale {shares[0]:.3f}, "
          f"no scale {shares[1]:.3f} ({time.time() - t0:.1f} s)")


@pytest.mark.parametrize("B,S,N", [(1, 1, 1), (2, 12, 768), (3, 7, 257)])
def test_seq_mean(ops, B, S, N):
    x = torch.randn((B, S, N), device=DEV, generator=gen(700 + N))
    buf, y, mask = guarded((B, N), 0, dtype=torch.float32, guard=3)
    ops.check(ops._lib.load().x2i_seq_mean_f32(ops._p(x), ops._p(y), B, S, N, ops._stream()), "seq_mean")
    torch.cuda.synchronize()
    share = R.check_seq_mean(f"seq_mean {(B, S, N)}", x, y)
    R.check_untouched(f"seq_mean {(B, S, N)}", buf, mask)
    assert torch.equal(ops.seq_mean(x), y)
    note("seq_mean", share)
    print(f"\n  seq_mean {(B, S, N)}: |err| / bound {share:.3f}")


def test_print_worst():
    """(last: the table of worst shares over everything this module ran)"""
    print("\n  worst share of the f32 allowance per launch and form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
