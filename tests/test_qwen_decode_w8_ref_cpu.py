"""CPU checks of the e4m3 decode linear's reference and checker (tests/qwen_decode_w8_ref.py): the dequantisation against torch's own
float8_e4m3fn, an f32 stand-in of the kernel's documented summation order that must pass, the likely bugs planted in it that must fail --
with what a whole-output rel-L2 threshold of the old kind would have said beside each -- and the boundary: include/x2i_qwen_decode_w8.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and every refusal of the entry point."""
import ctypes as C
import os

import pytest
import torch

from tests import fp8_ref as F8
from tests import gemm_ref as G
from tests import qwen_decode_w8_ref as WR
from tests import qwen_ref as QR
from tests.headers import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE, ERR_ALIGN = -1, -2, -3       # X2I_ERR_* of include/x2i.h


def w8_inputs(B, N, K, seed, rows_w=None, bias_std=0.5, split_scales=False):
    """bf16 X ~ N(0, 1), a weight ~ N(0, 1 / K) quantised by the library's own rule, bias, res.  split_scales: the second half of the rows
    (mode 1's `b` rows) is 8 times larger before quantisation, so the scales of the halves differ by a factor of at least 4"""
    g = torch.Generator().manual_seed(seed)
    rows = rows_w or N
    X = torch.randn((B, K), generator=g).bfloat16()
    W = torch.randn((rows, K), generator=g) * K ** -0.5
    if split_scales:
        W[rows // 2:] *= 8.0
    W8, scale = WR.quantize_rows(W.bfloat16())
    bias = (bias_std * torch.randn((rows,), generator=g)).bfloat16()
    res = torch.randn((B, N), generator=g).bfloat16()
    return X, W8, scale, bias, res


def test_dequantisation_agrees_with_torch_on_all_254_finite_codes():
    codes = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=torch.uint8)
    assert codes.numel() == 254
    ours = F8.decode(codes)
    theirs = codes.view(torch.float8_e4m3fn).to(torch.float64)
    assert torch.equal(ours, theirs) and bool(torch.isfinite(ours).all())
    assert bool(torch.isnan(F8.decode(torch.tensor([0x7F, 0xFF], dtype=torch.uint8))).all())
    # with a scale that is no power of two the product is still exact in float64: 24 + 4 significand bits
    s = torch.tensor([0.0123456789], dtype=torch.float32).expand(254)
    deq = WR.dequant(codes[:, None], s)[:, 0]
    assert torch.equal(deq, theirs * float(s[0]))
    # the quantiser never produces a NaN code, and an all-zero row gets scale 1 and codes 0
    W = torch.randn((8, 64), generator=torch.Generator().manual_seed(1)).bfloat16()
    W[3] = 0
    c8, sc = WR.quantize_rows(W)
    assert not bool(((c8 & 0x7F) == 0x7F).any()) and float(sc[3]) == 1.0 and bool((c8[3] == 0).all())
    assert bool((WR.dequant(c8, sc)[3] == 0).all())


MODE0 = [(1, 64, 64), (3, 104, 272), (8, 512, 1040), (8, 64, 4112)]
MODE1 = [(1, 64, 64), (3, 104, 272), (8, 512, 1040)]


@pytest.mark.parametrize("B,N,K", MODE0)
@pytest.mark.parametrize("with_bias,with_res", [(False, False), (True, False), (True, True), (False, True)])
def test_stand_in_of_the_documented_order_stays_inside_the_allowance(B, N, K, with_bias, with_res):
    X, W8, s, bias, res = w8_inputs(B, N, K, seed=N + K)
    bias, res = (bias if with_bias else None), (res if with_res else None)
    want, bound, delta = WR.linear_w8_expect(X, W8, s, bias, res)
    msg, worst, _, _ = G.check_block("stand-in B=%d N=%d K=%d" % (B, N, K), WR.stand_in(X, W8, s, bias, res), want, bound, delta=delta)
    assert msg is None, msg
    print("stand-in B=%d N=%d K=%d bias=%s res=%s: share of the f32 allowance used %.3f" % (B, N, K, with_bias, with_res, worst))
    assert worst < 1.0


@pytest.mark.parametrize("B,N,K", MODE1)
@pytest.mark.parametrize("with_bias", [False, True])
def test_stand_in_of_the_gate_stays_inside_the_allowance(B, N, K, with_bias):
    X, W8, s, bias, _ = w8_inputs(B, N, K, seed=N + K + 1, rows_w=2 * N, split_scales=True)
    assert float((s[N:] / s[:N]).min()) >= 4.0
    bias = bias if with_bias else None
    want, bound, delta = WR.gate_w8_expect(X, W8, s, bias)
    msg, worst, _, _ = G.check_block("stand-in gate B=%d N=%d K=%d" % (B, N, K), WR.stand_in(X, W8, s, bias, gate=True), want, bound, delta=delta)
    assert msg is None, msg
    print("stand-in gate B=%d N=%d K=%d bias=%s: share of the f32 allowance used %.3f" % (B, N, K, with_bias, worst))


def _rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm())


def test_planted_faults_are_rejected_and_what_a_rel_l2_threshold_would_have_said():
    """Each likely bug in the stand-in, on the shape where it bites: the per-element checker rejects every one.  Beside each, the
    whole-output rel-L2 of the faulty result against the old kind of threshold (fp8_ref.OLD_E4M3_REL_L2 = 4e-2, what the e4m3 outputs
    were once held to): the scale on a small bias passes it (1.3e-2), and the dropped last step at K = 4112 misses it by a hair (4.2e-2)."""
    old = F8.OLD_E4M3_REL_L2
    passed_old = []
    # (fault, B, N, K, gate, bias std): the bias of the order of the q|k|v biases' perturbation; K = 4112: lane 0 alone has a fifth step
    for fault, B, N, K, gate, bias_std in (("scale_on_bias", 3, 104, 272, False, 0.02), ("b_scale_index", 3, 104, 272, True, 0.5),
                                           ("halves_swapped", 3, 104, 272, False, 0.5), ("last_step_dropped", 8, 512, 1040, False, 0.5),
                                           ("last_step_dropped", 8, 64, 4112, False, 0.5)):
        X, W8, s, bias, res = w8_inputs(B, N, K, seed=K, rows_w=2 * N if gate else None, bias_std=bias_std, split_scales=gate)
        if gate:
            want, bound, delta = WR.gate_w8_expect(X, W8, s, bias)
            good, bad = WR.stand_in(X, W8, s, bias, gate=True), WR.stand_in(X, W8, s, bias, gate=True, fault=fault)
        else:
            want, bound, delta = WR.linear_w8_expect(X, W8, s, bias, res)
            good, bad = WR.stand_in(X, W8, s, bias, res), WR.stand_in(X, W8, s, bias, res, fault=fault)
        assert G.check_block(fault, good, want, bound, delta=delta)[0] is None
        msg = G.check_block(fault, bad, want, bound, delta=delta)[0]
        assert msg is not None, "%s at (%d, %d, %d) went through the per-element check" % (fault, B, N, K)
        r = _rel_l2(bad, want)
        print("%-18s (%d, %d, %d): rejected per element; whole-output rel-L2 %.3e %s the old threshold %.0e"
              % (fault, B, N, K, r, "PASSES" if r < old else "fails", old))
        if r < old:
            passed_old.append(fault)
    assert passed_old, "no planted fault passes the old rel-L2 threshold: the comparison shows nothing"


def test_dequantized_state_dict_replaces_the_seven_projections_and_nothing_else():
    cfg, lib = QR.library_stack(256, 2, 1, 512, 1)
    sd = QR.random_stack_state_dict(lib, seed=3)
    dq = WR.dequantized_state_dict(sd, 2, 1)
    assert set(dq) == set(sd)
    changed = {k for k in sd if not torch.equal(dq[k].double(), sd[k].double())}
    assert changed == {k for k in sd if k.endswith("_proj.weight")} and len(changed) == 7
    for k in changed:                          # within half an e4m3 ulp: 16 of 448 in the top binade, where the row's amax lies
        amax = sd[k].abs().amax(1, keepdim=True).double()
        assert bool(((dq[k] - sd[k].double()).abs() <= amax * (16.0 / 448.0) * (1 + 1e-6)).all())
        assert dq[k].dtype == torch.float64


def test_mixed_reference_is_the_decode_reference_when_both_state_dicts_are_one():
    """decode_reference_w8 restates qwen_decode_ref.decode_reference with the weights chosen by row; with the quantiser replaced by the
    identity it must say what that says, and with the real one the step rows must move while staying a drift, not another function"""
    from tests import qwen_decode_ref as DR
    cfg, lib = QR.library_stack(256, 2, 1, 512, 2)
    sd = QR.random_stack_state_dict(lib, seed=4)
    g = torch.Generator().manual_seed(5)
    B, S, T = 2, 12, 3
    x, steps = torch.randn((B, S, 256), generator=g).double(), torch.randn((B, T, 256), generator=g).double()
    pos = torch.arange(S)[None].expand(B, S)
    kw = dict(num_heads=2, num_kv_heads=1, eps=cfg.rms_norm_eps, dk=128, theta=1000000.0)
    want = DR.decode_reference(sd, x, steps, pos, [0, 3], [10, 12], **kw)
    real = WR.dequantized_state_dict
    try:
        WR.dequantized_state_dict = lambda sd, *a, **k: sd
        same = WR.decode_reference_w8(sd, x, steps, pos, [0, 3], [10, 12], **kw)
    finally:
        WR.dequantized_state_dict = real
    assert QR.rel_l2(same, want) < 1e-12
    mixed = WR.decode_reference_w8(sd, x, steps, pos, [0, 3], [10, 12], **kw)
    assert torch.equal(mixed[:, 0], want[:, 0]) and 1e-3 < QR.rel_l2(mixed[:, 1:], want[:, 1:]) < 0.2


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_the_header_is_the_bf16_prototype_with_the_scale_and_states_its_promises():
    path = os.path.join(ROOT, "include", "x2i_qwen_decode_w8.h")
    # the bf16 entry point's prototype with the scale inserted after ldw
    bf16 = header_prototypes(os.path.join(ROOT, "include", "x2i_qwen_decode.h"))["x2i_qwen_decode_linear_bf16"]
    assert header_prototypes(path)["x2i_qwen_decode_linear_w8_bf16"] == bf16[:4] + [C.c_void_p] + bf16[4:]
    text = open(path).read()
    assert "16 l + 1024 i + j" in text and "unspecified" in text and "bit-identical" in text       # the order and the two promises are stated


def test_entry_point_validates_its_arguments_without_a_gpu():
    from x2i_amd import qwen_decode_w8_ops
    lib = qwen_decode_w8_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    odd8, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1002)
    err = lambda: lib.x2i_last_error()
    f = lambda **kw: lib.x2i_qwen_decode_linear_w8_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("ldx", 64), ("W8", fake), ("ldw", 64), ("scale", fake), ("bias", None), ("res", None), ("ldr", 0), ("Y", fake), ("ldy", 64),
        ("B", 2), ("N", 64), ("K", 64), ("mode", 0), ("st", None))])
    assert f(K=72, ldx=72, ldw=80) == ERR_SHAPE and b"K=72" in err()      # a multiple of 8 is not enough
    assert f(K=0) == ERR_SHAPE and f(N=0) == ERR_SHAPE
    assert f(B=0) == ERR_SHAPE and b"B=0" in err()
    assert f(B=9) == ERR_SHAPE and b"B=9" in err()
    assert f(mode=2) == ERR_ARG and b"mode=2" in err()
    assert f(mode=1, res=fake, ldr=64) == ERR_ARG and b"residual" in err()
    assert f(scale=None) == ERR_ARG and b"w_scale" in err()
    assert f(X=None) == ERR_ARG and f(W8=None) == ERR_ARG and f(Y=None) == ERR_ARG
    for bad in (dict(W8=odd8), dict(X=odd8), dict(scale=odd2), dict(ldw=48), dict(ldw=72), dict(ldx=60), dict(ldx=56), dict(ldy=32),
                dict(res=fake, ldr=32)):
        assert f(**bad) == ERR_ALIGN and b"aligned" in err(), bad
