"""CPU checks of the Qwen2 prompt extension (tests/qwen_extend_ref.py, include/x2i_qwen_extend.h, Qwen2DecoderStack.extend,
handoff.common_prefix, --hip_keep_cache): the window reference against the full one and the likely bugs planted in it, the header against its
binding, the built library and INTEGRATION.md, every refusal of the two entry points on fake pointers, the common prefix on CPU tensors,
the flags' defaults and refusals, and extend's refusals on a CPU stack."""
import ctypes as C
import inspect
import os

import pytest
import torch

from tests import qwen_extend_ref as XR
from tests import qwen_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE, ERR_ALIGN = -1, -2, -3       # X2I_ERR_* of include/x2i.h


# ---------------------------------------------------------------------------------------------------------------- the window reference
@pytest.mark.parametrize("B,Hq,Hkv,dk,row0,n,k_lo", [(1, 1, 1, 128, 1, 1, None), (2, 4, 2, 128, 64, 64, [0, 10]), (1, 4, 2, 128, 70, 61, None),
                                                     (2, 14, 2, 64, 129, 150, [0, 100]), (1, 2, 1, 128, 30, 40, [50])])
def test_window_reference_is_the_full_references_rows_and_planted_bugs_are_caught(B, Hq, Hkv, dk, row0, n, k_lo):
    S = row0 + n
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=100 * row0 + n)
    scale = dk ** -0.5
    full = QR.attention_reference(Q, K, V, S, scale, k_lo)
    win = XR.window_reference(Q, K, V, row0, n, scale, k_lo)
    assert win.shape == (B, Hq, n, dk) and float((win - full[:, :, row0:]).abs().max()) <= 1e-12
    assert XR.check_window("window", win.bfloat16(), win, row0, k_lo) <= QR.TOL_O          # one output rounding passes
    # only the chunk's rows of Q are read
    Q2 = Q.clone()
    Q2[:, :, :row0] = 1e30
    assert torch.equal(XR.window_reference(Q2, K, V, row0, n, scale, k_lo), win)
    # the diagonal off by one: row i also sees key i + 1 (slot S holds one more key, as a cache does).  Row i's q under row i + 1's mask
    Kx, Vx = (torch.cat((t[:, :, :S], t[:, :, :1]), 2) for t in (K, V))
    leak = QR.attention_reference(torch.cat((Q[:, :, :1], Q[:, :, :S]), 2), Kx, Vx, S + 1, scale, k_lo)[:, :, row0 + 1:]
    with pytest.raises(AssertionError):
        XR.check_window("diagonal + 1", leak.bfloat16(), win, row0, k_lo)
    # row0 ignored: the chunk's rows computed as rows 0 .. n - 1
    if row0 > 0:
        Qs = Q[:, :, row0:]
        lo0 = None if k_lo is None else [0] * B
        early = QR.attention_reference(Qs, K, V, n, scale, lo0)
        with pytest.raises(AssertionError):
            XR.check_window("row0 ignored", early.bfloat16(), win, row0, k_lo)


def test_stack_criterion_restated():
    XR.assert_stack_criterion(3.0e-3, 4.5e-3)
    XR.assert_stack_criterion(6.7e-3, 4.5e-3)
    for bad in ((6.8e-3, 4.5e-3), (3.1e-2, 4.0e-2)):
        with pytest.raises(AssertionError):
            XR.assert_stack_criterion(*bad)


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_the_header_states_its_coordinates_and_both_promises():
    text = open(os.path.join(ROOT, "include", "x2i_qwen_extend.h")).read()
    assert "live data only" in text and "bit for bit" in text and "PHYSICAL CACHE SLOTS" in text


def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import qwen_extend_ops
    lib = qwen_extend_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    odd8, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1002)
    err = lambda: lib.x2i_last_error()
    rope = lambda **kw: lib.x2i_qwen_extend_rope_split_bf16(*[kw.get(k, d) for k, d in (
        ("qkv", fake), ("ld", 512), ("cos", fake), ("sin", fake), ("Q", fake), ("K", fake), ("VT", fake), ("B", 1), ("row0", 5), ("n", 3), ("cap", 64),
        ("Hq", 2), ("Hkv", 1), ("dk", 128), ("st", None))])
    attn = lambda **kw: lib.x2i_qwen_extend_attention_bf16(*[kw.get(k, d) for k, d in (
        ("Q", fake), ("K", fake), ("VT", fake), ("k_lo", None), ("O", fake), ("B", 1), ("Hq", 2), ("Hkv", 1), ("row0", 5), ("n", 3), ("cap", 64),
        ("dk", 128), ("scale", 0.1), ("ldo", 256), ("obs", 3 * 256), ("st", None))])
    for f in (rope, attn):
        assert f(row0=-1) == ERR_SHAPE and b"row0=-1" in err()
        assert f(n=0) == ERR_SHAPE and b"n=0" in err()
        assert f(row0=62, n=3) == ERR_SHAPE and b"row0=62" in err() and b"cap=64" in err()
        assert f(row0=2 ** 31 - 2, n=3) == ERR_SHAPE                                        # (no overflow in row0 + n)
        assert f(cap=72) == ERR_SHAPE and b"cap=72" in err()
        assert f(cap=0) == ERR_SHAPE
        assert f(dk=96) == ERR_SHAPE and b"dk=96" in err()
        assert f(dk=32) == ERR_SHAPE and b"dk=32" in err()
        assert f(B=0) == ERR_SHAPE and b"B=0" in err()
        assert f(Q=None) == ERR_ARG and f(K=None) == ERR_ARG and f(VT=None) == ERR_ARG
        for bad in (dict(Q=odd8), dict(K=odd8), dict(VT=odd8)):
            assert f(**bad) == ERR_ALIGN and b"aligned" in err() and b"0x1008" in err(), bad
    assert attn(Hq=3, Hkv=2) == ERR_SHAPE and b"Hq=3" in err()
    assert attn(scale=0.0) == ERR_ARG and b"scale=0" in err()
    assert attn(scale=-0.5) == ERR_ARG and b"scale=-0.5" in err()
    assert attn(scale=float("nan")) == ERR_ARG and attn(scale=float("inf")) == ERR_ARG
    assert attn(O=None) == ERR_ARG
    assert attn(ldo=248) == ERR_ALIGN and b"ldo=248" in err()                               # narrower than Hq * dk
    assert attn(ldo=258) == ERR_ALIGN and b"ldo=258" in err()
    assert attn(obs=770) == ERR_ALIGN and b"o_batch_stride=770" in err()
    assert attn(O=C.c_void_p(0x1004)) == ERR_ALIGN and b"0x1004" in err()
    assert attn(k_lo=odd2) == ERR_ALIGN and b"0x1002" in err()
    assert rope(qkv=None) == ERR_ARG and rope(cos=None) == ERR_ARG and rope(sin=None) == ERR_ARG
    assert rope(ld=504) == ERR_ALIGN and b"ld=504" in err()                                 # narrower than (Hq + 2 Hkv) dk
    assert rope(ld=516) == ERR_ALIGN and b"ld=516" in err()
    for bad in (dict(qkv=odd8), dict(cos=odd8), dict(sin=odd8)):
        assert rope(**bad) == ERR_ALIGN and b"0x1008" in err(), bad
    assert rope(Hq=65535, Hkv=1, ld=8 * 65537 * 128) == ERR_SHAPE and b"Hq=65535" in err()


# ---------------------------------------------------------------------------------------------------------------- the common prefix
def test_common_prefix_on_cpu_tensors():
    from x2i_amd.handoff import common_prefix
    g = torch.Generator().manual_seed(3)
    prev = torch.randint(0, 64, (2, 90), generator=g)
    ids = torch.cat((prev, torch.randint(0, 64, (2, 20), generator=g)), 1)
    assert common_prefix(prev, 89, ids) == 89 and isinstance(common_prefix(prev, 89, ids), int)     # identical ids: the valid cap
    assert common_prefix(prev, 90, ids) == 90 and common_prefix(prev, 200, ids) == 90
    other = ids.clone()
    other[1, 40] += 1
    assert common_prefix(prev, 89, other) == 40                                            # one of two samples differs at 40
    other = ids.clone()
    other[0, 0] += 1
    assert common_prefix(prev, 89, other) == 0
    assert common_prefix(prev, 89, ids[:, :30]) == 30                                      # a new prompt shorter than the kept one
    short = ids[:, :30].clone()
    short[0, 12] += 1
    assert common_prefix(prev, 89, short) == 12
    assert common_prefix(prev, 0, ids) == 0 and common_prefix(prev, 89, ids[:1]) == 0      # nothing valid; another batch size


# ---------------------------------------------------------------------------------------------------------------- flags and signatures
def test_keep_cache_defaults_and_the_flags_refusal():
    from x2i_amd.handoff import HipGenerate
    from x2i_amd.infer import inference_multi_turn as MT
    from x2i_amd.infer.harness import build_parser
    assert inspect.signature(HipGenerate.__init__).parameters["keep_cache"].default is False
    assert inspect.signature(HipGenerate.generate).parameters["keep_cache"].default is None
    assert inspect.signature(MT.MultiTurnConditioner.__init__).parameters["keep_cache"].default is False
    assert callable(HipGenerate.forget)
    assert "--hip_keep_cache" not in build_parser("qwenvl").format_help()                  # the shared parser is as it was
    with pytest.raises(ValueError, match="--hip_keep_cache.*--hip_generate"):
        MT.MultiTurnConditioner(os.path.join(ROOT, "no_such_checkpoint"), "cpu", keep_cache=True)
    with pytest.raises(ValueError, match="--hip_keep_cache.*--hip_generate"):
        MT.MultiTurnConditioner(None, "cpu", model=object(), processor=object(), keep_cache=True)
    sig = inspect.signature(__import__("x2i_amd.qwen", fromlist=["x"]).Qwen2DecoderStack.extend)
    assert list(sig.parameters)[1:] == ["cache", "keep", "inputs_embeds", "input_ids", "position_ids", "check", "merge", "embed_scale"]
    assert sig.parameters["check"].default is True and sig.parameters["position_ids"].default is None


# ---------------------------------------------------------------------------------------------------------------- extend on a CPU stack
OK = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=256, num_hidden_layers=2, vocab_size=16, device="cpu")


def test_extend_refuses_before_anything_launches():
    from x2i_amd._lib import X2IError
    from x2i_amd.qwen import Qwen2DecoderStack
    m = Qwen2DecoderStack(**OK)
    x = torch.zeros((2, 6, 128), dtype=torch.bfloat16)
    pos = torch.arange(10, 16)[None].expand(2, 6)
    c = m.new_cache(2, 70)                                                                  # cap 128
    with pytest.raises(ValueError, match="prefill"):
        m.extend(c, 10, inputs_embeds=x, position_ids=pos)                                 # never prefilled
    c._set_prompt(10, None, None, None, torch.arange(10)[None].expand(2, 10))
    state = lambda: (c.k_lo.tolist(), c.k_hi.tolist(), c.pos.tolist(), c.steps)
    before = state()
    with pytest.raises(ValueError, match="new_cache"):
        m.extend(object(), 10, inputs_embeds=x, position_ids=pos)
    with pytest.raises(ValueError, match="new_cache"):
        Qwen2DecoderStack(**OK).extend(c, 10, inputs_embeds=x, position_ids=pos)           # a foreign cache
    for keep in (0, -3):
        with pytest.raises(ValueError, match="keep"):
            m.extend(c, keep, inputs_embeds=x, position_ids=pos)
    with pytest.raises(ValueError, match="position_ids"):
        m.extend(c, 10, inputs_embeds=x)
    with pytest.raises(ValueError, match="position_ids"):
        m.extend(c, 10, inputs_embeds=x, position_ids=pos[:, :5])
    with pytest.raises(ValueError, match="cap"):
        m.extend(c, 122, inputs_embeds=x, position_ids=pos)                                # 122 + 6 + 1 > 128
    with pytest.raises(ValueError, match="cap"):
        m.extend(c, 10, inputs_embeds=x[:1], position_ids=pos[:1])                         # another batch size
    with pytest.raises(ValueError, match="exactly one"):
        m.extend(c, 10, position_ids=pos)
    with pytest.raises(ValueError, match="hole"):
        m.extend(c, 11, inputs_embeds=x, position_ids=pos)                                 # the keys end at 10
    c.k_lo.fill_(4)
    with pytest.raises(ValueError, match="start at slot 4"):
        m.extend(c, 4, inputs_embeds=x, position_ids=pos)
    c.k_lo.zero_()
    assert state() == before                                                               # nothing was set by a refused call
    with pytest.raises(ValueError, match="prefill only"):                                  # forward is as it was
        m(inputs_embeds=x, past_key_values=object())
    # a call that passes every check sets the cache's state and then meets the first launch: no fallback on the CPU
    with pytest.raises(X2IError):
        m.extend(c, 10, inputs_embeds=x, position_ids=pos)
    assert c.k_hi.tolist() == [16, 16] and c.pos.tolist() == [16, 16] and c.steps == 16
