"""CPU-side checks of token selection on the HIP path (no GPU): the float64 reference (tests/qwen_head_ref.py) against `transformers`'
RepetitionPenaltyLogitsProcessor followed by argmax, the mistakes that the reference must catch, handoff.head_plan, the extension header
include/x2i_qwen_head.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and every refusal of its two entry points."""
import ctypes as C
import os

import pytest
import torch

from tests import gemm_ref as G
from tests import qwen_head_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(B, V, K, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((B, K), generator=g).bfloat16()
    W = (torch.randn((V, K), generator=g) * K ** -0.5).bfloat16()
    if shift:
        W = (W.float() + shift * X[0].float()[None] / float(X[0].float().pow(2).sum())).bfloat16()      # every logit of sample 0 moves by shift
    ids = torch.randint(0, V, (B, 12), generator=g)
    return X, W, ids


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("shift", [0.0, -8.0])
def test_reference_is_the_librarys_processor_and_argmax_in_float64(shift):
    """seeded inputs, and a case with every logit negative (the `* penalty` branch everywhere)"""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    B, V, K = 1 if shift else 3, 200, 64
    X, W, ids = _inputs(B, V, K, seed=1, shift=shift)
    seen = HR.seen_of(ids, V)
    want, bound, delta = HR.head_expect(X, W, seen, 1.3)
    l = X.double() @ W.double().T
    if shift:
        assert bool((l < 0).all())
    lib = RepetitionPenaltyLogitsProcessor(HR.f32(1.3))(ids, l.clone())
    assert torch.equal(want, lib)
    assert torch.equal(HR.argmax_lowest(want), lib.argmax(-1))
    assert bool((bound > 0).all()) and bool((delta <= bound).all())
    # unseen elements keep gemm_expect's own bound; penalised ones are wider by max(p, 1 / p) and one rounding
    _, b0, _ = G.gemm_expect(X, W, out_f32=True)
    s = seen.bool()
    assert torch.equal(bound[~s], b0[~s]) and bool((bound[s] >= 1.3 * (b0[s] - G.U_F32 * l[s].abs())).all())
    # the f32 arithmetic of the library's processor lies inside the bound
    f = RepetitionPenaltyLogitsProcessor(1.3)(ids, (X.float() @ W.float().T))
    assert HR.count_over_bound(f, want, bound) == 0


def test_reference_has_a_case_where_the_penalty_changes_the_winner():
    B, V, K = 1, 200, 64
    X, W, _ = _inputs(B, V, K, seed=2)
    l = X.double() @ W.double().T
    top2 = l.topk(2, -1).indices[0]
    assert float(l[0, top2[0]]) > 0 and float(l[0, top2[0]]) / 1.5 < float(l[0, top2[1]])      # the seeded case: the winner falls behind
    seen = HR.seen_of(top2[:1][None], V)
    want, bound, _ = HR.head_expect(X, W, seen, 1.5)
    assert int(HR.argmax_lowest(l)) == int(top2[0]) and int(HR.argmax_lowest(want)) == int(top2[1])
    gap, allow = HR.margin(want, bound)
    assert float(gap) > float(allow) > 0


def test_reference_takes_the_hull_of_both_branches_where_the_sign_is_not_determined():
    X = torch.zeros((1, 64)).bfloat16()
    X[0, 0], X[0, 1] = 1.0, -1.0
    W = torch.zeros((2, 64)).bfloat16()
    W[0, 0], W[0, 1] = 3.0, 3.0                   # l = 0 exactly with delta = 6 U_ACC: either branch
    W[1, 0] = 2.0                                 # l = 2: determined
    seen = torch.ones((1, 2), dtype=torch.uint8)
    want, bound, delta = HR.head_expect(X, W, seen, 2.0)
    d = 6 * G.U_ACC
    assert float(want[0, 0]) == 0.0 and float(bound[0, 0]) >= 2.0 * d and float(want[0, 1]) == 1.0
    assert HR.count_over_bound(torch.tensor([[-2.0 * d, 1.0]]), want, bound) == 0        # l~ = -d took `* penalty`
    assert HR.count_over_bound(torch.tensor([[d / 2.0, 1.0]]), want, bound) == 0         # l~ = +d took `/ penalty`
    assert HR.count_over_bound(torch.tensor([[-2.5 * d, 1.0]]), want, bound) == 1


def test_reference_catches_injected_mistakes():
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    B, V, K = 2, 300, 128
    X, W, ids = _inputs(B, V, K, seed=3)
    W[250], W[17], W[123] = W[40], W[40], W[40]          # one row at four indices: equal logits by construction
    W[[17, 40, 123, 250]] = (W[40].float() + 4.0 * X[0].float() / float(X[0].float().pow(2).sum())).bfloat16()       # ... and sample 0's winner
    seen = HR.seen_of(ids, V)
    seen[:, [17, 40, 123, 250]] = 0
    want, bound, _ = HR.head_expect(X, W, seen, 1.3)
    gap, allow = HR.margin(want, bound, equals=(17, 40, 123, 250))
    assert float(gap[0]) > float(allow[0])
    assert int(HR.argmax_lowest(want)[0]) == 17
    good = RepetitionPenaltyLogitsProcessor(1.3)(ids, X.float() @ W.float().T)
    good = torch.where(seen.bool(), good, X.float() @ W.float().T)
    assert HR.count_over_bound(good, want, bound) == 0 and int(HR.argmax_lowest(good)[0]) == 17
    # highest index on ties
    highest = V - 1 - good.flip(-1).argmax(-1)
    assert int(highest[0]) == 250 and int(highest[0]) != int(HR.argmax_lowest(want)[0])
    # the branches swapped
    l = X.float() @ W.float().T
    swapped = torch.where(seen.bool(), torch.where(l < 0, l / 1.3, l * 1.3), l)
    assert HR.count_over_bound(swapped, want, bound) > 0
    # the penalty on unseen tokens too
    everywhere = torch.where(l < 0, l * 1.3, l / 1.3)
    assert HR.count_over_bound(everywhere, want, bound) > 0
    # a multiplication by the reciprocal in place of the true division stays inside this bound (it is one more rounding): the GPU test
    # compares bits with the library's processor for that
    recip = torch.where(seen.bool(), torch.where(l < 0, l * 1.3, l * (1.0 / torch.tensor(1.3))), l)
    assert HR.count_over_bound(recip, want, bound) == 0


def test_bookkeeping_reference():
    token, seq = torch.zeros(3, dtype=torch.long), torch.full((3, 6), -1)
    lengths, done, seen = torch.zeros(3, dtype=torch.long), torch.tensor([0, 1, 0], dtype=torch.uint8), torch.zeros((3, 10), dtype=torch.uint8)
    col = HR.select_reference(torch.tensor([4, 5, 7]), 2, token, seq, lengths, done, [7, 9], 3, seen)
    assert col == 3 and token.tolist() == [4, 3, 7] and seq[:, 2].tolist() == [4, 3, 7] and int((seq != -1).sum()) == 3
    assert lengths.tolist() == [1, 0, 1] and done.tolist() == [0, 1, 1] and seen.sum(-1).tolist() == [1, 1, 1]
    col = HR.select_reference(torch.tensor([4, 5, 7]), 6, token, seq, lengths, done, [7, 9], 3, seen)       # outside the columns: no store
    assert col == 7 and int((seq != -1).sum()) == 3 and lengths.tolist() == [2, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- head_plan
def test_head_plan_accepts_and_refuses_by_name():
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)
    from x2i_amd.handoff import head_plan
    assert head_plan([]) == 1.0 and head_plan(None) == 1.0
    assert head_plan([RepetitionPenaltyLogitsProcessor(1.05)]) == 1.05
    qwen = [RepetitionPenaltyLogitsProcessor(1.05), TemperatureLogitsWarper(0.1), TopKLogitsWarper(1), TopPLogitsWarper(0.001)]
    assert head_plan(qwen) == 1.05 and head_plan(qwen[::-1]) == 1.05 and head_plan(qwen[1:]) == 1.0
    for bad in (MinLengthLogitsProcessor(3, 1), NoRepeatNGramLogitsProcessor(2)):
        with pytest.raises(ValueError, match=type(bad).__name__):
            head_plan([RepetitionPenaltyLogitsProcessor(1.05), bad])
    with pytest.raises(ValueError, match="prompt_ignore_length"):
        head_plan([RepetitionPenaltyLogitsProcessor(1.05, prompt_ignore_length=4)])
    with pytest.raises(ValueError, match="RepetitionPenaltyLogitsProcessor"):
        head_plan([RepetitionPenaltyLogitsProcessor(1.05), RepetitionPenaltyLogitsProcessor(1.1)])
    zero = TemperatureLogitsWarper(0.5)
    zero.temperature = 0.0                       # (the constructor refuses it; a list can still carry one)
    with pytest.raises(ValueError, match="TemperatureLogitsWarper"):
        head_plan([zero])

    class Mine(TopKLogitsWarper):                # a subclass may compute anything
        pass
    with pytest.raises(ValueError, match="Mine"):
        head_plan([Mine(1)])
    with pytest.raises(ValueError, match="function"):
        head_plan([lambda ids, scores: scores])


def test_harness_takes_the_hip_head_flag_and_it_needs_hip_generate():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("qwenvl")
    assert p.parse_args(["--synthetic"]).hip_head is False
    assert p.parse_args(["--synthetic", "--hip_generate", "--hip_head"]).hip_head is True
    help_text = " ".join(p.format_help().split())
    assert "--hip_head" in help_text and "bf16 ulp" in help_text


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_the_headers_constants_are_the_bindings():
    from x2i_amd import qwen_head_ops
    text = open(os.path.join(ROOT, "include", "x2i_qwen_head.h")).read()
    assert "#define X2I_QWEN_HEAD_ROWS %d\n" % qwen_head_ops.ROWS in text
    assert qwen_head_ops.workspace_floats(2, 152064) == 4 + 2 * 2 * 9504 and qwen_head_ops.workspace_floats(1, 17) == 4 + 2 * 2


def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import qwen_head_ops
    lib = qwen_head_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    odd8, odd4, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1004), C.c_void_p(0x1002)
    err = lambda: lib.x2i_last_error()
    ws_ok = qwen_head_ops.workspace_floats(2, 100)
    la = lambda **kw: lib.x2i_qwen_head_logits_argmax_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("ldx", 64), ("W", fake), ("ldw", 64), ("seen", fake), ("lds", 100), ("pen", 1.05), ("logits", fake), ("ldl", 100), ("step", fake),
        ("ws", fake), ("wsn", ws_ok), ("B", 2), ("V", 100), ("K", 64), ("st", None))])
    assert la(B=0) < 0 and b"B=0" in err()
    assert la(B=9, wsn=10 ** 6) < 0 and b"B=9" in err()
    assert la(K=60) < 0 and b"K=60" in err()
    assert la(K=0) < 0 and la(V=0) < 0
    for bad in (0.0, -1.05, float("inf"), float("nan")):
        assert la(pen=bad) < 0 and b"penalty" in err()
    assert la(ldx=56) < 0 and la(ldw=68) < 0 and la(lds=99) < 0 and la(ldl=99) < 0 and b"aligned" in err()
    assert la(X=odd8) < 0 and b"aligned" in err()
    assert la(W=odd8) < 0 and b"aligned" in err()
    assert la(ws=odd8) < 0 and b"aligned" in err()
    assert la(logits=odd2) < 0 and b"aligned" in err()
    assert la(step=odd2) < 0 and b"aligned" in err()
    assert la(wsn=ws_ok - 1) < 0 and b"workspace too small" in err()
    assert la(V=113, lds=113, ldl=113) < 0 and b"workspace too small" in err()           # one more workgroup per sample
    for k in ("X", "W", "ws"):
        assert la(**{k: None}) < 0 and b"null" in err()
    sel = lambda **kw: lib.x2i_qwen_head_select(*[kw.get(k, d) for k, d in (
        ("ws", fake), ("wsn", ws_ok), ("step", fake), ("token", fake), ("seq", fake), ("ldseq", 32), ("ncols", 32), ("len", fake), ("done", fake),
        ("eos", fake), ("n_eos", 2), ("pad", 3), ("seen", fake), ("lds", 100), ("B", 2), ("V", 100), ("st", None))])
    assert sel(B=0) < 0 and b"B=0" in err()
    assert sel(B=9, wsn=10 ** 6) < 0 and b"B=9" in err()
    assert sel(V=0) < 0 and b"V=0" in err()
    assert sel(n_eos=9) < 0 and b"n_eos=9" in err()
    assert sel(n_eos=-1) < 0 and b"n_eos=-1" in err()
    assert sel(eos=None) < 0 and b"null" in err()
    assert sel(pad=100) < 0 and b"pad=100" in err()
    assert sel(pad=-1) < 0 and b"pad=-1" in err()
    assert sel(ldseq=31) < 0 and sel(ncols=-1) < 0 and sel(lds=99) < 0 and b"ld_seq" in err()
    assert sel(wsn=ws_ok - 1) < 0 and b"workspace too small" in err()
    assert sel(ws=odd8) < 0 and b"aligned" in err()
    assert sel(step=odd2) < 0 and b"aligned" in err()
    for k in ("token", "seq", "len", "eos"):
        assert sel(**{k: odd4}) < 0 and b"aligned" in err()
    for k in ("ws", "step", "token", "seq", "len", "done"):
        assert sel(**{k: None}) < 0 and b"null" in err()
