"""tests/sample_ref.py checked without a GPU: Philox's known answers, the reference's kept set against the installed `transformers`
warpers, the stated tie rule, planted faults that the verdict must catch, the coverage conditions of every case tests/test_sample_gpu.py
runs, and handoff.sample_plan."""
import numpy as np
import pytest
import torch

from tests import sample_ref as R


def test_philox_known_answers():
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        assert "%08x %08x %08x %08x" % R.philox4x32_10(ctr, key) == want
    # the kernel's uniform: 24 bits of word 0, the counter's two halves from offset + col
    x = R.philox4x32_10((2, 1, 3, 0), (7, 0))[0]
    assert R.uniform(7, 2 ** 32 - 3, 5, 3) == np.float32((x >> 8) * 2.0 ** -24) and 0 <= R.uniform(7, 2 ** 32 - 3, 5, 3) < 1
    assert R.uniform(7, 2 ** 64 - 2, 6, 0) == R.uniform(7, 0, 4, 0)          # modulo 2^64


def library_keep(p, temperature, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = TemperatureLogitsWarper(float(temperature))(None, torch.from_numpy(p)[None])
    if top_k > 0:
        s = TopKLogitsWarper(int(top_k))(None, s)
    if top_p < 1:
        s = TopPLogitsWarper(float(top_p))(None, s.double())      # (the library's softmax in float64: the cut is no matter of f32 rounding)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("V", [1, 17, 1000])
def test_kept_set_is_the_librarys_on_tie_free_rows(V):
    n = 0
    for seed in range(3):
        p = R.scores("normal", V, 40 + seed)
        assert np.unique(p).size == V
        for T in (0.1, 0.7, 1.0, 5.0):
            for k in (0, 1, 2, 50, V, V + 5):
                for pp in (1.0, 0.95, 0.8, 0.3, 1e-6):
                    ref = R.select(p, T, k, pp)
                    if not ref.margin > 0:
                        continue                                      # (the cut within rounding of a fraction: either answer is right)
                    assert np.array_equal(ref.keep, library_keep(p, T, k, pp)), (V, seed, T, k, pp)
                    if pp == 1e-6 or k == 1:
                        assert ref.count == 1 and ref.keep[p.argmax()]
                    if k >= V and pp == 1.0:
                        assert ref.count == V
                    n += 1
    assert n > 300


def test_the_tie_rule_keeps_or_drops_equal_values_together():
    # across the top-k boundary: the k-th and the (k + 1)-th are equal, both are kept
    p = R.scores("tie", 1000, 3, top_k=50)
    ref = R.select(p, 0.7, 50, 1.0)
    assert ref.count == 51 and ref.survivors == 51
    assert R.select(p, 0.7, 50, 1.0, topk_strict=True).count == 49
    # two levels: top-p keeps a level or drops it, where the library splits the run by sort position (the one deviation)
    p = R.scores("two", 70, 0)                                      # 10 tokens at 2, 60 at -1: the upper level holds 77 % of the mass
    for pp, want in ((0.5, 10), (0.76, 10), (0.78, 70), (0.99, 70)):
        ref = R.select(p, 1.0, 0, pp)
        assert ref.count == want and (ref.keep[::7].all()) and len(set(ref.keep[p == -1])) == 1
    assert 10 < library_keep(p, 1.0, 0, 0.9).sum() < 70
    # all equal: everything is kept under any top_p
    assert R.select(R.scores("flat", 33, 0), 0.1, 0, 1e-6).count == 33
    # -0 and +0 are one value
    assert R.select(np.array([0.0, -0.0, -1.0], np.float32), 1.0, 2, 1.0).count == 2


def planted_case():
    p = R.scores("normal", 17, 8)
    ref = R.select(p, 0.7, 0, 0.9)
    return p, ref


def test_the_verdict_catches_planted_faults():
    p, ref = planted_case()
    diag = (ref.count, ref.Z)
    us = [np.float32(u) for u in R.U_FIXED]
    assert all(R.admitted(ref, u).size == 1 for u in us)
    for u in us:
        n = R.draw(ref, u)
        assert R.verdict(ref, n, u, *diag) == []
        # an off-by-one token
        assert R.verdict(ref, n + 1, u, *diag) and R.verdict(ref, n - 1, u, *diag)
        # a wrong kept count, a Z outside eps
        assert R.verdict(ref, n, u, ref.count + 1, ref.Z) and R.verdict(ref, n, u, ref.count, ref.Z * (1 + 2 * R.eps(ref.count)))
    # a draw in descending order of the token index
    assert sum(bool(R.verdict(ref, R.draw(ref, u, descending=True), u, *diag)) for u in us) >= len(us) - 1
    # u from word 1: another value, another token's interval
    caught = 0
    for b in range(8):
        u0, u1 = R.uniform(9, 0, 4, b), R.uniform(9, 0, 4, b, word=1)
        assert u0 != u1
        caught += bool(R.verdict(ref, R.draw(ref, u1), u0, *diag))
    assert caught >= 6
    # `>` for `>=` at the top-k threshold: the tie across the boundary loses both tokens
    pt = R.scores("tie", 1000, 3, top_k=50)
    good, fault = R.select(pt, 0.7, 50, 1.0), R.select(pt, 0.7, 50, 1.0, topk_strict=True)
    assert R.verdict(good, R.draw(fault, 0.5), 0.5, fault.count, fault.Z)
    # `<=` for `<` at top-p: a top_p that equals a mass fraction exactly (taken as float64: no f32 top_p does) keeps one token more
    found = 0
    for seed in range(20):
        q = R.scores("normal", 17, 100 + seed)
        full = R.select(q, 1.0, 0, 1.0)
        order = np.argsort(-q)
        frac = np.cumsum((full.hi - full.lo)[order] * full.Z) / np.sum((full.hi - full.lo) * full.Z)
        tp = float(frac[2])                                          # the mass strictly above the fourth token
        good, fault = R.select(q, 1.0, 0, tp, top_p_exact=True), R.select(q, 1.0, 0, tp, top_p_exact=True, topp_inclusive=True)
        if fault.count == good.count + 1:
            found += 1
            assert good.count == 3 and R.verdict(good, R.draw(fault, 0.5), 0.5, fault.count, fault.Z)
    assert found >= 5


def test_every_gpu_case_meets_the_coverage_conditions_and_the_cases_cover_the_axes():
    cases = R.cases()
    assert 100 <= len(cases) <= 110 and len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        assert R.coverage(c) == [], c["id"]
    for axis, values in (("V", R.VS), ("B", R.BS), ("top_p", R.PS), ("temperature", R.TS), ("kind", R.KINDS)):
        assert {c[axis] for c in cases} == set(values), axis
    assert {min(c["top_k"], 51) if c["top_k"] != c["V"] + 5 else "V+5" for c in cases} >= {0, 1, 2, 50, "V+5"}
    assert {c["kind"] for c in cases if c["V"] == R.VS[-1]} == set(R.KINDS)
    assert all(c["temperature"] == 0.1 for c in cases if c["kind"] == "ramp")
    # what the kinds are for
    big = [c for c in cases if c["V"] == R.VS[-1]]
    ramp = [R.reference(c, 0) for c in big if c["kind"] == "ramp" and c["top_k"] == 0 and c["top_p"] == 1.0]
    assert ramp and all(r.count == R.VS[-1] and r.Z < 2.55 for r in ramp)                  # the whole row kept, nearly all of it without mass
    assert any(R.reference(c, 0).count == 1 for c in big if c["kind"] == "spike")
    assert all(R.reference(c, 0).count == c["V"] for c in cases if c["kind"] == "flat")
    assert all(R.rows(c)[0].argmax() == c["V"] - 1 for c in cases if c["kind"] == "lastmax")
    tie = [c for c in cases if c["kind"] == "tie" and 0 < c["top_k"] < c["V"] and c["top_p"] == 1.0]
    assert tie and all(R.reference(c, 0).count == c["top_k"] + 1 for c in tie)
    # draws with one admitted token are the rule, not the exception
    small = [(c, b) for c in cases for b in range(c["B"]) if R.reference(c, b).count <= 1024]
    assert len(small) > 200
    # the Philox draws cross 2^32 and 2^64
    assert any(o + c >= 2 ** 32 > o for _, o, c in R.PHILOX) and any(o + c >= 2 ** 64 for _, o, c in R.PHILOX)


def test_eps_is_what_the_docstring_derives():
    assert R.R == 25 * 2.0 ** -24 + 2.0 ** -23
    assert abs(R.eps(1024) - 3.3e-6) < 1e-7 and abs(R.eps(151936) - 1.2e-5) < 1e-6
    assert R.eps_cut(0.0, 0, 151936, 1e-6) < 1e-9 and R.eps_cut(0.8, 151936, 151936, 0.8) <= 2 * R.eps(151936)


# ---- handoff.sample_plan ----------------------------------------------------------------------------------------------------------------
def test_sample_plan_accepts_the_librarys_lists_and_refuses_the_rest_by_name():
    from transformers import GenerationConfig
    from transformers.generation import logits_process as LP
    from x2i_amd.handoff import head_plan, sample_plan
    gc = GenerationConfig(do_sample=True)
    rp, te, tk, tp = LP.RepetitionPenaltyLogitsProcessor(1.05), LP.TemperatureLogitsWarper(0.7), LP.TopKLogitsWarper(20), LP.TopPLogitsWarper(0.8)
    assert sample_plan(gc, [rp, te, tk, tp]) == (1.05, 0.7, 20, 0.8)
    assert sample_plan(gc, []) == (1.0, 1.0, 0, 1.0) and sample_plan(gc, None) == (1.0, 1.0, 0, 1.0)
    assert sample_plan(gc, [te, tp]) == (1.0, 0.7, 0, 0.8) and sample_plan(gc, [rp, tk]) == (1.05, 1.0, 20, 1.0)
    assert sample_plan(None, [tk]) == (1.0, 1.0, 20, 1.0)
    assert sample_plan(GenerationConfig(do_sample=False), [rp])[2] == 1             # a config that does not sample: the argmax
    # what Qwen2.5-VL ships, through the library's own list
    from transformers import Qwen2ForCausalLM
    from tests import qwen_ref as QR
    shipped = GenerationConfig(do_sample=True, temperature=0.1, top_k=50, top_p=0.001, repetition_penalty=1.05)
    procs = Qwen2ForCausalLM(QR.library_config(64, 2, 1, 128, 1))._get_logits_processor(shipped, input_ids_seq_length=4, device="cpu")
    assert [type(q).__name__ for q in procs] == ["RepetitionPenaltyLogitsProcessor", "TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper"]
    plan = sample_plan(shipped, procs)
    assert plan[0] == 1.05 and plan[2] == 50 and abs(plan[1] - 0.1) < 1e-12 and abs(plan[3] - 0.001) < 1e-12
    # the library's order only, one of each
    for bad in ([te, rp], [tk, te], [tp, tk], [te, te], [rp, te, tp, tk]):
        with pytest.raises(ValueError, match="order"):
            sample_plan(gc, bad)
    # every other processor, by its class name; a subclass too
    class MyTopK(LP.TopKLogitsWarper):
        pass
    others = [LP.MinPLogitsWarper(0.1), LP.TypicalLogitsWarper(0.9), LP.EpsilonLogitsWarper(0.01), LP.EtaLogitsWarper(0.01),
              LP.MinLengthLogitsProcessor(3, 1), LP.NoRepeatNGramLogitsProcessor(2), MyTopK(5)]
    for p in others:
        with pytest.raises(ValueError, match=type(p).__name__):
            sample_plan(gc, [rp, te, p])
    with pytest.raises(ValueError, match="num_beams=4"):
        sample_plan(GenerationConfig(do_sample=True, num_beams=4), [te])
    with pytest.raises(ValueError, match="TopPLogitsWarper has min_tokens_to_keep=2"):
        sample_plan(gc, [LP.TopPLogitsWarper(0.8, min_tokens_to_keep=2)])
    with pytest.raises(ValueError, match="TopKLogitsWarper has min_tokens_to_keep=3"):
        sample_plan(gc, [LP.TopKLogitsWarper(5, min_tokens_to_keep=3)])
    with pytest.raises(ValueError, match="TopKLogitsWarper has filter_value"):
        sample_plan(gc, [LP.TopKLogitsWarper(5, filter_value=-1e4)])
    with pytest.raises(ValueError, match="TopPLogitsWarper has filter_value"):
        sample_plan(gc, [LP.TopPLogitsWarper(0.5, filter_value=0.0)])
    with pytest.raises(ValueError, match="prompt_ignore_length"):
        sample_plan(gc, [LP.RepetitionPenaltyLogitsProcessor(1.1, prompt_ignore_length=3)])
    # head_plan is what it was: any order, the warpers dropped, its own messages
    assert head_plan([te, rp, tk, tp]) == 1.05 and head_plan([tk, tp]) == 1.0 and head_plan(None) == 1.0
    with pytest.raises(ValueError, match="hip_head cannot fuse the logits processor MinPLogitsWarper"):
        head_plan([LP.MinPLogitsWarper(0.1)])


def test_the_scripts_take_the_flags_and_refuse_them_without_hip_head():
    from x2i_amd.infer.harness import build_parser, sample_seed
    from x2i_amd.infer.inference_multi_turn import MultiTurnConditioner
    from x2i_amd.infer.inference_qwenvl import QwenVLConditioner
    p = build_parser("qwenvl")
    a = p.parse_args(["--synthetic"])
    assert a.hip_sample is False and a.hip_sample_seed is None and sample_seed(a) == 0
    a = p.parse_args(["--synthetic", "--hip_generate", "--hip_head", "--hip_sample", "--seed", "7"])
    assert a.hip_sample is True and sample_seed(a) == 7
    assert sample_seed(p.parse_args(["--synthetic", "--seed", "7", "--hip_sample_seed", "9"])) == 9
    help_text = " ".join(p.format_help().split())
    assert "--hip_sample" in help_text and "greedy only" not in help_text
    none = "/nonexistent/checkpoint/that/must/never/be/read"
    for make in (lambda: QwenVLConditioner(none, "cpu", hip_generate=True, hip_sample=True),
                 lambda: QwenVLConditioner(none, "cpu", hip_head=True, hip_sample=True),
                 lambda: MultiTurnConditioner(none, "cpu", hip_generate=True, hip_sample=True),
                 lambda: MultiTurnConditioner(none, "cpu", hip_sample=True)):
        with pytest.raises(ValueError, match="--hip_sample"):
            make()
