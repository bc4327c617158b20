"""CPU checks of tests/enc_attn_ref.py: the walk model against a brute-force softmax and a row-by-row statement of the defer rule; every input
kind meeting its coverage condition at every shape tests/test_encoder_attention_fp64_gpu.py launches; the CPU restatement of the kernels'
arithmetic inside the per-element allowance; every planted fault rejected on the new kinds; and, on the suite's EXISTING random inputs, zero
genuine rescales and the rescale faults giving the restatement's own bits -- with the per-tile verdict that passed them printed beside."""
import pytest
import torch

from tests import attn_ref
from tests import clip_ref as CR
from tests import enc_attn_ref as EA
from tests import qwen_ref as QR
from tests import qwen_vision_ref as VR
from tests import t5_ref as TR

ALL = [(e, k, c) for e in EA.ENTRIES for k, c in EA.cases_of(e)[0]]
ALL_IDS = ["%s-%s" % (e, i) for e in EA.ENTRIES for i in EA.cases_of(e)[1]]
RESCALE_FAULTS = ("no_o_rescale", "one_dblock", "alpha_lane0")
WORST = {}


BUILT = {}


def built(entry, kind, case):
    """(inputs, heads, coverage, output shape, (ref, allow)) of a case of the GPU module, built once"""
    key = (entry, kind, repr(case))
    if key not in BUILT:
        inp, heads, cov = EA.build(entry, kind, case)
        shape = EA.out_shape(heads)
        BUILT[key] = (inp, heads, cov, shape, EA.reference(heads, shape))
    return BUILT[key]


# ---------------------------------------------------------------------------------------------------------------- the walk model
def brute_row(s, ok, blocks, rule_keep, m0):
    """One row, plain Python: the running maximum over the key blocks with `rule_keep[step]` saying whether the maximum stays when the row
    grew by no more than THR (per row: always; wave-wide: only when every row of the wave did) -> (genuine per step, sum_j 2^(s_j - m) and m)"""
    m, l, gen = m0, 0.0, []
    for n, (k0, k1) in enumerate(blocks):
        sc = [float(s[j]) if bool(ok[j]) else EA.NEG_BIG for j in range(k0, k1)]
        new = max(m, max(sc))
        if new - m <= EA.THR and rule_keep[n]:
            new = m
        gen.append(new != m and l > 0)
        l = l * 2.0 ** (m - new) + sum(2.0 ** (v - new) for v in sc)
        m = new
    return gen, l, m


@pytest.mark.parametrize("mode", ["relbias", "causal", "ranged", "extend", "segment"])
def test_walk_model_is_the_brute_force_softmax_and_the_defer_rule_row_by_row(mode):
    """Small launches with a strong spike, so that rescales happen: the model's O is softmax(s) V to 1e-12, its final (m, l) give
    sum_j 2^s_j, and its genuine flags are those of brute_row"""
    S, dk = 150, 64
    if mode == "relbias":
        inp, heads, _ = EA.build_t5("spike", dk, S, 128, H=1)
    elif mode == "segment":
        inp, heads, _ = EA.build_vit("spike", 1, S, dk, [70, 80])
    elif mode == "extend":
        inp, heads, _ = EA.build_ext("dead", 1, 2, 1, dk, 192, 70, 80, None)
    else:
        inp, heads, _ = EA.build_causal("spike", 1, 2, 1, S, dk, [40] if mode == "ranged" else None, [140] if mode == "ranged" else None)
    ref, _ = EA.reference(heads, EA.out_shape(heads))
    n_gen = 0
    for hd in heads:
        steps, _, O = EA.walk(hd)
        live = torch.nonzero(hd.live)[:, 0]
        assert float((O[live] - ref[hd.b, hd.h, hd.out_row[live]]).abs().max()) < 1e-12
        for wv, (r0, r1, parts) in enumerate(hd.sched):
            mine = [s for s in steps if s["wave"] == wv]
            if not parts:
                assert not mine
                continue
            keep = [True] * len(mine) if hd.rule == "row" else [bool((s["growth"] <= EA.THR).all()) for s in mine]
            for r in range(r0, r1):
                gen, l, m = brute_row(hd.s2[r], hd.mask[r], parts[0], keep, hd.m0)
                assert gen == [bool(s["genuine"][r - r0]) for s in mine], (mode, wv, r)
                n_gen += sum(gen)
                if bool(hd.mask[r].any()):
                    want = float(torch.exp2(hd.s2[r][hd.mask[r]] - m).sum())
                    assert abs(l - want) <= 1e-12 * want
                else:
                    assert l == 0.0
    assert n_gen > 0


def test_wave_rule_moves_every_row_of_a_moving_wave_and_the_row_rule_only_its_own():
    """Two rows, two blocks, by hand: row 0 grows by 20 in block 1, row 1 by 3.  Wave-wide: both take their new maximum (row 1's alpha is
    2^-3); per row: row 1 keeps alpha = 1.  With row 0 growing by 5 nobody moves under either rule"""
    for grow, want_wave, want_row in ((20.0, [True, True], [True, False]), (5.0, [False, False], [False, False])):
        s = torch.tensor([[0.0, grow], [0.0, 3.0]], dtype=torch.float64)
        for rule, want in (("wave", want_wave), ("row", want_row)):
            hd = EA.Head(0, 0, torch.zeros((2, 1)), torch.zeros((2, 1)), torch.ones((2, 1)), 1.0, torch.ones((2, 2), dtype=torch.bool),
                         [(0, 2, [[(0, 1), (1, 2)]])], rule, EA.M_FLOOR, torch.ones(2, dtype=torch.bool), torch.arange(2))
            hd.s2 = s
            steps, _, _ = EA.walk(hd)
            assert [bool(v) for v in steps[1]["genuine"]] == want, (grow, rule)
            assert not bool(steps[0]["genuine"].any())      # leaving the floor is no rescale: l_run was 0


def test_merge_weights_of_the_resampler_parts_and_the_decode_chunks():
    """The parts cover the counted keys exactly once, in both splits and for ragged counts; the model's merge gives the softmax, and the
    dominant part's weight is 1 while the others' are 2^(m_p - m)"""
    for NQ, nk in ((64, 320), (64, 300), (8, 290), (33, 1001), (8, 33), (64, 1)):
        parts = EA.resampler_parts(NQ, nk)
        keys = sorted(j for p in parts for k0, k1 in p for j in range(k0, k1))
        assert keys == list(range(nk)) and len(parts) == (2 if NQ > 32 else 4)
    inp, heads, cov = EA.build_resampler("spike", 1, 8, 320, 320, [290], 2)
    ref, _ = EA.reference(heads, EA.out_shape(heads))
    _, merges, O = EA.walk(heads[0])
    assert float((O[:8] - ref[0, 0]).abs().max()) < 1e-12
    w = merges[0]["weights"][:, 5]           # row 5 is aligned with a key of part 2
    assert float(w[2]) == 1.0 and float(w.max()) == 1.0 and float(w[[0, 1, 3]].max()) < 2.0 ** -EA.THR
    inp, heads, cov = EA.build_decode("spike", 4, 2, 128, 768, [0], [768], 1)
    _, merges, _ = EA.walk(heads[0])
    w = merges[0]["weights"][:, 0]
    assert float(w[1]) == 1.0 and float(w[[0, 2]].max()) < 2.0 ** -EA.THR and cov["wide"] >= 1


# ---------------------------------------------------------------------------------------------------------------- the kinds
@pytest.mark.parametrize("entry,kind,case", ALL, ids=ALL_IDS)
def test_kind_meets_its_coverage_condition_and_the_restatement_stays_inside_the_allowance(entry, kind, case):
    """Every (entry point, kind, shape) of the GPU module: the inputs do what the kind is for (EA.meets: a genuine rescale, nothing inside
    BAND, and the kind's own condition), and the CPU restatement of the kernel's arithmetic stays inside the per-element allowance"""
    inp, heads, cov, shape, (ref, allow) = built(entry, kind, case)
    assert EA.meets(kind, cov), cov
    if kind == "spike" and entry not in ("decode",):
        assert cov["mixed"] >= 1 or cov["wide"] >= 1
    if inp.get("twice"):       # the construction plants a second, stronger spike in a later tile of rows that walk both
        assert cov["twice"] >= 1, cov
    worst = EA.check_elements("%s %s %s restated" % (entry, kind, case), EA.emulate(heads, shape), ref, allow)
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print("%s %s %s: %d genuine of %d row-steps (+%d merge weights, %d wide), %d mixed waves, %d deferred in (4, 7), %d at a last block, %d rows "
          "rescaled twice, largest growth %.2f; restatement uses %.3f of its allowance"
          % (entry, kind, case, cov["genuine"], cov["row_steps"], cov["merge"], cov["wide"], cov["mixed"], cov["deferred"], cov["last"], cov["twice"],
             cov["max_growth"], worst))


# (entry, kind, case index, faults that case must reject).  one_dblock needs a head wider than 32; a dropped merge weight needs the spike
# outside part 0; the decode kernel has no walk inside a chunk, so only its combine's faults apply; under the ramp every row's alpha is lane
# 0's up to the scores' own spread, so lane 0's alpha is a fault for spike and last, where a moving wave holds both kinds of row
RAMP_FAULTS = ("no_o_rescale", "one_dblock")
PLANTED = [("t5", "spike", 1, RESCALE_FAULTS), ("t5", "ramp", 2, RAMP_FAULTS), ("t5", "last", 3, RESCALE_FAULTS),
           ("clip", "spike", 0, RESCALE_FAULTS), ("qwen", "spike", 2, RESCALE_FAULTS), ("qwen", "ramp", 0, RAMP_FAULTS),
           ("qwen", "last", 1, RESCALE_FAULTS), ("extend", "dead", 0, RESCALE_FAULTS), ("extend", "spike", 1, RESCALE_FAULTS),
           ("vit", "spike", 3, RESCALE_FAULTS), ("vit", "ramp", 4, RAMP_FAULTS), ("vit", "last", 0, RESCALE_FAULTS),
           ("resampler", "spike", 1, RESCALE_FAULTS + ("drop_merge_weight",)), ("resampler", "ramp", 6, RAMP_FAULTS + ("drop_merge_weight",)),
           ("resampler", "last", 7, RESCALE_FAULTS + ("drop_merge_weight",)), ("decode", "spike", 1, ("drop_merge_weight",)),
           ("decode", "ramp", 3, ("drop_merge_weight",))]


@pytest.mark.parametrize("entry,kind,idx,faults", PLANTED, ids=["%s-%s-%d" % p[:3] for p in PLANTED])
def test_planted_faults_are_rejected_per_element_on_the_new_kinds(entry, kind, idx, faults):
    """Each fault in ONE head of the launch.  Beside the per-element verdict, what the per-tile rel-L2 bound TOL_O says of the same output"""
    case = EA.ENTRIES[entry][1][idx]
    inp, heads, cov, shape, (ref, allow) = built(entry, kind, case)
    for fault in faults + ("off_3pct",):
        out = EA.emulate(heads, shape, fault, only=0)
        sh = EA.shares(out, ref, allow)
        tiles = attn_ref.tile_errors(out, ref, shape[2])
        print("%s %s %s, %s: worst element %.1f x its allowance, %d elements over; worst tile rel-L2 %.2e (TOL_O %.0e: %s)"
              % (entry, kind, case, fault, float(sh.max()), int((sh > 1).sum()), float(tiles.max()), attn_ref.TOL_O,
                 "caught" if float(tiles.max()) > attn_ref.TOL_O else "PASSES"))
        with pytest.raises(AssertionError):
            EA.check_elements("planted " + fault, out, ref, allow)


def test_a_wave_wide_test_where_per_row_is_promised_shows_in_the_bits_of_the_other_rows():
    """The overlap layout: the rows below 150 are the same problem with and without the spike of the rows from 150 on.  The restatement
    gives them the same bits; with the wave-wide test planted, the rows that share a wave with a spiked row get other roundings (still
    inside the allowance: only the bit-for-bit comparison of the GPU test sees this fault)"""
    a, b = EA.build_vit_overlap(False), EA.build_vit_overlap(True)
    assert a[2]["genuine"] == 0 and b[2]["genuine"] >= 1 and b[2]["band"] == 0 and a[2]["band"] == 0
    shape, cut = EA.out_shape(a[1]), a[0]["cut"]
    assert torch.equal(EA.emulate(a[1], shape)[:, :, :cut], EA.emulate(b[1], shape)[:, :, :cut])
    fa, fb = EA.emulate(a[1], shape, "wave_rule"), EA.emulate(b[1], shape, "wave_rule")
    changed = (fa[:, :, :cut] != fb[:, :, :cut]).any(-1)
    assert bool(changed.any()) and not bool(changed[:, :, :128].any())         # rows of the wave 128..159, no others
    print("wave-wide test planted: %d of the %d rows 128..%d of the two heads change bits" % (int(changed.sum()), 2 * (cut - 128), cut - 1))
    ref, allow = EA.reference(b[1], shape)
    EA.check_elements("wave-wide fault, values", fb, ref, allow)


# ---------------------------------------------------------------------------------------------------------------- the existing inputs
def _existing():
    """(name, heads) of every input the existing T5, CLIP, Qwen2 and vision attention tests draw for their float64 comparison, whole, with
    their seeds.  (The resampler and decode tests draw theirs on the device; they are not recounted here.)"""
    from tests.test_clip_gpu import ATTENTION_CASES as CLIP
    from tests.test_qwen_gpu import ATTENTION_CASES as QWEN
    from tests.test_qwen_vision_gpu import ATTENTION_CASES as VIT
    from tests.test_t5_gpu import ATTENTION_CASES as T5
    for B, Hq, Hkv, S, dk, lo, hi in QWEN:
        Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=1000 * S + dk + Hq)
        yield "qwen %s" % ((B, Hq, Hkv, S, dk, lo, hi),), EA.problem_causal(Q, K, V, S, dk ** -0.5, lo, hi)
    for B, H, S, dk, R in T5:
        Q, K, V, table = TR.attention_inputs(B, H, S, dk, R, seed=1000 * S + dk + R)
        yield "t5 %s" % ((B, H, S, dk, R),), EA.problem_relbias(Q, K, V, table, S, R)
    for B, H, S in CLIP:
        Q, K, V = CR.attention_inputs(B, H, S, 64, seed=1000 * S + H)
        yield "clip %s" % ((B, H, S),), EA.problem_causal(Q, K, V, S, 64 ** -0.5)
    for B, H, S, dk, segs in VIT:
        pairs = [VR.segment_ranges(sg) for sg in segs]
        Q, K, V = VR.attention_inputs(B, H, S, dk, seed=1000 * S + dk + H)
        yield "vit %s" % ((B, H, S, dk, segs),), EA.problem_segment(Q, K, V, S, dk, dk ** -0.5, [p[0] for p in pairs], [p[1] for p in pairs])


def test_existing_random_inputs_hardly_ever_rescale_and_let_the_rescale_faults_through():
    """The gap this module closes.  Over the existing tests' own inputs the walk model counts the genuine rescales per head: none in the
    Qwen2 cases (the largest growth is 7.22, below THR) and in most others.  In a head without one the rescale faults give the
    restatement's own bits -- no check of any kind can see them there -- and that is asserted.  Where a draw does move a wave (growths just
    past 8, accidents of the seed: CLIP at S = 300, one vision case, some heads of the T5 product shape), the count is printed with what
    the per-tile bound says of the faulted restatement of those heads: such a case could have seen a fault, in the mode and width it runs"""
    total = moved = 0
    for name, heads in _existing():
        covs = [EA.coverage([hd]) for hd in heads]
        steps, gen = sum(c["row_steps"] for c in covs), sum(c["genuine"] for c in covs)
        total += steps
        moved += gen
        line = "%s: %d genuine of %d row-steps, largest growth %.2f" % (name, gen, steps, max(c["max_growth"] for c in covs))
        if name.startswith("qwen"):
            assert gen == 0, line
        still = [hd for hd, c in zip(heads, covs) if c["genuine"] == 0]
        moving = [hd for hd, c in zip(heads, covs) if c["genuine"] > 0]
        shape = EA.out_shape(heads)
        ref, allow = EA.reference(heads, shape)
        good = EA.emulate(still, shape)
        for fault in RESCALE_FAULTS:
            assert torch.equal(EA.emulate(still, shape, fault), good), (name, fault)
        line += "; %d of %d heads never rescale: %s give them identical bits" % (len(still), len(heads), ", ".join(RESCALE_FAULTS))
        if moving:
            good = EA.emulate(heads, shape)
            verdicts = []
            for fault in RESCALE_FAULTS:
                bad = good.clone()
                sel = [(hd.b, hd.h) for hd in moving]
                part = EA.emulate(moving, shape, fault)
                for b_, h_ in sel:
                    bad[b_, h_] = part[b_, h_]
                worst = float(attn_ref.tile_errors(bad, ref, shape[2]).max())
                verdicts.append("%s %.2e (%s)" % (fault, worst, "caught" if worst > attn_ref.TOL_O else "PASSES"))
            line += "; in the %d that do, the per-tile bound says: %s" % (len(moving), ", ".join(verdicts))
        assert float(attn_ref.tile_errors(EA.emulate(heads, shape), ref, shape[2]).max()) <= attn_ref.TOL_O
        print(line)
    print("existing inputs: %d genuine rescales in %d row-steps" % (moved, total))


def test_the_full_launch_beside_an_extension_case_moves_no_rescale_of_its_own():
    """tests/test_encoder_attention_fp64_gpu.py compares the extension with the full launch over the same buffers, bit for bit from the first
    32-row group without dead rows on.  That holds where the full launch's own rows >= S (zero rows of Q there) move no rescale: its walk,
    modelled here as the kernel runs it, has nothing inside BAND and rescales as the extension does"""
    for kind, case in EA.cases_of("extend")[0]:
        inp, heads, cov, shape, _ = built("extend", kind, case)
        B, Hq, Hkv, dk, cap, row0, n, k_lo = case
        S = row0 + n
        full = EA.coverage(EA.problem_causal(inp["Q"], inp["K"], inp["V"], S, dk ** -0.5, k_lo, [S] * B))
        assert full["band"] == 0 and full["genuine"] >= cov["genuine"] >= 1, (kind, case, full)


def test_print_worst():
    """(last: the restatement's worst share of the allowance per entry point, over every case above)"""
    print("\n  CPU restatement, worst share of the per-element allowance: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert WORST and all(v <= 1.0 for v in WORST.values())
