"""Every attention launch of the encoder and decoder extensions on inputs that FORCE the late softmax rescale, against float64 per element.

The kernels (encoder_attention.hip in its five modes, resampler_attn_kernel in both splits, decode_attention_kernel with its combine) keep a
running maximum while no row grew by more than 8 in the exp2 domain; the suite's random inputs make it move after a row's first tile only
by accident of a seed, in three cases (tests/test_enc_attn_ref_cpu.py counts it), so the rescale of l and O, the merge weights and the
wave-wide test went unchecked in most modes and widths.  Here every
case is built by tests/enc_attn_ref.py for one input kind -- spike, ramp, last, dead -- and asserts through the walk model, BEFORE it
launches, that its inputs do what the kind is for.  Then, per element,

    |O - ref| <= TOL_ROW |ref| + 2^-8 A + F32 A        (enc_attn_ref.reference: derived, nothing fitted to a kernel)

beside the family's per-tile rel-L2 bound TOL_O, the write set on a sentinel-filled buffer, and the bit-level promises: CLIP = Qwen2, the
extension = the full launch, a row of a vision segment independent of the other segments' rows, a masked twin of the spike changing
nothing.  The worst share of the allowance used per entry point is printed at the end (WORST)."""
import time

import pytest
import torch

from tests import attn_ref
from tests import enc_attn_ref as EA
from tests import resampler_ref as RR
from tests.test_clip_gpu import clip_ops, run_attention as run_clip                    # noqa: F401  (fixtures and launch helpers; the
from tests.test_qwen_decode_gpu import qd, run_decode_attention                        # noqa: F401   tests of those modules are not
from tests.test_qwen_extend_gpu import qx, run_extend_attention, run_full_attention    # noqa: F401   re-collected here)
from tests.test_qwen_gpu import qwen_ops, run_attention as run_qwen                    # noqa: F401
from tests.test_qwen_vision_gpu import run_attention as run_vit, vit_ops               # noqa: F401
from tests.test_resampler_gpu import rops, run_attention as run_resampler              # noqa: F401
from tests.test_t5_gpu import is_sentinel, run_attention as run_t5, t5_ops             # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
CLOCK = []          # when the module's first case started


def prepared(entry, kind, case):
    """the case's inputs and heads, its coverage condition asserted (a case does not skip itself: inputs that miss it fail)"""
    CLOCK.append(time.time())
    inp, heads, cov = EA.build(entry, kind, case)
    assert EA.meets(kind, cov), "%s %s %s: the inputs miss the kind's coverage condition: %r" % (entry, kind, case, cov)
    assert not inp.get("twice") or cov["twice"] >= 1, "%s %s %s: no row takes the two rescales the second spike is for: %r" % (entry, kind, case, cov)
    return inp, heads, cov


def on_gpu(inp, *names):
    return [inp[n].to(DEV) for n in names]


def check(entry, kind, case, O, heads, cov, tile_rows=64):
    """O [B, H, rows, d] against float64: per element, and per tile as the family is checked everywhere else"""
    name = "%s %s %s" % (entry, kind, case)
    ref, allow = EA.reference(heads, EA.out_shape(heads))
    O = O.float().cpu()
    assert tuple(O.shape) == tuple(ref.shape), (O.shape, ref.shape)
    worst = EA.check_elements(name, O, ref, allow)
    tile = attn_ref.check_tiles(name, O, ref, attn_ref.TOL_O, rows=tile_rows)
    WORST[entry] = max(WORST.get(entry, 0.0), worst)
    print("%s: %d genuine rescales of %d row-steps (%d rows twice), %d merge weights (%d wide), largest growth %.1f; worst element %.3f of its allowance, "
          "worst tile rel-L2 %.2e (bound %.0e)" % (name, cov["genuine"], cov["row_steps"], cov["twice"], cov["merge"], cov["wide"], cov["max_growth"], worst,
                                                    tile, attn_ref.TOL_O))


def masked_twins(K, u, dk, lo, hi, S):
    """K [1, Hkv, .., dk] of one sample with the spike's key shift, at twice the strength, at the keys k_lo - 1 and k_lo - 3 -- in the first
    walked tile, just below the range, where only the in-tile lower mask keeps them out -- and at k_hi, just beyond it: the aligned rows would
    score them 60 above an ordinary key"""
    for key in ([lo - 1, lo - 3] if lo is not None and lo >= 3 else []) + ([hi] if hi is not None and hi < S else []):
        K = EA.with_spike_at(K, u, key, dk ** -0.5 * EA.LOG2E, 2.0)
    return K


def wrote_exactly(buf, rows, cols):
    """nothing outside rows < `rows` and columns < `cols` of buf [B, rows + extra, cols + extra] is written, and every element inside is"""
    assert bool(is_sentinel(buf[:, rows:]).all()) and bool(is_sentinel(buf[:, :, cols:]).all())
    assert not bool(is_sentinel(buf[:, :rows, :cols]).any())


# ---------------------------------------------------------------------------------------------------------------- T5 (RELBIAS)
@pytest.mark.parametrize("kind,case", EA.cases_of("t5")[0], ids=EA.cases_of("t5")[1])
def test_t5_attention_rescales(t5_ops, kind, case):
    inp, heads, cov = prepared("t5", kind, case)
    Q, K, V, table = on_gpu(inp, "Q", "K", "V", "table")
    S, R = inp["S"], inp["R"]
    O, buf = run_t5(t5_ops, Q, K, V, table, S, R, extra_cols=8, extra_rows=3)
    check("t5", kind, case, O, heads, cov)
    wrote_exactly(buf, S, Q.shape[1] * Q.shape[3])
    assert torch.equal(run_t5(t5_ops, Q, K, V, table, S, R, extra_cols=8, extra_rows=3)[0], O)
    if kind != "ramp":     # the masked twin: the spike's key shift repeated at a padding key of the ragged last tile changes no bit
        K2 = EA.with_spike_at(inp["K"], inp["u"], S + 5, EA.LOG2E).to(DEV)
        assert torch.equal(run_t5(t5_ops, Q, K2, V, table, S, R, extra_cols=8, extra_rows=3)[0], O)


# ---------------------------------------------------------------------------------------------------------------- CLIP (CAUSAL_PLAIN)
@pytest.mark.parametrize("kind,case", EA.cases_of("clip")[0], ids=EA.cases_of("clip")[1])
def test_clip_attention_rescales_and_is_the_qwen_kernel_bit_for_bit(clip_ops, qwen_ops, kind, case):
    inp, heads, cov = prepared("clip", kind, case)
    Q, K, V = on_gpu(inp, "Q", "K", "V")
    B, H, S = case
    O, buf = run_clip(clip_ops, Q, K, V, S, extra_cols=8, extra_rows=3)
    check("clip", kind, case, O, heads, cov)
    wrote_exactly(buf, S, H * 64)
    Oq, _ = run_qwen(qwen_ops, Q, K, V, S, scale=64 ** -0.5)
    assert torch.equal(Oq, O), "CAUSAL_PLAIN and CAUSAL differ on %s inputs" % kind
    if kind != "ramp":     # the masked twin, in the padding beyond S
        K2 = EA.with_spike_at(inp["K"], inp["u"], S + 5, 64 ** -0.5 * EA.LOG2E).to(DEV)
        assert torch.equal(run_clip(clip_ops, Q, K2, V, S, extra_cols=8, extra_rows=3)[0], O)


# ---------------------------------------------------------------------------------------------------------------- Qwen2 prefill (CAUSAL)
@pytest.mark.parametrize("kind,case", EA.cases_of("qwen")[0], ids=EA.cases_of("qwen")[1])
def test_qwen_attention_rescales(qwen_ops, kind, case):
    """Rows before k_lo have a zero allowance: exactly 0.  With k_lo = 70 inside the wave 64..95 the spike sits on either side of it, in the
    first walked tile: key 70 itself carries a third of a spike for the aligned rows (an in-tile lower mask off by one loses it), and the
    masked twins -- the key shift at twice the strength at 69 and 67, at k_hi, and in the padding beyond S, per sample -- change no bit"""
    inp, heads, cov = prepared("qwen", kind, case)
    Q, K, V = on_gpu(inp, "Q", "K", "V")
    B, Hq, Hkv, S, dk, k_lo, k_hi = case
    O, buf = run_qwen(qwen_ops, Q, K, V, S, k_lo, k_hi, extra_cols=8, extra_rows=3)
    check("qwen", kind, case, O, heads, cov)
    wrote_exactly(buf, S, Hq * dk)
    assert torch.equal(run_qwen(qwen_ops, Q, K, V, S, k_lo, k_hi, extra_cols=8, extra_rows=3)[0], O)
    if B > 1:
        one = lambda v: None if v is None else v[:1]
        O1, _ = run_qwen(qwen_ops, Q[:1].contiguous(), K[:1].contiguous(), V[:1].contiguous(), S, one(k_lo), one(k_hi))
        assert torch.equal(O1[0], O[0])
    if kind != "ramp":
        K2 = EA.with_spike_at(inp["K"], inp["u"], S + 5, dk ** -0.5 * EA.LOG2E, 2.0)
        for b in range(B):
            K2[b:b + 1] = masked_twins(K2[b:b + 1], inp["u"][b:b + 1], dk, None if k_lo is None else k_lo[b], None if k_hi is None else k_hi[b], S)
        K2 = K2.to(DEV)
        assert not torch.equal(K2, K)
        O2, _ = run_qwen(qwen_ops, Q, K2, V, S, k_lo, k_hi, extra_cols=8, extra_rows=3)
        assert torch.equal(O2, O), "spikes at masked keys changed the result"


# ---------------------------------------------------------------------------------------------------------------- the prompt extension
@pytest.mark.parametrize("kind,case", EA.cases_of("extend")[0], ids=EA.cases_of("extend")[1])
def test_extend_attention_rescales_and_is_the_full_launch_where_the_geometry_is(qx, kind, case):
    """row0 = 70 lies inside the wave 64..95.  `dead`: live rows of that wave, and of the wave that holds S - 1, meet the spike while the
    wave's other rows are dead.  From row 96 on every 32-row group holds rows >= row0 only, and the full launch over the same buffers gives
    the same bits (its own rows >= S read the zero rows of Q there and, by the walk model of that launch, move no rescale either)"""
    inp, heads, cov = prepared("extend", kind, case)
    Q, K, V = on_gpu(inp, "Q", "K", "V")
    B, Hq, Hkv, dk, cap, row0, n, k_lo = case
    O, buf = run_extend_attention(qx, Q, K, V, row0, n, k_lo)
    check("extend", kind, case, O, heads, cov)
    wrote_exactly(buf, n, Hq * dk)
    assert torch.equal(run_extend_attention(qx, Q, K, V, row0, n, k_lo)[0], O)
    S = row0 + n
    full_cov = EA.coverage(EA.problem_causal(inp["Q"], inp["K"], inp["V"], S, dk ** -0.5, k_lo, [S] * B))
    assert full_cov["band"] == 0 and full_cov["genuine"] >= 1
    first = (row0 + 31) // 32 * 32
    full = run_full_attention(Q, K, V, S, k_lo)
    assert torch.equal(O[:, :, first - row0:], full[:, :, first:])
    # a function of live data only: the spike's key shift repeated in a slot beyond S changes no bit
    if kind != "ramp":
        K2 = EA.with_spike_at(inp["K"], inp["u"], S + 5, dk ** -0.5 * EA.LOG2E, 2.0)
        for b in range(B):     # and just below a k_lo inside tile 0 (keys 39 and 37 of the second sample)
            K2[b:b + 1] = masked_twins(K2[b:b + 1], inp["u"][b:b + 1], dk, None if k_lo is None else k_lo[b], None, S)
        assert torch.equal(run_extend_attention(qx, Q, K2.to(DEV), V, row0, n, k_lo)[0], O)


# ---------------------------------------------------------------------------------------------------------------- the vision towers (SEGMENT)
@pytest.mark.parametrize("kind,case", EA.cases_of("vit")[0], ids=EA.cases_of("vit")[1])
def test_vit_attention_rescales(vit_ops, kind, case):
    """One segment of five tiles at the three widths, frames with a spike per frame, windows with boundaries inside a tile.  The masked
    twin: the spike's key shift repeated at a key of the SECOND segment, which the spiked rows of the other segments do not count -- every
    row outside the second segment keeps its bits"""
    inp, heads, cov = prepared("vit", kind, case)
    Q, K, V = on_gpu(inp, "Q", "K", "V")
    H, S, dk, segs = case
    O, buf = run_vit(vit_ops, Q, K, V, S, dk, inp["lo"], inp["hi"], extra_cols=8, extra_rows=3)
    check("vit", kind, case, O, heads, cov)
    wrote_exactly(buf, S, H * dk)
    assert torch.equal(run_vit(vit_ops, Q, K, V, S, dk, inp["lo"], inp["hi"], extra_cols=8, extra_rows=3)[0], O)
    if len(segs) > 1 and kind != "ramp":
        a, b = segs[0], segs[0] + segs[1]
        K2 = EA.with_spike_at(inp["K"], inp["u"], a + segs[1] // 2, dk ** -0.5 * EA.LOG2E).to(DEV)
        O2, _ = run_vit(vit_ops, Q, K2, V, S, dk, inp["lo"], inp["hi"], extra_cols=8, extra_rows=3)
        assert torch.equal(O2[:, :, :a], O[:, :, :a]) and torch.equal(O2[:, :, b:], O[:, :, b:])
        if segs[1] >= 48:      # (the segment holds spiked rows, which score that key 30 higher now)
            assert not torch.equal(O2[:, :, a:b], O[:, :, a:b])


def test_vit_attention_row_is_bit_identical_when_other_rows_of_its_wave_get_the_spike(vit_ops):
    """The overlap layout (enc_attn_ref.OVERLAP): rows < 150 count the keys [0, 200), rows >= 150 the keys [40, 300); the wave 128..159 holds
    both and tile 2 holds key 150, which both count.  Second launch: rows 152, 157, .. aligned with that key, so their maximum moves by 30 at
    tile 2 -- K is unchanged.  The rows < 150 are the same problem in both launches and keep every bit: the defer test is per row
    (a wave-wide test changes rows among 128..149 on the CPU restatement, tests/test_enc_attn_ref_cpu.py)"""
    plain, spiked = EA.build_vit_overlap(False), EA.build_vit_overlap(True)
    assert plain[2]["genuine"] == 0 and spiked[2]["genuine"] >= 1 and plain[2]["band"] == 0 and spiked[2]["band"] == 0
    outs = []
    for inp, heads, cov in (plain, spiked):
        Q, K, V = on_gpu(inp, "Q", "K", "V")
        O, _ = run_vit(vit_ops, Q, K, V, inp["S"], inp["dk"], inp["lo"], inp["hi"])
        check("vit", "overlap" + ("+spike" if cov["genuine"] else ""), EA.OVERLAP, O, heads, cov)
        outs.append(O)
    cut = plain[0]["cut"]
    assert torch.equal(plain[0]["K"], spiked[0]["K"]) and torch.equal(plain[0]["Q"][:, :, :cut], spiked[0]["Q"][:, :, :cut])
    assert torch.equal(outs[0][:, :, :cut], outs[1][:, :, :cut])
    assert not torch.equal(outs[0][:, :, cut:], outs[1][:, :, cut:])


# ---------------------------------------------------------------------------------------------------------------- the resampler
@pytest.mark.parametrize("kind,case", EA.cases_of("resampler")[0], ids=EA.cases_of("resampler")[1])
def test_resampler_attention_rescales_and_merges(rops, kind, case):
    """NP = 2 (NQ 64, 33) and NP = 4 (NQ 8), the spike in each key part in turn so that the merge meets the dominant part in every
    position, ragged key counts; K = 100 and V = -100 at and beyond the count"""
    inp, heads, cov = prepared("resampler", kind, case)
    Q, K, V = on_gpu(inp, "Q", "K", "V")
    H, NQ, L, Lpad, counts, part = case
    B = len(counts)
    buf = run_resampler(rops, Q, K, V, counts, B, H, NQ, L, Lpad)
    wrote_exactly(buf, NQ, H * 128)
    O = RR.heads_of(buf[:, :NQ], H)
    check("resampler", kind, case, O, heads, cov, tile_rows=NQ)
    assert torch.equal(run_resampler(rops, Q, K, V, counts, B, H, NQ, L, Lpad), buf)
    if kind != "ramp" and min(counts) < Lpad:      # the masked twin: the first key beyond the count aligned with the spiked rows, at twice the strength
        K2 = EA.with_spike_at(inp["K"], inp["u"], min(counts), 128 ** -0.5 * EA.LOG2E, 2.0).to(DEV)
        assert not torch.equal(K2, K) and torch.equal(run_resampler(rops, Q, K2, V, counts, B, H, NQ, L, Lpad), buf)


# ---------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("kind,case", EA.cases_of("decode")[0], ids=EA.cases_of("decode")[1])
def test_decode_attention_combines_a_dominant_chunk(qd, kind, case):
    """The spike in the first, a middle and the last 256-key chunk of the range (every other head of a group aligned with it), ranges that
    cut chunks; ramp: every chunk 5.5 above the one before, so the combine's weights run 1, 2^-5.5, 2^-11"""
    inp, heads, cov = prepared("decode", kind, case)
    Qd, K, V = on_gpu(inp, "Qd", "K", "V")
    Hq, Hkv, dk, cap, k_lo, k_hi, chunk = case
    O, buf = run_decode_attention(qd, Qd, K, V, k_lo, k_hi)
    assert bool(is_sentinel(buf[:, Hq * dk:]).all()) and not bool(is_sentinel(buf[:, :Hq * dk]).any())
    check("decode", kind, case, O[:, :, None], heads, cov, tile_rows=1)
    assert torch.equal(run_decode_attention(qd, Qd, K, V, k_lo, k_hi)[0], O)
    if kind != "ramp" and (k_lo[0] >= 3 or k_hi[0] < cap):     # the masked twins: the keys just outside a range that cuts a chunk, aligned with the spiked heads
        K2 = masked_twins(inp["K"], inp["u"], dk, k_lo[0], k_hi[0], cap).to(DEV)
        assert not torch.equal(K2, K) and torch.equal(run_decode_attention(qd, Qd, K2, V, k_lo, k_hi)[0], O)


def test_print_worst():
    """(last: the worst share of the per-element allowance per entry point over everything this module ran, and the module's wall time)"""
    print("\n  worst share of the per-element allowance per entry point: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    if CLOCK:
        print("  wall time of the module: %.1f s" % (time.time() - CLOCK[0]))
    assert all(v <= 1.0 for v in WORST.values())
