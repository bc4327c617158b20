"""The float64 attention reference and the per-tile checker of tests/attn_ref.py, on the host at the model's ragged length (S = 4600: 72 key
tiles of 64, the last one partial, 8 padding rows).  A correct-kernel stand-in (fp32, P and dS rounded to bf16, bf16 outputs) passes every bound;
each of the kernel faults below, applied to that stand-in, is rejected -- and two of them slip past the whole-tensor check the backward tests
used before."""
import math

import pytest
import torch

from tests import attn_ref as R

S, SPAD = 4600, 4608
SCALE = 1.0 / math.sqrt(128.0)
BOUNDS = {"O": R.TOL_O, "dQ": R.TOL_DQ, "dK": R.TOL_DK, "dV": R.TOL_DV}


def standin(Q, K, V, dO, scale, nkeys=S):
    """What a correct bf16 kernel computes, in fp32: P = exp(s - lse) and dS = P (dP - D) rounded to bf16 before their products, D from the bf16 O,
    O / dQ / dK / dV rounded to bf16.  nkeys: how many keys enter the softmax -- S when the padding keys are masked; SPAD lets the zero padding
    keys in (a missing key mask), S // 64 * 64 drops the last, partial key tile."""
    f = torch.float32
    q, do = Q[:, :, :S].to(f), dO[:, :, :S].to(f)
    k, v = K[:, :, :nkeys].to(f), V[:, :, :nkeys].to(f)
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    pb = R.bf16_round(p)
    o = R.bf16_round(pb @ v)
    d = (do * o).sum(-1, keepdim=True)
    ds = R.bf16_round(p * (do @ v.transpose(-1, -2) - d))
    out = {"O": o, "lse2": lse.squeeze(-1) * R.LOG2E, "dQ": R.bf16_round((ds @ k) * scale),
           "dK": R.bf16_round((ds.transpose(-1, -2) @ q) * scale), "dV": R.bf16_round(pb.transpose(-1, -2) @ do)}
    for n in ("dK", "dV"):          # key rows the fault never reached stay zero, as a kernel's untouched output would
        full = torch.zeros(Q.shape[:2] + (S, 128), dtype=f)
        full[:, :, :min(nkeys, S)] = out[n][:, :, :S]
        out[n] = full
    return out


_cache = {}


def case(kind, H=2):
    """(float64 reference, stand-in) for B = 1, H heads, S = 4600 on `kind` inputs; computed once per module."""
    if kind not in _cache:
        Q, K, V, dO = R.make_inputs(kind, 1, H, S, SPAD, seed=4600 + len(kind))
        _cache[kind] = (Q, K, V, dO), R.reference(Q, K, V, dO, S, SCALE), standin(Q, K, V, dO, SCALE)
    return _cache[kind]


def failures(out, ref):
    """The names of the quantities whose check rejects `out` (every tile bound, and the lse2 row bound)."""
    bad = []
    for n, bound in BOUNDS.items():
        try:
            R.check_tiles(n, out[n], ref[n], bound)
        except AssertionError:
            bad.append(n)
    try:
        R.check_rows("lse2", out["lse2"], ref["lse2"], R.TOL_LSE2)
    except AssertionError:
        bad.append("lse2")
    return bad


def test_reference_backward_equals_autograd():
    """The explicit backward formulas of reference() against torch autograd through a float64 softmax attention on the same bf16 operands."""
    (Q, K, V, dO), ref, _ = case("random")
    q, k, v = (t[:, :, :S].double().requires_grad_(True) for t in (Q, K, V))
    s = (q @ k.transpose(-1, -2)) * SCALE
    o = torch.softmax(s, -1) @ v
    (o * dO[:, :, :S].double()).sum().backward()
    for n, want in (("O", o.detach()), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
        assert R.global_rel_l2(ref[n], want, S) < 1e-12, n
    assert float((ref["lse2"] - torch.logsumexp(s.detach(), -1) * R.LOG2E).abs().max()) < 1e-11
    assert float((ref["D"] - (o.detach() * dO[:, :, :S].double()).sum(-1)).abs().max()) < 1e-11


@pytest.mark.parametrize("kind", R.KINDS)
def test_correct_standin_passes_every_bound(kind):
    """(`peaked`: O and dV only -- the GPU tests use it for the sampling kernels, which write no lse2.  Its nearly one-hot rows make dP - D a
    cancellation, and the bf16 stand-in's dQ / dK tiles reach 7e-3 there; its lse2 sits near 30, where the host's fp32 logsumexp is 1.5e-5
    off.)"""
    _, ref, out = case(kind)
    for n, bound in BOUNDS.items():
        if kind == "peaked" and n in ("dQ", "dK"):
            continue
        worst = R.check_tiles(n, out[n], ref[n], bound)
        print(f"stand-in {kind:6s} {n:3s} worst tile {worst:.3e} median {float(R.tile_errors(out[n], ref[n], S).median()):.3e}")
    if kind != "peaked":
        R.check_rows("lse2", out["lse2"], ref["lse2"], R.TOL_LSE2)


def test_spike_inputs_move_the_running_maximum_at_the_chosen_tile():
    """`spike`: the spiked query rows' maximum score sits on the chosen key and exceeds the maximum over the keys before that tile by more than
    the kernels' defer threshold (8 in log2 units), so the online softmax has to rescale there; that key holds a share of the row's softmax,
    well short of all of it."""
    (Q, K, _, _), _, _ = case("spike")
    j = R.spike_key(S)
    s = (Q[0, :, R.SPIKE_ROW:S:64].double() @ K[0, :, :S].double().transpose(-1, -2)) * SCALE * R.LOG2E
    assert bool((s.argmax(-1) == j).all())
    jump = s[..., j] - s[..., :j // 64 * 64].amax(-1)
    p = torch.softmax(s / R.LOG2E, -1)[..., j]
    print(f"spike: jump {float(jump.min()):.2f} .. {float(jump.max()):.2f} (log2), share of the spiked key {float(p.min()):.2f} .. {float(p.max()):.2f}")
    assert float(jump.min()) > 9.0 and 0.1 < float(p.min()) and float(p.max()) < 0.4


def test_unmasked_padding_keys_fail_on_anti_inputs():
    (Q, K, V, dO), ref, _ = case("anti")
    bad = failures(standin(Q, K, V, dO, SCALE, nkeys=SPAD), ref)
    assert set(bad) == {"O", "dQ", "dK", "dV", "lse2"}, bad


def test_unmasked_padding_keys_pass_every_tile_bound_on_random_inputs():
    """The gap the `anti` inputs close: on the suite's usual inputs the 8 zero padding keys score exp(0 - ~9) against the valid keys, and the same
    fault stays below every tile bound of O, dQ, dK and dV -- a kernel test without `anti` inputs cannot see a missing key mask in its outputs.
    Only the absolute lse2 row bound notices (a shift of ~2e-4 in log2 units); the sampling kernels write no lse2."""
    (Q, K, V, dO), ref, _ = case("random")
    assert failures(standin(Q, K, V, dO, SCALE, nkeys=SPAD), ref) == ["lse2"]


def test_dropped_last_partial_key_tile_fails():
    (Q, K, V, dO), ref, _ = case("random")
    bad = failures(standin(Q, K, V, dO, SCALE, nkeys=S // 64 * 64), ref)
    assert {"O", "dQ", "dK", "dV"} <= set(bad), bad


@pytest.mark.parametrize("n", ["O", "dQ", "dK", "dV"])
def test_one_tile_replaced_by_its_neighbour_fails(n):
    _, ref, out = case("random")
    bad = out[n].clone()
    bad[0, 1, 40 * 64:41 * 64] = out[n][0, 1, 41 * 64:42 * 64]
    with pytest.raises(AssertionError, match=r"h=1, rows 2560\.\.2623\).*1 of 144 tiles"):
        R.check_tiles(n, bad, ref[n], BOUNDS[n])


def test_one_head_dk_off_by_one_part_in_128_fails():
    _, ref, out = case("random")
    bad = out["dK"].clone()
    bad[0, 0] *= 1 + 2 ** -7
    with pytest.raises(AssertionError, match=r"h=0"):
        R.check_tiles("dK", bad, ref["dK"], R.TOL_DK)


@pytest.mark.parametrize("n", ["O", "dQ", "dK", "dV"])
def test_two_heads_rows_swapped_fails(n):
    """A block-remap fault: one 128-row block written to the other head's rows and vice versa."""
    _, ref, out = case("random")
    bad = out[n].clone()
    bad[0, 0, 1280:1408], bad[0, 1, 1280:1408] = out[n][0, 1, 1280:1408], out[n][0, 0, 1280:1408]
    with pytest.raises(AssertionError, match=r"4 of 144 tiles"):
        R.check_tiles(n, bad, ref[n], BOUNDS[n])


def test_one_half_wrong_tile_passes_the_old_global_bound_at_model_size():
    """The gap the per-tile check closes: at B = 2, H = 24, S = 4600 (3456 row tiles) a single tile that is 50 % off moves the whole-tensor rel-L2
    of a correct kernel by less than the old 1.5e-2 bound.  The 48 heads are modelled as copies of this head (a sum of squares per head), then
    the tile check of the same tensor names the tile."""
    _, ref, out = case("random")
    for n in ("dQ", "dK", "dV", "O"):
        r, o = ref[n][:, :1], out[n][:, :1].double()
        bad = o.clone()
        bad[0, 0, 40 * 64:41 * 64] *= 1.5
        err_ok, err_bad, den = float(((o - r) ** 2).sum()), float(((bad - r) ** 2).sum()), float((r ** 2).sum())
        old = math.sqrt((47 * err_ok + err_bad) / (48 * den))
        assert old < R.OLD_GLOBAL_BOUND, (n, old)
        with pytest.raises(AssertionError, match=r"rows 2560\.\.2623"):
            R.check_tiles(n, bad, r, BOUNDS[n])
