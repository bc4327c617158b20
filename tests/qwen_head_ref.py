"""float64 reference of token selection (include/x2i_qwen_head.h): the vocabulary projection, RepetitionPenaltyLogitsProcessor, the argmax
with the lowest index among equals, and the bookkeeping of one generated token.  No GPU-only code here: the CPU tests import it too.

The kernel's logit is decode_linear's f32 sum, so its bound is gemm_ref.gemm_expect(X, W, out_f32=True)'s: |l~ - l| <= delta = U_ACC sum_k |w x|
(the output is the f32 value itself: U_F32 |l| on top).  A penalised element is one more f32 operation on l~:
    p = l < 0 ? l * pen : l / pen        |p~ - p| <= max(pen, 1 / pen) delta + U_F32 (|p| + max(pen, 1 / pen) delta)
Where |l| <= delta the sign of l~ is not determined and the kernel may have taken either branch: there the hull of both branches over
[l - delta, l + delta] is accepted."""
import torch

from tests import gemm_ref as G


def f32(v):
    """the f32 value of a Python float: what the kernel receives"""
    return float(torch.tensor(v, dtype=torch.float32))


def penalise(l, seen, penalty):
    """RepetitionPenaltyLogitsProcessor on scores l with `seen` a mask of the ids in input_ids, in l's dtype"""
    return torch.where(seen.bool(), torch.where(l < 0, l * penalty, l / penalty), l)


def seen_of(ids, V):
    """uint8 [B, V]: 1 at every id of ids [B, n] (pad ids included, as the library's processor has it)"""
    seen = torch.zeros((ids.shape[0], V), dtype=torch.uint8, device=ids.device)
    return seen.scatter_(1, ids.long(), 1)


def head_expect(X, W, seen=None, penalty=1.0):
    """(want, bound, delta) float64 [B, V] of the penalised f32 logits for X bf16 [B, K], W bf16 [V, K], seen [B, V] or None"""
    l, bound, d = G.gemm_expect(X, W, out_f32=True)
    if seen is None:
        return l, bound, d
    pen = f32(penalty)
    s = seen.bool().to(l.device)
    f = max(pen, 1.0 / pen)
    want = penalise(l, s, pen)
    dp = f * d
    bp = dp + G.U_F32 * (want.abs() + dp)
    # undetermined sign: either branch on any value of [l - d, l + d]
    lo, hi = l - d, l + d
    hull_lo = torch.minimum(lo * pen, lo / pen)
    hull_hi = torch.maximum(hi * pen, hi / pen)
    both = torch.maximum((hull_lo - want).abs(), (hull_hi - want).abs()) + G.U_F32 * torch.maximum(hull_lo.abs(), hull_hi.abs())
    bp = torch.where(l.abs() <= d, torch.maximum(bp, both), bp)
    return want, torch.where(s, bp, bound), torch.where(s, dp, d)


def argmax_lowest(p):
    """the LOWEST index of the largest value along the last axis (torch.argmax's rule, spelt out)"""
    V = p.shape[-1]
    top = p.max(-1, keepdim=True).values
    idx = torch.arange(V, device=p.device).expand_as(p)
    return torch.where(p == top, idx, torch.full_like(idx, V)).min(-1).values


def margin(want, bound, winner=None, equals=()):
    """(margin, allowance): the float64 gap between each row's winner and its best other element (`equals`: indices that hold the winner's own
    row of W and are equal by construction, left out), and twice the larger of the two elements' bounds.  A token is only DETERMINED by the
    reference where margin > allowance."""
    B = want.shape[0]
    rows = torch.arange(B, device=want.device)
    win = argmax_lowest(want) if winner is None else winner
    rest = want.clone()
    rest[rows, win] = -float("inf")
    for e in equals:
        rest[:, e] = -float("inf")
    second = rest.argmax(-1)
    gap = want[rows, win] - want[rows, second]
    return gap, 2 * torch.maximum(bound[rows, win], bound[rows, second])


def count_over_bound(got, want, bound):
    """elements of got outside want +- bound (NaN counts)"""
    return int((~((got.double().to(want.device) - want).abs() <= bound)).sum())


def select_reference(amax, col, token, sequences, lengths, done, eos, pad, seen=None):
    """The bookkeeping of x2i_qwen_head_select on CPU tensors, in place; amax int64 [B].  Returns the advanced column."""
    B = amax.shape[0]
    for b in range(B):
        was = bool(done[b])
        tok = int(pad) if was else int(amax[b])
        token[b] = tok
        if 0 <= col < sequences.shape[1]:
            sequences[b, col] = tok
        if not was:
            lengths[b] += 1
        done[b] = int(was or tok in [int(e) for e in eos])
        if seen is not None:
            seen[b, tok] = 1
    return col + 1
