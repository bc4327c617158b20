"""float64 references and bounds for Qwen2 decoding with a key/value cache (include/x2i_qwen_decode.h, Qwen2DecoderStack.prefill / decode_step).
No GPU-only code here: the CPU tests import it too.

  attention   one query per head over the keys k_lo <= j < k_hi, query head h on key/value head h // rep; an empty range is 0
  linear      tests/gemm_ref.gemm_expect (the epilogue contract of x2i_gemm_bf16); the gate's bound is derived below
  decoding    cached decoding restated on tests/qwen_ref.stack_reference: each sample's COMPACTED sequence (its valid prompt tokens, then the
              step tokens) under explicit positions; step t is row n_valid + t of that full causal forward

The gate, y = bf16(silu(a) b) with a = lin_a + bias_a, b = lin_b + bias_b both kept in f32:
  da = U_ACC mag_a, db = U_ACC mag_b          the f32 sums, as gemm_expect takes them (mag = sum |w x| + |bias|)
  ds = (|silu'(a)| + da) da + U_ACT |silu(a)| + ACT_TAIL |a|        gemm_ref._act_bound: the activation on a perturbed argument
  |s~ b~ - s b| <= ds |b| + |s| db + ds db + U_F32 |s b|            both factors perturbed, then the one f32 product
and the output's one rounding adds half a bf16 ulp (gemm_ref._round_bound).
"""
import torch

from tests import gemm_ref as G
from tests import qwen_ref as QR


def attention_reference(Qd, K, V, k_lo, k_hi, scale):
    """float64 O [B, Hq, dk] of Qd [B, Hq, dk], K and V [B, Hkv, cap, dk] (any dtype) on the CPU; ranges clamped into [0, cap]"""
    B, Hq, dk = Qd.shape
    Hkv, cap = K.shape[1], K.shape[2]
    rep = Hq // Hkv
    f = torch.float64
    out = torch.zeros((B, Hq, dk), dtype=f)
    for b in range(B):
        lo, hi = min(max(int(k_lo[b]), 0), cap), min(max(int(k_hi[b]), 0), cap)
        if hi <= lo:
            continue
        q = Qd[b].to(f).cpu()
        k, v = (t[b, :, lo:hi].to(f).cpu().repeat_interleave(rep, dim=0) for t in (K, V))
        s = torch.einsum("hd,hjd->hj", q, k) * scale
        out[b] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), v)
    return out


def gate_expect(X, W, bias=None):
    """Expected output of x2i_qwen_decode_linear_bf16 in mode 1: X [B, K], W [2N, K], bias [2N] or None (bf16) -> (want, bound, delta) float64
    [B, N]; the derivation is in the module's docstring"""
    N = W.shape[0] // 2
    la, ma = G.linear_f64(X, W[:N], None if bias is None else bias[:N])
    lb, mb = G.linear_f64(X, W[N:], None if bias is None else bias[N:])
    da, db = G.U_ACC * ma, G.U_ACC * mb
    s = G.act_f64(la, G.ACT_SILU)
    ds = G._act_bound(la, s, da, G.ACT_SILU)
    want = s * lb
    delta = ds * lb.abs() + s.abs() * db + ds * db + G.U_F32 * want.abs()
    return want, G._round_bound(want, delta, False), delta


def step_positions(next_pos, T):
    """[..., B] next positions -> [..., B, T]: step t runs at next_pos + t (every axis advances by one)"""
    return next_pos[..., None] + torch.arange(T)


def next_positions(position_ids, attention_mask):
    """The next-position rule on the CPU: 1 + the largest position id of a sample's valid tokens over all axes -> int64 [B]"""
    pos = position_ids if position_ids.dim() == 3 else position_ids[None]
    if attention_mask is not None:
        pos = pos.masked_fill((attention_mask == 0)[None], -1)
    return pos.amax(-1).amax(0) + 1


def decode_reference(sd, x, steps, position_ids, k_lo, k_hi, *, num_heads, num_kv_heads, eps, dk, theta, mrope_section=None, prefix="",
                     step_offset=0):
    """float64 hidden states [B, C, T, D] of T cached decode steps after a prompt: x [B, S, D] the embedded prompt (valid tokens of sample b
    at k_lo[b] .. k_hi[b] - 1; None: all), steps [B, T, D] the embedded step tokens, position_ids [B, S] or [3, B, S] the prompt's.  Each
    sample alone: its valid prompt tokens followed by the step tokens, positions the prompt's own followed by next, next + 1, ..; the
    rows of the step tokens of qwen_ref.stack_reference over that sequence."""
    from x2i_amd.qwen import rope_tables
    B, S, D = x.shape
    T = steps.shape[1]
    out = []
    for b in range(B):
        lo, hi = (0, S) if k_lo is None else (int(k_lo[b]), int(k_hi[b]))
        seq = torch.cat((x[b, lo:hi], steps[b]), 0)[None]
        pp = position_ids[..., b:b + 1, lo:hi]
        nxt = pp.amax(-1).amax(0) + 1 if pp.dim() == 3 else pp.amax(-1) + 1                  # [1]
        sp = step_positions(nxt + step_offset, T)                                              # [1, T]  (step_offset: a deliberate mistake, for the tests)
        pos = torch.cat((pp, sp.expand(*pp.shape[:-1], T)), -1)
        cos, sin = rope_tables(pos, dk, theta, mrope_section)
        hs = QR.stack_reference(sd, seq, cos, sin, num_heads=num_heads, num_kv_heads=num_kv_heads, eps=eps, prefix=prefix)
        out.append(hs[:, :, hi - lo:])
    return torch.cat(out, 0)
