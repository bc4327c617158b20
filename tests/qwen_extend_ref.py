"""float64 reference and criteria of the Qwen2 prompt extension (include/x2i_qwen_extend.h, Qwen2DecoderStack.extend, HipGenerate(keep_cache=True)).
No GPU-only code here: tests/test_qwen_extend_ref_cpu.py imports it too.

  window attention   rows [row0, row0 + n) of the causal attention over a cache, computed from those rows alone on tests/qwen_ref.py's mask
  stack criterion    the project's: the HIP path's error against the library in float64 is at most 1.5 x the error of the library's own
                     bf16 run on the same GPU, and below 3e-2 (tests/test_t5_gpu.py states it for the encoders)
"""
import torch

from tests import qwen_ref as QR

SENTINEL = 0x7F7F           # bf16 bits of 3.39e38: what the tests fill an output with to see what a kernel wrote


def poisoned(*shape, device="cuda"):
    t = torch.empty(shape, device=device, dtype=torch.bfloat16)
    t.view(torch.int16).fill_(SENTINEL)
    return t


def is_sentinel(t):
    return t.view(torch.int16) == SENTINEL


def window_reference(Q, K, V, row0, n, scale, k_lo=None):
    """float64 O [B, Hq, n, dk]: the query rows row0 .. row0 + n - 1 of Q [B, Hq, >= row0 + n, dk] over the keys k_lo[b] <= j <= i of K, V
    [B, Hkv, >= row0 + n, dk] (any dtype), on the CPU.  Only those rows of Q are read; the mask is rows [row0, row0 + n) of
    qwen_ref.counted(row0 + n, k_lo); a row with no counted key is 0, as qwen_ref.attention_reference has it."""
    B, Hq, _, dk = Q.shape
    rep = Hq // K.shape[1]
    S = row0 + n
    f = torch.float64
    ok = QR.counted(S, k_lo, None, B)[:, row0:S]
    out = torch.zeros((B, Hq, n, dk), dtype=f)
    for b in range(B):
        q = Q[b, :, row0:S].to(f).cpu()
        k, v = (t[b, :, :S].to(f).cpu().repeat_interleave(rep, dim=0) for t in (K, V))
        s = (q @ k.transpose(-1, -2) * scale).masked_fill(~ok[b], float("-inf"))
        live = ok[b].any(-1)
        p = torch.zeros_like(s)
        p[:, live] = torch.softmax(s[:, live], -1)
        out[b] = p @ v
    return out


def check_window(name, out, ref, row0, k_lo=None, bound=QR.TOL_O):
    """out [B, Hq, n, dk] (the chunk's rows) against window_reference's: qwen_ref.check_attention per (b, h, 64-row tile of the chunk), the rows
    before k_lo[b] -- chunk rows < k_lo[b] - row0 -- exactly 0; returns the worst tile's error"""
    lo = None if k_lo is None else [min(max(int(v) - row0, 0), out.shape[2]) for v in torch.as_tensor(k_lo).tolist()]
    return QR.check_attention(name, out, ref, bound, k_lo=lo)


def assert_stack_criterion(e_hip, e_lib):
    assert e_hip <= 1.5 * e_lib, "HIP %.3e > 1.5 x library bf16 %.3e" % (e_hip, e_lib)
    assert e_hip < 3e-2
