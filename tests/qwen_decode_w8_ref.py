"""float64 reference and bounds of the decode-step linear with an e4m3 weight (include/x2i_qwen_decode_w8.h, Qwen2DecoderStack.pack_w8 /
decode_step(w8=True)).  No GPU-only code here: the CPU tests import it too.

The reference is float64 over the DEQUANTISED weight, W[n][k] = w_scale[n] * e4m3(W8[n][k]) with tests/fp8_ref.decode: a 4-bit significand
times an f32 scale is exact in float64, so the quantised model is the model under test and nothing of the format's own error enters.

The allowance is tests/gemm_ref's, with one term more for the scale multiply.  With sum = sum_k e4m3(W8[n][k]) X[b][k] and s = w_scale[n]:
  mode 0   lin = s sum + bias,   d = U_ACC (|s| sum_k |w8 x| + |bias|) + U_F32 |s sum|
           (the f32 sum and the bias add as gemm_expect takes them; the one f32 multiply by the scale rounds s * sum once)
           then gemm_ref.epilogue_expect: the residual's U_F32 (|res| + |lin|) and the output's one rounding (_round_bound)
  mode 1   a and b each as `lin` above with their own scale (rows n and N + n), then qwen_decode_ref.gate_expect's derivation:
           ds = (|silu'(a)| + da) da + U_ACT |silu(a)| + ACT_TAIL |a|,  |s~ b~ - s b| <= ds |b| + |s| db + ds db + U_F32 |s b|,  one rounding
No constant here comes from the kernel under test.

stand_in() restates the kernel's DOCUMENTED summation order in f32 on the CPU (lane l of 64 sums k = 16 l + 1024 i + j ascending in one
chain, then the xor butterfly 32 .. 1, the scale, the bias, the residual, one rounding) and can plant the likely bugs, for
tests/test_qwen_decode_w8_ref_cpu.py.
"""
import torch

from tests import fp8_ref as F8
from tests import gemm_ref as G
from tests import qwen_decode_ref as DR
from tests import qwen_ref as QR

FAULTS = ("scale_on_bias", "b_scale_index", "halves_swapped", "last_step_dropped")


def dequant(W8, w_scale):
    """float64 [N, K] of the e4m3 codes W8 (torch.float8_e4m3fn or uint8) and the f32 row scales: exact"""
    return F8.decode(W8) * w_scale.double()[:, None]


def _sums(X, W8):
    """sum = X e4m3(W8)^T and mag = |X| |e4m3(W8)|^T in float64 (every product is exact, the sums carry float64's rounding only)"""
    w = F8.decode(W8)
    x = X.double()
    return x @ w.T, x.abs() @ w.abs().T


def _lin(X, W8, w_scale, bias):
    s = w_scale.double()[None]
    sm, mag = _sums(X, W8)
    lin = s * sm
    d = G.U_ACC * (s.abs() * mag) + G.U_F32 * lin.abs()
    if bias is not None:
        lin = lin + bias.double()
        d = d + G.U_ACC * bias.double().abs()
    return lin, d


def linear_w8_expect(X, W8, w_scale, bias=None, res=None):
    """Expected output of x2i_qwen_decode_linear_w8_bf16 in mode 0: X bf16 [B, K], W8 codes [N, K], w_scale f32 [N], bias bf16 [N] or None,
    res bf16 [B, N] or None -> (want, bound, delta) float64 [B, N] (delta: the f32 part of the bound)"""
    lin, d = _lin(X, W8, w_scale, bias)
    return G.epilogue_expect(lin, d, res=res)


def gate_w8_expect(X, W8, w_scale, bias=None):
    """... in mode 1: W8 [2N, K], w_scale [2N], bias [2N] or None -> (want, bound, delta) float64 [B, N]"""
    N = W8.shape[0] // 2
    la, da = _lin(X, W8[:N], w_scale[:N], None if bias is None else bias[:N])
    lb, db = _lin(X, W8[N:], w_scale[N:], None if bias is None else bias[N:])
    s = G.act_f64(la, G.ACT_SILU)
    ds = G._act_bound(la, s, da, G.ACT_SILU)
    want = s * lb
    delta = ds * lb.abs() + s.abs() * db + ds * db + G.U_F32 * want.abs()
    return want, G._round_bound(want, delta, False), delta


def quantize_rows(W):
    """x2i_quantize_rows_fp8 of a bf16 [N, K] weight on the CPU (tests/fp8_ref.quantize_expect, exact): (codes uint8, scales f32)"""
    return F8.quantize_expect(W)


def dequantized_state_dict(sd, num_heads, num_kv_heads, prefix=""):
    """The float64 state dict of the quantised model: q|k|v (quantised as ONE stacked matrix, row scales are per row so the split is the
    same), o_proj, gate|up and down_proj of every layer replaced by the dequantised values of their bf16 weights; everything else as is."""
    out = {}
    for k, v in sd.items():
        if k.endswith("_proj.weight"):
            codes, scale = quantize_rows(v.bfloat16().contiguous())
            out[k] = dequant(codes, scale)
        else:
            out[k] = v
    return out


def mixed_stack_reference(sd_prompt, sd_steps, x, n_prompt, cos, sin, *, num_heads, num_kv_heads, eps):
    """tests/qwen_ref.stack_reference with the weights chosen BY ROW: rows < n_prompt of every linear run on sd_prompt, the rows from
    n_prompt on on sd_steps (norm weights and biases are the same in both).  That is the model HipGenerate(w8=True) runs: the prompt pass
    stays on the bf16 weights and fills the key/value cache, the decode steps read the e4m3 weights and attend to those keys and values.
    x [B, S, D] -> float64 [B, C, S, D]."""
    f = torch.float64
    B, S, D = x.shape
    Hq, Hkv = num_heads, num_kv_heads
    x = x.to(f)
    c, s = cos.to(f)[:, None], sin.to(f)[:, None]
    ok = QR.counted(S, None, None, B)[:, None]
    n = 0
    while "layers.%d.input_layernorm.weight" % n in sd_prompt:
        n += 1
    dk = sd_prompt["layers.0.self_attn.q_proj.weight"].shape[0] // Hq

    def rope(t):
        t1, t2 = t[..., :dk // 2], t[..., dk // 2:]
        return torch.cat((t1 * c - t2 * s, t2 * c + t1 * s), -1)

    hs = [x]
    for i in range(n):
        p = "layers.%d." % i

        def lin(t, nm):
            y = torch.cat((t[:, :n_prompt] @ sd_prompt[p + nm + ".weight"].to(f).t(), t[:, n_prompt:] @ sd_steps[p + nm + ".weight"].to(f).t()), 1)
            return y + (sd_prompt[p + nm + ".bias"].to(f) if p + nm + ".bias" in sd_prompt else 0.0)

        w = lambda k: sd_prompt[p + k].to(f)
        h = QR.rms_reference(x, w("input_layernorm.weight"), eps)
        q = rope(lin(h, "self_attn.q_proj").view(B, S, Hq, dk).transpose(1, 2))
        k = rope(lin(h, "self_attn.k_proj").view(B, S, Hkv, dk).transpose(1, 2)).repeat_interleave(Hq // Hkv, dim=1)
        v = lin(h, "self_attn.v_proj").view(B, S, Hkv, dk).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
        sc = (q @ k.transpose(-1, -2) * dk ** -0.5).masked_fill(~ok, float("-inf"))
        a = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, S, Hq * dk)
        x = x + lin(a, "self_attn.o_proj")
        h = QR.rms_reference(x, w("post_attention_layernorm.weight"), eps)
        x = x + lin(QR.silu_f64(lin(h, "mlp.gate_proj")) * lin(h, "mlp.up_proj"), "mlp.down_proj")
        hs.append(x)
    hs[-1] = QR.rms_reference(x, sd_prompt["norm.weight"].to(f), eps)
    return torch.stack(hs, 1)


def decode_reference_w8(sd, x, steps, position_ids, k_lo, k_hi, *, num_heads, num_kv_heads, eps, dk, theta, mrope_section=None):
    """qwen_decode_ref.decode_reference for decode_step(w8=True) after a bf16 prefill: float64 hidden states [B, C, T, D] of the T step
    tokens, each sample's compacted sequence through mixed_stack_reference -- its valid prompt tokens on the state dict `sd`, the step
    tokens on dequantized_state_dict(sd)."""
    from x2i_amd.qwen import rope_tables
    dq = dequantized_state_dict(sd, num_heads, num_kv_heads)
    B, S, D = x.shape
    T = steps.shape[1]
    out = []
    for b in range(B):
        lo, hi = (0, S) if k_lo is None else (int(k_lo[b]), int(k_hi[b]))
        seq = torch.cat((x[b, lo:hi], steps[b]), 0)[None]
        pp = position_ids[..., b:b + 1, lo:hi]
        nxt = pp.amax(-1).amax(0) + 1 if pp.dim() == 3 else pp.amax(-1) + 1
        pos = torch.cat((pp, DR.step_positions(nxt, T).expand(*pp.shape[:-1], T)), -1)
        cos, sin = rope_tables(pos, dk, theta, mrope_section)
        hs = mixed_stack_reference(sd, dq, seq, hi - lo, cos, sin, num_heads=num_heads, num_kv_heads=num_kv_heads, eps=eps)
        out.append(hs[:, :, hi - lo:])
    return torch.cat(out, 0)


# ---------------------------------------------------------------------------------------------------------------- the documented order, in f32
def _lane_chain(X, W, K, fault=None):
    """f32 [B, N, 64]: per (sample, row) the 64 lane sums of the documented order.  X f32 [B, K], W f32 [N, K] (decoded codes)."""
    B, N = X.shape[0], W.shape[0]
    steps = (K + 1023) // 1024
    Kp = steps * 1024
    x = torch.zeros((B, Kp), dtype=torch.float32)
    w = torch.zeros((N, Kp), dtype=torch.float32)
    x[:, :K], w[:, :K] = X, W
    if fault == "halves_swapped":             # bytes (0, 1) and (2, 3) of every dword change places
        w = w.view(N, Kp // 4, 2, 2).flip(2).reshape(N, Kp)
    x = x.view(B, 1, steps, 64, 16)
    w = w.view(1, N, steps, 64, 16)
    if fault == "last_step_dropped" and K % 1024:
        steps_eff = steps - 1                 # the step that only some lanes take
    else:
        steps_eff = steps
    acc = torch.zeros((B, N, 64), dtype=torch.float32)
    for i in range(steps_eff):
        for j in range(16):
            acc = acc + w[:, :, i, :, j] * x[:, :, i, :, j]          # the product is exact in f32: an fma is this multiply and add
    return acc


def _butterfly(v):
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def stand_in(X, W8, w_scale, bias=None, res=None, gate=False, fault=None):
    """bf16 [B, N]: the kernel's documented arithmetic in f32 on the CPU; fault: None or one of FAULTS"""
    assert fault is None or fault in FAULTS
    K = X.shape[1]
    w = F8.decode(W8).float()
    dot = _butterfly(_lane_chain(X.float(), w, K, fault))            # [B, rows]
    s = w_scale.float()[None]
    rows = w.shape[0]
    if gate and fault == "b_scale_index":
        s = torch.cat((s[:, :rows // 2], s[:, :rows // 2]), 1)
    v = s * dot
    if bias is not None:
        v = v + (s * bias.float() if fault == "scale_on_bias" else bias.float())
    if gate:
        a, b = v[:, :rows // 2], v[:, rows // 2:]
        return (a * torch.sigmoid(a) * b).bfloat16()
    if res is not None:
        v = v + res.float()
    return v.bfloat16()
