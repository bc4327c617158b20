"""float64 references and checkers for the T5 encoder's kernels and host modules (include/x2i_t5.h, x2i_amd/t5.py).  No GPU-only code here:
the CPU tests of the checkers import it too.

  attention   softmax(q k^T + table[h][clamp(j - i, -R, R) + R]) v, no scale, keys < S; errors per (b, h, 64-row tile) as tests/attn_ref.py
  rms rows    w x rsqrt(mean(x^2) + eps), per element
  gated GELU  gelu_tanh(a) b, per element
  stack       the whole encoder stack restated in float64 from a state dict with the library's key names
"""
import math

import torch

from tests import attn_ref
from tests.gemm_ref import ACT_TAIL, U_ACT

# Worst 64-row tile, rel-L2 against float64: TOL_O of tests/attn_ref.py, kernels with the same arithmetic (f32 scores, bf16 P, f32 accumulation,
# one output rounding).  A CPU model of that arithmetic measures 2.1e-3 .. 3.0e-3 on the GPU tests' inputs; a kernel that rounds the scores to
# bf16 (as the library's bf16 path does) measures 1.4e-2 .. 3.2e-2 and fails.
TOL_O = attn_ref.TOL_O      # measured on MI355X: worst tile 2.98e-3 (B=2 H=64 S=512 dk=64); 2.14e-3 .. 2.60e-3 on the small cases (tests/test_t5_gpu.py)
# Per-element bound of the row kernels, relative to the float64 value: 2^-8 * 1.02.  One rounding to nearest in bf16 is within half an ulp =
# 2^-8 relative (8 significand bits), and the f32 arithmetic before it (mean of squares, reciprocal square root, two products) adds noise of
# order 1e-6, inside the 2 % margin (7.8e-5).  A kernel that rounds twice (normalised value to bf16, then weight * that to bf16, as the
# library's bf16 path does) can be 2^-7 off and fails this bound on about one element in ten (tests/test_t5_ref_cpu.py).
TOL_ROW = 2.0 ** -8 * 1.02  # = 3.984e-3; measured on MI355X: RMS rows 3.34e-3 .. 3.89e-3 worst element (a rounding near half an ulp just above a power of two)


# ---------------------------------------------------------------------------------------------------------------- attention
def clamped_index(S, R, device="cpu"):
    """[S, S] long: clamp(j - i, -R, R) + R for query i, key j"""
    pos = torch.arange(S, device=device)
    return (pos[None, :] - pos[:, None]).clamp(-R, R) + R


def attention_reference(Q, K, V, table, S, R, heads=8):
    """float64 O [B, H, S, dk] of Q, K, V [B, H, >= S, dk] (any dtype) and table [H, 2R+1]: scores q k^T + table[h][clamp(j - i) + R], no scale,
    softmax over the keys < S."""
    B, H, _, dk = Q.shape
    f = torch.float64
    idx = clamped_index(S, R, Q.device)
    out = torch.empty((B, H, S, dk), dtype=f, device=Q.device)
    for b in range(B):
        for h0 in range(0, H, heads):
            h1 = min(H, h0 + heads)
            q, k, v = (t[b, h0:h1, :S].to(f) for t in (Q, K, V))
            s = q @ k.transpose(-1, -2) + table[h0:h1].to(f)[:, idx]
            out[b, h0:h1] = torch.softmax(s, -1) @ v
    return out


def check_attention(name, out, ref, bound=TOL_O):
    """out [B, H, >= S, dk] against ref [B, H, S, dk]: every (b, h, 64-row tile) within rel-L2 `bound`; returns the worst tile's error"""
    return attn_ref.check_tiles(name, out, ref, bound)


def attention_inputs(B, H, S, dk, R, seed, Spad=None, device="cpu"):
    """q, k ~ N(0, 1) dk^(-1/4), v ~ N(0, 1) as bf16 [B, H, Spad, dk], zero beyond S; table ~ N(0, 1) f32 [H, 2R+1] (asymmetric)."""
    Spad = (S + 63) // 64 * 64 if Spad is None else Spad
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((B, H, S, dk), generator=g) for _ in range(3))
    q, k = q * dk ** -0.25, k * dk ** -0.25
    pad = lambda t: torch.cat([t, torch.zeros((B, H, Spad - S, dk))], 2).bfloat16().to(device)
    return pad(q), pad(k), pad(v), torch.randn((H, 2 * R + 1), generator=g).to(device)


# ---------------------------------------------------------------------------------------------------------------- rows
def rms_reference(x, w, eps):
    x, w = x.double(), w.double()
    return w * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps))


def _check_elements(name, y, want, bound):
    err = (y.double().cpu() - want.cpu()).abs()
    bad = ~(err <= bound.cpu())    # (NaN fails too)
    if bool(bad.any()):
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("%s: element %s is %r, float64 says %r: off by %.3e > %.3e; %d of %d elements over their bound"
                             % (name, i, float(y[i]), float(want[i]), float(err[i]), float(bound.cpu()[i]), int(bad.sum()), bad.numel()))
    return float((err / want.abs().cpu().clamp_min(1e-300)).max())


def check_rms(name, y, x, w, eps):
    """Per element |y - y64| <= 2^-8 * 1.02 * |y64|; returns the worst relative error"""
    want = rms_reference(x.cpu(), w.cpu(), eps)
    return _check_elements(name, y, want, TOL_ROW * want.abs())


def gelu_tanh_f64(x):
    """0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3), as x sigmoid(2u): the same function without the cancellation of 1 + tanh(u) far
    below zero, where tanh(u) rounds to -1 and the textbook form (gemm_ref.act_f64) returns -0 for a value of 1e-17"""
    x = x.double()
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def gated_gelu_reference(a, b):
    return gelu_tanh_f64(a) * b.double()


def check_gated_gelu(name, y, a, b):
    """Per element |y - g64 b| <= (2^-8 * 1.02 + U_ACT) |g64 b| + ACT_TAIL |a b|"""
    a, b = a.double().cpu(), b.double().cpu()
    want = gated_gelu_reference(a, b)
    return _check_elements(name, y, want, (TOL_ROW + U_ACT) * want.abs() + ACT_TAIL * (a * b).abs())


# ---------------------------------------------------------------------------------------------------------------- the whole stack
def stack_reference(sd, x, *, num_heads, d_kv, eps, table, R, prefix=""):
    """float64 restatement of the encoder stack: x [B, S, d_model] (the embedded input) through every block of the state dict `sd` (the
    library's key names under `prefix`) and the final norm.  table: float64 [H, 2R+1] of block 0's relative_attention_bias."""
    f = torch.float64
    w = lambda k: sd[prefix + k].to(f)
    B, S, _ = x.shape
    H, dk = num_heads, d_kv
    bias = table.to(f)[:, clamped_index(S, R)]
    x = x.to(f)
    n = 0
    while prefix + "block.%d.layer.0.layer_norm.weight" % n in sd:
        n += 1
    for i in range(n):
        p = "block.%d.layer." % i
        h = rms_reference(x, w(p + "0.layer_norm.weight"), eps)
        q, k, v = ((h @ w(p + "0.SelfAttention.%s.weight" % nm).t()).view(B, S, H, dk).transpose(1, 2) for nm in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) + bias, -1) @ v
        x = x + a.transpose(1, 2).reshape(B, S, H * dk) @ w(p + "0.SelfAttention.o.weight").t()
        h = rms_reference(x, w(p + "1.layer_norm.weight"), eps)
        g = gelu_tanh_f64(h @ w(p + "1.DenseReluDense.wi_0.weight").t()) * (h @ w(p + "1.DenseReluDense.wi_1.weight").t())
        x = x + g @ w(p + "1.DenseReluDense.wo.weight").t()
    return rms_reference(x, w("final_layer_norm.weight"), eps)


def library_config(d_model, heads, d_kv, d_ff, layers, vocab=64):
    from transformers import T5Config
    return T5Config(num_heads=heads, num_layers=layers, num_decoder_layers=0, layer_norm_epsilon=1e-6, is_encoder_decoder=False, is_decoder=False,
                    d_ff=d_ff, d_kv=d_kv, d_model=d_model, dense_act_fn="gelu_new", feed_forward_proj="gated-gelu", use_cache=False, vocab_size=vocab)


def library_stack(d_model, heads, d_kv, d_ff, layers, vocab=64):
    """(config, `transformers` T5Stack in float32 on the CPU, its own initialisation under a fixed seed)"""
    from transformers.models.t5.modeling_t5 import T5Stack
    cfg = library_config(d_model, heads, d_kv, d_ff, layers, vocab)
    torch.manual_seed(0)
    return cfg, T5Stack(cfg).eval().requires_grad_(False)


def random_stack_state_dict(stack, seed):
    """The test weights of a `transformers` T5Stack: the library's initialisation rounded to bf16, the 1-D (norm) weights perturbed by
    0.1 N(0, 1), the bias weights N(0, 2^2) (the default initialisation is near zero and would hide a wrong index); float32 tensors that hold
    bf16 values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in stack.state_dict().items():
        v = v.detach().float().clone()
        if k.endswith("relative_attention_bias.weight"):
            v = 2.0 * torch.randn(v.shape, generator=g)
        elif v.dim() == 1:
            v = v + 0.1 * torch.randn(v.shape, generator=g)
        sd[k] = v.bfloat16().float()
    return sd


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())
