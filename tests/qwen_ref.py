"""float64 references and checkers for the Qwen2 decoder prefill's kernels and host module (include/x2i_qwen.h, x2i_amd/qwen.py).  No GPU-only
code here: the CPU tests of the checkers import it too.

  attention   softmax(scale q k^T) v over the keys k_lo <= j < k_hi, j <= i, query head h on key/value head h // rep; a row with no counted
              key is 0; errors per (b, h, 64-row tile) as tests/attn_ref.py
  RoPE        rotate-half, from the f32 half tables the kernel gets, per element
  SwiGLU      silu(a) b, per element
  stack       the whole decoder stack restated in float64 from a state dict with the library's key names
"""
import torch

from tests import attn_ref
from tests.gemm_ref import ACT_TAIL, U_ACT
from tests.t5_ref import TOL_ROW, _check_elements, rel_l2, rms_reference  # noqa: F401  (rel_l2: for the tests that import this module)

# Worst 64-row tile, rel-L2 against float64: the project's bound for kernels with this arithmetic (f32 scores, bf16 P, f32 accumulation, one
# output rounding), as tests/t5_ref.py and tests/clip_ref.py take it.  t5_attn_kernel<128> measures 2.6e-3 against it on MI355X.
TOL_O = attn_ref.TOL_O
# RoPE per element: |y - e| <= TOL_ROW |e| + U_ROPE (|x1 c| + |x2 s|): one bf16 rounding of the result (half an ulp = 2^-8 relative, with the 2 %
# margin of TOL_ROW) plus the f32 arithmetic in front of it -- each product within 2^-24 of itself and the sum within 2^-24 of the result,
# which matters where the two products cancel and the result is far smaller than either.  2^-21 leaves a factor of eight over those ulps.
# Over 2^20 random elements on the CPU the one-rounding f32 form peaks at 0.98 of this bound and the library's bf16 form (each product and the
# sum rounded to bf16) exceeds it by three orders of magnitude (tests/test_qwen_ref_cpu.py).
U_ROPE = 2.0 ** -21


# ---------------------------------------------------------------------------------------------------------------- attention
def counted(S, k_lo=None, k_hi=None, B=1):
    """bool [B, S, S]: key j counts for row i of sample b iff k_lo[b] <= j < k_hi[b] and j <= i"""
    pos = torch.arange(S)
    lo = torch.zeros(B, dtype=torch.long) if k_lo is None else torch.as_tensor(k_lo, dtype=torch.long).cpu()
    hi = torch.full((B,), S, dtype=torch.long) if k_hi is None else torch.as_tensor(k_hi, dtype=torch.long).cpu()
    j = pos[None, None, :]
    return (j <= pos[None, :, None]) & (j >= lo[:, None, None]) & (j < hi[:, None, None])


def attention_reference(Q, K, V, S, scale, k_lo=None, k_hi=None):
    """float64 O [B, Hq, S, dk] of Q [B, Hq, >= S, dk] and K, V [B, Hkv, >= S, dk] (any dtype), on the CPU: the library's repeat_kv and
    masked softmax; a row with no counted key is 0."""
    B, Hq, _, dk = Q.shape
    rep = Hq // K.shape[1]
    f = torch.float64
    ok = counted(S, k_lo, k_hi, B)
    out = torch.zeros((B, Hq, S, dk), dtype=f)
    for b in range(B):
        q = Q[b, :, :S].to(f).cpu()
        k, v = (t[b, :, :S].to(f).cpu().repeat_interleave(rep, dim=0) for t in (K, V))
        s = (q @ k.transpose(-1, -2) * scale).masked_fill(~ok[b], float("-inf"))
        live = ok[b].any(-1)
        p = torch.zeros_like(s)
        p[:, live] = torch.softmax(s[:, live], -1)
        out[b] = p @ v
    return out


def check_attention(name, out, ref, bound=TOL_O, k_lo=None):
    """out [B, Hq, >= S, dk] against ref [B, Hq, S, dk]: every (b, h, 64-row tile) within rel-L2 `bound`, and the rows before k_lo[b] exactly 0;
    returns the worst tile's error"""
    if k_lo is not None:
        for b, lo in enumerate(torch.as_tensor(k_lo).tolist()):
            rows = out[b, :, :lo]
            assert bool((rows == 0).all()), "%s: rows before k_lo = %d of sample %d are not exactly 0 (largest |value| %r)" % (
                name, lo, b, float(rows.double().abs().max()))
    return attn_ref.check_tiles(name, out, ref, bound)


def attention_inputs(B, Hq, Hkv, S, dk, seed, Spad=None, device="cpu"):
    """q, k ~ 1.5 N(0, 1), v ~ N(0, 1) as bf16 [B, H*, Spad, dk], zero beyond S: at scale dk^-1/2 the scores have std 2.25 (the suite's
    `random` kind, tests/attn_ref.py), so a few keys carry each row and a key that leaks in moves it."""
    Spad = (S + 63) // 64 * 64 if Spad is None else Spad
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((B, Hq, S, dk), generator=g)
    k, v = (torch.randn((B, Hkv, S, dk), generator=g) for _ in range(2))
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:2] + (Spad - S, dk))], 2).bfloat16().to(device)
    return pad(1.5 * q), pad(1.5 * k), pad(v)


# ---------------------------------------------------------------------------------------------------------------- RoPE
def rope_reference(x, cos, sin):
    """float64 rotate-half RoPE of x [B, S, H, dk] under the half tables cos, sin [B, S, dk/2] -> (y, the bound's second factor |x1 c| + |x2 s|
    for each half)"""
    f = torch.float64
    x, c, s = x.to(f).cpu(), cos.to(f).cpu()[:, :, None], sin.to(f).cpu()[:, :, None]
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    y = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), -1)
    mag = torch.cat(((x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()), -1)
    return y, mag


def check_rope(name, y, x, cos, sin):
    """Per element |y - e| <= 2^-8 * 1.02 |e| + 2^-21 (|x1 c| + |x2 s|); y, x [B, S, H, dk]; returns the worst error over its bound"""
    want, mag = rope_reference(x, cos, sin)
    bound = TOL_ROW * want.abs() + U_ROPE * mag
    _check_elements(name, y, want, bound)
    return float(((y.double().cpu() - want).abs() / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------- SwiGLU
def silu_f64(x):
    x = x.double()
    return x * torch.sigmoid(x)


def check_swiglu(name, y, a, b):
    """Per element |y - s64 b| <= (2^-8 * 1.02 + U_ACT) |s64 b| + ACT_TAIL |a b|: the bound of check_quick_gelu / check_gated_gelu (the kernel's
    silu is silu_f, the form U_ACT and ACT_TAIL were derived for in tests/gemm_ref.py); returns the worst relative error"""
    a, b = a.double().cpu(), b.double().cpu()
    want = silu_f64(a) * b
    return _check_elements(name, y, want, (TOL_ROW + U_ACT) * want.abs() + ACT_TAIL * (a * b).abs())


# ---------------------------------------------------------------------------------------------------------------- the whole stack
def half_tables(cos, sin, mrope_section=None):
    """The library's rotary_emb(...) output -> the half tables [B, S, dk/2] the kernels take: for [3, B, S, dk] tables the mrope selection
    (chunk i of the frequencies from axis i % 3, as apply_multimodal_rotary_pos_emb), then the first half (the two halves are equal)."""
    if cos.dim() == 4:
        sec = list(mrope_section) * 2
        cos, sin = (torch.cat([m[i % 3] for i, m in enumerate(t.split(sec, dim=-1))], dim=-1) for t in (cos, sin))
    half = cos.shape[-1] // 2
    assert torch.equal(cos[..., :half], cos[..., half:]) and torch.equal(sin[..., :half], sin[..., half:])
    return cos[..., :half], sin[..., :half]


def stack_reference(sd, x, cos, sin, *, num_heads, num_kv_heads, eps, k_lo=None, k_hi=None, prefix=""):
    """float64 restatement of the decoder stack: x [B, S, D] (the embedded input) through every layer of the state dict `sd` (the library's
    key names under `prefix`) and the final norm -> every hidden state [B, C, S, D] in the HF convention.  cos, sin: half tables [B, S, dk/2]
    (any dtype; taken to float64 as they are).  A row with no counted key gets a zero attention output."""
    f = torch.float64
    w = lambda k: sd[prefix + k].to(f)
    B, S, D = x.shape
    Hq, Hkv = num_heads, num_kv_heads
    x = x.to(f)
    c, s = cos.to(f)[:, None], sin.to(f)[:, None]          # [B, 1, S, dk/2]
    ok = counted(S, k_lo, k_hi, B)[:, None]                 # [B, 1, S, S]
    live = ok.any(-1, keepdim=True)
    n = 0
    while prefix + "layers.%d.input_layernorm.weight" % n in sd:
        n += 1
    dk = w("layers.0.self_attn.q_proj.weight").shape[0] // Hq

    def rope(t):
        t1, t2 = t[..., :dk // 2], t[..., dk // 2:]
        return torch.cat((t1 * c - t2 * s, t2 * c + t1 * s), -1)

    hs = [x]
    for i in range(n):
        p = "layers.%d." % i
        lin = lambda t, nm: t @ w(p + nm + ".weight").t() + (w(p + nm + ".bias") if prefix + p + nm + ".bias" in sd else 0.0)
        h = rms_reference(x, w(p + "input_layernorm.weight"), eps)
        q = rope(lin(h, "self_attn.q_proj").view(B, S, Hq, dk).transpose(1, 2))
        k = rope(lin(h, "self_attn.k_proj").view(B, S, Hkv, dk).transpose(1, 2)).repeat_interleave(Hq // Hkv, dim=1)
        v = lin(h, "self_attn.v_proj").view(B, S, Hkv, dk).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
        sc = (q @ k.transpose(-1, -2) * dk ** -0.5).masked_fill(~ok, float("-inf"))
        pr = torch.where(live, torch.softmax(sc.masked_fill(~live, 0.0), -1), torch.zeros((), dtype=f))
        a = (pr @ v).transpose(1, 2).reshape(B, S, Hq * dk)
        x = x + lin(a, "self_attn.o_proj")
        h = rms_reference(x, w(p + "post_attention_layernorm.weight"), eps)
        x = x + lin(silu_f64(lin(h, "mlp.gate_proj")) * lin(h, "mlp.up_proj"), "mlp.down_proj")
        hs.append(x)
    hs[-1] = rms_reference(x, w("norm.weight"), eps)
    return torch.stack(hs, 1)


def library_config(hidden, heads, kv_heads, inter, layers, vocab=64, vl=False, theta=1000000.0):
    kw = dict(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
              num_key_value_heads=kv_heads, max_position_embeddings=8192, rms_norm_eps=1e-6, hidden_act="silu", bos_token_id=0, eos_token_id=1,
              pad_token_id=None, tie_word_embeddings=False, use_cache=False)
    if vl:
        from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLTextConfig
        dk = hidden // heads
        sec = [16, 24, 24] if dk == 128 else [8, 12, 12]
        return Qwen2_5_VLTextConfig(rope_parameters=dict(rope_type="default", mrope_section=sec, rope_theta=theta), **kw)
    from transformers import Qwen2Config
    return Qwen2Config(rope_parameters=dict(rope_type="default", rope_theta=theta), **kw)


def library_stack(hidden, heads, kv_heads, inter, layers, vocab=64, vl=False, attn="sdpa"):
    """(config, `transformers` Qwen2Model or Qwen2_5_VLTextModel in float32 on the CPU, its own initialisation under a fixed seed).
    attn_implementation sdpa: the eager path computes its softmax in float32 whatever the dtype and is NaN on the rows of left padding"""
    cfg = library_config(hidden, heads, kv_heads, inter, layers, vocab, vl)
    cfg._attn_implementation = attn
    if vl:
        from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VLTextModel as cls
    else:
        from transformers import Qwen2Model as cls
    torch.manual_seed(0)
    return cfg, cls(cfg).eval().requires_grad_(False)


def random_stack_state_dict(stack, seed):
    """The test weights of a library decoder: its initialisation (std 0.02) scaled to N(0, 1 / fan_in) for the matrices, so that the layers
    move the residual stream, all rounded to bf16; every 1-D tensor -- the norm weights and the q|k|v biases, whose defaults are one and
    zero and would hide a missing bias -- perturbed by 0.1 N(0, 1); the token table N(0, 1); float32 tensors that hold bf16 values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in stack.state_dict().items():
        v = v.detach().float().clone()
        if v.dim() == 1:
            v = v + 0.1 * torch.randn(v.shape, generator=g)
        elif k.startswith("embed_tokens"):
            v = torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * v.shape[1] ** -0.5
        sd[k] = v.bfloat16().float()
    return sd


def mrope_positions(B, S, seed, top=4000):
    """int64 [3, B, S]: three position axes that differ from each other (a text run, then a `grid` whose axes move at different rates)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S)[None].expand(B, S).clone()
    h = (t // 3 + torch.randint(0, 7, (B, 1), generator=g)).clamp_max(top)
    w = (t % 11 + torch.randint(0, 50, (B, S), generator=g)).clamp_max(top)
    return torch.stack((t, h, w))
