"""float64 references and checkers for the CLIP text encoder's kernels and host module (include/x2i_clip.h, x2i_amd/clip.py).  No GPU-only
code here: the CPU tests of the checkers import it too.

  attention   softmax_{j <= i}(scale q k^T) v; errors per (b, h, 64-row tile) as tests/attn_ref.py
  quick GELU  x sigmoid(1.702 x), per element
  pooling     both rules of CLIPTextModel (first maximum of the ids; first eos_token_id, 0 when there is none)
  model       the whole text model restated in float64 from a state dict with the library's key names
"""
import torch

from tests import attn_ref
from tests.gemm_ref import ACT_TAIL, U_ACT
from tests.t5_ref import TOL_ROW, _check_elements, rel_l2  # noqa: F401  (rel_l2: for the tests that import this module)

# Worst 64-row tile, rel-L2 against float64: the project's bound for kernels with this arithmetic (f32 scores, bf16 P, f32 accumulation, one
# output rounding), as tests/t5_ref.py takes it.  Measured on MI355X: worst tile 2.86e-3 (B=1 H=2 S=65);
# 1.81e-3 .. 2.60e-3 on the other cases (the comment above ATTENTION_CASES in tests/test_clip_gpu.py).
TOL_O = attn_ref.TOL_O
# quick-GELU per element: (TOL_ROW + U_ACT) |y64| + ACT_TAIL |x|, the form of t5_ref.check_gated_gelu.  The kernel's sigmoid is
# 1 / (1 + exp2(c x)) on v_exp_f32 / v_rcp_f32, the pair (and the form, silu_f's) that U_ACT = 2^-19 and ACT_TAIL = 2^-100 were derived for in
# tests/gemm_ref.py: the product c x in f32 moves the exponent by |c x| 2^-24, i.e. the result by |c x| ln 2 2^-24 relative -- 4e-7 at x = -4,
# where the function is 4.4e-3 |x| -- and where exp2 overflows (x < -52) the kernel returns -0 for a value below 2^-128 |x|.
# Measured on MI355X: worst relative error 3.05e-3 .. 3.89e-3 (bound 3.986e-3: a rounding near half an ulp just above a power of two).


# ---------------------------------------------------------------------------------------------------------------- attention
def attention_reference(Q, K, V, S, scale, heads=8):
    """float64 O [B, H, S, dk] of Q, K, V [B, H, >= S, dk] (any dtype): softmax over the keys j <= i of scale q k^T, as the library states it
    (masked_fill(triu(1), -inf))."""
    B, H, _, dk = Q.shape
    f = torch.float64
    future = torch.ones((S, S), dtype=torch.bool, device=Q.device).triu(1)
    out = torch.empty((B, H, S, dk), dtype=f, device=Q.device)
    for b in range(B):
        for h0 in range(0, H, heads):
            h1 = min(H, h0 + heads)
            q, k, v = (t[b, h0:h1, :S].to(f) for t in (Q, K, V))
            s = (q @ k.transpose(-1, -2) * scale).masked_fill(future, float("-inf"))
            out[b, h0:h1] = torch.softmax(s, -1) @ v
    return out


def check_attention(name, out, ref, bound=TOL_O):
    """out [B, H, >= S, dk] against ref [B, H, S, dk]: every (b, h, 64-row tile) within rel-L2 `bound`; returns the worst tile's error"""
    return attn_ref.check_tiles(name, out, ref, bound)


def attention_inputs(B, H, S, dk, seed, Spad=None, device="cpu"):
    """q, k ~ 1.5 N(0, 1), v ~ N(0, 1) as bf16 [B, H, Spad, dk], zero beyond S: at scale dk^-1/2 the scores have std 2.25 (the suite's
    `random` kind, tests/attn_ref.py), so a few keys carry each row and a key that leaks in from the future moves it."""
    Spad = (S + 63) // 64 * 64 if Spad is None else Spad
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((B, H, S, dk), generator=g) for _ in range(3))
    pad = lambda t: torch.cat([t, torch.zeros((B, H, Spad - S, dk))], 2).bfloat16().to(device)
    return pad(1.5 * q), pad(1.5 * k), pad(v)


# ---------------------------------------------------------------------------------------------------------------- quick GELU
def quick_gelu_f64(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def check_quick_gelu(name, y, x):
    """Per element |y - g64| <= (2^-8 * 1.02 + U_ACT) |g64| + ACT_TAIL |x|; returns the worst relative error"""
    x = x.double().cpu()
    want = quick_gelu_f64(x)
    return _check_elements(name, y, want, (TOL_ROW + U_ACT) * want.abs() + ACT_TAIL * x.abs())


# ---------------------------------------------------------------------------------------------------------------- pooling
def pool_index(ids, eos_token_id):
    """[B] long: the library's two rules, restated without argmax -- the first position of the largest id (eos_token_id == 2), else the first
    position that holds eos_token_id, 0 when none does"""
    out = []
    for row in ids.tolist():
        if eos_token_id == 2:
            out.append(row.index(max(row)))
        else:
            out.append(row.index(eos_token_id) if eos_token_id in row else 0)
    return torch.tensor(out, dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------------- the whole model
def layer_norm_f64(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def model_reference(sd, ids, *, num_heads, eps, eos_token_id, prefix=""):
    """float64 restatement of CLIPTextModel: (last_hidden_state [B, S, D], pooler_output [B, D]) of ids [B, S] under the state dict `sd` (the
    library's key names under `prefix`): embeddings, pre-LN layers under the causal mask, final norm, pooling."""
    f = torch.float64
    w = lambda k: sd[prefix + k].to(f)
    B, S = ids.shape
    x = w("embeddings.token_embedding.weight")[ids] + w("embeddings.position_embedding.weight")[:S]
    D = x.shape[-1]
    H, dk = num_heads, D // num_heads
    future = torch.ones((S, S), dtype=torch.bool).triu(1)
    n = 0
    while prefix + "encoder.layers.%d.layer_norm1.weight" % n in sd:
        n += 1
    for i in range(n):
        p = "encoder.layers.%d." % i
        lin = lambda t, nm: t @ w(p + nm + ".weight").t() + w(p + nm + ".bias")
        h = layer_norm_f64(x, w(p + "layer_norm1.weight"), w(p + "layer_norm1.bias"), eps)
        q, k, v = (lin(h, "self_attn.%s_proj" % nm).view(B, S, H, dk).transpose(1, 2) for nm in "qkv")
        s = (q @ k.transpose(-1, -2) * dk ** -0.5).masked_fill(future, float("-inf"))
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, D)
        x = x + lin(a, "self_attn.out_proj")
        h = layer_norm_f64(x, w(p + "layer_norm2.weight"), w(p + "layer_norm2.bias"), eps)
        x = x + lin(quick_gelu_f64(lin(h, "mlp.fc1")), "mlp.fc2")
    last = layer_norm_f64(x, w("final_layer_norm.weight"), w("final_layer_norm.bias"), eps)
    return last, last[torch.arange(B), pool_index(ids, eos_token_id)]


def library_config(hidden, heads, layers, inter, vocab=64, eos_token_id=2, max_pos=77, hidden_act="quick_gelu"):
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                          max_position_embeddings=max_pos, hidden_act=hidden_act, layer_norm_eps=1e-5, eos_token_id=eos_token_id,
                          bos_token_id=0, pad_token_id=1)


def library_model(hidden, heads, layers, inter, vocab=64, eos_token_id=2, max_pos=77):
    """(config, `transformers` CLIPTextModel in float32 on the CPU, its own initialisation under a fixed seed).
    The attention implementation is the library's default (sdpa): its eager one computes the softmax in float32 whatever the model's dtype"""
    from transformers import CLIPTextModel
    cfg = library_config(hidden, heads, layers, inter, vocab, eos_token_id, max_pos)
    torch.manual_seed(0)
    return cfg, CLIPTextModel(cfg).eval().requires_grad_(False)


def random_model_state_dict(model, seed):
    """The test weights of a `transformers` CLIPTextModel: the library's initialisation rounded to bf16 with every 1-D tensor -- the norm
    weights and all biases, whose defaults are one or zero and would hide a missing bias -- perturbed by 0.1 N(0, 1), and the two embedding
    tables N(0, 1) (the defaults, std 0.02 / 0.01, make every token nearly the same row); float32 tensors that hold bf16 values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        v = v.detach().float().clone()
        if v.dim() == 1:
            v = v + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("_embedding.weight"):
            v = torch.randn(v.shape, generator=g)
        sd[k] = v.bfloat16().float()
    return sd


def strip_prefix(sd):
    """The 5.x spelling of a state dict (no `text_model.`)"""
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}


def with_prefix(sd):
    """The 4.x spelling of a state dict (`text_model.` in front of every key)"""
    return {(k if k.startswith("text_model.") else "text_model." + k): v for k, v in sd.items()}


def ids_with_eos_at(B, S, vocab, positions, eos_token_id, seed):
    """int64 [B, S]: random ids below vocab - 1 with the pooled position planted: sample b's largest id (vocab - 1, for the legacy rule) or
    its first eos_token_id at positions[b]; later positions repeat the planted id (pad == eos), earlier ones never hold it"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 1, (B, S), generator=g)
    plant = vocab - 1 if eos_token_id == 2 else eos_token_id
    ids[ids == plant] = 3
    for b, p in enumerate(positions):
        ids[b, p:] = plant
    return ids
