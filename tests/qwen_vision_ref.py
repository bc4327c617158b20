"""float64 references and checkers for the Qwen2.5-VL vision tower's kernels and host module (include/x2i_vit.h, x2i_amd/qwen_vision.py).  No
GPU-only code here: the CPU tests of the checkers import it too.

  attention   softmax(scale q k^T) v over the keys row_lo[i] <= j < row_hi[i] (clamped into [0, S]); a row with an empty range is 0; errors per
              (b, h, 64-row tile) as tests/attn_ref.py
  RoPE        tests/qwen_ref.py's checker: the kernel shares its arithmetic with x2i_qwen_rope_split_bf16
  tower       the whole tower restated in float64 from a state dict with the library's key names
"""
import torch

from tests import attn_ref
from tests.qwen_ref import check_rope, silu_f64  # noqa: F401  (check_rope: for the tests that import this module)
from tests.t5_ref import TOL_ROW, rel_l2, rms_reference  # noqa: F401

TOL_O = attn_ref.TOL_O      # the family's bound (tests/qwen_ref.py)


def stored_width(dk):
    return 128 if dk == 80 else dk


# ---------------------------------------------------------------------------------------------------------------- attention
def segment_ranges(segments):
    """(row_lo, row_hi) as Python lists: a loop over consecutive segments of the given lengths; every row of a segment gets the segment"""
    lo, hi, start = [], [], 0
    for n in segments:
        for _ in range(n):
            lo.append(start)
            hi.append(start + n)
        start += n
    return lo, hi


def cu_ranges(cu):
    """segment_ranges of cumulative boundaries [0, ..., S]"""
    cu = [int(v) for v in cu]
    return segment_ranges([b - a for a, b in zip(cu[:-1], cu[1:])])


def counted(S, row_lo=None, row_hi=None, B=1):
    """bool [B, S, S]: key j counts for row i of sample b iff clamp(row_lo[b][i]) <= j < clamp(row_hi[b][i]), clamped into [0, S]"""
    lo = torch.zeros((B, S), dtype=torch.long) if row_lo is None else torch.as_tensor(row_lo, dtype=torch.long).cpu().reshape(B, S).clamp(0, S)
    hi = torch.full((B, S), S, dtype=torch.long) if row_hi is None else torch.as_tensor(row_hi, dtype=torch.long).cpu().reshape(B, S).clamp(0, S)
    j = torch.arange(S)[None, None, :]
    return (j >= lo[:, :, None]) & (j < hi[:, :, None])


def attention_reference(Q, K, V, S, dk, scale, row_lo=None, row_hi=None):
    """float64 O [B, H, S, dk] of Q, K, V [B, H, >= S, >= dk] (any dtype; only rows < S and columns < dk are read), on the CPU"""
    B, H = Q.shape[:2]
    f = torch.float64
    ok = counted(S, row_lo, row_hi, B)
    out = torch.zeros((B, H, S, dk), dtype=f)
    for b in range(B):
        q, k, v = (t[b, :, :S, :dk].to(f).cpu() for t in (Q, K, V))
        s = (q @ k.transpose(-1, -2) * scale).masked_fill(~ok[b], float("-inf"))
        live = ok[b].any(-1)
        p = torch.zeros_like(s)
        p[:, live] = torch.softmax(s[:, live], -1)
        out[b] = p @ v
    return out


def check_attention(name, out, ref, bound=TOL_O):
    """out [B, H, >= S, dk] against ref [B, H, S, dk]: every (b, h, 64-row tile) within rel-L2 `bound`; returns the worst tile's error"""
    return attn_ref.check_tiles(name, out, ref, bound)


def attention_inputs(B, H, S, dk, seed, Spad=None, device="cpu"):
    """q, k ~ 1.5 N(0, 1), v ~ N(0, 1) as bf16 [B, H, Spad, stored_width(dk)], zero beyond S and beyond dk (tests/qwen_ref.py's distribution)"""
    Spad = (S + 63) // 64 * 64 if Spad is None else Spad
    dkp = stored_width(dk)
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((B, H, S, dk), generator=g) for _ in range(3))

    def pad(t):
        full = torch.zeros((B, H, Spad, dkp))
        full[:, :, :S, :dk] = t
        return full.bfloat16().to(device)
    return pad(1.5 * q), pad(1.5 * k), pad(v)


# ---------------------------------------------------------------------------------------------------------------- the whole tower
def ordered_linear(x, w, b=None):
    """x @ w.T (+ b) in float64 with the K products of every element added ONE BY ONE in the order of k: an order that does not depend on
    the shapes, so that zero columns appended to x and w add exact zeros and leave every bit of the result alone (a BLAS call may block the
    sum by K and round differently)"""
    out = torch.zeros((x.shape[0], w.shape[0]), dtype=torch.float64)
    for k in range(x.shape[1]):
        out += x[:, k:k + 1] * w[:, k][None]
    return out if b is None else out + b


def mlp_reference(x, gate_w, gate_b, up_w, up_b, down_w, down_b, linear=ordered_linear):
    """float64 Qwen2_5_VLMLP: down(silu(gate(x)) * up(x)) from separate (unpadded) matrices"""
    return linear(silu_f64(linear(x, gate_w, gate_b)) * linear(x, up_w, up_b), down_w, down_b)


def packed_mlp_reference(x, gu_w, gu_b, down_w, down_b, linear=ordered_linear):
    """the same from the tower's packed storage: stacked [gate; up] (each padded to Fp rows) and down_proj with Fp columns"""
    hh = linear(x, gu_w, gu_b)
    Fp = gu_w.shape[0] // 2
    return linear(silu_f64(hh[:, :Fp]) * hh[:, Fp:], down_w, down_b)


def tower_reference(sd, pixel_rows, window_index, cu_window, cu_full, position_ids, *, num_heads, fullatt, unit=4, eps=1e-6, theta=10000.0):
    """float64 restatement of Qwen2_5_VisionTransformerPretrainedModel from the state dict `sd` (the library's key names): pixel_rows
    [S, C*T*P*P]; window_index over the merge units; cu_window / cu_full the cumulative boundaries of the window and the frame segments;
    position_ids [S, 2].  -> (last_hidden_state [S, D] in window order, pooler_output [S / unit, out] in the original order)"""
    f = torch.float64
    w = lambda k: sd[k].to(f)
    x = pixel_rows.to(f) @ w("patch_embed.proj.weight").reshape(sd["patch_embed.proj.weight"].shape[0], -1).t()
    S, D = x.shape
    H, dk = num_heads, D // num_heads
    window_index = torch.as_tensor(window_index)
    x = x.reshape(S // unit, unit, D)[window_index].reshape(S, D)
    dim = dk // 2
    inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))       # the library's f32 table ...
    ang = (position_ids.unsqueeze(-1) * inv_freq).flatten(1)                            # ... and f32 angles, then float64 from there on
    ang = ang.reshape(S // unit, unit, -1)[window_index].reshape(S, -1).to(f)
    c, s = ang.cos()[None], ang.sin()[None]             # [1, S, dk/2]

    def rope(t):                                        # [H, S, dk]
        t1, t2 = t[..., :dk // 2], t[..., dk // 2:]
        return torch.cat((t1 * c - t2 * s, t2 * c + t1 * s), -1)

    n = 0
    while "blocks.%d.norm1.weight" % n in sd:
        n += 1
    for i in range(n):
        p = "blocks.%d." % i
        lin = lambda t, nm: t @ w(p + nm + ".weight").t() + w(p + nm + ".bias")
        h = rms_reference(x, w(p + "norm1.weight"), eps)
        q, k, v = lin(h, "attn.qkv").reshape(S, 3, H, dk).permute(1, 2, 0, 3)
        q, k = rope(q), rope(k)
        a = torch.empty((H, S, dk), dtype=f)
        cu = [int(t) for t in (cu_full if i in fullatt else cu_window)]
        for s0, s1 in zip(cu[:-1], cu[1:]):             # a loop over the segments, as the library's non-flash path
            pr = torch.softmax(q[:, s0:s1] @ k[:, s0:s1].transpose(-1, -2) * dk ** -0.5, -1)
            a[:, s0:s1] = pr @ v[:, s0:s1]
        x = x + lin(a.transpose(0, 1).reshape(S, D), "attn.proj")
        h = rms_reference(x, w(p + "norm2.weight"), eps)
        x = x + lin(silu_f64(lin(h, "mlp.gate_proj")) * lin(h, "mlp.up_proj"), "mlp.down_proj")
    h = rms_reference(x, w("merger.ln_q.weight"), eps).reshape(S // unit, unit * D)
    h = torch.nn.functional.gelu(h @ w("merger.mlp.0.weight").t() + w("merger.mlp.0.bias"))
    h = h @ w("merger.mlp.2.weight").t() + w("merger.mlp.2.bias")
    return x, h[torch.argsort(window_index)]


def library_config(depth, hidden, heads, inter, out_hidden, fullatt):
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLVisionConfig
    return Qwen2_5_VLVisionConfig(depth=depth, hidden_size=hidden, num_heads=heads, intermediate_size=inter, out_hidden_size=out_hidden,
                                  fullatt_block_indexes=list(fullatt))


def library_tower(depth, hidden, heads, inter, out_hidden, fullatt, attn="sdpa"):
    """(config, `transformers` Qwen2_5_VisionTransformerPretrainedModel in float32 on the CPU, its own initialisation under a fixed seed)"""
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel
    cfg = library_config(depth, hidden, heads, inter, out_hidden, fullatt)
    cfg._attn_implementation = attn
    torch.manual_seed(0)
    return cfg, Qwen2_5_VisionTransformerPretrainedModel(cfg).eval().requires_grad_(False)


def random_tower_state_dict(tower, seed):
    """The test weights of a library tower: every matrix (the Conv3d kernel included) N(0, 1 / fan_in), so that the layers move the residual
    stream; every 1-D tensor -- the norm weights and the biases, whose defaults are one and zero and would hide a missing bias -- its
    default plus 0.1 N(0, 1); float32 tensors that hold bf16 values"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in tower.state_dict().items():
        v = v.detach().float().clone()
        if v.dim() == 1:
            v = (torch.ones_like(v) if "norm" in k or "ln_q" in k else torch.zeros_like(v)) + 0.1 * torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * (v.numel() // v.shape[0]) ** -0.5
        sd[k] = v.bfloat16().float()
    return sd


def pixel_rows(grid, seed, patch_dim=1176):
    """N(0, 1) patches [S, C*T*P*P] holding bf16 values, as the processor's normalised pixels roughly are"""
    S = sum(t * h * w for t, h, w in grid)
    return torch.randn((S, patch_dim), generator=torch.Generator().manual_seed(seed)).bfloat16().float()
