"""float64 references and helpers for the MiniCPM-o Resampler's kernels and host module (include/x2i_resampler.h, x2i_amd/resampler.py).
No GPU-only code here: the position table and ids, ln_kv with the position add, the learned-query attention with a key count per sample
and the whole module from a state dict, all in float64 on the CPU; a bf16 "library" comparator composed from torch.nn.LayerNorm,
torch.nn.MultiheadAttention and a matmul (the model's own module is not importable where the GPU tests run); and the error checks by
(sample, head) tile.  The `fault` arguments plant the mistakes the checkers are there to catch (tests/test_resampler_ref_cpu.py)."""
import numpy as np
import torch
import torch.nn as nn

from tests import attn_ref

SIDE = 70
DK = 128
TOL_O = attn_ref.TOL_O


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------------------- position table and ids
def position_table(D, side=SIDE, fault=None):
    """float64 [side, side, D] holding the FLOAT32 values the model's table holds: entry (row r, column c) is, quarter by quarter,
    sin(c w), cos(c w), sin(r w), cos(r w) with w_k = 1 / 10000 ** (k / (D / 4)); every step is taken in float32 by numpy, as the model
    takes it, because the rounded float32 values are the contract.  fault="swap": sin and cos change places inside each half."""
    q = D // 4
    w = np.zeros(q, dtype=np.float32)
    for k in range(q):
        w[k] = np.float32(k) / np.float32(q)
    w = (np.float32(1.0) / np.power(np.float32(10000.0), w)).astype(np.float32)
    t = np.zeros((side, side, D), dtype=np.float32)
    first, second = (np.cos, np.sin) if fault == "swap" else (np.sin, np.cos)
    for i in range(side):
        a = (np.float32(i) * w).astype(np.float32)
        t[:, i, 0 * q:1 * q] = first(a)
        t[:, i, 1 * q:2 * q] = second(a)
        t[i, :, 2 * q:3 * q] = first(a)
        t[i, :, 3 * q:4 * q] = second(a)
    return torch.from_numpy(t).double()


def position_ids(sizes, L, side=SIDE):
    """int64 [B, L]: patch p of a frame of h x w patches sits in row p // w, column p % w of the table; rows >= h * w take -1"""
    ids = torch.full((len(sizes), L), -1, dtype=torch.int64)
    for b, (h, w) in enumerate(sizes):
        for p in range(h * w):
            ids[b, p] = (p // w) * side + (p % w)
    return ids


# ---------------------------------------------------------------------------------------------------------------- ln_kv + positions
def layer_norm(x, w, b, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def ln_pos(x, w, b, eps, ids, pos):
    """float64 (XV, XK) of rows x [rows, D]: XV = LayerNorm(x), XK = XV + pos[ids] and XK = XV where ids < 0; ids beyond the table clamp"""
    xv = layer_norm(x, w, b, eps)
    ids = torch.as_tensor(ids, dtype=torch.long)
    add = pos.double()[ids.clamp(0, pos.shape[0] - 1)]
    add[ids < 0] = 0.0
    return xv, xv + add


# ---------------------------------------------------------------------------------------------------------------- attention
def attention_reference(Q, K, V, n_keys, scale, NQ=None, L=None, fault=None):
    """float64 O [B, H, NQ, 128] of Q [H, >= NQ, 128] (shared by the samples), K, V [B, H, >= L, 128] (any dtype; only rows < NQ / < L are
    read), on the CPU.  Key j of sample b counts iff j < clamp(n_keys[b], 0, L) (None: L everywhere); a sample with no key gets 0.
    fault="one_more": one key too many counts."""
    B, H = K.shape[:2]
    NQ = Q.shape[1] if NQ is None else NQ
    L = K.shape[2] if L is None else L
    f = torch.float64
    n = [L] * B if n_keys is None else [min(max(int(v), 0), L) for v in n_keys]
    if fault == "one_more":
        n = [min(v + 1, L) for v in n]
    q = Q[:, :NQ].to(f).cpu()
    out = torch.zeros((B, H, NQ, DK), dtype=f)
    for b in range(B):
        if n[b] == 0:
            continue
        # the mask is by index: what K and V hold at and beyond n[b] is never read (a masked_fill would still meet it in p @ v)
        k, v = K[b, :, :n[b]].to(f).cpu(), V[b, :, :n[b]].to(f).cpu()
        out[b] = torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v
    return out


def heads_of(O, H):
    """token-major [B, NQ, >= 128 H] -> [B, H, NQ, 128]"""
    B, NQ = O.shape[:2]
    return O[:, :, :H * DK].reshape(B, NQ, H, DK).permute(0, 2, 1, 3)


def check_attention(name, out, ref, bound=TOL_O):
    """out, ref [B, H, NQ, 128]: every (b, h) tile within rel-L2 `bound` (a tile of zeros must be met exactly: its error is then
    |out| / 1e-150 and fails); returns the worst tile's error"""
    return attn_ref.check_tiles(name, out, ref, bound, rows=max(ref.shape[2], 1))


# ---------------------------------------------------------------------------------------------------------------- the whole module
def module_reference(sd, x, sizes, *, num_heads, eps=1e-6, table=None, fault=None):
    """float64 output [B, NQ, D] of the Resampler with state dict `sd` (the model's names) on x [B, L, kv_dim] and grids `sizes`.  table:
    [>= h, >= w, D] position table (default: position_table(D)).  Rows >= h * w of x reach nothing."""
    f = torch.float64
    sd = {k: v.to(f).cpu() for k, v in sd.items()}
    x = x.to(f).cpu()
    B, L = x.shape[:2]
    D, H = sd["query"].shape[1], num_heads
    NQ = sd["query"].shape[0]
    table = position_table(D) if table is None else table.to(f)
    side = table.shape[1]
    pos = table.reshape(-1, D)
    ids = position_ids(sizes, L, side)
    w_in, b_in = sd["attn.in_proj_weight"], sd["attn.in_proj_bias"]
    q = layer_norm(sd["query"], sd["ln_q.weight"], sd["ln_q.bias"], eps) @ w_in[:D].T + b_in[:D]
    Q = q.view(NQ, H, DK).permute(1, 0, 2)
    x0 = x.reshape(B * L, -1) @ sd["kv_proj.weight"].T
    xv, xk = ln_pos(x0, sd["ln_kv.weight"], sd["ln_kv.bias"], eps, ids.reshape(-1), pos)
    k = (xk @ w_in[D:2 * D].T + b_in[D:2 * D]).view(B, L, H, DK).permute(0, 2, 1, 3)
    v = (xv @ w_in[2 * D:].T + b_in[2 * D:]).view(B, L, H, DK).permute(0, 2, 1, 3)
    o = attention_reference(Q, k, v, [h * w for h, w in sizes], DK ** -0.5, fault=fault)
    o = o.permute(0, 2, 1, 3).reshape(B * NQ, D)
    y = o @ sd["attn.out_proj.weight"].T + sd["attn.out_proj.bias"]
    z = layer_norm(y, sd["ln_post.weight"], sd["ln_post.bias"], eps)
    return (z @ sd["proj"]).view(B, NQ, D)


class LibraryResampler(nn.Module):
    """The comparator: the same module composed from torch.nn's own LayerNorm, MultiheadAttention (key_padding_mask, need_weights left at
    its default) and a matmul, with the model's parameter names.  Runs in the dtype and on the device it is moved to."""

    def __init__(self, num_queries, embed_dim, num_heads, kv_dim, eps=1e-6):
        super().__init__()
        self.num_queries, self.embed_dim, self.num_heads = num_queries, embed_dim, num_heads
        self.query = nn.Parameter(torch.zeros(num_queries, embed_dim))
        self.kv_proj = nn.Linear(kv_dim, embed_dim, bias=False)
        self.attn = nn.MultiheadAttention(embed_dim, num_heads)
        self.ln_q, self.ln_kv, self.ln_post = (nn.LayerNorm(embed_dim, eps=eps) for _ in range(3))
        self.proj = nn.Parameter(torch.zeros(embed_dim, embed_dim))
        self.register_buffer("table", position_table(embed_dim).float(), persistent=False)

    @torch.no_grad()
    def forward(self, x, tgt_sizes=None):
        sizes = [tuple(int(v) for v in s) for s in (tgt_sizes.tolist() if isinstance(tgt_sizes, torch.Tensor) else tgt_sizes)]
        B, L = x.shape[:2]
        # a frame's position rows are a corner of the table, zero rows behind them; no per-patch host work (the bench times this forward)
        pos = x.new_zeros((B, L, self.embed_dim))
        for b, (h, w) in enumerate(sizes):
            pos[b, :h * w] = self.table[:h, :w].reshape(h * w, -1).to(x.dtype)
        counts = torch.tensor([h * w for h, w in sizes], device=x.device)
        padding = torch.arange(L, device=x.device)[None, :] >= counts[:, None]
        kv = self.ln_kv(self.kv_proj(x))
        q = self.ln_q(self.query)[:, None, :].repeat(1, B, 1)
        out = self.attn(q, (kv + pos).transpose(0, 1), kv.transpose(0, 1), key_padding_mask=padding)[0]
        return self.ln_post(out.transpose(0, 1)) @ self.proj


def random_state_dict(num_queries, embed_dim, kv_dim, seed):
    """float32 state dict (values exactly representable in bf16): matrices N(0, 1 / fan_in), queries N(0, 1), biases 0.1 N(0, 1), norm
    weights 1 + 0.1 N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    D = embed_dim
    r = lambda *s: torch.randn(s, generator=g)
    sd = {"query": r(num_queries, D), "kv_proj.weight": r(D, kv_dim) * kv_dim ** -0.5, "attn.in_proj_weight": r(3 * D, D) * D ** -0.5,
          "attn.in_proj_bias": 0.1 * r(3 * D), "attn.out_proj.weight": r(D, D) * D ** -0.5, "attn.out_proj.bias": 0.1 * r(D),
          "proj": r(D, D) * D ** -0.5}
    for n in ("ln_q", "ln_kv", "ln_post"):
        sd[n + ".weight"] = 1.0 + 0.1 * r(D)
        sd[n + ".bias"] = 0.1 * r(D)
    return {k: v.bfloat16().float() for k, v in sd.items()}


def random_input(sizes, L, kv_dim, seed, garbage=1.0):
    """float32 x [B, L, kv_dim] (bf16-representable): N(0, 1) in the rows < h * w, finite garbage of amplitude `garbage` beyond them"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((len(sizes), L, kv_dim), generator=g)
    junk = garbage * 30.0 * torch.randn((len(sizes), L, kv_dim), generator=g)
    for b, (h, w) in enumerate(sizes):
        x[b, h * w:] = junk[b, h * w:]
    return x.bfloat16().float()
