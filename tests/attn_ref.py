"""float64 reference of head-dim-128 attention (forward and backward) and a per-tile checker, for the attention kernels' tests.

Layout as the kernels take it: Q, K, V, dO [B, H, Spad, 128] (head-major, zero beyond S).  The reference runs per (b, h) in float64 on the
tensors' device with the explicit formulas, a few heads at a time (one S x S float64 matrix is 170 MB at S = 4608).

The checker measures rel-L2 per (b, h, 64-row tile) over the rows < S, not over the whole tensor: at B = 2, H = 24, S = 4608 one tile that is
50 % wrong moves a whole-tensor rel-L2 by about 8.5e-3, while the product kernels' worst tiles measure 3e-3 to 5e-3.  No GPU-only code here: the CPU
tests of the checker import it too."""
import math

import torch

LOG2E = 1.4426950408889634

# Worst-tile bounds (rel-L2 per 64-row tile against float64; lse2 / D: absolute per row), shared by the CPU tests of the checker and the GPU
# tests of the kernels.  Each is the worst tile measured over the GPU cases (tests/test_attention_fp64_gpu.py and
# test_fused_attention_backward_vs_autograd) times about 1.5, rounded up, and below 1e-2 so that a tile 1 % off fails.
TOL_O = 5e-3      # measured 3.2e-3 (attention_lse, B=2 H=24 S=4600 random); sampling kernels 3.0e-3
TOL_DQ = 7.5e-3   # measured 4.9e-3 (B=2 H=24 S=4600 random)
TOL_DK = 7e-3     # measured 4.7e-3 (B=1 H=24 S=4470 random)
TOL_DV = 5e-3     # measured 3.1e-3 (B=1 H=24 S=4608 random)
TOL_LSE2 = 6e-6   # log2 units: measured 3.8e-6 (B=2 H=24 S=4600 random; lse2 ~ 15, a few fp32 ulps)
TOL_D = 2.5e-6    # measured 1.6e-6 (B=3 H=5 S=4600 random)

# the old whole-tensor bound of the backward tests, kept here only to show what it misses (tests/test_attn_ref_cpu.py)
OLD_GLOBAL_BOUND = 1.5e-2


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def reference(Q, K, V, dO, S, scale, heads=4):
    """float64 attention on the first S rows of bf16 (or any) Q, K, V [B, H, >=S, 128]: O = softmax(scale Q K^T) V, per (b, h).
    Returns a dict of float64 tensors: O, dQ, dK, dV [B, H, S, 128]; lse2 (log2-sum-exp, log2 units, as the kernels write it) and
    D = rowsum(dO * O) [B, H, S].  dO None: forward only (O, lse2).  For a prescaled Q (scale = ln 2) this is softmax(ln2 Qs K^T) V on the
    bf16 Qs the kernel saw."""
    B, H = Q.shape[:2]
    dev = Q.device
    f = torch.float64
    out = {k: torch.empty((B, H, S, 128), dtype=f, device=dev) for k in (("O", "dQ", "dK", "dV") if dO is not None else ("O",))}
    out["lse2"] = torch.empty((B, H, S), dtype=f, device=dev)
    if dO is not None:
        out["D"] = torch.empty((B, H, S), dtype=f, device=dev)
    flat = lambda t: t.reshape(B * H, t.shape[2], t.shape[3])
    q_all, k_all, v_all = flat(Q), flat(K), flat(V)
    do_all = flat(dO) if dO is not None else None
    for i in range(0, B * H, heads):
        j = min(i + heads, B * H)
        q, k, v = (t[i:j, :S].to(f) for t in (q_all, k_all, v_all))
        s = (q @ k.transpose(-1, -2)) * scale
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        del s
        l = p.sum(-1, keepdim=True)
        p /= l
        o = p @ v
        out["O"].view(B * H, S, 128)[i:j] = o
        out["lse2"].view(B * H, S)[i:j] = (m + torch.log(l)).squeeze(-1) * LOG2E
        if dO is None:
            continue
        do = do_all[i:j, :S].to(f)
        d = (do * o).sum(-1, keepdim=True)
        out["D"].view(B * H, S)[i:j] = d.squeeze(-1)
        out["dV"].view(B * H, S, 128)[i:j] = p.transpose(-1, -2) @ do
        ds = do @ v.transpose(-1, -2)
        ds -= d
        ds *= p
        del p
        out["dQ"].view(B * H, S, 128)[i:j] = (ds @ k) * scale
        out["dK"].view(B * H, S, 128)[i:j] = (ds.transpose(-1, -2) @ q) * scale
        del ds
    return out


def tile_errors(out, ref, S, rows=64):
    """rel-L2 per (b, h, row tile) over rows < S of out, ref [B, H, >=S, C] (float64, on ref's device): [B, H, ceil(S / rows)]."""
    B, H = ref.shape[:2]
    a = out[:, :, :S].to(device=ref.device, dtype=torch.float64)
    b = ref[:, :, :S].to(torch.float64)
    nt = (S + rows - 1) // rows
    num = torch.zeros((B, H, nt * rows), dtype=torch.float64, device=ref.device)
    den = torch.zeros_like(num)
    num[:, :, :S] = ((a - b) ** 2).sum(-1)
    den[:, :, :S] = (b ** 2).sum(-1)
    return (num.view(B, H, nt, rows).sum(-1) / den.view(B, H, nt, rows).sum(-1).clamp_min(1e-300)).sqrt()


def check_tiles(name, out, ref, bound, rows=64, S=None):
    """Assert that every (b, h, row tile) of out [B, H, >=S, C] is within rel-L2 `bound` of ref over the rows < S (S: ref's row count by default).
    Returns the worst tile's error; on failure the message names that tile, its error, the median and the number of tiles over the bound."""
    S = ref.shape[2] if S is None else S
    e = tile_errors(out, ref, S, rows)
    worst = float(e.max())
    if not worst <= bound:      # (NaN fails too)
        b, h, t = (int(x) for x in torch.nonzero(e == e.max())[0]) if math.isfinite(worst) else \
            (int(x) for x in torch.nonzero(~torch.isfinite(e))[0])
        raise AssertionError(f"{name}: tile (b={b}, h={h}, rows {t * rows}..{min(S, (t + 1) * rows) - 1}) rel-L2 {worst:.3e} > {bound:.1e}; "
                             f"median {float(e.median()):.3e}, {int((~(e <= bound)).sum())} of {e.numel()} tiles over the bound")
    return worst


def check_rows(name, out, ref, bound, S=None):
    """Assert |out - ref| <= bound on every row < S of out, ref [B, H, >=S] (lse2, D).  Returns the worst absolute error."""
    S = ref.shape[2] if S is None else S
    e = (out[:, :, :S].to(device=ref.device, dtype=torch.float64) - ref[:, :, :S].to(torch.float64)).abs()
    worst = float(e.max())
    if not worst <= bound:
        b, h, r = (int(x) for x in torch.nonzero(~(e < worst) if math.isfinite(worst) else ~torch.isfinite(e))[0])
        raise AssertionError(f"{name}: row (b={b}, h={h}, s={r}) off by {worst:.3e} > {bound:.1e}; {int((~(e <= bound)).sum())} of {e.numel()} "
                             f"rows over the bound")
    return worst


def global_rel_l2(out, ref, S):
    """The whole-tensor rel-L2 over rows < S (what the backward tests used to bound)."""
    a, b = out[:, :, :S].to(device=ref.device, dtype=torch.float64), ref[:, :, :S].to(torch.float64)
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------------------- inputs
KINDS = ("random", "peaked", "anti", "spike")


def make_inputs(kind, B, H, S, Spad, seed, device="cpu"):
    """bf16 Q, K, V, dO [B, H, Spad, 128] on `device` (drawn there), zero beyond S (the kernels' header), for one input kind:
      random  Q, K ~ 1.5 N(0, 1), V, dO ~ N(0, 1) (the suite's style; at scale 1/sqrt(128) the scores have std ~2.3, row maxima near +9)
      peaked  Q, K ~ 2.65 N(0, 1): scores with std ~7, nearly one-hot rows
      anti    Q = -10 u + noise, K = +10 u + noise along one shared unit direction u per head: every valid score is about -9, so the zero
              padding keys, were they let into the softmax, would dominate it
      spike   random with one direction w per head projected out of every row, then row SPIKE_ROW of every 64-row query tile set to
              9 w, and 9 w + 0.3 N(0, 1) for ONE key row in a late key tile (spike_key): those query rows score 0 against every other key
              and ~7.2 (natural units; ~10.3 in log2, past the kernels' defer threshold of 8) against that key, so at its tile their
              running maximum jumps and the online softmax has to rescale -- in the forward kernels and in the statistics pass, in every
              wave that holds such a row.  The key takes ~1/5 of those rows' softmax, the other rows see it as an ordinary key"""
    assert kind in KINDS, kind
    g = torch.Generator(device=device).manual_seed(seed)
    shp = (B, H, S, 128)
    Q, K, V, dO = (torch.randn(shp, generator=g, device=device) for _ in range(4))
    if kind == "random":
        Q, K = Q * 1.5, K * 1.5
    elif kind == "peaked":
        Q, K = Q * 2.65, K * 2.65
    elif kind == "anti":
        u = torch.randn((B, H, 1, 128), generator=g, device=device)
        u /= u.norm(dim=-1, keepdim=True)
        Q, K = Q - 10.0 * u, K + 10.0 * u
    else:
        w = torch.randn((B, H, 1, 128), generator=g, device=device)
        w /= w.norm(dim=-1, keepdim=True)
        Q, K = 1.5 * Q, 1.5 * K
        Q, K = Q - (Q * w).sum(-1, keepdim=True) * w, K - (K * w).sum(-1, keepdim=True) * w
        Q[:, :, SPIKE_ROW::64] = 9.0 * w
        K[:, :, spike_key(S)] = 0.2 * K[:, :, spike_key(S)] + 9.0 * w[:, :, 0]
    pad = lambda t: torch.cat([t, torch.zeros((B, H, Spad - S, 128), device=device)], 2).bfloat16()
    return pad(Q), pad(K), pad(V), pad(dO)


SPIKE_ROW = 37


def spike_key(S):
    """The key row the `spike` inputs align with the spiked query rows: row 13 of key tile ceil(S / 64) - 3."""
    return ((S + 63) // 64 - 3) * 64 + 13
