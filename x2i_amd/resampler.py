"""The MiniCPM-o Resampler on the HIP path: a drop-in for the perceiver behind `model.resampler` of MiniCPM-o 2.6 (Resampler of the model's
own resampler.py), which get_vllm_embedding calls on the SigLIP tower's output whenever a prompt holds pixels.

A call holds B frames of L patch rows each, x [B, L, kv_dim]; frame b has n_b = h_b * w_b <= L patches and the rest of its rows is
whatever the tower left there (finite, meaningless).  NQ learned queries cross-attend over the n_b patches of every frame: the keys are
ln_kv(kv_proj(x)) plus a 2-D sin/cos position row, the values the same without the position row.

Launch list per chunk of at most 16 frames (every launch in libx2i_hip.so; include/x2i_resampler.h and x2i.h):
  gemm        kv_proj, no bias                                                                       x2i_gemm_bf16
  ln_pos      XV = ln_kv(.), XK = XV + pos[ids] in one pass (padding rows: XK = XV)                  x2i_resampler_ln_pos_bf16
  gemm x 2    k = XK Wk^T + bk and v = XV Wv^T + bv, side by side into one [rows, 2 D] buffer
  kv_split    -> K [B,H,Lpad,128], V^T [B,H,128,Lpad]                                                x2i_resampler_kv_split_bf16
  attention   the NQ cached query rows against keys [0, n_b), scale = 128 ** -0.5                    x2i_resampler_attention_bf16
  gemm        out_proj + bias
  ln_affine   ln_post                                                                                x2i_ln_affine_bf16
  gemm        @ proj (a transposed packed copy)

Q is no function of the input: ln_q(query) through the q slice of in_proj, plus its bias, as [H][NQpad][128].  It is computed once, by
ln_affine and gemm, and kept until the parameters change (_apply, pack_(), load_state_dict).  The scale 128 ** -0.5 goes on the f32
scores inside the kernel; the reference rounds q / sqrt(128) to bf16 first.

The position table is the reference's: float32 via numpy for the 70 x 70 grid, cast to bf16 once.  Channel quarter by quarter: sin and
cos of the COLUMN index times omega, then sin and cos of the ROW index times omega, omega_k = 10000 ** -(k / (D / 4)).
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops, resampler_ops
from ._packed import WB, PackedModule

MAX_SIDE = 70          # the reference's max_size: the table is built once for 70 x 70 and never grown
CHUNK = 16             # frames per pass over the workspaces
DK = resampler_ops.DK


def sincos_table(embed_dim, side=MAX_SIDE):
    """float32 [side, side, embed_dim]: entry (r, c) is [sin(c w), cos(c w), sin(r w), cos(r w)] with w_k = 1 / 10000 ** (k / (D / 4)),
    k < D / 4, every step in float32 as numpy takes it"""
    if embed_dim % 4:
        raise ValueError("x2i_amd Resampler: the sin/cos position table needs embed_dim %% 4 == 0 (got %d)" % embed_dim)
    quarter = embed_dim // 4
    omega = np.arange(quarter, dtype=np.float32)
    omega /= np.float32(quarter)
    omega = (1.0 / 10000 ** omega).astype(np.float32)
    ang = np.arange(side, dtype=np.float32)[:, None] * omega[None, :]          # [side, D/4]: the angle of index i
    half = np.concatenate([np.sin(ang), np.cos(ang)], axis=1)                   # [side, D/2]
    table = np.empty((side, side, embed_dim), dtype=np.float32)
    table[:, :, :2 * quarter] = half[None, :, :]       # first half of the channels: the column index
    table[:, :, 2 * quarter:] = half[:, None, :]       # second half: the row index
    return torch.from_numpy(table)


def position_ids(sizes, L, side=MAX_SIDE):
    """int32 [B, L]: patch p of a frame with grid (h, w) takes (p // w) * side + p % w, rows >= h * w take -1"""
    ids = torch.full((len(sizes), L), -1, dtype=torch.int32)
    for b, (h, w) in enumerate(sizes):
        p = torch.arange(h * w)
        ids[b, :h * w] = (torch.div(p, w, rounding_mode="floor") * side + p % w).to(torch.int32)
    return ids


class ResamplerPlan:
    """Everything of a call that depends on (tgt_sizes, L) alone (Resampler.plan)"""


class Resampler(PackedModule):
    """Drop-in for MiniCPM-o's `model.resampler`.  forward(x [B, L, kv_dim], tgt_sizes [B, 2]) -> bf16 [B, NQ, embed_dim]."""

    _copies = "_projT"

    def __init__(self, num_queries=64, embed_dim=3584, num_heads=None, kv_dim=1152, eps=1e-6, device="cuda", dtype=torch.bfloat16):
        super().__init__(device)
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        num_heads = embed_dim // DK if num_heads is None else num_heads
        if embed_dim <= 0 or embed_dim % DK or num_heads != embed_dim // DK:
            raise ValueError("x2i_amd Resampler: the HIP attention kernel serves heads of 128 only, embed_dim // 128 of them as the model's "
                             "init_resampler builds them (got embed_dim=%r, num_heads=%r)" % (embed_dim, num_heads))
        if not 1 <= num_queries <= resampler_ops.NQ_MAX:
            raise ValueError("x2i_amd Resampler: 1 .. %d queries (got %r)" % (resampler_ops.NQ_MAX, num_queries))
        if kv_dim is None or kv_dim == embed_dim or kv_dim <= 0 or kv_dim % 8:
            raise ValueError("x2i_amd Resampler: kv_dim must be a positive multiple of 8 other than embed_dim, so that kv_proj is a Linear "
                             "(an Identity kv_proj is not built; got %r)" % (kv_dim,))
        self.num_queries, self.embed_dim, self.num_heads, self.kv_dim, self.eps = num_queries, embed_dim, num_heads, kv_dim, eps
        self.max_size = (MAX_SIDE, MAX_SIDE)
        dev, D, param = torch.device(device), embed_dim, self._param
        self.query = param(num_queries, D)
        self.kv_proj = WB(param(D, kv_dim))
        self.attn = nn.Module()
        self.attn.in_proj_weight = param(3 * D, D)
        self.attn.in_proj_bias = param(3 * D)
        self.attn.add_module("out_proj", WB(param(D, D), param(D)))
        self.ln_q = WB(param(D), param(D))
        self.ln_kv = WB(param(D), param(D))
        self.ln_post = WB(param(D), param(D))
        self.proj = param(D, D)
        # not parameters: the reference keeps its table in a non-persistent buffer, so a state dict does not carry it
        self._pos = sincos_table(D).to(torch.bfloat16).reshape(MAX_SIDE * MAX_SIDE, D).to(dev)
        self._projT = None
        self._Q = None

    @property
    def device(self):
        return self.query.device

    def _moved(self, fn):
        super()._moved(fn)
        self._pos = self._bf16(fn(self._pos))     # no storage is fused here: the table is what refuses another dtype, before a parameter moves
        self._Q = None

    @torch.no_grad()
    def pack_(self):
        """The transposed copy of `proj` ([in, out], used as x @ proj) from the parameter as it is now; the cached Q is dropped"""
        self._projT = self.proj.t().contiguous()
        self._Q = None
        return self

    @classmethod
    def from_hf(cls, module, device=None):
        """A bf16 copy of an instantiated Resampler (the model's `resampler`) on `device` (default: the module's)"""
        device = module.query.device if device is None else torch.device(device)
        kv = getattr(module.kv_proj, "weight", None)
        m = cls(num_queries=module.num_queries, embed_dim=module.embed_dim, num_heads=module.num_heads,
                kv_dim=None if kv is None else kv.shape[1], eps=module.ln_kv.eps, device=device)
        m.load_state_dict({k: v.detach().to(device=device, dtype=torch.bfloat16) for k, v in module.state_dict().items()}, strict=True)
        return m

    def init_random_(self, seed=0):
        """Random weights in place (tools; there are no checkpoints offline): matrices N(0, 1 / fan_in), the queries N(0, 1), biases
        0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1)"""
        def rule(n, p, r):
            if n.startswith("ln_") and n.endswith(".weight"):
                return 1.0 + 0.1 * r
            if n == "query":
                return r
            if p.dim() == 1:
                return 0.1 * r
            return r * p.shape[0 if n == "proj" else 1] ** -0.5

        self._init_random(seed, rule)
        return self.pack_()

    # ------------------------------------------------------------------ the cached queries
    @torch.no_grad()
    def _queries(self):
        """Q bf16 [H, NQpad, 128]: ln_q(query) W_q^T + b_q, head by head; rows >= NQ are zero (the kernel reads and never uses them)"""
        if self._Q is None:
            D, H, NQ = self.embed_dim, self.num_heads, self.num_queries
            qn = ops.ln_affine(self.query, self.ln_q.weight, self.ln_q.bias, self.eps)
            q = ops.gemm(qn, self.attn.in_proj_weight[:D], self.attn.in_proj_bias[:D], M=NQ)
            Q = torch.zeros((H, resampler_ops.pad32(NQ), DK), device=self.device, dtype=torch.bfloat16)
            Q[:, :NQ] = q.view(NQ, H, DK).transpose(0, 1)
            self._Q = Q
        return self._Q

    # ------------------------------------------------------------------ plan
    @torch.no_grad()
    def plan(self, tgt_sizes, L):
        """All the host work of a call, once per (sizes, L): the position ids (-1 in the padding rows), the key counts and the workspaces of
        one chunk of at most 16 frames.  tgt_sizes: [B, 2] (h, w) per frame, a tensor (ONE host read) or a list; L: rows per frame.  The
        result lives on the module's device and is valid until the module moves."""
        sizes = tuple(tuple(int(v) for v in s) for s in (tgt_sizes.tolist() if isinstance(tgt_sizes, torch.Tensor) else tgt_sizes))
        L = int(L)
        if not sizes or L < 1 or any(len(s) != 2 or min(s) < 1 or s[0] * s[1] > L for s in sizes):
            raise ValueError("x2i_amd Resampler: tgt_sizes must be rows (h, w) of positive sizes with h * w <= L = %d patches (got %r)" % (L, sizes))
        if any(max(s) > MAX_SIDE for s in sizes):
            raise ValueError("x2i_amd Resampler: a frame of more than %d patches on a side is beyond the position table (got %r)" % (MAX_SIDE, sizes))
        dev, D, H, NQ = self.device, self.embed_dim, self.num_heads, self.num_queries
        p = ResamplerPlan()
        p.sizes, p.L, p.B, p.device = sizes, L, len(sizes), dev
        p.Lpad = Lpad = resampler_ops.pad64(L)
        p.position_ids = position_ids(sizes, L)               # (on the CPU)
        p.ids = p.position_ids.reshape(-1).to(dev)
        p.n_keys = torch.tensor([h * w for h, w in sizes], dtype=torch.int32).to(dev)
        if dev.type == "cuda":
            bf = dict(device=dev, dtype=torch.bfloat16)
            Bc = min(p.B, CHUNK)
            M = Bc * L
            # K and V^T are zeroed once: kv_split writes rows / columns s < L only, and the attention kernel needs them finite up to Lpad
            p.ws = dict(X0=torch.empty((M, D), **bf), XV=torch.empty((M, D), **bf), XK=torch.empty((M, D), **bf), KV=torch.empty((M, 2 * D), **bf),
                        K=torch.zeros((Bc, H, Lpad, DK), **bf), VT=torch.zeros((Bc, H, DK, Lpad), **bf), ATT=torch.empty((Bc * NQ, D), **bf),
                        Y=torch.empty((Bc * NQ, D), **bf), Z=torch.empty((Bc * NQ, D), **bf))
        return p

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x, tgt_sizes=None, plan=None):
        """x: [B, L, kv_dim] on the module's device (any float dtype; rounded to bf16), the SigLIP tower's output; tgt_sizes: int [B, 2]
        (h, w) with h * w the frame's patch count.  -> bf16 [B, NQ, embed_dim].  Rows >= h * w of a frame are never read past ln_kv: no
        result depends on them.  With a plan (self.plan(tgt_sizes, L)) the call only enqueues: no host read, no synchronisation, one
        allocation (the result).  Without one, the sizes are read once and the plan of the last shape is kept."""
        D, H, NQ, eps = self.embed_dim, self.num_heads, self.num_queries, self.eps
        if x.dim() != 3 or x.shape[2] != self.kv_dim or not x.shape[0] or not x.shape[1]:
            raise ValueError("x2i_amd Resampler: x must be [B, L, kv_dim = %d] (got %s)" % (self.kv_dim, tuple(x.shape)))
        B, L = x.shape[0], x.shape[1]
        if plan is None:
            if tgt_sizes is None:
                raise ValueError("x2i_amd Resampler: tgt_sizes (or a plan) is needed, as in the reference")
            plan = self._plan_for(tuple((int(h), int(w)) for h, w in tgt_sizes.tolist()), L)      # the one host read
        if plan.device != self.device or not hasattr(plan, "ws"):
            raise ValueError("x2i_amd Resampler: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        if (plan.B, plan.L) != (B, L):
            raise ValueError("x2i_amd Resampler: the plan is for %d frames of %d rows, x holds %d of %d" % (plan.B, plan.L, B, L))
        if x.device != self.device:
            raise ops._lib.X2IError("x2i_amd: x must live on the model's device (got %s)" % x.device)
        if self._projT is None:
            self.pack_()
        if x.dtype != torch.bfloat16:
            x = x.to(torch.bfloat16)
        if not x.is_contiguous():
            x = x.contiguous()
        Q = self._queries()
        ws, Lpad, att = plan.ws, plan.Lpad, self.attn
        X0, XV, XK, KV, K, VT, ATT, Y, Z = (ws[k] for k in ("X0", "XV", "XK", "KV", "K", "VT", "ATT", "Y", "Z"))
        w_k, w_v, b_k, b_v = att.in_proj_weight[D:2 * D], att.in_proj_weight[2 * D:], att.in_proj_bias[D:2 * D], att.in_proj_bias[2 * D:]
        out = torch.empty((B, NQ, D), device=self.device, dtype=torch.bfloat16)
        for b0 in range(0, B, CHUNK):
            Bc = min(CHUNK, B - b0)
            M = Bc * L
            ops.gemm(x, self.kv_proj.weight, None, out=X0, M=M, a_offset=b0 * L * self.kv_dim)
            resampler_ops.ln_pos(X0, self.ln_kv.weight, self.ln_kv.bias, eps, plan.ids[b0 * L:b0 * L + M], self._pos, XV, XK, rows=M)
            ops.gemm(XK, w_k, b_k, out=KV, M=M, ldc=2 * D)
            ops.gemm(XV, w_v, b_v, out=KV, M=M, ldc=2 * D, c_offset=D)
            resampler_ops.kv_split(KV[:, :D], KV[:, D:], K, VT, Bc, L, Lpad, H)
            resampler_ops.attention(Q, K, VT, ATT, Bc, H, NQ, L, Lpad, DK ** -0.5, D, NQ * D, plan.n_keys[b0:b0 + Bc])
            ops.gemm(ATT, att.out_proj.weight, att.out_proj.bias, out=Y, M=Bc * NQ)
            ops.ln_affine(Y[:Bc * NQ], self.ln_post.weight, self.ln_post.bias, eps, out=Z[:Bc * NQ])
            ops.gemm(Z, self._projT, None, out=out, M=Bc * NQ, c_offset=b0 * NQ * D)
        return out
