"""The Qwen2.5-VL vision tower on the HIP path: a drop-in for `transformers`' Qwen2_5_VisionTransformerPretrainedModel, the module behind
`model.visual` of Qwen2.5-VL 3B / 7B, which runs first whenever a prompt holds pixels (image2image, imagetext2image, video2image, x2image).

One packed sequence holds every patch of every image and frame, in WINDOW ORDER (the library's window_index permutation of the 2 x 2 merge
units).  A layer attends inside windows (segments of 4 .. 64 tokens) or, in the fullatt_block_indexes layers, inside one frame; both are a
key range per query row, row_lo[i] <= j < row_hi[i], which is all x2i_vit_attention_bf16 knows of them (include/x2i_vit.h).

Launch list (every launch in libx2i_hip.so; include/x2i_vit.h, x2i_qwen.h, x2i_t5.h and x2i.h):
  gemm          the patch embedding: Conv3d(kernel = stride) as a [hidden, C*T*P*P] linear          x2i_gemm_bf16
  (torch gather into window order)
  per layer, nine launches:
  rms_rows      norm1 (Qwen2_5_VLRMSNorm == T5LayerNorm)                                            x2i_t5_rms_rows_bf16
  gemm          qkv + bias                                                                          x2i_gemm_bf16
  rope_split    rotate-half RoPE on q, k -> Q, K [1,H,Spad,dkp], V^T                                x2i_vit_rope_split_bf16
  attention     bidirectional, a key range per row (windows or frames)                              x2i_vit_attention_bf16
  gemm          proj + bias + residual (one rounding)
  rms_rows      norm2
  gemm          stacked [gate_proj; up_proj] + bias
  swiglu        silu(a) * b                                                                         x2i_qwen_swiglu_bf16
  gemm          down_proj + bias + residual
  the merger, three launches: rms_rows (ln_q) -> view [S/4, 4 hidden] -> gemm + bias + GELU(erf) -> gemm + bias
  (torch gather back into the original order)

Packed storage, built at construction; the parameters carry the library's names and are views of it (re-pointed in _apply, as
Qwen2DecoderStack's are), so a tower's state dict loads strictly:
  * [gate_proj; up_proj] stacked, each padded with zero rows (and zero biases) from the intermediate width F (3420) to Fp, the next
    multiple of 64 (3456); down_proj gains Fp - F zero columns.  Exact: silu(0) * 0 = 0 meets a zero column.  Every GEMM of a full-width
    layer then has K % 64 == 0 and takes the GEMM's fast path
  * the patch embedding's Conv3d weight [hidden, C, T, P, P] is the first C*T*P*P = 1176 columns of a [hidden, 1216] matrix whose other
    columns are zero; the pixel rows are copied (and rounded to bf16) into a workspace [S, 1216] whose last 40 columns were zeroed once
"""
import torch
import torch.nn as nn

from . import ops, qwen_ops, t5_ops, vit_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(depth=32, hidden_size=1280, hidden_act="silu", intermediate_size=3420, num_heads=16, in_channels=3, patch_size=14,
               spatial_merge_size=2, temporal_patch_size=2, window_size=112, out_hidden_size=3584, fullatt_block_indexes=(7, 15, 23, 31))
_EPS = 1e-6     # the library's Qwen2_5_VLRMSNorm(eps=1e-6) in the blocks and in the merger
_THETA = 10000.0


# ---------------------------------------------------------------------------------------------------------------- the host work of a call
def vision_position_ids(grid, merge):
    """int64 [S, 2] (h, w) of every patch, block-major over the merge x merge units, repeated over t: the library's get_vision_position_ids
    for a list of (t, h, w)"""
    out = []
    for t, h, w in grid:
        hp, wp = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        shape = (h // merge, merge, w // merge, merge)
        hp, wp = (p.reshape(shape).transpose(1, 2).flatten() for p in (hp, wp))
        out.append(torch.stack([hp, wp], dim=-1).repeat(t, 1))
    return torch.cat(out, dim=0)


def vision_window_index(grid, merge, window_size, patch_size):
    """(window_index int64 [S / merge^2] over the merge units, cu_window_seqlens int32 over tokens): the library's get_vision_window_index.
    A window is win x win merge units (win = window_size / merge / patch_size); windows at the right and bottom edges are smaller, and the
    library's padding gives a whole empty row / column of windows when the grid divides evenly, which unique_consecutive removes."""
    win, unit = window_size // merge // patch_size, merge * merge
    index, cu, base, off = [], [torch.zeros(1, dtype=torch.int64)], 0, 0
    for t, h, w in grid:
        gh, gw = h // merge, w // merge
        idx = torch.arange(t * gh * gw).reshape(t, gh, gw)
        ph, pw = win - gh % win, win - gw % win
        nh, nw = (gh + ph) // win, (gw + pw) // win
        idx = torch.nn.functional.pad(idx, (0, pw, 0, ph), "constant", -100)
        idx = idx.reshape(t, nh, win, nw, win).permute(0, 1, 3, 2, 4).reshape(t, nh * nw, win, win)
        lens = (idx != -100).sum([2, 3]).reshape(-1)
        idx = idx.reshape(-1)
        index.append(idx[idx != -100] + base)
        cu.append(lens.cumsum(0) * unit + off)
        base += t * gh * gw
        off += t * h * w
    return torch.cat(index), torch.unique_consecutive(torch.cat(cu).to(torch.int32))


def vision_cu_seqlens(grid):
    """int32 cumulative frame boundaries: h * w tokens per frame, t frames per entry (the library's get_vision_cu_seqlens)"""
    lens = torch.tensor([h * w for t, h, w in grid for _ in range(t)], dtype=torch.int64)
    return torch.nn.functional.pad(lens.cumsum(0, dtype=torch.int32), (1, 0), value=0)


def row_ranges(cu, S):
    """(row_lo, row_hi) int32 [1, S] of cumulative boundaries cu (cu[0] = 0, cu[-1] = S): row i of segment s gets [cu[s], cu[s + 1]).
    bucketize on cu's device, no host read."""
    seg = torch.bucketize(torch.arange(S, device=cu.device, dtype=cu.dtype), cu[1:], right=True)
    return cu[seg].to(torch.int32)[None].contiguous(), cu[seg + 1].to(torch.int32)[None].contiguous()


class VisionPlan:
    """Everything of a call that depends on grid_thw alone (Qwen2_5VisionTower.plan)"""


class Qwen2_5VisionTower(PackedModule):
    """Drop-in for transformers' Qwen2_5_VisionTransformerPretrainedModel.  forward(pixel_rows, grid_thw) -> BaseModelOutputWithPooling."""

    def __init__(self, config=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        f = config_fields(_FIELDS, config, kw, "Qwen2_5VisionTower")
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        if f["hidden_act"] != "silu":
            raise ValueError("x2i_amd Qwen2_5VisionTower: hidden_act=%r is not built (silu only)" % (f["hidden_act"],))
        D, H, F, L = f["hidden_size"], f["num_heads"], f["intermediate_size"], f["depth"]
        if H <= 0 or D % H or D // H not in (64, 80, 128):
            raise ValueError("x2i_amd Qwen2_5VisionTower: the HIP attention kernel is built for head widths 64, 80 and 128 (got hidden_size=%r, num_heads=%r)" % (D, H))
        if F <= 0 or L < 1 or f["out_hidden_size"] % 8:
            raise ValueError("x2i_amd Qwen2_5VisionTower: need a layer, a positive intermediate_size and out_hidden_size % 8 == 0")
        if f["window_size"] // f["spatial_merge_size"] // f["patch_size"] < 1:
            raise ValueError("x2i_amd Qwen2_5VisionTower: window_size must hold at least one merge unit")
        f["fullatt_block_indexes"] = tuple(f["fullatt_block_indexes"])
        f["head_dim"] = D // H
        self.config = config_object("Qwen2_5VisionTowerConfig", f)
        self.spatial_merge_size = f["spatial_merge_size"]          # (the surrounding model reads it)
        self.spatial_merge_unit = unit = f["spatial_merge_size"] ** 2
        self.patch_dim = Kpe = f["in_channels"] * f["temporal_patch_size"] * f["patch_size"] ** 2
        self.Fp, self.Kp = Fp, Kp = vit_ops.pad64(F), vit_ops.pad64(Kpe)
        param, view = self._param, self._view
        cols = lambda n: (slice(None), slice(0, n))
        self._store("pe", D, Kp, zero=True)
        self.patch_embed = nn.Module()
        self.patch_embed.add_module("proj", WB(view("pe", cols(Kpe), (D, f["in_channels"], f["temporal_patch_size"], f["patch_size"], f["patch_size"]))))
        blocks = []
        for i in range(L):
            self._store("%d.gu.w" % i, 2 * Fp, D, zero=True)
            self._store("%d.gu.b" % i, 2 * Fp, zero=True)
            self._store("%d.down" % i, D, Fp, zero=True)
            att = nn.Module()
            att.add_module("qkv", WB(param(3 * D, D), param(3 * D)))
            att.add_module("proj", WB(param(D, D), param(D)))
            mlp = nn.Module()
            mlp.add_module("gate_proj", WB(view("%d.gu.w" % i, slice(0, F)), view("%d.gu.b" % i, slice(0, F))))
            mlp.add_module("up_proj", WB(view("%d.gu.w" % i, slice(Fp, Fp + F)), view("%d.gu.b" % i, slice(Fp, Fp + F))))
            mlp.add_module("down_proj", WB(view("%d.down" % i, cols(F)), param(D)))
            blk = nn.Module()
            blk.add_module("norm1", WB(param(D)))
            blk.add_module("norm2", WB(param(D)))
            blk.add_module("attn", att)
            blk.add_module("mlp", mlp)
            blocks.append(blk)
        self.blocks = nn.ModuleList(blocks)
        self.merger = nn.Module()
        self.merger.add_module("ln_q", WB(param(D)))
        mm = nn.Module()
        mm.add_module("0", WB(param(unit * D, unit * D), param(unit * D)))
        mm.add_module("2", WB(param(f["out_hidden_size"], unit * D), param(f["out_hidden_size"])))
        self.merger.add_module("mlp", mm)

    @classmethod
    def from_hf(cls, visual, device=None):
        """A bf16 copy of an instantiated library tower on `device` (default: the tower's)"""
        w = visual.merger.ln_q.weight
        device = w.device if device is None else torch.device(device)
        m = cls(visual.config, device=device)
        m.load_state_dict({k: v.detach().to(device=device, dtype=torch.bfloat16) for k, v in visual.state_dict().items()}, strict=True)
        return m

    def init_random_(self, seed=0):
        """Random weights in place (tools; there are no checkpoints offline): matrices N(0, 1 / fan_in), biases 0.1 N(0, 1), norms 1 + 0.1 N(0, 1)"""
        def rule(n, p, r):
            if "norm" in n or "ln_q" in n:
                return 1.0 + 0.1 * r
            return 0.1 * r if p.dim() == 1 else r * (p.numel() // p.shape[0]) ** -0.5

        self._init_random(seed, rule)
        return self

    # ------------------------------------------------------------------ plan
    @torch.no_grad()
    def plan(self, grid_thw):
        """All the host work of a call, once per grid: the window permutation and its inverse, the key ranges of the window layers and of the
        full-attention layers, the half RoPE tables in window order and the workspaces.  grid_thw: [n, 3] (t, h, w) per image / video, a tensor
        (ONE host read, as the library's) or a list.  A restatement of the library's get_vision_position_ids, get_vision_window_index and
        get_vision_attention_seqlens; the result lives on the module's device and is valid until the module moves."""
        c = self.config
        grid = tuple(tuple(int(v) for v in g) for g in (grid_thw.tolist() if isinstance(grid_thw, torch.Tensor) else grid_thw))
        m, unit, dk, D, H = c.spatial_merge_size, self.spatial_merge_unit, c.head_dim, c.hidden_size, c.num_heads
        if not grid or any(len(g) != 3 or min(g) < 1 or g[1] % m or g[2] % m for g in grid):
            raise ValueError("x2i_amd Qwen2_5VisionTower: grid_thw must be rows (t, h, w) with h and w multiples of the merge size %d, so that the token "
                             "count divides by the merge unit %d (got %r)" % (m, unit, grid))
        dev = self.device
        p = VisionPlan()
        p.grid, p.device = grid, dev
        p.S = S = sum(t * h * w for t, h, w in grid)
        p.Spad = Spad = vit_ops.pad64(S)
        widx, cu_win = vision_window_index(grid, m, c.window_size, c.patch_size)
        p.window_index = widx.to(dev)
        p.reverse = torch.argsort(widx).to(dev)
        p.perm = (widx[:, None] * unit + torch.arange(unit)).flatten().to(dev)     # tokens: the merge units move whole
        p.cu_window_seqlens = cu_win.to(dev)
        p.cu_seqlens = vision_cu_seqlens(grid).to(dev)
        p.win_lo, p.win_hi = row_ranges(p.cu_window_seqlens, S)
        p.full_lo, p.full_hi = row_ranges(p.cu_seqlens, S)
        # the library's f32 expression: inv_freq = 1 / theta^(2k / dim) over dim = dk / 2, angle = position * inv_freq for h then w
        p.position_ids = vision_position_ids(grid, m).to(dev)
        dim = dk // 2
        inv_freq = (1.0 / (_THETA ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))).to(dev)
        ang = (p.position_ids.unsqueeze(-1) * inv_freq).flatten(1)
        ang = ang.reshape(S // unit, unit, -1)[p.window_index].reshape(1, S, dk // 2)
        p.cos, p.sin = ang.cos().contiguous(), ang.sin().contiguous()
        if dev.type == "cuda":
            bf = dict(device=dev, dtype=torch.bfloat16)
            dkp = vit_ops.stored_width(dk)
            # PX's padding columns, and Q, K, V^T, are zeroed once: rope_split writes rows / columns s < S, d < dk only, and the attention
            # kernel needs the rows and columns < dk of K and V^T finite up to Spad
            p.ws = dict(PX=torch.zeros((S, self.Kp), **bf), X0=torch.empty((S, D), **bf), XA=torch.empty((S, D), **bf), XB=torch.empty((S, D), **bf),
                        NRM=torch.empty((S, D), **bf), QKV=torch.empty((S, 3 * D), **bf), Q=torch.zeros((1, H, Spad, dkp), **bf),
                        K=torch.zeros((1, H, Spad, dkp), **bf), VT=torch.zeros((1, H, dkp, Spad), **bf), ATT=torch.empty((S, D), **bf),
                        HH=torch.empty((S, 2 * self.Fp), **bf), G=torch.empty((S, self.Fp), **bf), M1=torch.empty((S // unit, unit * D), **bf),
                        M2=torch.empty((S // unit, c.out_hidden_size), **bf))
        return p

    # ------------------------------------------------------------------ forward
    def _block(self, i, plan, x, out):
        """block i on the rows x [S, hidden] (window order) -> out (which may be x): nine launches"""
        c, ws, blk = self.config, plan.ws, self.blocks[i]
        D, H, dk, S, Spad = c.hidden_size, c.num_heads, c.head_dim, plan.S, plan.Spad
        XB, NRM, QKV, Q, K, VT, ATT, HH, G = (ws[k] for k in ("XB", "NRM", "QKV", "Q", "K", "VT", "ATT", "HH", "G"))
        lo, hi = (plan.full_lo, plan.full_hi) if i in c.fullatt_block_indexes else (plan.win_lo, plan.win_hi)
        t5_ops.rms_rows(x, blk.norm1.weight, _EPS, out=NRM)
        ops.gemm(NRM, blk.attn.qkv.weight, blk.attn.qkv.bias, out=QKV, M=S)
        vit_ops.rope_split(QKV, plan.cos, plan.sin, Q, K, VT, 1, S, Spad, H, dk)
        vit_ops.attention(Q, K, VT, ATT, 1, H, S, Spad, dk, dk ** -0.5, D, S * D, lo, hi)
        ops.gemm(ATT, blk.attn.proj.weight, blk.attn.proj.bias, out=XB, M=S, res=x, ldr=D)
        t5_ops.rms_rows(XB, blk.norm2.weight, _EPS, out=NRM)
        ops.gemm(NRM, self._fused["%d.gu.w" % i], self._fused["%d.gu.b" % i], out=HH, M=S)
        qwen_ops.swiglu(HH, out=G)
        ops.gemm(G, self._fused["%d.down" % i], blk.mlp.down_proj.bias, out=out, M=S, res=XB, ldr=D)

    @torch.no_grad()
    def forward(self, pixel_rows, grid_thw=None, plan=None, **unused):
        """pixel_rows: [S, C*T*P*P] patches as the library's processor flattens them (any float dtype; rounded to bf16), on the module's
        device.  -> BaseModelOutputWithPooling: pooler_output bf16 [S / 4, out_hidden_size], the merged rows in the ORIGINAL order;
        last_hidden_state bf16 [S, hidden_size] in WINDOW order, as the library has it.  With a plan (self.plan(grid_thw)) the call only
        enqueues: no host read, no synchronisation, two allocations (the two results).  Without one, grid_thw is read once and the plan of
        the last grid is kept."""
        if plan is None:
            if grid_thw is None:
                raise ValueError("Qwen2_5VisionTower: pass grid_thw or a plan")
            plan = self._plan_for(tuple(tuple(int(v) for v in g) for g in grid_thw.tolist()))     # the one host read
        S = plan.S
        if plan.device != self.device or not hasattr(plan, "ws"):
            raise ValueError("x2i_amd Qwen2_5VisionTower: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        if pixel_rows.dim() != 2 or tuple(pixel_rows.shape) != (S, self.patch_dim):
            raise ValueError("x2i_amd Qwen2_5VisionTower: pixel rows must be [S, C*T*P*P] = [%d, %d] for grid %r (got %s)" % (S, self.patch_dim, plan.grid, tuple(pixel_rows.shape)))
        if pixel_rows.device != self.device:
            raise ops._lib.X2IError("x2i_amd: pixel rows must live on the model's device (got %s)" % pixel_rows.device)
        plan.ws["PX"][:, :self.patch_dim].copy_(pixel_rows)
        return self.forward_from_workspace(plan)

    def pixel_workspace(self, plan):
        """The tower's padded pixel rows of a plan: bf16 [S, Kp = 1216], of which forward_from_workspace reads everything.  Columns
        1176 .. 1215 were zeroed once, when the plan was made, and must stay zero: a front end writes [:, :1176] only
        (x2i_amd/qwen_image.py: out=this, row_stride=1216, out_dtype=bfloat16)."""
        if plan.device != self.device or not hasattr(plan, "ws"):
            raise ValueError("x2i_amd Qwen2_5VisionTower: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        return plan.ws["PX"]

    @torch.no_grad()
    def forward_from_workspace(self, plan):
        """Everything of forward after its copy of the pixel rows: the rows are those that stand in pixel_workspace(plan), already bf16.
        Only enqueues, like forward with a plan."""
        from transformers.modeling_outputs import BaseModelOutputWithPooling
        c = self.config
        D, L, unit = c.hidden_size, len(self.blocks), self.spatial_merge_unit
        S = plan.S
        ws = plan.ws
        PX, X0, XA, NRM, M1, M2 = (ws[k] for k in ("PX", "X0", "XA", "NRM", "M1", "M2"))
        ops.gemm(PX, self._fused["pe"], out=X0, M=S)
        torch.index_select(X0, 0, plan.perm, out=XA)      # into window order: a torch gather
        last = torch.empty((S, D), device=self.device, dtype=torch.bfloat16)
        for i in range(L):
            self._block(i, plan, XA, last if i + 1 == L else XA)
        t5_ops.rms_rows(last, self.merger.ln_q.weight, _EPS, out=NRM)
        fc1, fc2 = getattr(self.merger.mlp, "0"), getattr(self.merger.mlp, "2")
        ops.gemm(NRM.view(S // unit, unit * D), fc1.weight, fc1.bias, out=M1, M=S // unit, act=ops.ACT_GELU_ERF)
        ops.gemm(M1, fc2.weight, fc2.bias, out=M2, M=S // unit)
        return BaseModelOutputWithPooling(last_hidden_state=last, pooler_output=torch.index_select(M2, 0, plan.reverse))
