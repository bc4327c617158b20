"""The InternVL2.5 vision path on the HIP path: InternVisionTower is a drop-in for `model.vision_model` (InternVisionModel of the model's own
modeling_intern_vit.py: InternViT-300M, 24 layers of width 1024, 16 heads of 64, 1025 tokens per 448 x 448 tile) and InternVLVision for
the chat model's `extract_feature` -- the tower, the class token dropped, pixel_shuffle(0.5) and `mlp1` -- which runs first whenever a
prompt holds pixels (image2image, imagetext2image).

A call holds B tiles [B, 3, gh*P, gw*P]; every tile is S = 1 + gh*gw tokens (the class token first) and attention is bidirectional over
all of them: no key ranges.

Launch list (every launch in libx2i_hip.so; include/x2i_internvit.h, x2i_siglip.h, x2i_vit.h, x2i_t5.h and x2i.h):
  patch_rows     the tiles as rows [B*L, Kp = 640] of the patch embedding                             x2i_internvit_patch_rows_bf16
  gemm           Conv2d(kernel = stride) as a [hidden, Kp] linear + bias, written into rows 1.. of X    x2i_gemm_bf16
  embed          row 0 = class + pos[0], rows 1.. += pos[1..], in place                               x2i_internvit_embed_bf16
  per layer, eight launches (ten with qk_normalization):
  ln_affine      norm1 (rms_rows for norm_type = 'rms_norm')                                          x2i_ln_affine_bf16 / x2i_t5_rms_rows_bf16
  gemm           qkv (+ bias)
  [rms_rows x 2  q_norm over the q columns and k_norm over the k columns of the QKV rows, in place]
  head_split     -> Q, K [B,H,Spad,dk], V^T [B,H,dk,Spad]                                              x2i_siglip_head_split_bf16
  attention      bidirectional, all S keys, scale = dk ** -0.5                                        x2i_vit_attention_bf16
  gemm           proj + bias, gate = ls1, res = X:   X = X + ls1 * (acc + bias), one rounding
  ln_affine      norm2
  gemm           fc1 + bias + GELU(erf)
  gemm           fc2 + bias, gate = ls2, res = X
  the tail (InternVLVision), three launches:
  shuffle_ln     class token dropped, pixel_shuffle(0.5), mlp1.0 = LayerNorm(4 hidden)                 x2i_internvit_shuffle_ln_bf16
  gemm           mlp1.1 + bias + GELU(erf)
  gemm           mlp1.3 + bias

LayerScale rides in the GEMM's gate epilogue: `res + gate[n] * (acc + bias[n])` with gate an f32 [hidden] vector shared by every row
(gate_batch_stride = 0) is exactly `hidden + ls * proj(x)`, rounded once where the library rounds three times (the linear, the product,
the sum).  The f32 vectors are COPIES of the bf16 parameters ls1 / ls2 (exact), made at load and again in _apply; pack_() makes them again
after the parameters were written in place.  The Conv2d weight [hidden, 3, P, P] is the first 3*P*P = 588 columns of a [hidden, Kp = 640]
matrix whose other columns are zero (a view).

The position table of a grid comes from the reference's own torch call -- float32 bicubic F.interpolate(align_corners=False) of the patch
rows of position_embedding on the CPU, cast to bf16, behind the class row -- once per grid.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import internvit_ops, ops, siglip_ops, t5_ops, vit_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, intermediate_size=4096, image_size=448, patch_size=14,
               layer_norm_eps=1e-6, hidden_act="gelu", norm_type="layer_norm", qk_normalization=False, qkv_bias=True, num_channels=3)


def layers_to_run(select_layer, num_layers):
    """How many encoder layers produce hidden_states[select_layer] of the NL + 1 entries the reference keeps: -1 -> NL, -k -> NL + 1 - k"""
    n = select_layer if select_layer >= 0 else num_layers + 1 + select_layer
    if not 0 <= n <= num_layers:
        raise ValueError("x2i_amd InternVisionTower: select_layer=%r is outside the %d hidden states of %d layers" % (select_layer, num_layers + 1, num_layers))
    return n


class InternVisionPlan:
    """Everything of a call that depends on (B, gh, gw) alone (InternVisionTower.plan)"""


class InternVisionTower(PackedModule):
    """Drop-in for `model.vision_model`.  forward(pixel_values [B, 3, gh*P, gw*P]) -> BaseModelOutputWithPooling(last_hidden_state bf16
    [B, 1 + gh*gw, hidden], pooler_output = its class row); select_layer picks the reference's hidden_states[select_layer] instead.
    Eval only."""

    _eval_only = True
    _copies = "_ls"

    def __init__(self, config=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        f = config_fields(_FIELDS, config, kw, "InternVisionTower")
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation); dtype=%r is not built" % (dtype,))
        if f["hidden_act"] != "gelu":
            raise ValueError("x2i_amd InternVisionTower: hidden_act=%r is not built (gelu, the erf form, only)" % (f["hidden_act"],))
        if f["norm_type"] not in ("layer_norm", "rms_norm"):
            raise ValueError("x2i_amd InternVisionTower: norm_type=%r is not one of layer_norm, rms_norm" % (f["norm_type"],))
        D, H, F_, NL, P = f["hidden_size"], f["num_attention_heads"], f["intermediate_size"], f["num_hidden_layers"], f["patch_size"]
        if H <= 0 or D % H or D // H not in (64, 128):
            raise ValueError("x2i_amd InternVisionTower: the HIP path serves head widths 64 and 128 (got hidden_size=%r, num_attention_heads=%r)" % (D, H))
        if F_ <= 0 or F_ % 8 or NL < 1:
            raise ValueError("x2i_amd InternVisionTower: need a layer and intermediate_size a positive multiple of 8")
        if f["num_channels"] != 3 or not 1 <= P <= 32 or f["image_size"] // P < 1:
            raise ValueError("x2i_amd InternVisionTower: need 3 channels, patch_size in 1..32 and image_size >= patch_size")
        f["head_dim"] = D // H
        self.config = config_object("InternVisionTowerConfig", f)
        self.side = side = f["image_size"] // P         # patches per side of the position table
        self.patch_dim = Kpe = 3 * P * P
        self.Kp = Kp = internvit_ops.pad64(Kpe)
        self.rms = f["norm_type"] == "rms_norm"
        self._store("pe", D, Kp, zero=True)
        self._ls = None
        self._pos = {}
        param = self._param
        norm = lambda: WB(param(D), None if self.rms else param(D))
        emb = nn.Module()
        emb.class_embedding = param(1, 1, D)
        emb.add_module("patch_embedding", WB(self._view("pe", (slice(None), slice(0, Kpe)), (D, 3, P, P)), param(D)))
        emb.position_embedding = param(1, 1 + side * side, D)
        self.embeddings = emb
        layers = []
        for _ in range(NL):
            att = nn.Module()
            att.add_module("qkv", WB(param(3 * D, D), param(3 * D) if f["qkv_bias"] else None))
            if f["qk_normalization"]:
                att.add_module("q_norm", WB(param(D)))
                att.add_module("k_norm", WB(param(D)))
            att.add_module("proj", WB(param(D, D), param(D)))
            mlp = nn.Module()
            mlp.add_module("fc1", WB(param(F_, D), param(F_)))
            mlp.add_module("fc2", WB(param(D, F_), param(D)))
            layer = nn.Module()
            layer.add_module("attn", att)
            layer.add_module("mlp", mlp)
            layer.add_module("norm1", norm())
            layer.add_module("norm2", norm())
            layer.ls1 = param(D)
            layer.ls2 = param(D)
            layers.append(layer)
        self.encoder = nn.Module()
        self.encoder.add_module("layers", nn.ModuleList(layers))
        self.eval()

    @property
    def _pe(self):
        """The patch embedding's [hidden, Kp] matrix, of which the Conv2d weight is a view"""
        return self._fused["pe"]

    def _moved(self, fn):
        super()._moved(fn)
        self._pos = {}

    @torch.no_grad()
    def pack_(self):
        """The f32 copies of ls1 / ls2 that the GEMM's gate epilogue reads (the module docstring), from the parameters as they are now;
        the cached position tables are dropped with them"""
        self._ls = [(layer.ls1.float().contiguous(), layer.ls2.float().contiguous()) for layer in self.encoder.layers]
        self._pos = {}
        return self

    @classmethod
    def from_hf(cls, vision_model, device=None):
        """A bf16 copy of an instantiated tower (the model's `vision_model`) on `device` (default: the tower's)"""
        w = vision_model.embeddings.class_embedding
        device = w.device if device is None else torch.device(device)
        m = cls(vision_model.config, device=device)
        m.load_state_dict({k: v.detach().to(device=device, dtype=torch.bfloat16) for k, v in vision_model.state_dict().items()}, strict=True)
        return m

    def init_random_(self, seed=0):
        """Random weights in place (tools; there are no checkpoints offline): matrices N(0, 1 / fan_in), the class token and the position
        table N(0, 0.02^2), biases 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1), ls1 / ls2 0.1 (1 + 0.5 N(0, 1))"""
        def rule(n, p, r):
            if n.endswith("position_embedding") or n.endswith("class_embedding"):
                return 0.02 * r
            if n.endswith(".ls1") or n.endswith(".ls2"):
                return 0.1 * (1.0 + 0.5 * r)
            if "norm" in n and n.endswith(".weight"):
                return 1.0 + 0.1 * r
            return 0.1 * r if p.dim() == 1 else r * (p.numel() // p.shape[0]) ** -0.5

        self._init_random(seed, rule)
        return self.pack_()

    # ------------------------------------------------------------------ the host work of a call
    @torch.no_grad()
    def position_table(self, gh, gw):
        """bf16 [1 + gh*gw, hidden] on the module's device: the class row of position_embedding, then its patch rows resampled to the grid
        by the reference's own call (float32 bicubic, align_corners=False, on the CPU; the identity at the native grid), cast to bf16"""
        key = (int(gh), int(gw))
        t = self._pos.get(key)
        if t is None:
            pos = self.embeddings.position_embedding.detach().cpu()
            grid = pos[:, 1:, :].float().reshape(1, self.side, self.side, -1).permute(0, 3, 1, 2)
            grid = F.interpolate(grid, size=key, mode="bicubic", align_corners=False).reshape(1, -1, key[0] * key[1]).permute(0, 2, 1).to(pos.dtype)
            t = self._pos[key] = torch.cat([pos[:, :1, :], grid], dim=1)[0].contiguous().to(self.device)
        return t

    @torch.no_grad()
    def plan(self, B, gh, gw):
        """All the host work of a call, once per (B, gh, gw): the position table of the grid and the workspaces.  The result lives on the
        module's device and is valid until the module moves or its weights are loaded again."""
        c = self.config
        B, gh, gw = int(B), int(gh), int(gw)
        if B < 1 or gh < 1 or gw < 1:
            raise ValueError("x2i_amd InternVisionTower: need B, gh, gw >= 1 (got %r, %r, %r)" % (B, gh, gw))
        dev = self.device
        D, H, dk, F_ = c.hidden_size, c.num_attention_heads, c.head_dim, c.intermediate_size
        p = InternVisionPlan()
        p.B, p.gh, p.gw, p.L, p.device = B, gh, gw, gh * gw, dev
        p.S = S = 1 + gh * gw
        p.Spad = Spad = internvit_ops.pad64(S)
        p.pos = self.position_table(gh, gw)
        if dev.type == "cuda":
            bf = dict(device=dev, dtype=torch.bfloat16)
            M = B * S
            # Q, K, V^T are zeroed once: head_split writes rows / columns s < S only, and the attention kernel needs K and V^T finite up to Spad
            p.ws = dict(PX=torch.empty((B * p.L, self.Kp), **bf), X=torch.empty((B, S, D), **bf), NRM=torch.empty((M, D), **bf),
                        QKV=torch.empty((M, 3 * D), **bf), Q=torch.zeros((B, H, Spad, dk), **bf), K=torch.zeros((B, H, Spad, dk), **bf),
                        VT=torch.zeros((B, H, dk, Spad), **bf), ATT=torch.empty((M, D), **bf), HH=torch.empty((M, F_), **bf))
        return p

    def _check_pixels(self, pixel_values):
        P = self.config.patch_size
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or pixel_values.shape[2] % P or pixel_values.shape[3] % P or not pixel_values.shape[0] \
                or not pixel_values.shape[2] or not pixel_values.shape[3]:
            raise ValueError("x2i_amd InternVisionTower: pixel_values must be [B, 3, gh*P, gw*P] tiles with P = %d (got %s)" % (P, tuple(pixel_values.shape)))
        return pixel_values.shape[0], pixel_values.shape[2] // P, pixel_values.shape[3] // P

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def hidden_state(self, pixel_values, select_layer=-1, plan=None, out=None):
        """bf16 [B, 1 + gh*gw, hidden]: the reference's last_hidden_state (select_layer = -1) or hidden_states[select_layer].  pixel_values:
        [B, 3, gh*P, gw*P] (any float dtype; rounded to bf16), on the module's device.  With a plan (self.plan(B, gh, gw)) the call only
        enqueues: no host read, no synchronisation, one allocation (the result; none with `out`, a contiguous bf16 [B, S, hidden])."""
        c = self.config
        D, H, P, eps, dk = c.hidden_size, c.num_attention_heads, c.patch_size, c.layer_norm_eps, c.head_dim
        B, gh, gw = self._check_pixels(pixel_values)
        n_run = layers_to_run(select_layer, c.num_hidden_layers)
        if plan is None:
            plan = self._plan_for(B, gh, gw)
        if (plan.B, plan.gh, plan.gw) != (B, gh, gw):
            raise ValueError("x2i_amd InternVisionTower: the plan is for %d tiles of %d x %d patches, pixel_values holds %d of %d x %d"
                             % (plan.B, plan.gh, plan.gw, B, gh, gw))
        if plan.device != self.device or not hasattr(plan, "ws"):
            raise ValueError("x2i_amd InternVisionTower: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        if pixel_values.device != self.device:
            raise ops._lib.X2IError("x2i_amd: pixel_values must live on the model's device (got %s)" % pixel_values.device)
        if self._ls is None:
            self.pack_()
        if pixel_values.dtype != torch.bfloat16:
            pixel_values = pixel_values.to(torch.bfloat16)
        if pixel_values.stride(3) != 1:
            pixel_values = pixel_values.contiguous()
        ws, emb = plan.ws, self.embeddings
        PX, X, NRM, QKV, Q, K, VT, ATT, HH = (ws[k] for k in ("PX", "X", "NRM", "QKV", "Q", "K", "VT", "ATT", "HH"))
        L, S, Spad, M, scale = plan.L, plan.S, plan.Spad, B * plan.S, dk ** -0.5
        if out is None:
            out = torch.empty((B, S, D), device=self.device, dtype=torch.bfloat16)
        elif out.shape != (B, S, D) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("x2i_amd InternVisionTower: out must be a contiguous bf16 [%d, %d, %d] tensor on %s" % (B, S, D, self.device))
        first = out if n_run == 0 else X
        internvit_ops.patch_rows(pixel_values, PX, P, self.Kp)
        ops.gemm(PX, self._pe, emb.patch_embedding.bias, out=first, M=L, batch=B, a_batch_stride=L * self.Kp, c_offset=D, c_batch_stride=S * D)
        internvit_ops.embed(first, emb.class_embedding, plan.pos)
        for i in range(n_run):
            layer = self.encoder.layers[i]
            att, ls = layer.attn, self._ls[i]
            dst = out if i == n_run - 1 else X          # the last layer's fc2 writes the result: res = X is read, out written
            if self.rms:
                t5_ops.rms_rows(X, layer.norm1.weight, eps, out=NRM)
            else:
                ops.ln_affine(X, layer.norm1.weight, layer.norm1.bias, eps, out=NRM)
            ops.gemm(NRM, att.qkv.weight, getattr(att.qkv, "bias", None), out=QKV, M=M)
            if c.qk_normalization:
                t5_ops.rms_rows(QKV[:, :D], att.q_norm.weight, eps, out=QKV[:, :D], rows=M, ldx=3 * D, ldy=3 * D)
                t5_ops.rms_rows(QKV[:, D:2 * D], att.k_norm.weight, eps, out=QKV[:, D:2 * D], rows=M, ldx=3 * D, ldy=3 * D)
            siglip_ops.head_split(QKV, Q, K, VT, B, S, Spad, H, dk)
            vit_ops.attention(Q, K, VT, ATT, B, H, S, Spad, dk, scale, D, S * D)
            ops.gemm(ATT, att.proj.weight, att.proj.bias, out=X, M=M, gate=ls[0], res=X)
            if self.rms:
                t5_ops.rms_rows(X, layer.norm2.weight, eps, out=NRM)
            else:
                ops.ln_affine(X, layer.norm2.weight, layer.norm2.bias, eps, out=NRM)
            ops.gemm(NRM, layer.mlp.fc1.weight, layer.mlp.fc1.bias, out=HH, M=M, act=ops.ACT_GELU_ERF)
            ops.gemm(HH, layer.mlp.fc2.weight, layer.mlp.fc2.bias, out=dst, M=M, gate=ls[1], res=X)
        return out

    def forward(self, pixel_values=None, output_hidden_states=None, return_dict=None, pixel_embeds=None, select_layer=-1, plan=None, **unused):
        from transformers.modeling_outputs import BaseModelOutputWithPooling
        if pixel_values is None or pixel_embeds is not None or output_hidden_states:
            raise ValueError("x2i_amd InternVisionTower: pixel_values only; one hidden state per call (select_layer), not the tuple of all")
        last = self.hidden_state(pixel_values, select_layer=select_layer, plan=plan)
        return BaseModelOutputWithPooling(last_hidden_state=last, pooler_output=last[:, 0, :])


class InternVLVisionPlan:
    """Everything of an InternVLVision call that depends on (B, g) alone: the tower's plan, the tail's buffers, the static pixel and result
    buffers and, with graph=True, the captured graph and its stream-K workspace"""


class InternVLVision(PackedModule):
    """Stands in for the chat model's extract_feature: forward(pixel_values [B, 3, g*P, g*P]) -> bf16 [B, (g/2)^2, H_llm].
    tower: an InternVisionTower; mlp1: the chat model's `mlp1` (LayerNorm(4 hidden), Linear, GELU, Linear; copied in bf16 to the tower's
    device) or the LLM's width (an int: parameters left uninitialised, see init_random_).  The parameter names are the chat model's
    (`vision_model.*`, `mlp1.0.*`, `mlp1.1.*`, `mlp1.3.*`).

    graph=True: the plan of a shape owns a static pixel buffer and the result buffer; the first call of a shape runs eagerly on a side
    stream (the warm-up a capture needs), the second captures ONE torch.cuda.graph on a single stream with no parallel branches, with a
    stream-K workspace of its own attached to every GEMM (ops.streamk_scope), and later calls copy the pixels in and replay.  The returned
    tensor is a copy of the result buffer."""

    _eval_only = True

    def __init__(self, tower, mlp1, downsample_ratio=0.5, ps_version="v2", select_layer=-1, graph=False):
        if not isinstance(tower, InternVisionTower):
            raise TypeError("InternVLVision: tower must be an InternVisionTower")
        super().__init__(tower.device)
        if float(downsample_ratio) != 0.5:
            raise ValueError("x2i_amd InternVLVision: downsample_ratio=%r is not built (0.5 only)" % (downsample_ratio,))
        if ps_version not in ("v1", "v2"):
            raise ValueError("x2i_amd InternVLVision: ps_version=%r is not one of v1, v2" % (ps_version,))
        D = tower.config.hidden_size
        if 4 * D > 4096:
            raise ValueError("x2i_amd InternVLVision: hidden_size=%d: the shuffled rows of 4 * hidden_size are beyond the row kernel's 4096" % D)
        self.n_run = layers_to_run(int(select_layer), tower.config.num_hidden_layers)
        self.select_layer, self.ps_version, self.downsample_ratio, self.graph = int(select_layer), ps_version, 0.5, bool(graph)
        dev = tower.device
        self.vision_model = tower
        if isinstance(mlp1, nn.Module):
            src = {k: v.detach().to(device=dev, dtype=torch.bfloat16) for k, v in mlp1.state_dict().items()}
            Hl = src["3.weight"].shape[0]
            eps = getattr(getattr(mlp1, "0", None), "eps", 1e-5)
        else:
            src, Hl, eps = None, int(mlp1), 1e-5
        if Hl <= 0 or Hl % 8:
            raise ValueError("x2i_amd InternVLVision: the LLM width must be a positive multiple of 8 (got %r)" % (Hl,))
        self.llm_hidden_size, self.ln_eps = Hl, float(eps)
        param = self._param
        m = nn.Module()
        m.add_module("0", WB(param(4 * D), param(4 * D)))
        m.add_module("1", WB(param(Hl, 4 * D), param(Hl)))
        m.add_module("3", WB(param(Hl, Hl), param(Hl)))
        self.mlp1 = m
        if src is not None:
            m.load_state_dict(src, strict=True)
        self.eval()

    @property
    def device(self):
        return self.vision_model.device

    def pack_(self):
        """The tower's copies again; the plans (their graphs captured the tower's old copies) are dropped"""
        self._plans = {}
        self.vision_model.pack_()
        return self

    def init_random_(self, seed=0):
        """Random weights in place, the tower's included (tools): InternVisionTower.init_random_'s rules"""
        self.vision_model.init_random_(seed)
        self._init_random(seed + 1, lambda n, p, r: 1.0 + 0.1 * r if n == "0.weight" else (0.1 * r if p.dim() == 1 else r * p.shape[1] ** -0.5),
                          root=self.mlp1)
        self._plans = {}
        return self

    @torch.no_grad()
    def plan(self, B, g):
        """The tower's plan of B tiles on a g x g grid and the tail's buffers; g must be even (pixel_shuffle(0.5) merges 2 x 2 tokens)"""
        B, g = int(B), int(g)
        if g < 2 or g % 2:
            raise ValueError("x2i_amd InternVLVision: the grid must be even, %d x %d is not (pixel_shuffle(0.5) merges 2 x 2 tokens)" % (g, g))
        tw = self.vision_model
        c = tw.config
        p = InternVLVisionPlan()
        p.B, p.g, p.T = B, g, (g // 2) ** 2
        p.tower = tw.plan(B, g, g)
        p.device = dev = tw.device
        p.calls, p.graph, p.sk_ws = 0, None, None
        if dev.type == "cuda":
            bf = dict(device=dev, dtype=torch.bfloat16)
            P, D, Hl = c.patch_size, c.hidden_size, self.llm_hidden_size
            p.PIX = torch.zeros((B, 3, g * P, g * P), **bf)
            p.HS = torch.empty((B, 1 + g * g, D), **bf)
            p.SL = torch.empty((B * p.T, 4 * D), **bf)
            p.H1 = torch.empty((B * p.T, Hl), **bf)
            p.OUT = torch.empty((B, p.T, Hl), **bf)
        return p

    def _plan_for(self, B, g):
        p = self._plans.get((B, g))
        if p is None:
            while len(self._plans) >= 4:      # a few shapes stay resident (each with its graph): 1, 2 and 13 tiles are the usual ones
                self._plans.pop(next(iter(self._plans)))
            p = self._plans[(B, g)] = self.plan(B, g)
        return p

    def _run(self, pixels, p):
        """Every launch of a call, from `pixels` into p.OUT; only enqueues"""
        m = self.mlp1
        self.vision_model.hidden_state(pixels, select_layer=self.select_layer, plan=p.tower, out=p.HS)
        internvit_ops.shuffle_ln(p.HS, getattr(m, "0").weight, getattr(m, "0").bias, self.ln_eps, p.SL, p.g, v1=self.ps_version == "v1")
        ops.gemm(p.SL, getattr(m, "1").weight, getattr(m, "1").bias, out=p.H1, M=p.B * p.T, act=ops.ACT_GELU_ERF)
        ops.gemm(p.H1, getattr(m, "3").weight, getattr(m, "3").bias, out=p.OUT, M=p.B * p.T)

    @torch.no_grad()
    def forward(self, pixel_values, plan=None, graph=None):
        tw = self.vision_model
        B, gh, gw = tw._check_pixels(pixel_values)
        if gh != gw:
            raise ValueError("x2i_amd InternVLVision: the grid must be square, %d x %d is not (extract_feature takes h = w)" % (gh, gw))
        if plan is None:
            plan = self._plan_for(B, gh)
        if (plan.B, plan.g) != (B, gh):
            raise ValueError("x2i_amd InternVLVision: the plan is for %d tiles of %d x %d patches, pixel_values holds %d of %d x %d"
                             % (plan.B, plan.g, plan.g, B, gh, gw))
        if plan.device != self.device or not hasattr(plan, "OUT"):
            raise ValueError("x2i_amd InternVLVision: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        if pixel_values.device != self.device:
            raise ops._lib.X2IError("x2i_amd: pixel_values must live on the model's device (got %s)" % pixel_values.device)
        if not (self.graph if graph is None else graph):
            self._run(pixel_values, plan)
            return plan.OUT.clone()
        plan.PIX.copy_(pixel_values)
        if plan.graph is None and plan.calls == 0:
            # the very first call of a shape runs eagerly on a side stream (the warm-up a capture needs); the next one is the capture
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._run(plan.PIX, plan)
            torch.cuda.current_stream().wait_stream(side)
        else:
            if plan.graph is None:
                plan.sk_ws = ops.StreamKWorkspace(self.device)      # the graph owns its stream-K workspace, as the captured denoise step does
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g), ops.streamk_scope(plan.sk_ws):
                    self._run(plan.PIX, plan)
                plan.graph = g
            plan.graph.replay()
            plan.sk_ws.poll()
        plan.calls += 1
        return plan.OUT.clone()
