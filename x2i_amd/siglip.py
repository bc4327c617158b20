"""The MiniCPM-o SigLIP vision tower on the HIP path: a drop-in for the NaViT SigLIP module behind `model.vpm` of MiniCPM-o 2.6
(SiglipVisionTransformer of the model's own modeling_navit_siglip.py; `transformers`' Idefics2VisionTransformer is the same module under
another name), which runs first whenever a prompt holds pixels (image2image, imagetext2image, video2image).

A call holds B images, each ONE STRIP of L patches (pixel_values [B, 3, P, P*L], patch p at columns P*p .. P*p + P-1); image b has
n_b = h_b * w_b <= L patches and the rest of its strip is padding.  Attention is bidirectional inside an image: the keys that count for
every row of image b, its padding rows included, are [0, n_b) -- a key range per row, which is all x2i_vit_attention_bf16 knows of it.

Launch list (every launch in libx2i_hip.so; include/x2i_siglip.h, x2i_vit.h and x2i.h):
  patch_rows     the strips as rows [B*L, Kp] of the patch embedding                                   x2i_siglip_patch_rows_bf16
  gemm           Conv2d(kernel = stride) as a [hidden, Kp] linear + bias                               x2i_gemm_bf16
  add_positions  + position_embedding[bucketised ids], in place                                        x2i_siglip_add_positions_bf16
  per layer, eight launches:
  ln_affine      layer_norm1                                                                           x2i_ln_affine_bf16
  gemm           q | k | v + bias
  head_split     -> Q, K [B,H,Spad,dkp'], V^T [B,H,dkp',Spad]                                          x2i_siglip_head_split_bf16
  attention      bidirectional, keys [0, n_b), scale = dk ** -0.5 of the REAL head width               x2i_vit_attention_bf16
  gemm           out_proj + bias + residual (one rounding)
  ln_affine      layer_norm2
  gemm           fc1 + bias + GELU(tanh)
  gemm           fc2 + bias + residual
  ln_affine      post_layernorm

Packed storage.  The parameters carry the library's names, so a tower's state dict loads strictly:
  * q | k | v are packed into one [3*H*dkp, hidden] weight and bias with dkp = 80 for the tower's 72-wide heads (dkp = dk for 64, 80 and
    128): rows and bias entries dk .. dkp-1 of every head are zero.  Columns dk .. dkp-1 of Q and K are then exactly 0 and the scores are
    those of the 72-wide head; the attention runs with dk = dkp and the scale of the real width; the same columns of V and so of the
    attention's output are 0 and meet zero columns of the packed out_proj [hidden, H*dkp].  These are COPIES of the q_proj / k_proj /
    v_proj / out_proj parameters (a head-padded matrix is no view of the unpadded one), made at load and again in _apply; pack_() makes
    them again after the parameters were written in place.  (dkp' above is the width x2i_vit.h stores heads at: 128 for heads of 80.)
  * fc1 is padded with zero rows (and zero bias) from the intermediate width F (4304) to Fp, the next multiple of 64 (4352), and fc2 with
    zero columns: gelu(0) = 0 meets a zero column, and fc2 stays on the GEMM's fast path (K % 64 == 0).  The parameters are views.
  * the Conv2d weight [hidden, 3, P, P] is the first 3*P*P = 588 columns of a [hidden, Kp = 640] matrix whose other columns are zero.
The padding costs 80/72 on the attention and on the q|k|v and out_proj GEMMs, about 5 % of the tower's FLOPs.
"""
import functools

import torch
import torch.nn as nn

from . import ops, siglip_ops, vit_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(hidden_size=1152, num_attention_heads=16, num_hidden_layers=27, intermediate_size=4304, image_size=980, patch_size=14,
               layer_norm_eps=1e-6, hidden_act="gelu_pytorch_tanh", num_channels=3)


def padded_head_width(dk):
    """The head width the packed weights carry: 80 for the tower's 72, the width itself for 64, 80 and 128; None for anything else"""
    return 80 if dk == 72 else (dk if dk in (64, 80, 128) else None)


# ---------------------------------------------------------------------------------------------------------------- the host work of a call
@functools.lru_cache(maxsize=None)
def bucket_position_ids(h, w, side):
    """int64 [h * w]: the position ids SiglipVisionEmbeddings.forward gives an image of h x w patches with tgt_sizes = (h, w), by the same
    torch calls on the CPU -- float32 boundaries, a float32 arange of the fractional coordinates whose step is 1 / an int32 tensor, and
    bucketize(right=True).  The float rounding decides the bucket edges, so this is no integer formula."""
    boundaries = torch.arange(1 / side, 1.0, 1 / side)
    nh, nw = torch.tensor(h, dtype=torch.int32), torch.tensor(w, dtype=torch.int32)
    fh = torch.arange(0, 1 - 1e-6, 1 / nh)
    fw = torch.arange(0, 1 - 1e-6, 1 / nw)
    if fh.numel() != h or fw.numel() != w:      # (the reference's masked assignment would fail the same way)
        raise ValueError("x2i_amd SiglipVisionTower: the fractional coordinates of a %d x %d grid have %d x %d entries" % (h, w, fh.numel(), fw.numel()))
    bh = torch.bucketize(fh, boundaries, right=True)
    bw = torch.bucketize(fw, boundaries, right=True)
    return (bh[:, None] * side + bw).flatten()


class SiglipPlan:
    """Everything of a call that depends on (tgt_sizes, L) alone (SiglipVisionTower.plan)"""


class SiglipVisionTower(PackedModule):
    """Drop-in for the SigLIP tower behind MiniCPM-o's `model.vpm`.  forward(pixel_values, patch_attention_mask, tgt_sizes) ->
    BaseModelOutputWithPooling(last_hidden_state bf16 [B, L, hidden], pooler_output None)."""

    _copies = "_packed"

    def __init__(self, config=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        f = config_fields(_FIELDS, config, kw, "SiglipVisionTower")
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        if f["hidden_act"] != "gelu_pytorch_tanh":
            raise ValueError("x2i_amd SiglipVisionTower: hidden_act=%r is not built (gelu_pytorch_tanh only)" % (f["hidden_act"],))
        D, H, F, NL, P = f["hidden_size"], f["num_attention_heads"], f["intermediate_size"], f["num_hidden_layers"], f["patch_size"]
        if H <= 0 or D % H or padded_head_width(D // H) is None:
            raise ValueError("x2i_amd SiglipVisionTower: the HIP attention kernel serves head widths 64, 72 (padded to 80), 80 and 128 "
                             "(got hidden_size=%r, num_attention_heads=%r)" % (D, H))
        if F <= 0 or NL < 1 or D % 8:
            raise ValueError("x2i_amd SiglipVisionTower: need a layer, a positive intermediate_size and hidden_size % 8 == 0")
        if f["num_channels"] != 3 or not 1 <= P <= 32 or f["image_size"] // P < 1:
            raise ValueError("x2i_amd SiglipVisionTower: need 3 channels, patch_size in 1..32 and image_size >= patch_size")
        f["head_dim"] = dk = D // H
        self.config = config_object("SiglipVisionTowerConfig", f)
        self.side = side = f["image_size"] // P         # patches per side of the position table
        self.patch_dim = Kpe = 3 * P * P
        self.dkp = padded_head_width(dk)
        self.Fp, self.Kp = Fp, Kp = siglip_ops.pad64(F), siglip_ops.pad64(Kpe)
        self._packed = None
        param, view = self._param, self._view
        cols = lambda n: (slice(None), slice(0, n))
        self._store("pe", D, Kp, zero=True)
        self.embeddings = nn.Module()
        self.embeddings.add_module("patch_embedding", WB(view("pe", cols(Kpe), (D, 3, P, P)), param(D)))
        self.embeddings.add_module("position_embedding", WB(param(side * side, D)))
        layers = []
        for i in range(NL):
            self._store("%d.fc1.w" % i, Fp, D, zero=True)
            self._store("%d.fc1.b" % i, Fp, zero=True)
            self._store("%d.fc2" % i, D, Fp, zero=True)
            att = nn.Module()
            for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                att.add_module(nm, WB(param(D, D), param(D)))
            mlp = nn.Module()
            mlp.add_module("fc1", WB(view("%d.fc1.w" % i, slice(0, F)), view("%d.fc1.b" % i, slice(0, F))))
            mlp.add_module("fc2", WB(view("%d.fc2" % i, cols(F)), param(D)))
            layer = nn.Module()
            layer.add_module("self_attn", att)
            layer.add_module("layer_norm1", WB(param(D), param(D)))
            layer.add_module("mlp", mlp)
            layer.add_module("layer_norm2", WB(param(D), param(D)))
            layers.append(layer)
        self.encoder = nn.Module()
        self.encoder.add_module("layers", nn.ModuleList(layers))
        self.post_layernorm = WB(param(D), param(D))

    @torch.no_grad()
    def pack_(self):
        """The head-padded copies of the attention projections (the module docstring), from the parameters as they are now"""
        c = self.config
        D, H, dk, dkp = c.hidden_size, c.num_attention_heads, c.head_dim, self.dkp
        packed = []
        for layer in self.encoder.layers:
            att = layer.self_attn
            w = torch.zeros((3, H, dkp, D), device=self.device, dtype=torch.bfloat16)
            b = torch.zeros((3, H, dkp), device=self.device, dtype=torch.bfloat16)
            for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
                w[j, :, :dk] = getattr(att, nm).weight.view(H, dk, D)
                b[j, :, :dk] = getattr(att, nm).bias.view(H, dk)
            o = torch.zeros((D, H, dkp), device=self.device, dtype=torch.bfloat16)
            o[:, :, :dk] = att.out_proj.weight.view(D, H, dk)
            packed.append((w.view(3 * H * dkp, D), b.view(3 * H * dkp), o.view(D, H * dkp)))
        self._packed = packed
        return self

    @classmethod
    def from_hf(cls, vpm, device=None):
        """A bf16 copy of an instantiated tower (the model's `vpm`, or an Idefics2VisionTransformer) on `device` (default: the tower's)"""
        w = vpm.post_layernorm.weight
        device = w.device if device is None else torch.device(device)
        m = cls(vpm.config, device=device)
        m.load_state_dict({k: v.detach().to(device=device, dtype=torch.bfloat16) for k, v in vpm.state_dict().items()}, strict=True)
        return m

    def init_random_(self, seed=0):
        """Random weights in place (tools; there are no checkpoints offline): matrices N(0, 1 / fan_in), the position table N(0, 0.02^2),
        biases 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1)"""
        def rule(n, p, r):
            if n.endswith("position_embedding.weight"):
                return 0.02 * r
            if "norm" in n and n.endswith(".weight"):
                return 1.0 + 0.1 * r
            return 0.1 * r if p.dim() == 1 else r * (p.numel() // p.shape[0]) ** -0.5

        self._init_random(seed, rule)
        return self.pack_()

    # ------------------------------------------------------------------ plan
    @torch.no_grad()
    def plan(self, tgt_sizes, L):
        """All the host work of a call, once per (sizes, L): the bucketised position ids (padding patches get id 0), the key ranges and the
        workspaces.  tgt_sizes: [B, 2] (h, w) per image, a tensor (ONE host read) or a list; L: patches per strip.  The result lives on the
        module's device and is valid until the module moves."""
        c = self.config
        sizes = tuple(tuple(int(v) for v in s) for s in (tgt_sizes.tolist() if isinstance(tgt_sizes, torch.Tensor) else tgt_sizes))
        L = int(L)
        if not sizes or L < 1 or any(len(s) != 2 or min(s) < 1 or s[0] * s[1] > L for s in sizes):
            raise ValueError("x2i_amd SiglipVisionTower: tgt_sizes must be rows (h, w) of positive sizes with h * w <= L = %d patches (got %r)" % (L, sizes))
        if any(max(s) > self.side for s in sizes):
            raise ValueError("x2i_amd SiglipVisionTower: an image of more than image_size // patch_size = %d patches on a side is beyond the "
                             "position table (got %r)" % (self.side, sizes))
        dev = self.device
        B, D, H = len(sizes), c.hidden_size, c.num_attention_heads
        p = SiglipPlan()
        p.sizes, p.L, p.B, p.device = sizes, L, B, dev
        p.Spad = Spad = siglip_ops.pad64(L)
        ids = torch.zeros((B, L), dtype=torch.int64)
        for b, (h, w) in enumerate(sizes):
            ids[b, :h * w] = bucket_position_ids(h, w, self.side)
        p.position_ids = ids                                   # (the library's, on the CPU)
        p.ids = ids.to(torch.int32).reshape(-1).to(dev)
        counts = torch.tensor([h * w for h, w in sizes], dtype=torch.int32)
        p.row_lo = torch.zeros((B, L), dtype=torch.int32, device=dev)
        p.row_hi = counts[:, None].expand(B, L).contiguous().to(dev)
        if dev.type == "cuda":
            bf = dict(device=dev, dtype=torch.bfloat16)
            M, dkp, dks = B * L, self.dkp, siglip_ops.stored_width(self.dkp)
            # Q, K, V^T are zeroed once: head_split writes rows / columns s < L, d < dkp only, and the attention kernel needs the rows and
            # columns < dkp of K and V^T finite up to Spad
            p.ws = dict(PX=torch.empty((M, self.Kp), **bf), X=torch.empty((M, D), **bf), NRM=torch.empty((M, D), **bf),
                        QKV=torch.empty((M, 3 * H * dkp), **bf), Q=torch.zeros((B, H, Spad, dks), **bf), K=torch.zeros((B, H, Spad, dks), **bf),
                        VT=torch.zeros((B, H, dks, Spad), **bf), ATT=torch.empty((M, H * dkp), **bf), HH=torch.empty((M, self.Fp), **bf))
        return p

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, pixel_values, patch_attention_mask=None, tgt_sizes=None, plan=None, **unused):
        """pixel_values: [B, 3, P, P*L], one strip of L patches per image (any float dtype; rounded to bf16), on the module's device.
        tgt_sizes: int [B, 2] (h, w) with h * w the image's patch count; without it the sizes are the reference's fallback, h = 1 and w = the
        number of ones in patch_attention_mask [B, 1, L] (all of L without a mask).  With tgt_sizes the mask is not read: it is the prefix of
        h * w ones per image by construction.  -> BaseModelOutputWithPooling(last_hidden_state bf16 [B, L, hidden], pooler_output None);
        rows >= h * w of an image are finite and mean nothing.  With a plan (self.plan(tgt_sizes, L)) the call only enqueues: no host read,
        no synchronisation, one allocation (the result).  Without one, the sizes are read once and the plan of the last shape is kept."""
        from transformers.modeling_outputs import BaseModelOutputWithPooling
        c = self.config
        D, H, P, eps, dk, dkp = c.hidden_size, c.num_attention_heads, c.patch_size, c.layer_norm_eps, c.head_dim, self.dkp
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or pixel_values.shape[2] != P or pixel_values.shape[3] % P or not pixel_values.shape[3]:
            raise ValueError("x2i_amd SiglipVisionTower: pixel_values must be [B, 3, P, P*L] strips with P = %d (got %s)" % (P, tuple(pixel_values.shape)))
        B, L = pixel_values.shape[0], pixel_values.shape[3] // P
        if plan is None:
            if tgt_sizes is not None:
                sizes = tuple((int(h), int(w)) for h, w in tgt_sizes.tolist())      # the one host read
            elif patch_attention_mask is not None:
                sizes = tuple((1, int(n)) for n in patch_attention_mask.reshape(B, -1).sum(-1).tolist())
            else:
                sizes = ((1, L),) * B
            plan = self._plan_for(sizes, L)
        if plan.device != self.device or not hasattr(plan, "ws"):
            raise ValueError("x2i_amd SiglipVisionTower: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        if (plan.B, plan.L) != (B, L):
            raise ValueError("x2i_amd SiglipVisionTower: the plan is for %d strips of %d patches, pixel_values holds %d of %d" % (plan.B, plan.L, B, L))
        if pixel_values.device != self.device:
            raise ops._lib.X2IError("x2i_amd: pixel_values must live on the model's device (got %s)" % pixel_values.device)
        if self._packed is None:
            self.pack_()
        if pixel_values.dtype != torch.bfloat16:
            pixel_values = pixel_values.to(torch.bfloat16)
        if pixel_values.stride(3) != 1 or pixel_values.stride(1) != P * pixel_values.stride(2):
            pixel_values = pixel_values.contiguous()
        ws, emb = plan.ws, self.embeddings
        PX, X, NRM, QKV, Q, K, VT, ATT, HH = (ws[k] for k in ("PX", "X", "NRM", "QKV", "Q", "K", "VT", "ATT", "HH"))
        M, Spad, scale = B * L, plan.Spad, dk ** -0.5
        siglip_ops.patch_rows(pixel_values, PX, P, self.Kp)
        ops.gemm(PX, self._fused["pe"], emb.patch_embedding.bias, out=X, M=M)
        siglip_ops.add_positions(X, plan.ids, emb.position_embedding.weight)
        for i, layer in enumerate(self.encoder.layers):
            qkv_w, qkv_b, out_w = self._packed[i]
            ops.ln_affine(X, layer.layer_norm1.weight, layer.layer_norm1.bias, eps, out=NRM)
            ops.gemm(NRM, qkv_w, qkv_b, out=QKV, M=M)
            siglip_ops.head_split(QKV, Q, K, VT, B, L, Spad, H, dkp)
            vit_ops.attention(Q, K, VT, ATT, B, H, L, Spad, dkp, scale, H * dkp, L * H * dkp, plan.row_lo, plan.row_hi)
            ops.gemm(ATT, out_w, layer.self_attn.out_proj.bias, out=X, res=X, M=M)
            ops.ln_affine(X, layer.layer_norm2.weight, layer.layer_norm2.bias, eps, out=NRM)
            ops.gemm(NRM, self._fused["%d.fc1.w" % i], self._fused["%d.fc1.b" % i], out=HH, M=M, act=ops.ACT_GELU_TANH)
            ops.gemm(HH, self._fused["%d.fc2" % i], layer.mlp.fc2.bias, out=X, res=X, M=M)
        last = torch.empty((B, L, D), device=self.device, dtype=torch.bfloat16)
        ops.ln_affine(X, self.post_layernorm.weight, self.post_layernorm.bias, eps, out=last)
        return BaseModelOutputWithPooling(last_hidden_state=last, pooler_output=None)
