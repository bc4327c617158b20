"""The CLIP text encoder on the HIP path: a drop-in for `transformers`' CLIPTextModel.

The reference meets it as the first of its two prompt encoders: every sampling script's text baseline (infer/inference_*.py
get_t5_input_embeds: `clip_model(ids, output_hidden_states=False).pooler_output`, 77 tokens) and the distillation teacher's `text_encoder`
(train/train_qwenvl.py:665,778).  Its pooled output is the `pooled_projections` vector of FluxTransformer2DModel.

Launch list of one layer (every launch in libx2i_hip.so; include/x2i_clip.h, x2i_t5.h and x2i.h):
  ln_affine           layer_norm1                                   x2i_ln_affine_bf16
  gemm                stacked q|k|v projection + bias               x2i_gemm_bf16
  head_split          -> Q, K [B,H,Spad,64], V^T [B,H,64,Spad]      x2i_t5_head_split_bf16
  attention_causal    softmax_{j <= i}(dk^-1/2 q k^T) v             x2i_clip_attention_bf16
  gemm                out_proj + bias + residual (one rounding)     x2i_gemm_bf16
  ln_affine           layer_norm2
  gemm                fc1 + bias
  quick_gelu          x sigmoid(1.702 x)                            x2i_clip_quick_gelu_bf16
  gemm                fc2 + bias + residual
in front of them embed (x2i_clip_embed_bf16), behind them the final ln_affine and pool (x2i_clip_pool_bf16).

Parameter names are the library's 4.x keys (`text_model.embeddings.token_embedding.weight`, ...), the ones the reference's checkpoints
carry; load_state_dict and from_pretrained also accept the 5.x spelling of the same keys, without the `text_model.` prefix.  The q|k|v
weights and biases are views into stacked storage (as t5.T5Stack's are).
"""
import json
import os

import torch
import torch.nn as nn

from . import clip_ops, ops, t5_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
               max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)
PREFIX = "text_model."


class CLIPTextOutput(tuple):
    """What the library's BaseModelOutputWithPooling offers the callers: `.last_hidden_state` / `[0]` and `.pooler_output` / `[1]`."""

    def __new__(cls, last_hidden_state, pooler_output):
        return super().__new__(cls, (last_hidden_state, pooler_output))

    @property
    def last_hidden_state(self):
        return self[0]

    @property
    def pooler_output(self):
        return self[1]


def _canonical_keys(state_dict):
    """The module's own (4.x, `text_model.`-prefixed) names for a state dict in either spelling; the 4.x buffer `embeddings.position_ids`
    (persistent in old checkpoints, arange(max_position_embeddings) by construction) is not a parameter and is dropped."""
    out = {}
    for k, v in state_dict.items():
        k = k if k.startswith(PREFIX) else PREFIX + k
        if k == PREFIX + "embeddings.position_ids":
            continue
        if k in out:
            raise ValueError("x2i_amd CLIPTextModel: the state dict carries %r in both spellings" % k)
        out[k] = v
    return out


class CLIPTextModel(PackedModule):
    """Drop-in for transformers.CLIPTextModel as the reference calls it: `model(input_ids, output_hidden_states=False)` ->
    `.pooler_output` bf16 [B, hidden], `.last_hidden_state` bf16 [B, S, hidden]."""

    def __init__(self, config=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        f = config_fields(_FIELDS, config, kw, "CLIPTextModel")
        if f["hidden_act"] != "quick_gelu":
            raise ValueError("x2i_amd CLIPTextModel: hidden_act=%r is not built (quick_gelu only)" % (f["hidden_act"],))
        D, H, F = f["hidden_size"], f["num_attention_heads"], f["intermediate_size"]
        if H <= 0 or D % H or D // H != 64:
            raise ValueError("x2i_amd CLIPTextModel: the HIP causal attention kernel is built for 64-wide heads (hidden_size %r / %r heads)" % (D, H))
        if F % 8:
            raise ValueError("x2i_amd CLIPTextModel: intermediate_size must be a multiple of 8")
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        self.config = config_object("CLIPTextConfig", f)
        param = self._param
        view = lambda name, r0, r1: self._view(name, slice(r0, r1))
        tm = nn.Module()
        emb = nn.Module()
        emb.add_module("token_embedding", WB(param(f["vocab_size"], D)))
        emb.add_module("position_embedding", WB(param(f["max_position_embeddings"], D)))
        tm.add_module("embeddings", emb)
        layers = []
        for i in range(f["num_hidden_layers"]):
            self._store("%d.qkv.w" % i, 3 * D, D)
            self._store("%d.qkv.b" % i, 3 * D)
            att = nn.Module()
            for j, nm in enumerate("qkv"):
                att.add_module(nm + "_proj", WB(view("%d.qkv.w" % i, j * D, (j + 1) * D), view("%d.qkv.b" % i, j * D, (j + 1) * D)))
            att.add_module("out_proj", WB(param(D, D), param(D)))
            mlp = nn.Module()
            mlp.add_module("fc1", WB(param(F, D), param(F)))
            mlp.add_module("fc2", WB(param(D, F), param(D)))
            layer = nn.Module()
            layer.add_module("self_attn", att)
            layer.add_module("layer_norm1", WB(param(D), param(D)))
            layer.add_module("mlp", mlp)
            layer.add_module("layer_norm2", WB(param(D), param(D)))
            layers.append(layer)
        enc = nn.Module()
        enc.add_module("layers", nn.ModuleList(layers))
        tm.add_module("encoder", enc)
        tm.add_module("final_layer_norm", WB(param(D), param(D)))
        self.text_model = tm

    _canonical_keys = staticmethod(_canonical_keys)     # load_state_dict takes either spelling of the library's keys (with or without `text_model.`)

    def init_random_(self, seed=0):
        """Random weights in place on the device (tools and smoke runs; there are no checkpoints offline): linears N(0, 1 / fan_in), norm
        weights 1 + 0.1 N(0, 1), biases 0.1 N(0, 1), the token table N(0, 0.02^2) and the position table N(0, 0.01^2) as the library draws them."""
        def rule(n, p, r):
            if n.endswith("token_embedding.weight"):
                return 0.02 * r
            if n.endswith("position_embedding.weight"):
                return 0.01 * r
            if p.dim() == 2:
                return r * p.shape[1] ** -0.5
            if "layer_norm" in n and n.endswith(".weight"):
                return 1.0 + 0.1 * r
            return 0.1 * r

        self._init_random(seed, rule)
        return self

    def _workspace(self, B, S):
        ws = self._ws.get((B, S))
        if ws is not None:
            return ws
        c = self.config
        D, H, F = c.hidden_size, c.num_attention_heads, c.intermediate_size
        Spad = clip_ops.pad64(S)
        bf = dict(device=self.device, dtype=torch.bfloat16)
        ws = dict(Spad=Spad, X=torch.empty((B * S, D), **bf), NRM=torch.empty((B * S, D), **bf), QKV=torch.empty((B * S, 3 * D), **bf),
                  Q=torch.zeros((B, H, Spad, 64), **bf), K=torch.zeros((B, H, Spad, 64), **bf), VT=torch.zeros((B, H, 64, Spad), **bf),
                  ATT=torch.empty((B * S, D), **bf), HH=torch.empty((B * S, F), **bf))
        self._ws = {(B, S): ws}  # keep one shape resident
        return ws

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, output_hidden_states=False, **unused):
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        if output_hidden_states:
            raise ValueError("x2i_amd CLIPTextModel: output_hidden_states is not built")
        if position_ids is not None:
            raise ValueError("x2i_amd CLIPTextModel: position_ids are not built (positions are 0 .. S-1)")
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise ValueError("x2i_amd CLIPTextModel: attention masks are not built; attention_mask must be None or all ones")
        c = self.config
        D, H, F, eps = c.hidden_size, c.num_attention_heads, c.intermediate_size, c.layer_norm_eps
        input_ids = input_ids.reshape(-1, input_ids.shape[-1])
        B, S = input_ids.shape
        if S > c.max_position_embeddings:
            raise ValueError("x2i_amd CLIPTextModel: %d tokens, the position table has %d" % (S, c.max_position_embeddings))
        if input_ids.dtype != torch.int64:
            input_ids = input_ids.long()
        input_ids = input_ids.contiguous()
        tm = self.text_model
        if input_ids.device != tm.final_layer_norm.weight.device:
            raise ops._lib.X2IError("x2i_amd: input_ids must live on the model's device (got %s)" % input_ids.device)
        ws = self._workspace(B, S)
        X, NRM, QKV, Q, K, VT, ATT, HH, Spad = (ws[k] for k in ("X", "NRM", "QKV", "Q", "K", "VT", "ATT", "HH", "Spad"))
        clip_ops.embed(input_ids, tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight, out=X)
        M, scale = B * S, 64 ** -0.5
        for i, layer in enumerate(tm.encoder.layers):
            att, mlp = layer.self_attn, layer.mlp
            ops.ln_affine(X, layer.layer_norm1.weight, layer.layer_norm1.bias, eps, out=NRM)
            ops.gemm(NRM, self._fused["%d.qkv.w" % i], self._fused["%d.qkv.b" % i], out=QKV, M=M)
            t5_ops.head_split(QKV, Q, K, VT, B, S, Spad, H, 64)
            clip_ops.attention_causal(Q, K, VT, ATT, B, H, S, Spad, 64, scale, D, S * D)
            ops.gemm(ATT, att.out_proj.weight, att.out_proj.bias, out=X, res=X, M=M)
            ops.ln_affine(X, layer.layer_norm2.weight, layer.layer_norm2.bias, eps, out=NRM)
            ops.gemm(NRM, mlp.fc1.weight, mlp.fc1.bias, out=HH, M=M)
            clip_ops.quick_gelu(HH, out=HH)
            ops.gemm(HH, mlp.fc2.weight, mlp.fc2.bias, out=X, res=X, M=M)
        last = torch.empty((B, S, D), device=X.device, dtype=torch.bfloat16)
        ops.ln_affine(X, tm.final_layer_norm.weight, tm.final_layer_norm.bias, eps, out=last)
        pooled = clip_ops.pool(input_ids, last, c.eos_token_id)
        return CLIPTextOutput(last, pooled)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=torch.bfloat16, device=None):
        """config.json + model.safetensors, or model.safetensors.index.json and its shards, with the library's keys in either spelling."""
        from safetensors.torch import load_file
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, "config.json")) as fh:
            cfg = json.load(fh)
        device = device if device is not None else "cuda"
        model = cls(device=device, dtype=torch_dtype, **{k: cfg[k] for k in _FIELDS if cfg.get(k) is not None})
        index = os.path.join(d, "model.safetensors.index.json")
        if os.path.exists(index):
            with open(index) as fh:
                files = sorted(set(json.load(fh)["weight_map"].values()))
        else:
            files = ["model.safetensors"]
        sd = {}
        for fn in files:
            for k, v in load_file(os.path.join(d, fn)).items():
                sd[k] = v.to(torch_dtype) if v.is_floating_point() else v
        model.load_state_dict(sd, strict=True)
        return model
