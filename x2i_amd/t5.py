"""The T5 encoder on the HIP path: drop-ins for `transformers`' T5Stack (encoder-only) and T5EncoderModel.

The reference meets this encoder in two places: the T5Stack inside the legacy projector heads (model_internvl/proj.py:153-159,167 ->
x2i_amd.proj.Proj / Proj2 / Proj3 with hip_t5=True) and the distillation teacher's prompt encoder `text_encoder_2`
(train/train_qwenvl.py:666,778: T5EncoderModel, T5-XXL, 512 tokens, no mask).

Launch list of one layer (every launch in libx2i_hip.so; include/x2i_t5.h and x2i.h):
  rms_rows            T5LayerNorm                                   x2i_t5_rms_rows_bf16
  gemm                fused q|k|v projection, no bias               x2i_gemm_bf16
  head_split          -> Q, K [B,H,Spad,dk], V^T [B,H,dk,Spad]      x2i_t5_head_split_bf16
  attention_relbias   softmax(q k^T + bias) v, no scale             x2i_t5_attention_bf16
  gemm                o projection + residual (one rounding)        x2i_gemm_bf16
  rms_rows, gemm      T5LayerNorm, stacked [wi_0; wi_1]
  gated_gelu          gelu_new(a) * b                               x2i_t5_gated_gelu_bf16
  gemm                wo + residual
and one final rms_rows.  Parameter names are the library's, so `t5stack.*` / `encoder.*` keys of existing checkpoints load strictly; the
q|k|v and wi_0|wi_1 weights are views into stacked storage (as flux._P's are).
"""
import json
import math
import os

import torch
import torch.nn as nn

from . import ops, t5_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(d_model=512, d_kv=64, num_heads=8, d_ff=2048, num_layers=6, layer_norm_epsilon=1e-6, relative_attention_num_buckets=32,
               relative_attention_max_distance=128, feed_forward_proj="gated-gelu", dense_act_fn="gelu_new", vocab_size=32128, is_decoder=False)


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """The bidirectional bucket of T5Attention._relative_position_bucket, operation by operation in the same float32 arithmetic, so that
    bucket boundaries agree with the library bit for bit."""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, if_large)


def relative_bias_table(weight, num_buckets=32, max_distance=128, buckets=None):
    """f32 [H, 2R+1], R = max_distance: the bias of key offset r = j - i at index r + R.  The bucket function saturates at max_distance, so
    table[h][clamp(j - i, -R, R) + R] == T5Attention.compute_bias(S, S)[0, h, i, j] for every S.  weight: relative_attention_bias.weight
    [num_buckets, H]; buckets: the precomputed bucket of each offset (on weight's device), or None."""
    if buckets is None:
        R = max_distance
        buckets = relative_position_bucket(torch.arange(-R, R + 1, dtype=torch.long), num_buckets, max_distance).to(weight.device)
    return weight.detach().float()[buckets].t().contiguous()


class T5Output(tuple):
    """What the library's BaseModelOutput offers the callers: `.last_hidden_state` and `[0]`."""

    def __new__(cls, last_hidden_state):
        return super().__new__(cls, (last_hidden_state,))

    @property
    def last_hidden_state(self):
        return self[0]


class T5Stack(PackedModule):
    """Encoder-only drop-in for transformers.models.t5.modeling_t5.T5Stack (gated-GELU feed-forward, relative attention bias in block 0)."""

    def __init__(self, config=None, embed_tokens=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        f = config_fields(_FIELDS, config, kw, "T5Stack")
        if f["is_decoder"]:
            raise ValueError("x2i_amd T5Stack: only the encoder is built (is_decoder=True)")
        if f["feed_forward_proj"] not in ("gated-gelu",):
            raise ValueError("x2i_amd T5Stack: feed_forward_proj=%r is not built (gated-gelu only)" % (f["feed_forward_proj"],))
        if f["dense_act_fn"] not in ("gelu_new",):
            raise ValueError("x2i_amd T5Stack: dense_act_fn=%r is not built (gelu_new only)" % (f["dense_act_fn"],))
        if f["d_kv"] not in (32, 64, 128):
            raise ValueError("x2i_amd T5Stack: the HIP attention kernel is built for d_kv in {32, 64, 128} (got %r)" % (f["d_kv"],))
        if f["d_model"] % 8 or f["d_ff"] % 8:
            raise ValueError("x2i_amd T5Stack: d_model and d_ff must be multiples of 8")
        if not 0 < f["relative_attention_max_distance"] <= 2047 or f["relative_attention_num_buckets"] < 4:
            raise ValueError("x2i_amd T5Stack: relative_attention_max_distance must be in 1..2047 and relative_attention_num_buckets >= 4")
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        self.config = config_object("T5StackConfig", f)
        D, dk, H, F = f["d_model"], f["d_kv"], f["num_heads"], f["d_ff"]
        inner = H * dk
        param = self._param
        view = lambda name, r0, r1: WB(self._view(name, slice(r0, r1)))
        self.embed_tokens = WB(embed_tokens if embed_tokens is not None else param(f["vocab_size"], D))
        blocks = []
        for i in range(f["num_layers"]):
            self._store("%d.qkv" % i, 3 * inner, D)
            self._store("%d.wi" % i, 2 * F, D)
            att = nn.Module()
            for j, nm in enumerate("qkv"):
                att.add_module(nm, view("%d.qkv" % i, j * inner, (j + 1) * inner))
            att.add_module("o", WB(param(D, inner)))
            if i == 0:
                att.add_module("relative_attention_bias", WB(param(f["relative_attention_num_buckets"], H)))
            l0 = nn.Module()
            l0.add_module("SelfAttention", att)
            l0.add_module("layer_norm", WB(param(D)))
            ff = nn.Module()
            ff.add_module("wi_0", view("%d.wi" % i, 0, F))
            ff.add_module("wi_1", view("%d.wi" % i, F, 2 * F))
            ff.add_module("wo", WB(param(D, F)))
            l1 = nn.Module()
            l1.add_module("DenseReluDense", ff)
            l1.add_module("layer_norm", WB(param(D)))
            blk = nn.Module()
            blk.add_module("layer", nn.ModuleList([l0, l1]))
            blocks.append(blk)
        self.block = nn.ModuleList(blocks)
        self.final_layer_norm = WB(param(D))
        R = f["relative_attention_max_distance"]
        # the bucket of every key offset -R..R, evaluated once on the CPU (where the float64 references evaluate the library's expression too)
        self._buckets_cpu = relative_position_bucket(torch.arange(-R, R + 1, dtype=torch.long), f["relative_attention_num_buckets"], R)
        self._buckets = None
        self._table = None

    def _moved(self, fn):
        super()._moved(fn)
        self._table, self._buckets = None, None

    def init_random_(self, seed=0):
        """Random weights in place on the device (tools and smoke runs; there are no checkpoints offline), at the library's scales: linears
        N(0, 1 / fan_in), q a further d_kv^-1/2 (the scores carry no softmax scale), norms 1 + 0.1 N(0, 1), token table and bias N(0, 1)."""
        def rule(n, p, r):
            if p.dim() == 1:
                return 1.0 + 0.1 * r
            if n.endswith("relative_attention_bias.weight") or n.startswith("embed_tokens"):
                return r
            return r * (p.shape[1] ** -0.5 * (self.config.d_kv ** -0.5 if n.endswith("SelfAttention.q.weight") else 1.0))

        self._init_random(seed, rule)
        return self

    # ------------------------------------------------------------------ bias table and workspace
    def bias_table(self):
        """f32 [H, 2R+1] of block 0's relative_attention_bias, rebuilt when the weight changes (cache keyed on its version counter)."""
        w = self.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        key = (w._version, w.data_ptr(), str(w.device))
        if self._table is None or self._table[0] != key:
            if self._buckets is None or self._buckets.device != w.device:
                self._buckets = self._buckets_cpu.to(w.device)
            self._table = (key, relative_bias_table(w, buckets=self._buckets))
        return self._table[1]

    def _workspace(self, B, S):
        ws = self._ws.get((B, S))
        if ws is not None:
            return ws
        c = self.config
        D, dk, H, F = c.d_model, c.d_kv, c.num_heads, c.d_ff
        inner, Spad = H * dk, t5_ops.pad64(S)
        bf = dict(device=self.device, dtype=torch.bfloat16)
        ws = dict(Spad=Spad, X=torch.empty((B * S, D), **bf), NRM=torch.empty((B * S, D), **bf), QKV=torch.empty((B * S, 3 * inner), **bf),
                  Q=torch.zeros((B, H, Spad, dk), **bf), K=torch.zeros((B, H, Spad, dk), **bf), VT=torch.zeros((B, H, dk, Spad), **bf),
                  ATT=torch.empty((B * S, inner), **bf), HH=torch.empty((B * S, 2 * F), **bf), G=torch.empty((B * S, F), **bf))
        self._ws = {(B, S): ws}  # keep one shape resident
        return ws

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, input_ids=None, inputs_embeds=None, attention_mask=None, **unused):
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("T5Stack: pass exactly one of input_ids and inputs_embeds")
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise ValueError("x2i_amd T5Stack: attention masks are not built; attention_mask must be None or all ones")
        c = self.config
        D, dk, H, F, eps = c.d_model, c.d_kv, c.num_heads, c.d_ff, c.layer_norm_epsilon
        inner, R = H * dk, c.relative_attention_max_distance
        B, S = (input_ids if input_ids is not None else inputs_embeds).shape[:2]
        ws = self._workspace(B, S)
        X, NRM, QKV, Q, K, VT, ATT, HH, G, Spad = (ws[k] for k in ("X", "NRM", "QKV", "Q", "K", "VT", "ATT", "HH", "G", "Spad"))
        if input_ids is not None:
            if input_ids.device != X.device:
                raise ops._lib.X2IError("x2i_amd: input_ids must live on the model's device (got %s)" % input_ids.device)
            torch.index_select(self.embed_tokens.weight, 0, input_ids.reshape(-1), out=X)   # the token lookup is a torch gather
        else:
            ops._req(inputs_embeds, torch.bfloat16, "inputs_embeds")
            X.copy_(inputs_embeds.reshape(B * S, D))
        table = self.bias_table()
        M = B * S
        for i, blk in enumerate(self.block):
            att, ff = blk.layer[0], blk.layer[1]
            t5_ops.rms_rows(X, att.layer_norm.weight, eps, out=NRM)
            ops.gemm(NRM, self._fused["%d.qkv" % i], out=QKV, M=M)
            t5_ops.head_split(QKV, Q, K, VT, B, S, Spad, H, dk)
            t5_ops.attention_relbias(Q, K, VT, table, ATT, B, H, S, Spad, dk, R, inner, S * inner)
            ops.gemm(ATT, att.SelfAttention.o.weight, out=X, res=X, M=M)
            t5_ops.rms_rows(X, ff.layer_norm.weight, eps, out=NRM)
            ops.gemm(NRM, self._fused["%d.wi" % i], out=HH, M=M)
            t5_ops.gated_gelu(HH, out=G)
            ops.gemm(G, ff.DenseReluDense.wo.weight, out=X, res=X, M=M)
        out = torch.empty((B, S, D), device=X.device, dtype=torch.bfloat16)
        t5_ops.rms_rows(X, self.final_layer_norm.weight, eps, out=out)
        return T5Output(out)


class T5EncoderModel(nn.Module):
    """Drop-in for transformers.T5EncoderModel as the distillation teacher calls it (train/train_qwenvl.py:666,778):
    `text_encoder_2(input_ids, output_hidden_states=False)[0]` -> bf16 [B, S, d_model].  Keys: shared.weight, encoder.*"""

    def __init__(self, config=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__()
        f = config_fields(_FIELDS, config, kw, "T5Stack")
        self.shared = WB(torch.empty((f["vocab_size"], f["d_model"]), device=torch.device(device), dtype=dtype))
        self.encoder = T5Stack(config, embed_tokens=self.shared.weight, device=device, dtype=dtype, **kw)   # tied, as the library ties them
        self.config = self.encoder.config

    @property
    def dtype(self):
        return torch.bfloat16

    @property
    def device(self):
        return self.encoder.device

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, output_hidden_states=False, **unused):
        if output_hidden_states:
            raise ValueError("x2i_amd T5EncoderModel: output_hidden_states is not built")
        return self.encoder(input_ids=input_ids, inputs_embeds=inputs_embeds, attention_mask=attention_mask)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=torch.bfloat16, device=None):
        """config.json + model.safetensors, or model.safetensors.index.json and its shards, with the library's keys."""
        from safetensors.torch import load_file
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, "config.json")) as fh:
            cfg = json.load(fh)
        device = device if device is not None else "cuda"
        model = cls(device=device, dtype=torch_dtype, **{k: cfg[k] for k in _FIELDS if k in cfg})
        index = os.path.join(d, "model.safetensors.index.json")
        if os.path.exists(index):
            with open(index) as fh:
                files = sorted(set(json.load(fh)["weight_map"].values()))
        else:
            files = ["model.safetensors"]
        sd = {}
        for fn in files:
            for k, v in load_file(os.path.join(d, fn)).items():
                if k.startswith("shared.") or k.startswith("encoder."):   # a full T5 checkpoint's decoder / lm_head are not this model's
                    sd[k] = v.to(torch_dtype)
        # the token table is tied: checkpoints carry it under one name or both
        if "shared.weight" in sd:
            sd.setdefault("encoder.embed_tokens.weight", sd["shared.weight"])
        elif "encoder.embed_tokens.weight" in sd:
            sd["shared.weight"] = sd["encoder.embed_tokens.weight"]
        model.load_state_dict(sd, strict=True)
        return model
