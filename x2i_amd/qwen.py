"""The Qwen2 decoder prefill on the HIP path: a drop-in for the decoder stack inside every MLLM the reference conditions on -- `transformers`'
Qwen2Model (MiniCPM-o's Qwen2.5-7B, InternVL2.5's Qwen2.5-3B / Qwen2-0.5B) and Qwen2_5_VLTextModel (Qwen2.5-VL 3B / 7B) -- run ONCE over
the prompt and returning every layer's hidden state as the projector's input [B, C, S, H] (x2i_amd/handoff.py has the layout's story).

Launch list of one layer (every launch in libx2i_hip.so; include/x2i_qwen.h, x2i_t5.h and x2i.h):
  rms_rows      input_layernorm (Qwen2RMSNorm == T5LayerNorm)                 x2i_t5_rms_rows_bf16   (one launch per sample, see below)
  gemm          stacked q|k|v projection + bias                               x2i_gemm_bf16
  rope_split    rotate-half RoPE on q, k -> Q, K [B,H*,Spad,dk], V^T          x2i_qwen_rope_split_bf16
  attention     causal, grouped key/value heads, per-sample key range         x2i_qwen_attention_bf16
  gemm          o_proj + residual (one rounding)                              x2i_gemm_bf16
  rms_rows      post_attention_layernorm
  gemm          stacked [gate_proj; up_proj]
  swiglu        silu(a) * b                                                   x2i_qwen_swiglu_bf16
  gemm          down_proj + residual -> the next entry of the slab
and one final rms_rows.  The slab IS the residual stream: layer i reads slab[:, i] and its down projection writes slab[:, i + 1] through
the GEMM's residual epilogue (batch = B, M = S, the slab's batch stride); the last layer writes a scratch buffer that the final norm reads.
No stack / cat copy.  The norm kernel addresses its rows by one stride, and the samples of slab[:, i] are C*S*H apart, so the two norms that
touch the slab (input_layernorm reading it, the final norm writing it) are launched once per sample: nine launches per layer at B = 1,
8 + B otherwise.

Parameter names are the library's, so a decoder's state dict loads strictly; the q|k|v weights and biases and the gate|up weights are views
into stacked storage (as T5Stack's are).  The towers in front of the stack have HIP paths of their own (x2i_amd/qwen_vision.py, siglip.py,
resampler.py, whisper.py, internvit.py) or stay on PyTorch.  The stack takes `inputs_embeds`, or `input_ids` with an optional `merge=` plan
(x2i_amd/merge.py): the token lookup and the embedding merge of MiniCPM-o and InternVL are one launch of include/x2i_merge.h that writes
entry 0 of the slab.  (Qwen2.5-VL's masked_scatter sits inside the library's model forward and reaches the stack as inputs_embeds.)

Decoding with a key/value cache (include/x2i_qwen_decode.h; the generated answer the reference conditions on under --use_answer) is three
more methods: new_cache(B, capacity), prefill(cache, ...) -- forward's slab bit for bit, written through the cache's per-layer K / V^T with
Spad = cap -- and decode_step(cache, ...), one token per sample, eight launches per layer:
  rms_rows, decode_linear (q|k|v + bias), decode_rope_append (slot k_hi), decode_attention (keys [k_lo, k_hi + 1)), decode_linear (o_proj +
  residual), rms_rows, decode_linear (gate|up with the SwiGLU gate), decode_linear (down_proj + residual -> the next entry of the output)
The cache layout: a step appends at PHYSICAL slot k_hi[b] -- for a right-padded prompt the first padding slot -- so the valid keys stay one
contiguous run under either padding; the token's POSITION comes from the RoPE table of the cache's next position, never from the slot.
forward itself stays prefill only.  extend(cache, keep, ...) runs a chunk of n new rows against a cache that holds the keys before them (a
chat's next turn, chunked prefill): the prompt pass's launches at M = B * n with rope_split and the attention replaced by
x2i_qwen_extend_rope_split_bf16 / x2i_qwen_extend_attention_bf16 (include/x2i_qwen_extend.h), which work in cache slots from `keep` on; the
keys end at keep + n afterwards and decode_step goes on from there.  pack_w8() adds e4m3 copies of a layer's four decode weights (one f32 scale per output row) and
decode_step(..., w8=True) runs its four decode_linear launches on them (include/x2i_qwen_decode_w8.h): half the weight bytes per token; the
prompt pass keeps the bf16 weights.
"""
import torch
import torch.nn as nn

from . import merge_ops, ops, qwen_ops, t5_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, num_hidden_layers=28, rms_norm_eps=1e-6,
               vocab_size=152064, hidden_act="silu", head_dim=None, rope_theta=1000000.0, rope_type="default", mrope_section=None,
               layer_types=None, use_sliding_window=False)


def rope_tables(position_ids, dk, theta, mrope_section=None, _scratch=None):
    """f32 (cos, sin) [B, S, dk/2] in plain torch on the ids' device: the HALF tables of the library's rotary embedding (its own are these
    concatenated with themselves), evaluated as the library evaluates them in float32 -- inv_freq = 1 / theta^(2k/dk) in f32, the angle its
    f32 product with the position.  position_ids: [B, S], or [3, B, S] with mrope_section (e.g. [16, 24, 24]): chunk i of the dk/2
    frequencies takes the positions of axis i % 3, which is what apply_multimodal_rotary_pos_emb selects.
    (_scratch: a dict of preallocated buffers, the stack's; then only cos and sin are allocated.)"""
    dev = position_ids.device
    half = dk // 2
    sc = {} if _scratch is None else _scratch
    inv_freq = sc.get("inv_freq")
    if inv_freq is None:
        inv_freq = sc["inv_freq"] = (1.0 / (theta ** (torch.arange(0, dk, 2, dtype=torch.float) / dk))).to(dev)
    if position_ids.dim() == 3:
        if position_ids.shape[0] != 3 or mrope_section is None or sum(mrope_section) != half:
            raise ValueError("rope_tables: position_ids [3, B, S] need an mrope_section that sums to dk/2 = %d (got %s, %r)"
                             % (half, tuple(position_ids.shape), mrope_section))
    elif position_ids.dim() != 2:
        raise ValueError("rope_tables: position_ids must be [B, S] or [3, B, S] (got %s)" % (tuple(position_ids.shape),))
    pos = sc.get("posf")
    if pos is None or pos.shape != position_ids.shape:
        pos = sc["posf"] = torch.empty(position_ids.shape, device=dev, dtype=torch.float32)
    pos.copy_(position_ids)
    B, S = position_ids.shape[-2:]
    ang = sc.get("ang")
    if ang is None or ang.shape != (B, S, half):
        ang = sc["ang"] = torch.empty((B, S, half), device=dev, dtype=torch.float32)
    if position_ids.dim() == 2:
        torch.mul(pos[..., None], inv_freq, out=ang)
    else:
        c0 = 0
        for i, n in enumerate(mrope_section):
            torch.mul(pos[i % 3][..., None], inv_freq[c0:c0 + n], out=ang[..., c0:c0 + n])
            c0 += n
    return torch.cos(ang), torch.sin(ang)


def key_ranges(attention_mask):
    """(k_lo, k_hi) int32 [B] of a 0/1 mask [B, S] whose valid keys are one contiguous run per sample: k_lo the first valid position, k_hi =
    k_lo + their count (an all-zero row gives the empty range [0, 0)).  Torch ops on the mask's device, no synchronisation."""
    m = attention_mask != 0
    k_lo = m.to(torch.int32).argmax(-1).to(torch.int32)   # the first maximum: the first valid position (0 for an all-zero row)
    return k_lo, k_lo + m.sum(-1, dtype=torch.int32)


def mask_state(attention_mask):
    """(ok, all_ones) of a 0/1 mask [B, S] in ONE host read: ok -- every sample's valid keys are a non-empty contiguous run"""
    m = attention_mask != 0
    S = m.shape[-1]
    cnt = m.sum(-1)
    first = m.to(torch.int32).argmax(-1)
    last = S - 1 - m.flip(-1).to(torch.int32).argmax(-1)
    ok = ((cnt > 0) & (last - first + 1 == cnt)).all()
    return tuple(bool(v) for v in torch.stack((ok, (cnt == S).all())).tolist())


def _rope_fields(config):
    """rope_theta / rope_type / mrope_section of a library config: `rope_parameters` (5.x) or `rope_theta` + `rope_scaling` (4.x, remote code)"""
    rp = getattr(config, "rope_parameters", None) or getattr(config, "rope_scaling", None) or {}
    out = {}
    theta = rp.get("rope_theta", getattr(config, "rope_theta", None))
    if theta is not None:
        out["rope_theta"] = float(theta)
    out["rope_type"] = rp.get("rope_type", rp.get("type", "default")) or "default"
    if rp.get("mrope_section") is not None:
        out["mrope_section"] = list(rp["mrope_section"])
    return out


class Qwen2DecoderStack(PackedModule):
    """Prefill-only drop-in for transformers' Qwen2Model / Qwen2_5_VLTextModel (the module handoff.find_decoder finds).
    forward(...) -> the hidden-state slab bf16 [B, num_layers + 1, S, H].  Decoding with a key/value cache is new_cache / prefill /
    decode_step, below; forward itself keeps none."""

    def __init__(self, config=None, embed_tokens=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        self._xws = {}          # the extension's workspace of the resident (B, n): beside _ws, which a turn's extension must not evict
        f = config_fields(_FIELDS, config, kw, "Qwen2DecoderStack", extra=_rope_fields)
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        if f["hidden_act"] != "silu":
            raise ValueError("x2i_amd Qwen2DecoderStack: hidden_act=%r is not built (silu only)" % (f["hidden_act"],))
        if f["layer_types"] is not None and any(t != "full_attention" for t in f["layer_types"]):
            raise ValueError("x2i_amd Qwen2DecoderStack: sliding-window layers are not built (layer_types=%r)" % (f["layer_types"],))
        if f["layer_types"] is None and f["use_sliding_window"]:
            raise ValueError("x2i_amd Qwen2DecoderStack: sliding-window layers are not built (use_sliding_window=True)")
        if f["rope_type"] not in ("default", "mrope"):
            raise ValueError("x2i_amd Qwen2DecoderStack: rope type %r is not built (default and mrope only)" % (f["rope_type"],))
        D, Hq, Hkv, F = f["hidden_size"], f["num_attention_heads"], f["num_key_value_heads"], f["intermediate_size"]
        dk = f["head_dim"] or D // Hq
        if dk not in (64, 128):
            raise ValueError("x2i_amd Qwen2DecoderStack: the HIP attention kernel is built for head widths 64 and 128 (got %r)" % (dk,))
        if Hkv <= 0 or Hq % Hkv:
            raise ValueError("x2i_amd Qwen2DecoderStack: num_attention_heads must be a multiple of num_key_value_heads")
        if D % 8 or F % 8 or f["num_hidden_layers"] < 1:
            raise ValueError("x2i_amd Qwen2DecoderStack: hidden_size and intermediate_size must be multiples of 8, and there must be a layer")
        if f["mrope_section"] is not None and sum(f["mrope_section"]) != dk // 2:
            raise ValueError("x2i_amd Qwen2DecoderStack: mrope_section %r does not sum to head_dim / 2 = %d" % (f["mrope_section"], dk // 2))
        f["head_dim"] = dk
        self.config = config_object("Qwen2DecoderStackConfig", f)
        nq, nkv = Hq * dk, Hkv * dk
        param = self._param
        view = lambda name, r0, r1: self._view(name, slice(r0, r1))
        self.embed_tokens = WB(embed_tokens if embed_tokens is not None else param(f["vocab_size"], D))
        layers = []
        for i in range(f["num_hidden_layers"]):
            self._store("%d.qkv.w" % i, nq + 2 * nkv, D)
            self._store("%d.qkv.b" % i, nq + 2 * nkv)
            self._store("%d.gu" % i, 2 * F, D)
            att = nn.Module()
            for nm, r0, r1 in (("q_proj", 0, nq), ("k_proj", nq, nq + nkv), ("v_proj", nq + nkv, nq + 2 * nkv)):
                att.add_module(nm, WB(view("%d.qkv.w" % i, r0, r1), view("%d.qkv.b" % i, r0, r1)))
            att.add_module("o_proj", WB(param(D, nq)))
            mlp = nn.Module()
            mlp.add_module("gate_proj", WB(view("%d.gu" % i, 0, F)))
            mlp.add_module("up_proj", WB(view("%d.gu" % i, F, 2 * F)))
            mlp.add_module("down_proj", WB(param(D, F)))
            layer = nn.Module()
            layer.add_module("self_attn", att)
            layer.add_module("mlp", mlp)
            layer.add_module("input_layernorm", WB(param(D)))
            layer.add_module("post_attention_layernorm", WB(param(D)))
            layers.append(layer)
        self.layers = nn.ModuleList(layers)
        self.norm = WB(param(D))

    @classmethod
    def from_hf(cls, decoder, device=None):
        """A copy of an instantiated library decoder (Qwen2Model / Qwen2_5_VLTextModel) on `device` (default: the decoder's).  The token
        table is shared with the decoder, not copied, when it already is a bf16 tensor on that device."""
        w = decoder.embed_tokens.weight
        device = w.device if device is None else torch.device(device)
        share = w.dtype == torch.bfloat16 and w.device == device
        m = cls(decoder.config, embed_tokens=w.detach() if share else None, device=device)
        sd = {k: v.detach().to(device=device, dtype=torch.bfloat16) for k, v in decoder.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        return m

    def init_random_(self, seed=0):
        """Random weights in place on the device (tools and smoke runs; there are no checkpoints offline): linears N(0, 1 / fan_in), biases
        0.1 N(0, 1), norms 1 + 0.1 N(0, 1), token table N(0, 1)."""
        def rule(n, p, r):
            if n.endswith("norm.weight") or n.endswith("layernorm.weight"):
                return 1.0 + 0.1 * r
            if p.dim() == 1:
                return 0.1 * r
            return r if n.startswith("embed_tokens") else r * p.shape[1] ** -0.5

        self._init_random(seed, rule)
        return self.pack_()

    # ------------------------------------------------------------------ e4m3 weights of the decode steps
    _w8 = None      # per layer {"qkv", "o", "gu", "down"} -> (codes e4m3 [N, K], scale f32 [N]); None before pack_w8() and after the weights changed

    @torch.no_grad()
    def pack_w8(self):
        """Quantises the four decode weights of every layer -- the fused q|k|v, o_proj, the fused gate|up and down_proj -- to OCP e4m3 with
        one f32 scale per output row (ops.quantize_rows_fp8 on the device: scale = amax / 448; an all-zero row gets scale 1 and codes 0,
        so it decodes to zeros) for decode_step(w8=True), which then streams half the weight bytes per token.  Biases, norms, embed_tokens
        (and the surrounding model's lm_head) stay bf16.  The bf16 weights STAY: the prompt pass is compute-bound and runs on them, so the
        pack costs memory on top -- one byte per element of the four matrices plus 4 bytes per row, about 6.5 GB for the 7B decoder
        (28 layers of 233 M elements).  _apply, load_state_dict and init_random_ drop the pack; the next pack_w8() rebuilds it."""
        c = self.config
        if c.hidden_size % 16 or c.intermediate_size % 16:
            raise ValueError("x2i_amd Qwen2DecoderStack.pack_w8: hidden_size and intermediate_size must be multiples of 16 (a lane's 16-byte "
                             "load is 16 e4m3 weights)")
        q = ops.quantize_rows_fp8
        self._w8 = [dict(qkv=q(self._fused["%d.qkv.w" % i]), o=q(layer.self_attn.o_proj.weight), gu=q(self._fused["%d.gu" % i]),
                         down=q(layer.mlp.down_proj.weight)) for i, layer in enumerate(self.layers)]
        return self

    def _moved(self, fn):
        super()._moved(fn)
        self._w8 = None
        self._xws = {}

    def pack_(self):
        """The weights were written in place: the e4m3 pack is stale, and only pack_w8() makes it again"""
        self._w8 = None
        return self

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B, S):
        ws = self._ws.get((B, S))
        if ws is not None:
            return ws
        c = self.config
        D, dk, Hq, Hkv, F = c.hidden_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.intermediate_size
        nq, nkv, Spad = Hq * dk, Hkv * dk, qwen_ops.pad64(S)
        dev = self.device
        bf = dict(device=dev, dtype=torch.bfloat16)
        # Q, K, V^T are zeroed once: rope_split writes rows / columns < S only, and the attention kernel needs the rest finite
        ws = dict(Spad=Spad, X1=torch.empty((B * S, D), **bf), X2=torch.empty((B * S, D), **bf), NRM=torch.empty((B * S, D), **bf),
                  QKV=torch.empty((B * S, nq + 2 * nkv), **bf), Q=torch.zeros((B, Hq, Spad, dk), **bf), K=torch.zeros((B, Hkv, Spad, dk), **bf),
                  VT=torch.zeros((B, Hkv, dk, Spad), **bf), ATT=torch.empty((B * S, nq), **bf), HH=torch.empty((B * S, 2 * F), **bf),
                  G=torch.empty((B * S, F), **bf), arange=torch.arange(S, device=dev)[None].expand(B, S), rope={},
                  merge_err=torch.zeros((1,), device=dev, dtype=torch.int32))   # set by a plain input_ids pass that met an id outside the table
        self._ws = {(B, S): ws}  # keep one shape resident
        return ws

    def _extend_workspace(self, B, n):
        ws = self._xws.get((B, n))
        if ws is not None:
            return ws
        c = self.config
        D, nq, nkv, F = c.hidden_size, c.num_attention_heads * c.head_dim, c.num_key_value_heads * c.head_dim, c.intermediate_size
        bf = dict(device=self.device, dtype=torch.bfloat16)
        ws = dict(X1=torch.empty((B * n, D), **bf), X2=torch.empty((B * n, D), **bf), NRM=torch.empty((B * n, D), **bf),
                  QKV=torch.empty((B * n, nq + 2 * nkv), **bf), ATT=torch.empty((B * n, nq), **bf), HH=torch.empty((B * n, 2 * F), **bf),
                  G=torch.empty((B * n, F), **bf), rope={}, merge_err=torch.zeros((1,), device=self.device, dtype=torch.int32))
        self._xws = {(B, n): ws}  # keep one shape resident
        return ws

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, inputs_embeds=None, input_ids=None, attention_mask=None, position_ids=None, check_mask=True, use_cache=None,
                past_key_values=None, merge=None, embed_scale=1.0, **unused):
        """-> bf16 [B, C, S, H], C = num_layers + 1: entry i < L is the INPUT of layer i, the last entry the final norm's output (the HF
        `hidden_states` convention).  attention_mask: None or 0/1 [B, S] whose valid keys are one contiguous run per sample (left, right or
        two-sided padding); check_mask=True verifies that with one host read (ValueError otherwise), False skips the check (graph capture).
        position_ids: None (arange(S), as the library's forward), [B, S], or [3, B, S] / [4, B, S] for M-RoPE (of four, the first -- the text
        positions the library builds its mask from -- is dropped).  After the first call at a (B, S) a forward allocates the slab and the two
        RoPE tables and nothing else (with a mask: the two range vectors and their torch temporaries too).  Rows before a left-padded
        sample's first valid token hold finite values that the library does not define.
        input_ids are looked up by the merge kernel (include/x2i_merge.h), which writes slab[:, 0] directly; merge: a merge.MergePlan for
        the same [B, S], whose feature rows (vision, audio) the same ONE launch puts in the places the prompt reserves for them -- there
        is no inputs_embeds tensor and no copy; embed_scale: see _prompt_pass."""
        if use_cache or past_key_values is not None:
            raise ValueError("x2i_amd Qwen2DecoderStack: prefill only; use_cache=True and past_key_values are not built")
        return self._prompt_pass(None, inputs_embeds, input_ids, attention_mask, position_ids, check_mask, merge, embed_scale)

    def _prompt_pass(self, cache, inputs_embeds, input_ids, attention_mask, position_ids, check_mask, merge=None, embed_scale=1.0):
        """forward's launches; with a cache (prefill) rope_split and the attention run with Spad = cap on the cache's own per-layer K / V^T, and
        the cache's ranges and next positions are set: the same kernels on the same values, so the slab is bit-identical.
        embed_scale: what the token rows (not the feature rows) are multiplied by, one f32 multiply and one rounding (MiniCPM's scale_emb)."""
        self._one_input(inputs_embeds, input_ids, merge)
        c = self.config
        D, dk, Hq, Hkv = c.hidden_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads
        nq, C = Hq * dk, len(self.layers) + 1
        B, S = (input_ids if input_ids is not None else inputs_embeds).shape[:2]
        if cache is not None and (cache.B != B or S + 1 > cache.cap):
            raise ValueError("x2i_amd Qwen2DecoderStack.prefill: a prompt of [B, S] = [%d, %d] does not fit a cache of B = %d, cap = %d (S + 1 <= cap)"
                             % (B, S, cache.B, cache.cap))
        k_lo = k_hi = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, S):
                raise ValueError("x2i_amd Qwen2DecoderStack: attention_mask must be a 0/1 [B, S] = [%d, %d] tensor (got %s)" % (B, S, tuple(attention_mask.shape)))
            all_ones = False
            if check_mask:
                ok, all_ones = mask_state(attention_mask)
                if not ok:
                    raise ValueError("x2i_amd Qwen2DecoderStack: the valid keys of every sample must be one non-empty contiguous run of attention_mask")
            if not all_ones:
                k_lo, k_hi = key_ranges(attention_mask)
        ws = self._workspace(B, S)
        QKV, Q, K, VT, ATT, Spad = (ws[k] for k in ("QKV", "Q", "K", "VT", "ATT", "Spad"))
        dev = QKV.device
        if cache is not None:
            Q, Spad = cache.Q, cache.cap
        position_ids = ws["arange"] if position_ids is None else self._position_axes(position_ids)
        if tuple(position_ids.shape[-2:]) != (B, S):
            position_ids = position_ids.expand(*position_ids.shape[:-2], B, S)
        cos, sin = rope_tables(position_ids.to(dev), dk, c.rope_theta, c.mrope_section, _scratch=ws["rope"])
        if cache is not None:
            cache._set_prompt(S, k_lo, k_hi, attention_mask, position_ids.to(dev))
        slab = torch.empty((B, C, S, D), device=dev, dtype=torch.bfloat16)
        self._write_entry0(slab, ws, inputs_embeds, input_ids, merge, embed_scale)
        scale = dk ** -0.5
        kv = (lambda i: (cache.K[i], cache.VT[i])) if cache is not None else (lambda i: (K, VT))
        return self._layers(slab, ws, lambda i: qwen_ops.rope_split(QKV, cos, sin, Q, *kv(i), B, S, Spad, Hq, Hkv, dk),
                            lambda i: qwen_ops.attention(Q, *kv(i), ATT, B, Hq, Hkv, S, Spad, dk, scale, nq, S * nq, k_lo, k_hi))

    @staticmethod
    def _one_input(inputs_embeds, input_ids, merge=None):
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("Qwen2DecoderStack: pass exactly one of input_ids and inputs_embeds")
        if merge is not None and input_ids is None:
            raise ValueError("Qwen2DecoderStack: merge= goes with input_ids (with inputs_embeds the merge has been done)")

    def _position_axes(self, position_ids):
        """Of four position axes the first (the text positions the library builds its mask from) is dropped; three need an mrope_section"""
        if position_ids.dim() == 3 and position_ids.shape[0] == 4:
            position_ids = position_ids[1:]
        if position_ids.dim() == 3 and self.config.mrope_section is None:
            raise ValueError("x2i_amd Qwen2DecoderStack: three position axes need an mrope_section in the configuration")
        return position_ids

    def _write_entry0(self, slab, ws, inputs_embeds, input_ids, merge, embed_scale):
        """Entry 0 of the slab, for a prompt or a chunk: the token lookup and the embedding merge are ONE launch (without a plan: every row
        a table row, ws's merge_err set by an id outside the table); inputs_embeds are copied."""
        if input_ids is not None:
            if input_ids.device != slab.device:
                raise ops._lib.X2IError("x2i_amd: input_ids must live on the model's device (got %s)" % input_ids.device)
            if merge is not None:
                merge.launch(slab[:, 0], input_ids, self.embed_tokens.weight, embed_scale)
            else:
                merge_ops.embed_merge(slab[:, 0], ws["merge_err"], ids=input_ids.contiguous(), table=self.embed_tokens.weight, scale=embed_scale)
        else:
            ops._req(inputs_embeds, torch.bfloat16, "inputs_embeds")
            slab[:, 0].copy_(inputs_embeds)

    def _own(self, cache, method):
        if not isinstance(cache, Qwen2DecodeCache) or cache.owner() is not self:
            raise ValueError("x2i_amd Qwen2DecoderStack.%s: the cache must come from this stack's new_cache()" % method)

    def _layers(self, slab, ws, rope_split, attention):
        """The launches of every layer and the final norm over the rows of slab [B, C, S, D], whose entry 0 is written: the residual stream
        goes through the slab as the module's docstring has it.  rope_split(i) and attention(i) are layer i's two launches that know where
        Q, K and V^T live (a workspace, or a cache at a first slot): QKV -> Q, K, V^T and Q, K, V^T -> ATT.  ws: buffers for S rows."""
        c = self.config
        D, dk, Hq, F, eps, L = c.hidden_size, c.head_dim, c.num_attention_heads, c.intermediate_size, c.rms_norm_eps, len(self.layers)
        X1, X2, NRM, QKV, ATT, HH, G = (ws[k] for k in ("X1", "X2", "NRM", "QKV", "ATT", "HH", "G"))
        B, C, S = slab.shape[:3]
        nq, M, sbs, SD = Hq * dk, B * S, C * S * D, S * D
        for i, layer in enumerate(self.layers):
            for b in range(B):   # (the samples of slab[:, i] are C*S*D apart; the norm's rows have one stride)
                t5_ops.rms_rows(slab[b, i], layer.input_layernorm.weight, eps, out=NRM[b * S:(b + 1) * S])
            ops.gemm(NRM, self._fused["%d.qkv.w" % i], self._fused["%d.qkv.b" % i], out=QKV, M=M)
            rope_split(i)
            attention(i)
            ops.gemm(ATT, layer.self_attn.o_proj.weight, out=X1, M=S, batch=B, a_batch_stride=S * nq, c_batch_stride=SD, ldc=D,
                     res=slab, res_offset=i * SD, res_batch_stride=sbs, ldr=D)
            t5_ops.rms_rows(X1, layer.post_attention_layernorm.weight, eps, out=NRM)
            ops.gemm(NRM, self._fused["%d.gu" % i], out=HH, M=M)
            qwen_ops.swiglu(HH, out=G)
            if i + 1 < L:
                ops.gemm(G, layer.mlp.down_proj.weight, out=slab, M=S, batch=B, a_batch_stride=S * F, c_offset=(i + 1) * SD, c_batch_stride=sbs,
                         ldc=D, res=X1, res_batch_stride=SD, ldr=D)
            else:
                ops.gemm(G, layer.mlp.down_proj.weight, out=X2, M=M, res=X1, ldr=D)
        for b in range(B):
            t5_ops.rms_rows(X2[b * S:(b + 1) * S], self.norm.weight, eps, out=slab[b, L])
        return slab

    # ------------------------------------------------------------------ decoding with a key/value cache
    def new_cache(self, B, capacity):
        """A Qwen2DecodeCache for B samples and at least `capacity` keys per sample (prompt + generated tokens), rounded up to 64."""
        return Qwen2DecodeCache(self, B, capacity)

    @torch.no_grad()
    def prefill(self, cache, inputs_embeds=None, input_ids=None, attention_mask=None, position_ids=None, check_mask=True, merge=None, embed_scale=1.0, **unused):
        """forward's arguments and forward's slab [B, C, S, H], bit for bit: the same launches, but rope_split and the attention run with
        Spad = cap on the cache's own per-layer K / V^T.  Sets the cache's key ranges (from the mask) and every sample's next position: one
        more than the largest position id of its valid tokens over all axes -- for plain Qwen2 the count of valid tokens, for Qwen2.5-VL what
        the library's rope_deltas yields.  Refuses S + 1 > cap."""
        self._own(cache, "prefill")
        return self._prompt_pass(cache, inputs_embeds, input_ids, attention_mask, position_ids, check_mask, merge, embed_scale)

    @torch.no_grad()
    def extend(self, cache, keep, inputs_embeds=None, input_ids=None, position_ids=None, check=True, merge=None, embed_scale=1.0):
        """A chunk of n new rows against a cache that holds the keys before them (a chat's next turn; chunked prefill) -> bf16 [B, C, n, H],
        the hidden states of the new rows only, HF convention as forward.
        keep: a host int, a SLOT index, the same for every sample: slots [0, keep) of the cache are kept, the chunk goes to slots keep ..
        keep + n - 1, and what the cache held from keep on (decode passes past an end token, a longer old prompt) is dropped by setting
        k_hi = keep + n on the device; k_lo stays.  Needs a prefilled cache, keep >= 1, n >= 1 and keep + n + 1 <= cap (prefill's rule).
        check=True makes one host read of k_lo, k_hi and raises ValueError when a sample's k_hi < keep (a hole) or k_lo >= keep; False
        skips it.  position_ids: those of the chunk, [B, n], or [3, B, n] / [4, B, n] for M-RoPE -- required, because the position is not
        the slot.  Afterwards cache.pos is 1 + the largest position id of the chunk over all axes and cache.steps = keep + n; a
        decode_step goes on from there, eager or replayed from a graph captured on this cache (it reads k_hi and pos from the device).
        Per layer: the prompt pass's launches at M = B * n with x2i_qwen_extend_rope_split_bf16 / x2i_qwen_extend_attention_bf16
        (include/x2i_qwen_extend.h) on cache.Q / K[i] / VT[i]; inputs_embeds, input_ids, merge and embed_scale as forward's, for the
        chunk."""
        from . import qwen_extend_ops as qx
        self._own(cache, "extend")
        if cache.steps is None:
            raise ValueError("x2i_amd Qwen2DecoderStack.extend: prefill(cache, ...) comes first")
        self._one_input(inputs_embeds, input_ids, merge)
        if position_ids is None:
            raise ValueError("x2i_amd Qwen2DecoderStack.extend: position_ids of the chunk are required (the position is not the slot)")
        keep = int(keep)
        if keep < 1:
            raise ValueError("x2i_amd Qwen2DecoderStack.extend: keep = %d keeps nothing; a whole prompt is prefill's" % keep)
        c = self.config
        D, dk, Hq, Hkv, L = c.hidden_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads, len(self.layers)
        B, n = (input_ids if input_ids is not None else inputs_embeds).shape[:2]
        if cache.B != B or n < 1 or keep + n + 1 > cache.cap:
            raise ValueError("x2i_amd Qwen2DecoderStack.extend: a chunk of [B, n] = [%d, %d] at slot keep = %d does not fit a cache of B = %d, "
                             "cap = %d (n >= 1, keep + n + 1 <= cap)" % (B, n, keep, cache.B, cache.cap))
        position_ids = self._position_axes(position_ids)
        if position_ids.dim() not in (2, 3) or tuple(position_ids.shape[-2:]) != (B, n):
            raise ValueError("x2i_amd Qwen2DecoderStack.extend: position_ids must be [B, n] = [%d, %d], or [3, B, n] / [4, B, n] (got %s)"
                             % (B, n, tuple(position_ids.shape)))
        if check:
            lo, hi = torch.stack((cache.k_lo, cache.k_hi)).tolist()
            if min(hi) < keep:
                raise ValueError("x2i_amd Qwen2DecoderStack.extend: keep = %d leaves a hole: a sample's keys end at slot %d" % (keep, min(hi)))
            if max(lo) >= keep:
                raise ValueError("x2i_amd Qwen2DecoderStack.extend: keep = %d keeps no key of a sample whose keys start at slot %d" % (keep, max(lo)))
        ws = self._extend_workspace(B, n)
        dev = ws["X1"].device
        position_ids = position_ids.to(dev)
        cos, sin = rope_tables(position_ids, dk, c.rope_theta, c.mrope_section, _scratch=ws["rope"])
        cache._set_extension(keep, n, position_ids)
        slab = torch.empty((B, L + 1, n, D), device=dev, dtype=torch.bfloat16)
        self._write_entry0(slab, ws, inputs_embeds, input_ids, merge, embed_scale)
        QKV, ATT, nq, cap, scale = ws["QKV"], ws["ATT"], Hq * dk, cache.cap, dk ** -0.5
        return self._layers(slab, ws, lambda i: qx.rope_split(QKV, cos, sin, cache.Q, cache.K[i], cache.VT[i], B, keep, n, cap, Hq, Hkv, dk),
                            lambda i: qx.attention(cache.Q, cache.K[i], cache.VT[i], ATT, B, Hq, Hkv, keep, n, cap, dk, scale, nq, n * nq, cache.k_lo))

    @torch.no_grad()
    def decode_step(self, cache, inputs_embeds=None, input_ids=None, out=None, w8=False):
        """One token per sample against the cache: inputs_embeds bf16 [B, 1, H] (or [B, H]) or input_ids [B, 1] (or [B]) -> the hidden states
        bf16 [B, C, 1, H] of that token (HF convention, as forward).  out: a [B, C, H] view to write instead, e.g. column t of a caller's
        [B, C, T, H] answer slab, slab[:, :, t] (last stride 1, H-rows 16-byte aligned); it IS the residual stream, no copy.
        The new key and value go to physical slot k_hi[b] (under right padding that overwrites the first padding slot), so the valid keys stay
        the one run [k_lo, k_hi) under either padding; the position comes from the RoPE table of the cache's next position, not from the slot.
        k_hi and the position then advance ON THE DEVICE: no host read, and after the first step no allocation but the output, so a step can
        be captured in a graph and replayed (a replay does not pass through here: its caller counts the steps, cache.steps).  Launches per
        layer: rms, qkv linear, rope_append, attention, o_proj linear + residual, rms, gate|up linear with the gate, down linear + residual.
        w8=True: the four linears of each layer read the e4m3 weights of pack_w8() (qwen_decode_w8_ops.linear_w8); everything else is
        unchanged.  Without a pack it raises ValueError."""
        from . import qwen_decode_ops as qd
        if w8 and self._w8 is None:
            raise ValueError("x2i_amd Qwen2DecoderStack.decode_step: w8=True needs the e4m3 weights; call pack_w8() first (and again after the "
                             "weights were loaded, moved or re-initialised)")
        self._one_input(inputs_embeds, input_ids)
        self._own(cache, "decode_step")
        if cache.steps is None:
            raise ValueError("x2i_amd Qwen2DecoderStack.decode_step: prefill(cache, ...) comes first")
        if cache.steps + 1 > cache.cap:
            raise ValueError("x2i_amd Qwen2DecoderStack.decode_step: the cache is full (cap = %d keys)" % cache.cap)
        c = self.config
        D, dk, Hq, Hkv, F, eps, L = c.hidden_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.intermediate_size, c.rms_norm_eps, len(self.layers)
        B, cap, C = cache.B, cache.cap, L + 1
        if out is None:
            out4 = torch.empty((B, C, 1, D), device=cache.K.device, dtype=torch.bfloat16)
            out = out4[:, :, 0]
        else:
            ops._req(out, torch.bfloat16, "out")
            if tuple(out.shape) != (B, C, D) or out.stride(2) != 1 or out.stride(1) % 8 or out.stride(0) % 8 or out.data_ptr() % 16:
                raise ValueError("x2i_amd Qwen2DecoderStack.decode_step: out must be a bf16 [B, C, H] = [%d, %d, %d] view with 16-byte aligned rows"
                                 % (B, C, D))
            out4 = out.unsqueeze(2)
        if input_ids is not None:
            if input_ids.device != out.device:
                raise ops._lib.X2IError("x2i_amd: input_ids must live on the model's device (got %s)" % input_ids.device)
            torch.index_select(self.embed_tokens.weight, 0, input_ids.reshape(B), out=cache.X0)
        else:
            ops._req(inputs_embeds, torch.bfloat16, "inputs_embeds")
            cache.X0.copy_(inputs_embeds.reshape(B, D))
        out[:, 0].copy_(cache.X0)
        cos, sin = cache._step_tables()             # from the next position, which then advances; slot = k_hi, k_hi += 1
        X1, X2, NRM, QKV, Qd, ATT, G, ws, slot, k_lo, k_hi = (cache.X1, cache.X2, cache.NRM, cache.QKV, cache.Qd, cache.ATT, cache.G, cache.ws,
                                                              cache.slot, cache.k_lo, cache.k_hi)
        sb, sc, scale = out.stride(0), out.stride(1), dk ** -0.5
        if w8:
            from .qwen_decode_w8_ops import linear_w8
            lin = lambda i, nm, X, W, bias=None, **kw: linear_w8(X, self._w8[i][nm][0], self._w8[i][nm][1], bias, **kw)
        else:
            lin = lambda i, nm, X, W, bias=None, **kw: qd.linear(X, W, bias, **kw)
        for i, layer in enumerate(self.layers):
            t5_ops.rms_rows(out[:, i], layer.input_layernorm.weight, eps, out=NRM, rows=B, ldx=sb)
            lin(i, "qkv", NRM, self._fused["%d.qkv.w" % i], self._fused["%d.qkv.b" % i], out=QKV)
            qd.rope_append(QKV, cos, sin, slot, Qd, cache.K[i], cache.VT[i], B, Hq, Hkv, cap, dk)
            qd.attention(Qd, cache.K[i], cache.VT[i], k_lo, k_hi, ATT, ws, B, Hq, Hkv, cap, dk, scale)
            lin(i, "o", ATT, layer.self_attn.o_proj.weight, res=out, res_offset=i * sc, ldr=sb, out=X1)
            t5_ops.rms_rows(X1, layer.post_attention_layernorm.weight, eps, out=NRM)
            lin(i, "gu", NRM, self._fused["%d.gu" % i], gate=True, out=G)
            if i + 1 < L:
                lin(i, "down", G, layer.mlp.down_proj.weight, res=X1, out=out, y_offset=(i + 1) * sc, ldy=sb, B=B, N=D)
            else:
                lin(i, "down", G, layer.mlp.down_proj.weight, res=X1, out=X2)
        t5_ops.rms_rows(X2, self.norm.weight, eps, out=out[:, L], rows=B, ldy=sb)
        cache.steps += 1
        return out4


class Qwen2DecodeCache:
    """The keys and values of one generation, and everything a decode step needs so that it allocates nothing (Qwen2DecoderStack.new_cache):
      K  bf16 [L, B, Hkv, cap, dk], VT bf16 [L, B, Hkv, dk, cap]   zeroed once: the kernels need them finite, not empty
      k_lo, k_hi int32 [B]    the valid keys of each sample, one contiguous run; a step appends at slot k_hi and advances it
      pos int64 [B], or [3, B] with an mrope_section    the next position of each sample (the RoPE table's argument, not a slot)
      steps    host-side count of an upper bound of k_hi (None before a prefill); a caller that replays a captured step adds to it itself;
               an extension sets it to keep + n
    and the step's scratch rows, the prefill's Q [B, Hq, cap, dk] and the attention's split workspace."""

    def __init__(self, stack, B, capacity):
        import weakref
        from . import qwen_decode_ops as qd
        c = stack.config
        D, dk, Hq, Hkv, F, L = c.hidden_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.intermediate_size, len(stack.layers)
        if B < 1 or capacity < 1:
            raise ValueError("x2i_amd Qwen2DecodeCache: B and capacity must be positive (got %r, %r)" % (B, capacity))
        if B > 8:
            raise ValueError("x2i_amd Qwen2DecodeCache: the decode kernels take 1..8 samples (got B = %d)" % B)
        if Hq // Hkv > 16:
            raise ValueError("x2i_amd Qwen2DecodeCache: a group of %d query heads per key/value head is above 16" % (Hq // Hkv))
        self.owner = weakref.ref(stack)
        self.B, self.cap = B, qwen_ops.pad64(capacity)
        cap, dev = self.cap, stack.device
        bf = dict(device=dev, dtype=torch.bfloat16)
        self.K = torch.zeros((L, B, Hkv, cap, dk), **bf)
        self.VT = torch.zeros((L, B, Hkv, dk, cap), **bf)
        self.Q = torch.zeros((B, Hq, cap, dk), **bf)
        self.k_lo = torch.zeros((B,), device=dev, dtype=torch.int32)
        self.k_hi = torch.zeros((B,), device=dev, dtype=torch.int32)
        self.slot = torch.zeros((B,), device=dev, dtype=torch.int32)
        self.mrope = c.mrope_section is not None
        self.pos = torch.zeros((3, B) if self.mrope else (B,), device=dev, dtype=torch.int64)
        self.steps = None
        nq, nkv = Hq * dk, Hkv * dk
        self.X0, self.X1, self.X2, self.NRM = (torch.empty((B, D), **bf) for _ in range(4))
        self.QKV = torch.empty((B, nq + 2 * nkv), **bf)
        self.Qd = torch.empty((B, Hq, dk), **bf)
        self.ATT = torch.empty((B, nq), **bf)
        self.G = torch.empty((B, F), **bf)
        self.ws = torch.empty((qd.workspace_floats(B, Hq, cap, dk),), device=dev, dtype=torch.float32)
        f32 = dict(device=dev, dtype=torch.float32)
        self._inv_freq = (1.0 / (c.rope_theta ** (torch.arange(0, dk, 2, dtype=torch.float) / dk))).to(dev)    # rope_tables' own
        self._section = c.mrope_section
        self._posf = torch.empty(self.pos.shape, **f32)
        self._ang, self._cos, self._sin = (torch.empty((B, dk // 2), **f32) for _ in range(3))

    def _set_prompt(self, S, k_lo, k_hi, attention_mask, position_ids):
        """After a prompt of S tokens: ranges from the mask ([0, S) without one), next position = 1 + the largest position id of the valid tokens"""
        if k_lo is None:
            if attention_mask is None:
                self.k_lo.zero_()
                self.k_hi.fill_(S)
            else:
                k_lo, k_hi = key_ranges(attention_mask)
        if k_lo is not None:
            self.k_lo.copy_(k_lo)
            self.k_hi.copy_(k_hi)
        self._set_next_position(position_ids, attention_mask)
        self.steps = S

    def _set_next_position(self, position_ids, attention_mask=None):
        """pos = 1 + the largest position id over all axes (of the valid tokens, with a mask).  On the device, no host read."""
        pos = position_ids if position_ids.dim() == 3 else position_ids[None]
        if attention_mask is not None:
            pos = pos.masked_fill((attention_mask == 0).to(pos.device)[None], -1)
        self.pos.copy_((pos.amax(-1).amax(0) + 1).expand_as(self.pos) if self.mrope else pos.amax(-1)[0] + 1)

    def _adopt(self, other, P):
        """Slots [0, P) of another cache of the same stack and batch size (a conversation that outgrew it): K / V^T of every layer and k_lo
        copied over with torch ops; the keys end at P until an extension follows."""
        self.K[:, :, :, :P].copy_(other.K[:, :, :, :P])
        self.VT[..., :P].copy_(other.VT[..., :P])
        self.k_lo.copy_(other.k_lo)
        self.k_hi.fill_(P)
        self.steps = P

    def _set_extension(self, keep, n, position_ids):
        """After a chunk of n rows at slots keep .. keep + n - 1 (Qwen2DecoderStack.extend): the keys end at keep + n, whatever lay behind is
        dropped, k_lo stays; next position = 1 + the largest position id of the chunk over all axes.  On the device, no host read."""
        self.k_hi.fill_(keep + n)
        self._set_next_position(position_ids)
        self.steps = keep + n

    def _step_tables(self):
        """(cos, sin) f32 [B, dk/2] of the next positions, rope_tables' arithmetic into buffers of the cache; then slot = k_hi, k_hi += 1,
        pos += 1, all on the device."""
        self._posf.copy_(self.pos)
        if not self.mrope:
            torch.mul(self._posf[:, None], self._inv_freq, out=self._ang)
        else:
            c0 = 0
            for i, n in enumerate(self._section):
                torch.mul(self._posf[i % 3][:, None], self._inv_freq[c0:c0 + n], out=self._ang[:, c0:c0 + n])
                c0 += n
        torch.cos(self._ang, out=self._cos)
        torch.sin(self._ang, out=self._sin)
        self.slot.copy_(self.k_hi)
        self.k_hi.add_(1)
        self.pos.add_(1)
        return self._cos, self._sin
