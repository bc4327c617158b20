"""MLLM -> projector hand-off.

The reference gets its conditioning tensor by running `generate(max_new_tokens=128, output_hidden_states=True)` and then
`torch.cat/stack`-ing the per-layer tuple of the PROMPT pass into [B, C, S, H] (infer/inference_qwenvl.py:121-132,176-179;
inference_minicpm.py:116-118,174-177): 127 decode steps whose states are thrown away unless --use_answer, plus a 78-106 MB
copy per sample.  `HiddenStateSlab` produces the same tensor from ONE prefill forward: hooks on the decoder stack write every
layer's hidden state straight into a preallocated [B, C, S, H] buffer (C = n_layers + 1, the HF `hidden_states` convention:
entry i < n_layers is the INPUT of layer i, the last entry is the output of the final norm), which is the projector's input.
Plain PyTorch on purpose: the MLLM is not on the accelerated path, only the layout contract with it is.
"""
import torch
import torch.nn as nn


def find_decoder(model):
    """The text decoder stack inside an HF causal / conditional-generation model: the module owning `.layers` (ModuleList)
    and `.norm`.  Qwen2.5-VL, MiniCPM-o and InternVL all wrap a Qwen2/LLaMA-style decoder of this shape."""
    best = None
    for m in model.modules():
        layers = getattr(m, "layers", None)
        if isinstance(layers, nn.ModuleList) and hasattr(m, "norm") and hasattr(m, "embed_tokens"):
            if best is None or len(layers) > len(best.layers):
                best = m
    if best is None:
        raise RuntimeError("handoff: no decoder stack (layers + norm + embed_tokens) found in %s" % type(model).__name__)
    return best


class HiddenStateSlab:
    def __init__(self, decoder, dtype=torch.bfloat16):
        self.decoder, self.dtype = decoder, dtype
        self.n_layers = len(decoder.layers)
        self.C = self.n_layers + 1
        self.slab = None
        self._handles = []
        self._seen = 0
        self._extra = 0

    # ---- hooks
    def _store(self, idx, h):
        if self._seen >= self.C:  # a later decoder pass (a decode step of generate()): the conditioning is the PROMPT pass only
            self._extra += 1
            return
        if self.slab is None or self.slab.shape[0] != h.shape[0] or self.slab.shape[2] != h.shape[1] or self.slab.device != h.device:
            self.slab = torch.empty((h.shape[0], self.C, h.shape[1], h.shape[2]), device=h.device, dtype=self.dtype)
        self.slab[:, idx].copy_(h)
        self._seen += 1

    def attach(self):
        self.detach()
        for i, layer in enumerate(self.decoder.layers):
            def pre(mod, args, kwargs, i=i):
                h = args[0] if args else kwargs["hidden_states"]
                self._store(i, h)
            self._handles.append(layer.register_forward_pre_hook(pre, with_kwargs=True))
        self._handles.append(self.decoder.norm.register_forward_hook(lambda mod, args, out: self._store(self.n_layers, out)))
        return self

    def detach(self):
        for h in self._handles:
            h.remove()
        self._handles = []

    def __enter__(self):
        return self.attach()

    def __exit__(self, *exc):
        self.detach()

    # ---- one prefill forward -> [B, C, S, H]
    @torch.no_grad()
    def prefill(self, model, **inputs):
        return self.capture(lambda: model(**inputs, use_cache=False))

    @torch.no_grad()
    def capture(self, run):
        """Drive the MLLM with any callable -- a plain forward, or the model's own multimodal `generate(max_new_tokens=1)` /
        `chat()` wrapper that builds inputs_embeds from pixels / audio first (MiniCPM-o, InternVL) -- and keep the hidden states
        of the FIRST decoder pass, i.e. the prompt pass the reference stacks (infer/inference_minicpm.py:116-118,174-177;
        infer/inference_internvl.py:159-188).  Later passes (decode steps) are ignored, so this works with the stock HF
        remote code and does not need the reference's patched `generate()` that returns hidden states."""
        self._seen = self._extra = 0
        with self:
            run()
        if self._seen != self.C:
            raise RuntimeError("handoff: captured %d hidden states, expected %d (did the decoder stack run?)" % (self._seen, self.C))
        return self.slab


class HipPrefill:
    """HiddenStateSlab's `prefill(model, **inputs)` / `capture(run)` with the decoder stack itself on the HIP path (x2i_amd/qwen.py:
    Qwen2DecoderStack, a bf16 copy of the decoder's weights on its device; the token table is shared).  During the call the decoder
    module's `forward` is replaced ON THE INSTANCE: the surrounding model still builds `inputs_embeds` (vision / audio towers, the
    embedding merge), `attention_mask` and `position_ids` as it always does, the replacement runs the HIP stack on them -- which writes
    the [B, C, S, H] slab directly -- and hands the surrounding model the library's output object with last_hidden_state = slab[:, -1].
    The original `forward` is restored afterwards, on exceptions too.  Only the FIRST decoder pass is served (the prompt pass): the stack
    keeps no key/value cache, so a second pass -- a decode step of generate() -- raises; such callers need --full_generate."""

    def __init__(self, model, check_mask=True):
        from .qwen import Qwen2DecoderStack
        self.decoder = find_decoder(model)
        self.stack = Qwen2DecoderStack.from_hf(self.decoder)
        self.n_layers = len(self.decoder.layers)
        self.C = self.n_layers + 1
        self.check_mask = check_mask
        self.slab = None

    def _forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, use_cache=None, **kw):
        from transformers.modeling_outputs import BaseModelOutputWithPast
        if self.slab is not None:
            raise RuntimeError("handoff.HipPrefill: the decoder ran a second time (a decode step of generate()?); the HIP stack serves the "
                               "prompt pass only and keeps no key/value cache -- run with --full_generate (and without --hip_decoder) instead")
        if isinstance(attention_mask, dict):
            raise RuntimeError("handoff.HipPrefill: the decoder was handed prepared mask tensors (generate()?); it needs the 0/1 [B, S] attention_mask")
        if past_key_values is not None and past_key_values.get_seq_length() > 0:
            raise RuntimeError("handoff.HipPrefill: a non-empty key/value cache was passed; the HIP stack serves the prompt pass only (--full_generate)")
        if inputs_embeds is not None:
            inputs_embeds = inputs_embeds.to(torch.bfloat16)
        self.slab = self.stack(inputs_embeds=inputs_embeds, input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                               check_mask=self.check_mask)
        return BaseModelOutputWithPast(last_hidden_state=self.slab[:, -1], past_key_values=None)

    @torch.no_grad()
    def prefill(self, model, **inputs):
        return self.capture(lambda: model(**inputs, use_cache=False))

    @torch.no_grad()
    def capture(self, run):
        self.slab = None
        had = "forward" in self.decoder.__dict__
        saved = self.decoder.__dict__.get("forward")
        self.decoder.forward = self._forward
        try:
            run()
        finally:
            if had:
                self.decoder.forward = saved
            else:
                del self.decoder.forward
        if self.slab is None:
            raise RuntimeError("handoff: the decoder stack did not run")
        slab, self.slab = self.slab, None
        return slab


def find_visual(model):
    """The vision tower of a Qwen2.5-VL model: `model.visual` (Qwen2_5_VLModel) or `model.model.visual` (Qwen2_5_VLForConditionalGeneration)"""
    for m in (model, getattr(model, "model", None)):
        v = getattr(m, "visual", None) if m is not None else None
        if isinstance(v, nn.Module):
            return v
    raise RuntimeError("handoff: no vision tower (model.visual / model.model.visual) found in %s" % type(model).__name__)


class HipVision:
    """The vision tower behind `model.visual` on the HIP path (x2i_amd/qwen_vision.py: Qwen2_5VisionTower, a bf16 copy of the tower's weights on
    its device).  install() replaces the tower module's `forward` ON THE INSTANCE and remove() restores it; between the two the surrounding
    model's get_image_features / get_video_features and its embedding merge run as they always do and get the library's output object from
    the HIP tower.  Also a context manager.  Independent of HipPrefill: under either kind of slab, and under generate()."""

    def __init__(self, model):
        from .qwen_vision import Qwen2_5VisionTower
        self.visual = find_visual(model)
        self.tower = Qwen2_5VisionTower.from_hf(self.visual)
        self.calls = 0
        self._installed = False

    def _forward(self, hidden_states, grid_thw=None, **kw):
        self.calls += 1
        return self.tower(hidden_states, grid_thw=grid_thw)

    def install(self):
        if not self._installed:
            self._had = "forward" in self.visual.__dict__
            self._saved = self.visual.__dict__.get("forward")
            self.visual.forward = self._forward
            self._installed = True
        return self

    def remove(self):
        if self._installed:
            if self._had:
                self.visual.forward = self._saved
            else:
                del self.visual.forward
            self._installed = False

    def __enter__(self):
        return self.install()

    def __exit__(self, *exc):
        self.remove()


def prefill_hidden_states(model, dtype=torch.bfloat16, **inputs):
    """Convenience wrapper: [B, C, S, H] conditioning tensor of `inputs` from one forward of `model`."""
    return HiddenStateSlab(find_decoder(model), dtype).prefill(model, **inputs)
