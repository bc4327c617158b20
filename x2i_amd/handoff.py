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


class _Patch:
    """Attribute `name` of obj replaced ON THE INSTANCE by a callable: install() (idempotent, returns self) sets it and remove() (idempotent)
    puts back what the instance's own __dict__ held, or deletes the attribute where it held none, so that the class's attribute shows
    again.  `_original` is what getattr gave at install (the bound method the replacement may fall back to).  Also a context manager,
    which restores on exceptions too.  The hand-offs below derive from it."""
    _installed = False

    def __init__(self, obj, name, replacement):
        self._patched = (obj, name, replacement)

    def install(self):
        if not self._installed:
            obj, name, replacement = self._patched
            self._had, self._saved, self._original = name in obj.__dict__, obj.__dict__.get(name), getattr(obj, name, None)
            setattr(obj, name, replacement)
            self._installed = True
        return self

    def remove(self):
        if self._installed:
            obj, name, _ = self._patched
            if self._had:
                setattr(obj, name, self._saved)
            else:
                delattr(obj, name)
            self._installed = False

    def __enter__(self):
        return self.install()

    def __exit__(self, *exc):
        self.remove()


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
        with _Patch(self.decoder, "forward", self._forward):
            run()
        if self.slab is None:
            raise RuntimeError("handoff: the decoder stack did not run")
        slab, self.slab = self.slab, None
        return slab


def head_plan(processors):
    """What HipGenerate(hip_head=True) makes of a list of `transformers` logits processors: -> the repetition penalty that the head kernel
    applies (1.0: none).  Needs no GPU.  Accepted, in any order: RepetitionPenaltyLogitsProcessor without prompt_ignore_length (at most one;
    its penalty is taken), and TemperatureLogitsWarper (temperature > 0), TopKLogitsWarper, TopPLogitsWarper -- monotone maps that keep the top
    element, so they cannot move an argmax and are dropped (what Qwen2.5-VL's generation_config brings).  Anything else, a subclass included,
    raises ValueError naming the class: there is no silent fallback to the torch processors."""
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    penalty = None
    for p in processors or []:
        name = type(p).__name__
        if type(p) is RepetitionPenaltyLogitsProcessor:
            if p.prompt_ignore_length:
                raise ValueError("handoff.HipGenerate: hip_head cannot fuse %s with prompt_ignore_length=%r (the kernel penalises every id of "
                                 "the sequence); run without --hip_head" % (name, p.prompt_ignore_length))
            if penalty is not None:
                raise ValueError("handoff.HipGenerate: hip_head fuses one %s, and the list holds two; run without --hip_head" % name)
            penalty = float(p.penalty)
        elif type(p) is TemperatureLogitsWarper:
            if not p.temperature > 0:
                raise ValueError("handoff.HipGenerate: hip_head cannot drop %s with temperature=%r (not a monotone map); run without "
                                 "--hip_head" % (name, p.temperature))
        elif type(p) in (TopKLogitsWarper, TopPLogitsWarper):
            pass
        else:
            raise ValueError("handoff.HipGenerate: hip_head cannot fuse the logits processor %s (it fuses RepetitionPenaltyLogitsProcessor and "
                             "drops TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper); run without --hip_head" % name)
    return 1.0 if penalty is None else penalty


def sample_plan(generation_config, processors):
    """What HipGenerate(hip_head=True, sample=True) makes of a generation_config and a list of `transformers` logits processors: -> (penalty,
    temperature, top_k, top_p), what the head launch and x2i_sample_select_f32 (include/ext/sample/x2i_sample.h) apply; 1.0, 1.0, 0 and 1.0
    where the list has no such processor.  Needs no GPU.  Accepted: what head_plan accepts, at most one of each and in the library's order
    only (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper: the order the kernels apply them
    in), TopPLogitsWarper with min_tokens_to_keep = 1, both filters with the value -inf.  A generation_config that does not sample
    (do_sample false) gives top_k = 1, the argmax.  Refused with a ValueError naming the class, before anything runs: any other processor
    (MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper, ...), a subclass included; num_beams > 1."""
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    beams = getattr(generation_config, "num_beams", 1) or 1
    if beams > 1:
        raise ValueError("handoff.HipGenerate: sample draws one token per sample, and this generation_config asks for num_beams=%r; run with "
                         "--full_generate instead" % (beams,))
    order = (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper)
    penalty, temperature, top_k, top_p, rank = 1.0, 1.0, 0, 1.0, -1
    for p in processors or []:
        name = type(p).__name__
        if type(p) not in order:
            raise ValueError("handoff.HipGenerate: sample cannot fuse the logits processor %s (it fuses %s); run with --full_generate instead"
                             % (name, ", ".join(c.__name__ for c in order)))
        if order.index(type(p)) <= rank:
            raise ValueError("handoff.HipGenerate: sample fuses at most one of each processor, in the library's order (%s), and %s comes after "
                             "%s; run with --full_generate instead" % (", ".join(c.__name__ for c in order), name, order[rank].__name__))
        rank = order.index(type(p))
        if getattr(p, "filter_value", -float("inf")) != -float("inf"):
            raise ValueError("handoff.HipGenerate: sample removes a filtered token, and %s has filter_value=%r; run with --full_generate instead"
                             % (name, p.filter_value))
        if type(p) is RepetitionPenaltyLogitsProcessor:
            if p.prompt_ignore_length:
                raise ValueError("handoff.HipGenerate: hip_head cannot fuse %s with prompt_ignore_length=%r (the kernel penalises every id of "
                                 "the sequence); run with --full_generate instead" % (name, p.prompt_ignore_length))
            penalty = float(p.penalty)
        elif type(p) is TemperatureLogitsWarper:
            temperature = float(p.temperature)
            if not (temperature > 0 and temperature < float("inf")):
                raise ValueError("handoff.HipGenerate: sample needs a positive finite temperature, and %s has %r" % (name, p.temperature))
        else:
            if getattr(p, "min_tokens_to_keep", 1) != 1:
                raise ValueError("handoff.HipGenerate: sample keeps at least one token, and %s has min_tokens_to_keep=%r; run with "
                                 "--full_generate instead" % (name, p.min_tokens_to_keep))
            if type(p) is TopKLogitsWarper:
                top_k = int(p.top_k)
            else:
                top_p = float(p.top_p)
                if not 0 < top_p <= 1:
                    raise ValueError("handoff.HipGenerate: sample needs 0 < top_p <= 1, and %s has %r" % (name, p.top_p))
    if generation_config is not None and not getattr(generation_config, "do_sample", False):
        top_k = 1
    return penalty, temperature, top_k, top_p


def _common_prefix(prev_ids, prev_valid, ids):
    """common_prefix as a 0-dim int64 tensor on the ids' device: no host read"""
    m = min(int(prev_valid), prev_ids.shape[1], ids.shape[1])
    if prev_ids.shape[0] != ids.shape[0] or m < 1:
        return torch.zeros((), device=ids.device, dtype=torch.long)
    same = (prev_ids[:, :m].to(ids.device) == ids[:, :m]).all(0)
    return same.long().cumprod(0).sum()


def common_prefix(prev_ids, prev_valid, ids):
    """-> P, a host int: the longest common prefix of the token ids prev_ids [B, >= prev_valid] and ids [B, S] over ALL samples (the first
    column where any sample differs ends it), capped at prev_valid, the count of kept tokens that are valid, and at S.  Pure torch, works on
    CPU tensors, one host read.  Another batch size gives 0."""
    return int(_common_prefix(prev_ids, prev_valid, ids))


class GenerateResult:
    """What HipGenerate.generate returns: prompt bf16 [B, C, S, H] (the prompt pass, HipPrefill's slab), answer bf16 [B, C, T - 1, H] (the
    decode passes: column t is the pass whose input is generated token t; the pass of the last token never runs, the HF convention),
    sequences int64 [B, S + T] (the prompt's ids, then the T generated tokens; the pad token after a sample's end token) and lengths int64
    [B] (a sample's generated tokens up to and including its end token)."""

    def __init__(self, prompt, answer, sequences, lengths):
        self.prompt, self.answer, self.sequences, self.lengths = prompt, answer, sequences, lengths


class HipGenerate:
    """Greedy `generate(output_hidden_states=True)` with the decoder stack on the HIP path over the prompt AND over the generated tokens
    (x2i_amd/qwen.py: Qwen2DecoderStack.prefill / decode_step on a key/value cache): what the reference conditions on under --use_answer
    (infer/inference_qwenvl.py:125-129,176).  The prompt pass goes through the surrounding model exactly as HipPrefill's does -- `forward`
    replaced on the instance and restored afterwards, on exceptions too -- so the model still builds inputs_embeds, mask and position ids
    and applies its own lm_head.  Every later step is: a gather from embed_tokens, decode_step, model.get_output_embeddings(), the
    optional `transformers` logits processors (torch), argmax.  With graph=True the gather, the step and the lm_head are captured ONCE in a
    torch.cuda.graph (one stream, no parallel branches) and replayed; the processors and the argmax follow each replay as torch ops.
    Finished samples are tracked on the device and the host looks once every `check_every` steps.  The cache and the graph captured on it
    stay resident between calls and serve every later call of the same batch size and rounded capacity (prompt + new tokens).
    With hip_head=True (off by default; per call generate(hip_head=...)) the step's tail is on the HIP path too (x2i_amd/qwen_head_ops.py):
    the lm_head, the repetition penalty and a per-workgroup argmax in one launch, the choice of the token with the end-token bookkeeping in
    a second, both inside the captured step, so a generated token is one graph replay and no torch op; token 0 goes through the same two
    kernels on each sample's last valid prompt row.  head_plan decides which processor lists fuse; any other raises.  A token is then the
    argmax of f32-accumulated logits that were never rounded to bf16: where the top two logits lie within one bf16 ulp the torch head ties
    them and takes the lower index, so the two paths can pick different tokens there.
    With sample=True (off by default; per call generate(sample=..., seed=...); needs hip_head) a generation_config that samples is no longer
    refused: the head launch also writes its f32 scores and x2i_sample_select_f32 (x2i_amd/sample_binding.py, include/ext/sample/x2i_sample.h)
    stands in the place of the argmax -- temperature, top-k, top-p and one inverse-CDF draw, for token 0 and inside the captured step.
    sample_plan decides which generation_config and processor lists fuse; any other raises.  The draws come from Philox4x32-10 under {seed,
    offset}, kept in device memory with the loop's other state; the counter of a token is the offset plus its column, the offset advances by
    the tokens a call generated, and a call with an explicit seed restarts at offset 0, so the same seed and inputs give the same sequences,
    eager or replayed.  Tokens of equal score are kept or dropped by top-p together (the library splits such a run by sort position).
    With w8=True (off by default; per call generate(w8=...)) the four linears of every layer of a decode step read e4m3 weights with one
    f32 scale per output row (Qwen2DecoderStack.pack_w8, made once at first use and kept beside the bf16 weights, which the prompt pass
    still runs on): half the weight bytes per token.  The lm_head stays bf16 under either head.  The captured steps hold their weights by
    pointer, so the graphs are kept per value of w8.
    With keep_cache=True (off by default; per call generate(keep_cache=...)) the instance keeps what the previous call left -- its
    sequences, the per-sample lengths, the decoder's position ids and the hidden rows cat(prompt, answer) along S, besides the cache itself
    -- and a call whose prompt starts with those tokens runs only the rest of it: Qwen2DecoderStack.extend(cache, keep=P, ...) on rows
    [P:] of the model's inputs_embeds / position_ids, P = common_prefix(...) over the valid tokens of the previous call, sequences[:, :S +
    n - 1] (n the largest length: the pass of the last generated token never ran; passes after a sample's end token hold the pad token,
    as the sequences do).  GenerateResult.prompt is then the kept rows, bit for bit what the earlier calls returned, followed by the new
    rows.  Reuse needs the same B, no padding in either call (mask None or all ones), P >= 1, S - P >= 1 and the decoder's
    position_ids[..., :P] equal to the kept ones; otherwise the call runs the whole prefill as today and `reuse_note` says why.  `reused`
    is the last call's P (0: a whole prefill).  The extra cost of a reused turn is one host read.  The capacity is rounded up to a
    multiple of 1024 slots instead of 64, so that cache and graphs survive several turns; a turn that does not fit gets a larger cache,
    slots [0, P) of K / V^T copied over, and the captured graphs (which hold the old cache by pointer) are dropped.  forget() drops the
    conversation; so does any call with keep_cache off.
    THE CALLER'S PROMISE under keep_cache: a token match cannot see changed pixels or audio -- the placeholder ids of an image are the
    same for every image -- so the features under a matching prefix must be unchanged from the previous call (a chat history whose
    images never change, as inference_multi_turn's)."""

    def __init__(self, model, check_mask=True, hip_head=False, w8=False, keep_cache=False, sample=False, seed=0):
        from .qwen import Qwen2DecoderStack
        self.decoder = find_decoder(model)
        self.stack = Qwen2DecoderStack.from_hf(self.decoder)
        self.n_layers = len(self.decoder.layers)
        self.C = self.n_layers + 1
        self.check_mask = check_mask
        self.hip_head = hip_head
        self.w8 = w8
        self.keep_cache = keep_cache
        self.sample = sample
        self._rng = [int(seed), 0]      # under sample: the seed, and the offset of the next call (the tokens generated so far)
        self.reused, self.reuse_note = 0, ""
        self.slab = self._cache = None
        self._state = {}
        self._conv = None       # under keep_cache: what the previous call left (_remember)
        self._keep = False      # this call's keep_cache

    def forget(self):
        """Drops the kept conversation: the next call runs its whole prompt"""
        self._conv = None

    def _reusable(self, B, S, ids, attention_mask, pos):
        """-> (P, why not): how many leading slots of the kept conversation this call's prompt [B, S] can stand on.  One host read."""
        conv = self._conv
        if conv is None:
            return 0, "no kept conversation"
        if conv["B"] != B or ids is None or tuple(ids.shape) != (B, S):
            return 0, "another batch size"
        kept = conv["pos"]
        if pos.dim() != kept.dim():
            return 0, "other position axes"
        m = min(conv["valid"], S)
        one = torch.ones((), device=pos.device, dtype=torch.long)
        p_pos = (pos[..., :m] == kept[..., :m]).reshape(-1, m).all(0).long().cumprod(0).sum()
        full = one if attention_mask is None else (attention_mask != 0).all().long().to(pos.device)
        P, p_pos, full, was_full = torch.stack((_common_prefix(conv["sequences"], conv["valid"], ids).to(pos.device), p_pos, full,
                                                conv["unpadded"])).tolist()      # the one host read
        if not (full and was_full):
            return 0, "a padded batch"
        if P < 1 or S - P < 1:
            return 0, "no common prefix" if P < 1 else "nothing new after the common prefix"
        if p_pos < P:
            return 0, "the position ids under the common prefix changed"
        return P, ""

    def _remember(self, res):
        """After a call under keep_cache: what the next one stands on"""
        S, n = res.prompt.shape[2], res.sequences.shape[1] - res.prompt.shape[2]
        dev = res.prompt.device
        pos = torch.cat((self._pos_prompt, self._pos_next[..., None] + torch.arange(n - 1, device=dev)), -1)
        hidden = torch.cat((res.prompt, res.answer), 2) if n > 1 else res.prompt
        self._conv = dict(B=res.prompt.shape[0], sequences=res.sequences, valid=S + n - 1, lengths=res.lengths, pos=pos, hidden=hidden,
                          unpadded=self._unpadded)
        return res

    def _forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, use_cache=None, **kw):
        from transformers.modeling_outputs import BaseModelOutputWithPast
        if self.slab is not None:
            raise RuntimeError("handoff.HipGenerate: the surrounding model ran the decoder a second time; only its prompt pass goes through it")
        if isinstance(attention_mask, dict):
            raise RuntimeError("handoff.HipGenerate: the decoder was handed prepared mask tensors; it needs the 0/1 [B, S] attention_mask")
        if past_key_values is not None and past_key_values.get_seq_length() > 0:
            raise RuntimeError("handoff.HipGenerate: a non-empty key/value cache was passed; the HIP stack keeps its own")
        if inputs_embeds is not None:
            inputs_embeds = inputs_embeds.to(torch.bfloat16)
        B, S = (input_ids if input_ids is not None else inputs_embeds).shape[:2]
        # one cache stays resident, with the step captured on it: the next call at the same (B, cap) reuses both (a prefill resets the ranges
        # and positions; what older generations left in K / V^T outside the new ranges is finite, which is all the kernels ask)
        unit = 1024 if self._keep else 64
        key = (B, (S + self._new_tokens + unit - 1) // unit * unit)
        P, conv = 0, None
        if self._keep:
            dev = self.stack.device
            pos = torch.arange(S, device=dev)[None].expand(B, S) if position_ids is None else position_ids.to(dev)
            if pos.dim() == 3 and pos.shape[0] == 4:
                pos = pos[1:]
            pos = pos.expand(*pos.shape[:-2], B, S)
            P, self.reuse_note = self._reusable(B, S, self._ids, attention_mask, pos)
            conv, self._conv = self._conv, None      # (the cache is rewritten from here on: a call that fails leaves no conversation)
            self._pos_prompt = pos
            self._unpadded = (torch.ones((), device=dev, dtype=torch.long) if attention_mask is None
                              else (attention_mask != 0).all().long().to(dev))
        self.reused = P
        if self._state.get("key") != key:
            old = self._state.get("cache")
            self._state = dict(key=key, cache=self.stack.new_cache(B, key[1]))     # (the captured graphs held the old cache by pointer)
            if P:
                self._state["cache"]._adopt(old, P)
        self._cache = self._state["cache"]
        if P:
            cut = lambda t: None if t is None else t[:, P:]
            new = self.stack.extend(self._cache, P, inputs_embeds=cut(inputs_embeds), input_ids=cut(input_ids), position_ids=pos[..., P:],
                                    check=False)       # (the kept conversation is unpadded and reaches P: nothing to look up)
            self.slab = torch.cat((conv["hidden"][:, :, :P], new), 2)
        else:
            self.slab = self.stack.prefill(self._cache, inputs_embeds=inputs_embeds, input_ids=input_ids, attention_mask=attention_mask,
                                           position_ids=position_ids, check_mask=self.check_mask)
        if self._keep:
            self._pos_next = self._cache.pos.clone()
        return BaseModelOutputWithPast(last_hidden_state=self.slab[:, -1], past_key_values=None)

    @staticmethod
    def refuse_sampling(generation_config):
        if generation_config is not None and getattr(generation_config, "do_sample", False) and getattr(generation_config, "top_k", None) != 1:
            raise ValueError("handoff.HipGenerate: greedy decoding only, and this generation_config samples (do_sample=True, top_k=%r); "
                             "run with --full_generate (and without --hip_generate) instead" % (getattr(generation_config, "top_k", None),))

    @torch.no_grad()
    def generate(self, model, max_new_tokens=128, eos_token_id=None, pad_token_id=None, logits_processor=None, graph=True, check_every=16,
                 generation_config=None, hip_head=None, w8=None, keep_cache=None, sample=None, seed=None, **inputs):
        """-> GenerateResult.  inputs: the model's forward arguments of the prompt (input_ids required; attention_mask, pixel_values, ...).
        eos_token_id: an id, a list of ids or None (never stop early); pad_token_id: what follows a sample's end token (default: the first
        end token, else 0).  logits_processor: a list of callables (input_ids [B, len], scores f32 [B, V]) -> scores.  hip_head: None takes
        the constructor's; True needs a list that head_plan accepts.  w8: None takes the constructor's; True runs the decode steps on the
        stack's e4m3 weights (packed at first use).  keep_cache: None takes the constructor's; True stands on what the previous call left
        where the prompt allows it and keeps this call's for the next (the class docstring has the rules and the caller's promise).
        sample: None takes the constructor's; True needs hip_head and a generation_config and list that sample_plan accepts.  seed: None goes
        on in the instance's stream of draws; a value restarts it at offset 0 under that seed."""
        generation_config = generation_config if generation_config is not None else getattr(model, "generation_config", None)
        sample = bool(self.sample if sample is None else sample)
        if not sample:
            self.refuse_sampling(generation_config)
        elif not (self.hip_head if hip_head is None else hip_head):
            raise ValueError("handoff.HipGenerate: sample draws the tokens of the hip_head step: not without hip_head (--hip_sample needs "
                             "--hip_generate --hip_head)")
        if max_new_tokens < 1:
            raise ValueError("handoff.HipGenerate: max_new_tokens must be at least 1")
        ids = inputs.get("input_ids")
        if ids is None:
            raise ValueError("handoff.HipGenerate: input_ids are required (the generated tokens are appended to them)")
        eos = [] if eos_token_id is None else ([int(eos_token_id)] if not isinstance(eos_token_id, (list, tuple)) else [int(e) for e in eos_token_id])
        pad = int(pad_token_id) if pad_token_id is not None else (eos[0] if eos else 0)
        processors = list(logits_processor or [])
        hip_head = self.hip_head if hip_head is None else hip_head
        w8 = bool(self.w8 if w8 is None else w8)
        self._keep, self._ids = bool(self.keep_cache if keep_cache is None else keep_cache), ids
        self.reused, self.reuse_note = 0, ""
        if not self._keep:
            self._conv = None     # (this call's prefill resets the cache the conversation stood on)
        head = model.get_output_embeddings()
        if hip_head:       # every refusal comes before anything runs
            import inspect
            samp = None
            if sample:
                penalty, *samp = sample_plan(generation_config, processors)
                if seed is not None:
                    self._rng = [int(seed), 0]
            else:
                penalty = head_plan(processors)
            if len(eos) > 8:
                raise ValueError("handoff.HipGenerate: hip_head takes at most 8 end tokens (got %d)" % len(eos))
            if getattr(head, "bias", None) is not None or head.weight.dtype != torch.bfloat16 or not head.weight.is_contiguous():
                raise ValueError("handoff.HipGenerate: hip_head needs a contiguous bf16 lm_head weight and no bias")
            if not 0 <= pad < head.weight.shape[0]:
                raise ValueError("handoff.HipGenerate: hip_head needs a pad token inside the vocabulary (got %d)" % pad)
            if "logits_to_keep" in inspect.signature(model.forward).parameters and "logits_to_keep" not in inputs:
                inputs = dict(inputs, logits_to_keep=1)       # the model's own logits are not used: one position, not all S
        if w8 and self.stack._w8 is None:
            self.stack.pack_w8()
        self.slab = self._cache = None
        self._new_tokens = max_new_tokens
        with _Patch(self.decoder, "forward", self._forward):
            out = model(**inputs, use_cache=False)
        if self.slab is None:
            raise RuntimeError("handoff: the decoder stack did not run")
        prompt, cache, self.slab, self._cache = self.slab, self._cache, None, None
        dev = prompt.device
        B, C, S, H = prompt.shape
        T = max_new_tokens
        rows = torch.arange(B, device=dev)
        last = (cache.k_hi - 1).long()                                   # the last valid token of each sample, under either padding
        if hip_head:
            res = self._generate_hip_head(prompt, cache, ids, head.weight, penalty, eos, pad, T, rows, last, graph, check_every, w8, samp)
            return self._remember(res) if self._keep else res
        sequences = torch.full((B, S + T), pad, device=dev, dtype=torch.long)
        sequences[:, :S] = ids
        answer = torch.empty((B, C, max(T - 1, 0), H), device=dev, dtype=torch.bfloat16)
        done = torch.zeros((B,), device=dev, dtype=torch.bool)
        lengths = torch.zeros((B,), device=dev, dtype=torch.long)
        eos_t = torch.tensor(eos, device=dev, dtype=torch.long) if eos else None
        st = self._state
        if "token" not in st:       # the captured step's input and output live with the cache
            st["token"] = torch.empty((B,), device=dev, dtype=torch.long)
            st["step_out"] = torch.empty((B, C, H), device=dev, dtype=torch.bfloat16)
        token, step_out = st["token"], st["step_out"]

        def pick(t, scores):
            """token t from the f32 scores [B, V] of the pass before it: processors, argmax, the end-token bookkeeping, all on the device"""
            for p in processors:
                scores = p(sequences[:, :S + t], scores)
            nxt = torch.where(done, torch.full_like(token, pad), scores.argmax(-1))
            token.copy_(nxt)
            sequences[:, S + t] = nxt
            lengths.add_((~done).long())
            if eos_t is not None:
                done.logical_or_((nxt[:, None] == eos_t[None]).any(-1))

        pick(0, out.logits[rows, last].float())
        if st.get("head") is not head:      # (a graph holds the lm_head it was captured with)
            st.pop("graph", None)
            st["head"] = head
        graphs = st.setdefault("graph", {})     # w8 -> (graph, logits): a captured step holds its weights by pointer
        if graphs and st.get("w8_pack") is not self.stack._w8:       # ... and a new pack is new pointers
            graphs.pop(True, None)
        st["w8_pack"] = self.stack._w8
        t = 1
        while t < T:
            if check_every and t % check_every == 0 and eos_t is not None and bool(done.all()):      # the one host read per check_every steps
                break
            if not graph:
                cache_out = answer[:, :, t - 1]
                self.stack.decode_step(cache, input_ids=token, out=cache_out, w8=w8)
                logits = head(cache_out[:, -1])
            else:
                if w8 not in graphs and w8 not in st.setdefault("warm", set()):
                    # the very first step runs eagerly on a side stream (the warm-up a capture needs); the next one is the capture
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        self.stack.decode_step(cache, input_ids=token, out=step_out, w8=w8)
                        logits = head(step_out[:, -1])
                    torch.cuda.current_stream().wait_stream(side)
                    st["warm"].add(w8)
                else:
                    if w8 not in graphs:
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            self.stack.decode_step(cache, input_ids=token, out=step_out, w8=w8)
                            captured = head(step_out[:, -1])
                        cache.steps -= 1                 # (a capture runs nothing: the replay below is this step)
                        graphs[w8] = (g, captured)
                    graphs[w8][0].replay()
                    cache.steps += 1
                    logits = graphs[w8][1]
                answer[:, :, t - 1].copy_(step_out)
            pick(t, logits.float())
            t += 1
        n = int(lengths.max()) if eos_t is not None else T                # (tokens after every sample's end are dropped: one host read)
        n = max(n, 1)
        res = GenerateResult(prompt, answer[:, :, :n - 1], sequences[:, :S + n], lengths)
        return self._remember(res) if self._keep else res

    def _generate_hip_head(self, prompt, cache, ids, W, penalty, eos, pad, T, rows, last, graph, check_every, w8=False, samp=None):
        """generate()'s loop with the head kernels: every word of the loop's state lives in buffers that stay with the cache, so that the
        captured step (gather, decode_step, the copy into the answer at the device counter's column, both head kernels) replays.
        samp: None, or [temperature, top_k, top_p]: the head launch also writes its f32 scores and x2i_sample_select_f32 stands in the place
        of the greedy select; the draw's counter is the random-number offset plus the step counter, both in device memory."""
        from . import qwen_head_ops as HO
        from . import sample_binding as SB
        dev = prompt.device
        B, C, S, H = prompt.shape
        V = W.shape[0]
        st = self._state
        hkey = (W.data_ptr(), V, penalty, pad, tuple(eos), None if samp is None else tuple(samp))         # what a captured step holds by value
        if st.get("hkey") != hkey or st["h_answer"].shape[2] < T - 1:
            st.pop("hgraph", None)
            st["hkey"] = hkey
            st["h_token"] = torch.zeros((B,), device=dev, dtype=torch.long)
            st["h_out"] = torch.empty((B, C, H), device=dev, dtype=torch.bfloat16)
            st["h_answer"] = torch.empty((B, C, max(T - 1, 1), H), device=dev, dtype=torch.bfloat16)
            st["h_seq"] = torch.empty((B, st["key"][1]), device=dev, dtype=torch.long)
            st["h_seen"] = torch.empty((B, V), device=dev, dtype=torch.uint8)
            st["h_ws"] = torch.empty((HO.workspace_floats(B, V),), device=dev, dtype=torch.float32)
            st["h_step"] = torch.zeros((1,), device=dev, dtype=torch.int32)
            st["h_base"] = torch.zeros((1,), device=dev, dtype=torch.long)
            st["h_done"] = torch.zeros((B,), device=dev, dtype=torch.uint8)
            st["h_len"] = torch.zeros((B,), device=dev, dtype=torch.long)
            st["h_eos"] = torch.tensor(eos, device=dev, dtype=torch.long) if eos else None
            st["h_logits"] = torch.empty((B, V), device=dev, dtype=torch.float32) if samp is not None else None
            st["h_rng"] = torch.zeros((2,), device=dev, dtype=torch.long)
        hgraphs = st.setdefault("hgraph", {})   # w8 -> graph: a captured step holds its weights by pointer
        if hgraphs and st.get("h_w8_pack") is not self.stack._w8:    # ... and a new pack is new pointers
            hgraphs.pop(True, None)
        st["h_w8_pack"] = self.stack._w8
        token, step_out, abuf, seq, seen, ws = st["h_token"], st["h_out"], st["h_answer"], st["h_seq"], st["h_seen"], st["h_ws"]
        step, base, done, lengths, eos_t = st["h_step"], st["h_base"], st["h_done"], st["h_len"], st["h_eos"]
        seq.fill_(pad)
        seq[:, :S] = ids
        seen.zero_().scatter_(1, ids.long(), 1)                    # every id of input_ids, pad ids included (the library's processor)
        step.fill_(S)                                              # the column of token 0
        base.fill_(S + 1)                                          # the pass of token t - 1 runs with the counter at S + t: answer column t - 1
        done.zero_()
        lengths.zero_()
        logits, rng = st["h_logits"], st["h_rng"]
        if samp is not None:
            rng.copy_(SB.rng_state(self._rng[0], self._rng[1], dev))

        def pick(x):
            HO.logits_argmax(x, W, ws, seen=seen, penalty=penalty, step=step, logits=logits)
            if samp is None:
                HO.select(ws, step, token, seq, lengths, done, pad, V, eos=eos_t, seen=seen)
            else:
                SB.select(logits, ws, step, token, seq, lengths, done, pad, temperature=samp[0], top_k=samp[1], top_p=samp[2], rng=rng,
                          eos=eos_t, seen=seen)

        def one_step():
            self.stack.decode_step(cache, input_ids=token, out=step_out, w8=w8)
            abuf.index_copy_(2, step.long() - base, step_out.unsqueeze(2))
            pick(step_out[:, -1])

        pick(prompt[:, -1][rows, last].contiguous())               # token 0: the same two kernels on each sample's last valid row
        t = 1
        while t < T:
            if check_every and t % check_every == 0 and eos_t is not None and bool(done.all()):      # the one host read per check_every steps
                break
            if not graph:
                one_step()
            elif w8 not in hgraphs and w8 not in st.setdefault("hwarm", set()):
                side = torch.cuda.Stream()                         # the warm-up a capture needs
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    one_step()
                torch.cuda.current_stream().wait_stream(side)
                st["hwarm"].add(w8)
            else:
                if w8 not in hgraphs:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        one_step()
                    cache.steps -= 1                               # (a capture runs nothing: the replay below is this step)
                    hgraphs[w8] = g
                hgraphs[w8].replay()
                cache.steps += 1
            t += 1
        n = int(lengths.max()) if eos_t is not None else T                # (tokens after every sample's end are dropped: one host read)
        n = max(n, 1)
        if samp is not None:
            self._rng[1] += n                                         # the next call goes on in the stream
        return GenerateResult(prompt, abuf[:, :, :n - 1].clone(), seq[:, :S + n].clone(), lengths.clone())


def find_visual(model):
    """The vision tower of a Qwen2.5-VL model: `model.visual` (Qwen2_5_VLModel) or `model.model.visual` (Qwen2_5_VLForConditionalGeneration)"""
    for m in (model, getattr(model, "model", None)):
        v = getattr(m, "visual", None) if m is not None else None
        if isinstance(v, nn.Module):
            return v
    raise RuntimeError("handoff: no vision tower (model.visual / model.model.visual) found in %s" % type(model).__name__)


class HipVision(_Patch):
    """The vision tower behind `model.visual` on the HIP path (x2i_amd/qwen_vision.py: Qwen2_5VisionTower, a bf16 copy of the tower's weights on
    its device).  install() replaces the tower module's `forward` ON THE INSTANCE and remove() restores it; between the two the surrounding
    model's get_image_features / get_video_features and its embedding merge run as they always do and get the library's output object from
    the HIP tower.  Also a context manager.  Independent of HipPrefill: under either kind of slab, and under generate()."""

    def __init__(self, model):
        from .qwen_vision import Qwen2_5VisionTower
        self.visual = find_visual(model)
        self.tower = Qwen2_5VisionTower.from_hf(self.visual)
        self.calls = self.in_place = 0
        _Patch.__init__(self, self.visual, "forward", self._forward)

    def _forward(self, hidden_states, grid_thw=None, **kw):
        """Rows that ARE the [:, :1176] view of the tower's padded workspace for this grid (HipQwenImage(tower=...) wrote them there, bf16)
        are not copied: the tower runs from its workspace, and `in_place` counts it.  Any other input takes the copying forward."""
        self.calls += 1
        tower = self.tower
        if (isinstance(grid_thw, torch.Tensor) and hidden_states.dtype == torch.bfloat16 and hidden_states.device == tower.device
                and hidden_states.dim() == 2 and hidden_states.stride() == (tower.Kp, 1)):
            plan = tower._plan_for(tuple(tuple(int(v) for v in g) for g in grid_thw.tolist()))     # the one host read, as forward's
            if hidden_states.data_ptr() == tower.pixel_workspace(plan).data_ptr() and tuple(hidden_states.shape) == (plan.S, tower.patch_dim):
                self.in_place += 1
                return tower.forward_from_workspace(plan)
            return tower(hidden_states, plan=plan)
        return tower(hidden_states, grid_thw=grid_thw)


def find_vpm(model):
    """The SigLIP vision tower of a MiniCPM-o model: `model.vpm`"""
    v = getattr(model, "vpm", None)
    if isinstance(v, nn.Module):
        return v
    raise RuntimeError("handoff: no vision tower (model.vpm) found in %s" % type(model).__name__)


class HipSiglip(_Patch):
    """The vision tower behind `model.vpm` on the HIP path (x2i_amd/siglip.py: SiglipVisionTower, a bf16 copy of the tower's weights on its
    device).  HipVision's interface: install() replaces the tower module's `forward` ON THE INSTANCE and remove() restores it; between the
    two the surrounding model's get_vllm_embedding, its Resampler (the model's own, or HipResampler's when that is installed too) and its
    embedding scatter run as they always do and get the library's output object from the HIP tower.  Also a context manager.  Independent
    of the kind of slab, and the same under generate()."""

    def __init__(self, model):
        from .siglip import SiglipVisionTower
        self.vpm = find_vpm(model)
        self.tower = SiglipVisionTower.from_hf(self.vpm)
        self.calls = 0
        _Patch.__init__(self, self.vpm, "forward", self._forward)

    def _forward(self, pixel_values, patch_attention_mask=None, tgt_sizes=None, **kw):
        self.calls += 1
        return self.tower(pixel_values, patch_attention_mask=patch_attention_mask, tgt_sizes=tgt_sizes)


def find_resampler(model):
    """The perceiver of a MiniCPM-o model: `model.resampler`"""
    r = getattr(model, "resampler", None)
    if isinstance(r, nn.Module):
        return r
    raise RuntimeError("handoff: no resampler (model.resampler) found in %s" % type(model).__name__)


class HipResampler(_Patch):
    """The perceiver behind `model.resampler` on the HIP path (x2i_amd/resampler.py: Resampler, a bf16 copy of the module's weights on its
    device).  HipSiglip's interface: install() replaces the module's `forward` ON THE INSTANCE and remove() restores it; between the two
    the surrounding model's get_vllm_embedding and its embedding scatter run as they always do and get a [B, NQ, D] tensor from the HIP
    module.  Also a context manager.  Independent of HipSiglip: either, both or neither may be installed."""

    def __init__(self, model):
        from .resampler import Resampler
        self.module = find_resampler(model)
        self.resampler = Resampler.from_hf(self.module)
        self.calls = 0
        _Patch.__init__(self, self.module, "forward", self._forward)

    def _forward(self, x, tgt_sizes=None, **kw):
        self.calls += 1
        return self.resampler(x, tgt_sizes=tgt_sizes)


def find_apm(model):
    """The Whisper audio encoder of a MiniCPM-o model: `model.apm`"""
    a = getattr(model, "apm", None)
    if isinstance(a, nn.Module):
        return a
    raise RuntimeError("handoff: no audio tower (model.apm) found in %s" % type(model).__name__)


class HipAudio(_Patch):
    """The audio tower behind `model.apm`, with `model.audio_projection_layer` and `model.audio_avg_pooler`, on the HIP path
    (x2i_amd/whisper.py: WhisperAudioTower, a bf16 copy of the modules' weights on their device).  The model's `apm` is never called as a
    module for this -- get_audio_embedding builds the mask and picks hidden_states[-1] itself -- so install() replaces
    `get_audio_embedding` ON THE INSTANCE and remove() restores it; the replacement takes (data, chunk_length=-1, dummy=True) and returns
    the model's list (per prompt) of lists (per audio) of [n_b, E] tensors, [] for no audio.  What it does not serve goes to the original:
    a model in training mode, or one whose audio_encoder_layer is not -1.  The embedding scatter (get_omni_embedding) and the streaming
    path stay the model's own.  Also a context manager.  Independent of HipSiglip and HipResampler, and of the kind of slab."""

    def __init__(self, model):
        from .whisper import WhisperAudioTower
        self.model = model
        self.apm = find_apm(model)
        proj = getattr(model, "audio_projection_layer", None)
        if not isinstance(proj, nn.Module):
            raise RuntimeError("handoff: no audio projector (model.audio_projection_layer) found in %s" % type(model).__name__)
        cfg = getattr(model, "config", None)
        step = getattr(cfg, "audio_pool_step", None)
        if step is None:
            pooler = getattr(model, "audio_avg_pooler", None)
            k = getattr(pooler, "kernel_size", None)
            step = k[0] if isinstance(k, (tuple, list)) else k
        if step is None:
            raise RuntimeError("handoff: no pooling step (model.config.audio_pool_step / model.audio_avg_pooler) found in %s" % type(model).__name__)
        self.tower = WhisperAudioTower.from_hf(self.apm, proj, int(step))
        self.calls = 0
        _Patch.__init__(self, self.model, "get_audio_embedding", self._get_audio_embedding)

    def _get_audio_embedding(self, data, chunk_length=-1, dummy=True):
        model = self.model
        if model.training or getattr(model, "audio_encoder_layer", -1) != -1:
            return self._original(data, chunk_length=chunk_length, dummy=dummy)
        mel = data.get("audio_features", [])
        if len(mel) == 0:
            return []
        lens_raw = data.get("audio_feature_lens", [])
        lens = [int(n) for group in lens_raw for n in (group.reshape(-1).tolist() if isinstance(group, torch.Tensor) else group)]
        self.calls += 1
        out, counts = self.tower(mel, feature_lens=lens, chunk_frames=int(chunk_length * 50) if chunk_length > 0 else 0)
        final, idx = [], 0
        for group in lens_raw:
            mine = []
            for _ in range(len(group)):
                mine.append(out[idx, :counts[idx], :])
                idx += 1
            final.append(mine)
        return final


class _HipFeatureExtractor:
    """What HipLogMel puts in a processor's `feature_extractor`: every attribute is the original's (hop_length, model_input_names, ...),
    and a call in the form the MiniCPM-o processor uses runs LogMel"""

    def __init__(self, original, logmel, owner):
        self.__dict__.update(_fe=original, _logmel=logmel, _owner=owner)

    def __getattr__(self, name):
        return getattr(self._fe, name)

    def __call__(self, raw_speech, *args, **kw):
        from transformers.feature_extraction_utils import BatchFeature
        fe, lm = self._fe, self._logmel
        served = (not args and set(kw) <= {"sampling_rate", "padding", "return_attention_mask", "return_tensors"}
                  and kw.get("sampling_rate") == 16000 and kw.get("padding") == "max_length" and kw.get("return_attention_mask") is True
                  and kw.get("return_tensors") == "pt" and fe.sampling_rate == 16000
                  and isinstance(raw_speech, (list, tuple)) and len(raw_speech) > 0
                  and all(getattr(w, "ndim", 0) == 1 and 1 <= len(w) <= lm.n_samples for w in raw_speech))
        if not served:
            return fe(raw_speech, *args, **kw)
        self._owner.calls += 1
        T = lm.T
        features, lens = lm(list(raw_speech), out_dtype=torch.float32, T_out=T)
        mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(torch.int32)          # on the host: the processor slices by its sums
        return BatchFeature({"input_features": features, "attention_mask": mask})


class HipLogMel(_Patch):
    """The log-mel front end in front of the audio tower on the HIP path (x2i_amd/logmel.py: LogMel, the tables of the processor's own
    WhisperFeatureExtractor on `device`).  install() replaces `feature_extractor` ON THE PROCESSOR INSTANCE by an object that forwards every
    attribute to the original and serves the call the MiniCPM-o processor makes (sampling_rate=16000, padding="max_length",
    return_attention_mask=True, return_tensors="pt", 1-D waveforms of at most n_samples): `input_features` float32
    [n, n_mels, n_samples / 160] ON THE DEVICE and `attention_mask` on the host with L_b ones per row, so the processor's slicing by
    lengths reads nothing back.  Any other call goes to the original.  remove() restores it.  Also a context manager.  Independent of
    HipAudio; with both, get_audio_embedding takes the device features as they are."""

    def __init__(self, processor, device="cuda"):
        from .logmel import LogMel
        fe = getattr(processor, "feature_extractor", None)
        if fe is None or not callable(fe):
            raise RuntimeError("handoff: no feature extractor (processor.feature_extractor) found in %s" % type(processor).__name__)
        self.processor = processor
        self.logmel = LogMel.from_hf(fe, device)
        self.calls = 0
        _Patch.__init__(self, processor, "feature_extractor", _HipFeatureExtractor(fe, self.logmel, self))


class _HipImageProcessor:
    """What HipImage puts in a processor's `image_processor`: every attribute is the original's (get_slice_image_placeholder, version,
    max_slice_nums, ...), and a call in the form the MiniCPM-o processor uses runs ImageFrontEnd: on images none of which is sliced, or,
    for a HipImage(slices=True), on sliced images too"""

    def __init__(self, original, front, owner):
        self.__dict__.update(_ip=original, _front=front, _owner=owner, _feature=type(original.preprocess([[]])))

    def __getattr__(self, name):
        return getattr(self._ip, name)

    def _route(self, images, args, kw):
        """(the nested list of RGB PIL images, the call's max_slice_nums) of a call that is served, else the reason it is not"""
        from PIL import Image
        ip = self._ip
        if args or not set(kw) <= {"do_pad", "max_slice_nums", "return_tensors"}:
            return "another form of call"
        if isinstance(images, Image.Image):
            images = [[images]]
        elif isinstance(images, (list, tuple)) and len(images) and isinstance(images[0], Image.Image):
            images = [images]
        if not isinstance(images, (list, tuple)) or not len(images) or not all(isinstance(g, (list, tuple)) and len(g) for g in images):
            return "an empty or unknown batch"
        slices = kw.get("max_slice_nums")
        slices = ip.max_slice_nums if slices is None else int(slices)
        for im in (im for g in images for im in g):
            if not isinstance(im, Image.Image) or im.mode != "RGB":
                return "an input that is not an RGB image of 8 bits per channel"
            if not self._owner.slices:
                if ip.get_sliced_grid(im.size, slices) is not None:
                    return "an image that is sliced"
                why = self._front.served(*im.size)          # a side over 70 patches, a scale whose LDS plan does not fit
            else:
                grid = ip.get_sliced_grid(im.size, slices)
                if (None if grid is None else tuple(grid)) != self._front.sliced_grid(im.size[0], im.size[1], slices):
                    return "a slicing grid other than the front end's"
                why = self._front.served(im.size[0], im.size[1], slices)
            if why is not None:
                return why
        return [list(g) for g in images], (slices if self._owner.slices else 1)

    def __call__(self, images, *args, **kw):
        import numpy as np
        routed = self._route(images, args, kw)
        if isinstance(routed, str):
            self._owner.fallbacks += 1
            self._owner.last_reason = routed
            return self._ip(images, *args, **kw)
        self._owner.calls += 1
        routed, slices = routed
        flat = [im for g in routed for im in g]
        if slices > 1:                                      # per image [source image, crops ...], in a row like the original's
            values, tgt = self._front.sliced(flat, slices)
        else:
            values, tgt = self._front(flat)
            values = [[v] for v in values]
        pixel_values, image_sizes, tgt_sizes, at = [], [], [], 0
        for g in routed:
            pixel_values.append([v for vs in values[at:at + len(g)] for v in vs])
            image_sizes.append([im.size for im in g])
            tgt_sizes.append(np.vstack(tgt[at:at + len(g)]))
            at += len(g)
        # the processor's own feature type converts host values the way the original's return does; a tensor it would drop, so the
        # device tensors go in afterwards, in the original's key order
        feat = self._feature(data={"image_sizes": image_sizes, "tgt_sizes": tgt_sizes}, tensor_type=kw.get("return_tensors"))
        feat.data = {"pixel_values": pixel_values, "image_sizes": feat.data["image_sizes"], "tgt_sizes": feat.data["tgt_sizes"]}
        return feat


class HipImage(_Patch):
    """The image front end in front of the SigLIP tower on the HIP path (x2i_amd/image.py: ImageFrontEnd with the processor's own
    scale_resolution, mean and std on `device`).  install() replaces `image_processor` ON THE PROCESSOR INSTANCE by an object that forwards
    every attribute to the original and serves the call the MiniCPM-o processor makes (images, do_pad=, max_slice_nums=, return_tensors=):
    the processor's own batch-feature type with `pixel_values` float32 [3, 14, 14 L] ON THE DEVICE and `image_sizes` and `tgt_sizes` as
    the original gives them, nothing read back.  The WHOLE call goes to the original where an image would be sliced under the call's
    max_slice_nums, is not an RGB PIL image, has a side over 70 patches or a scale the kernel refuses, or the call has another form;
    `calls` and `fallbacks` count the two routes and `last_reason` says why the last fallback happened.  remove() restores the original.
    Also a context manager.  Independent of HipSiglip and the other hand-offs.
    slices=True (not the default) also serves a call with images that are sliced under the call's max_slice_nums: per image the source image
    and the crops of the processor's grid, row by row, in one list like the original's, `tgt_sizes` one row per entry; the crops cost one
    more launch per group of equally sized images (include/frontend/tiles/x2i_image_tiles.h).  Every other refusal stays."""

    def __init__(self, processor, device="cuda", slices=False):
        from .image import ImageFrontEnd
        ip = getattr(processor, "image_processor", None)
        if ip is None or not callable(ip) or not callable(getattr(ip, "get_sliced_grid", None)):
            raise RuntimeError("handoff: no MiniCPM-o image processor (processor.image_processor) found in %s" % type(processor).__name__)
        self.processor = processor
        self.front = ImageFrontEnd.from_hf(ip, device)
        self.slices = bool(slices)
        self.calls = self.fallbacks = 0
        self.last_reason = None
        _Patch.__init__(self, processor, "image_processor", _HipImageProcessor(ip, self.front, self))


class _HipQwenImageProcessor:
    """What HipQwenImage puts in a processor's `image_processor`: every attribute is the original's, and a call in the form the Qwen2.5-VL
    processor uses (images=, return_tensors="pt" and overrides that change nothing) runs QwenImageFrontEnd"""

    def __init__(self, original, front, owner):
        self.__dict__.update(_ip=original, _front=front, _owner=owner, _feature=self._feature_type(original))

    def __getattr__(self, name):
        return getattr(self._ip, name)

    @staticmethod
    def _feature_type(ip):
        """The batch-feature type the original returns: the one its class's module (or a base class's) names BatchFeature"""
        import sys
        for klass in type(ip).__mro__:
            t = getattr(sys.modules.get(klass.__module__), "BatchFeature", None)
            if isinstance(t, type):
                return t
        from transformers.feature_extraction_utils import BatchFeature
        return BatchFeature

    def _route(self, images, args, kw):
        """The list of RGB PIL images / uint8 arrays of a call that is served, else the reason it is not"""
        import numpy as np
        from PIL import Image
        ip = self._ip
        if args:
            return "another form of call"
        if kw.get("videos") is not None:
            return "videos= is passed"
        for k, v in kw.items():
            if k == "return_tensors":
                if v is not None and str(getattr(v, "value", v)) != "pt":
                    return "return_tensors = %r" % (v,)
            elif k != "videos" and v is not None and not (hasattr(ip, k) and _same_setting(getattr(ip, k), v)):
                return "a per-call override the front end does not model: %s" % k
        if isinstance(images, (Image.Image, np.ndarray)):
            images = [images]
        if isinstance(images, (list, tuple)) and len(images) and all(isinstance(g, (list, tuple)) for g in images):
            images = [im for g in images for im in g]
        if not isinstance(images, (list, tuple)) or not len(images):
            return "an empty or unknown batch"
        for im in images:
            if isinstance(im, Image.Image):
                if im.mode != "RGB":
                    return "an input that is not an RGB image of 8 bits per channel"
                w, h = im.size
            elif isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.shape[0] and im.shape[1]:
                h, w = im.shape[:2]
            else:
                return "an input that is not an RGB image of 8 bits per channel"
            why = self._front.served(w, h)                  # smart_resize's aspect ratio, a side over 11760, a scale whose LDS plan does not fit
            if why is not None:
                return why
        return list(images)

    def __call__(self, images=None, *args, **kw):
        routed = self._route(images, args, kw)
        if isinstance(routed, str):
            self._owner.fallbacks += 1
            self._owner.last_reason = routed
            return self._ip(images, *args, **kw)
        self._owner.calls += 1
        front, tower = self._front, self._owner.tower
        if tower is None:
            rows, grid = front(routed)
        else:                                               # bf16 rows straight into the tower's padded workspace of this grid
            sizes = [(im.size[1], im.size[0]) if hasattr(im, "size") and not hasattr(im, "shape") else im.shape[:2] for im in routed]
            key = tuple((1, H // 14, W // 14) for H, W in (front.smart_resize(h, w) for h, w in sizes))
            plan = tower._plan_for(key)
            rows, grid = front(routed, out_dtype=torch.bfloat16, out=tower.pixel_workspace(plan), row_stride=tower.Kp)
        # the library's feature type converts the host grid the way the original's return does; the device rows go in afterwards, in the
        # original's key order
        feat = self._feature(data={"image_grid_thw": grid}, tensor_type=kw.get("return_tensors"))
        feat.data = {"pixel_values": rows, "image_grid_thw": feat.data["image_grid_thw"]}
        return feat


def _same_setting(have, given):
    """Whether a per-call override equals the processor's own setting (sizes compare as dicts, lists as tuples)"""
    norm = lambda v: dict(v) if hasattr(v, "keys") else (tuple(v) if isinstance(v, (list, tuple)) else v)     # noqa: E731
    try:
        return bool(norm(have) == norm(given))
    except Exception:
        return False


class HipQwenImage(_Patch):
    """The image front end in front of the Qwen2.5-VL vision tower on the HIP path (x2i_amd/qwen_image.py: QwenImageFrontEnd with the
    processor's own mean, std and pixel bounds on `device`).  install() replaces `image_processor` ON THE PROCESSOR INSTANCE by an object that
    forwards every attribute to the original and serves the call the Qwen2.5-VL processor makes (images=, return_tensors="pt"): the library's
    batch-feature type with `pixel_values` float32 [S, 1176] ON THE DEVICE and `image_grid_thw` as the original gives it, nothing read back.
    The WHOLE call goes to the original where an image is not an RGB PIL image or a uint8 [H, W, 3] array, a size is refused (aspect ratio
    over 200, a side over 11760, a scale the kernel's LDS plan does not fit), per-call overrides are present that differ from the
    processor's settings (do_resize=False, another size, resample, patch_size, ...), or videos= is passed; `calls` and `fallbacks` count
    the two routes and `last_reason` says why the last fallback happened.  remove() restores the original.  Also a context manager.
    tower: a Qwen2_5VisionTower (HipVision(model).tower).  The rows are then written as bf16 straight into the tower's padded workspace of the
    call's grid and `pixel_values` IS that workspace's [:, :1176] view, which HipVision recognises and does not copy; bf16 is the one
    rounding the tower's own copy makes, so the tower computes the same bits."""

    def __init__(self, processor, device="cuda", tower=None):
        from .qwen_image import QwenImageFrontEnd
        ip = getattr(processor, "image_processor", None)
        if ip is None or not callable(ip) or not hasattr(ip, "image_mean") or not hasattr(ip, "merge_size"):
            raise RuntimeError("handoff: no Qwen2.5-VL image processor (processor.image_processor) found in %s" % type(processor).__name__)
        self.processor, self.tower = processor, tower
        self.front = QwenImageFrontEnd.from_hf(ip, device)
        self.calls = self.fallbacks = 0
        self.last_reason = None
        _Patch.__init__(self, processor, "image_processor", _HipQwenImageProcessor(ip, self.front, self))


def find_extract_feature(model):
    """What extract_feature of an InternVL2.5 chat model runs: (`model.vision_model`, `model.mlp1`), of a model that has the method"""
    v, m = getattr(model, "vision_model", None), getattr(model, "mlp1", None)
    if isinstance(v, nn.Module) and isinstance(m, nn.Module) and callable(getattr(model, "extract_feature", None)):
        return v, m
    raise RuntimeError("handoff: no extract_feature with model.vision_model and model.mlp1 found in %s" % type(model).__name__)


class HipInternVision(_Patch):
    """What `extract_feature` of an InternVL2.5 chat model computes -- `model.vision_model` (InternViT), the class token dropped,
    pixel_shuffle and `model.mlp1` -- on the HIP path (x2i_amd/internvit.py: InternVLVision over an InternVisionTower, a bf16 copy of the
    modules' weights on their device).  The shuffle and mlp1 live in the chat model and not in vision_model, so install() replaces
    `extract_feature` ON THE INSTANCE and remove() restores it; the replacement takes pixel_values [B, 3, 448, 448] and returns the
    model's [B, num_image_token, H_llm].  select_layer, downsample_ratio and ps_version are read off the model.  A model in training mode
    goes to the original.  With graph=True (the default here) every call after the second of a shape replays one captured graph.  The
    embedding scatter and the language model stay the model's own.  HipAudio's interface; also a context manager.  Independent of the
    kind of slab."""

    def __init__(self, model, graph=True):
        from .internvit import InternVisionTower, InternVLVision
        self.model = model
        vision_model, mlp1 = find_extract_feature(model)
        cfg = getattr(model, "config", None)
        pick = lambda name, default: getattr(model, name, getattr(cfg, name, default))
        self.vision = InternVLVision(InternVisionTower.from_hf(vision_model), mlp1, downsample_ratio=pick("downsample_ratio", 0.5),
                                     ps_version=pick("ps_version", "v2"), select_layer=pick("select_layer", -1), graph=graph)
        self.calls = 0
        _Patch.__init__(self, self.model, "extract_feature", self._extract_feature)

    def _extract_feature(self, pixel_values):
        if self.model.training:
            return self._original(pixel_values)
        self.calls += 1
        return self.vision(pixel_values)


def generate_positions(attention_mask, pad_position=0):
    """The position ids the library's generate() derives from a 0/1 [B, S] mask for the prompt pass: the count of valid tokens before each
    row, and pad_position in the padding -- 0 in `transformers` 5.x (_prepare_position_ids_for_generation), 1 in 4.x; the rows of the
    padding are in the slab the projector reads, so the value is the library's and not a free choice.  None without a mask (the stack's
    arange)."""
    if attention_mask is None:
        return None
    return (attention_mask.long().cumsum(-1) - 1).masked_fill_(attention_mask == 0, pad_position)


class _PromptHandoff(_Patch):
    """What the two prompt hand-offs share: the decoder stack on the HIP path called DIRECTLY -- not through the surrounding causal LM, so no
    lm_head runs on the prompt -- and HipAudio's interface around it: install() replaces `generate` ON THE INSTANCE by one prompt pass and
    remove() restores it; also a context manager, which restores on exceptions too."""

    def _find(self, model, lm_name):
        from .qwen import Qwen2DecoderStack
        lm = getattr(model, lm_name, None)
        if not isinstance(lm, nn.Module):
            raise RuntimeError("handoff: no language model (model.%s) found in %s" % (lm_name, type(model).__name__))
        if model.training:
            raise ValueError("handoff.%s: the model is in training mode (its dummy-feature branches are not built); call .eval() first"
                             % type(self).__name__)
        self.model = model
        self.decoder = find_decoder(lm)
        self.stack = Qwen2DecoderStack.from_hf(self.decoder)
        self.n_layers = len(self.decoder.layers)
        self.C = self.n_layers + 1
        self.calls = 0
        _Patch.__init__(self, self.model, "generate", self._generate)


class HipInternVLPrompt(_PromptHandoff):
    """The prompt pass of an InternVL2.5 chat model (Qwen2 language model) with the embedding merge and the decoder stack on the HIP path:
    prompt(input_ids, attention_mask, pixel_values) -> the [B, C, S, H] slab.  The features come from `model.extract_feature(pixel_values)`
    -- the model's own, or HipInternVision's when that is installed -- the rows of `img_context_token_id` are ranked on the device
    (merge.MergePlan.from_placeholder: the row order of the model's `input_embeds[selected] = vit_embeds.reshape(-1, C)`), and ONE launch
    writes token rows and feature rows into entry 0 of the slab the stack then runs on.  Without pixels the ids run alone.  Positions are
    the library generate()'s (generate_positions).  check=True costs one host read after the merge launch and raises ValueError when the
    prompt's context tokens and the feature rows differ in number (the model's own assert) or an id lies outside the table.
    install() makes `model.generate(pixel_values=, input_ids=, attention_mask=)` return the per-layer tuple of that slab (views, no copy):
    the contract of the reference's modified generate()."""

    def __init__(self, model, check_mask=True, check=True, img_context_token_id=None):
        if not callable(getattr(model, "extract_feature", None)):
            raise RuntimeError("handoff: no extract_feature found in %s" % type(model).__name__)
        self._find(model, "language_model")
        self.check_mask, self.check = check_mask, check
        self.img_context_token_id = img_context_token_id

    @torch.no_grad()
    def prompt(self, input_ids, attention_mask=None, pixel_values=None, visual_features=None, position_ids=None):
        from .merge import MergePlan
        plan = None
        if pixel_values is not None or visual_features is not None:
            token = self.img_context_token_id if self.img_context_token_id is not None else getattr(self.model, "img_context_token_id", None)
            if token is None:
                raise ValueError("handoff.HipInternVLPrompt: pixels were given and img_context_token_id is not set (on the model or here)")
            feats = visual_features if visual_features is not None else self.model.extract_feature(pixel_values)
            plan = MergePlan.from_placeholder(input_ids, token, check=self.check).set_features(vision=feats.to(torch.bfloat16))
        slab = self.stack(input_ids=input_ids, attention_mask=attention_mask, merge=plan, check_mask=self.check_mask,
                          position_ids=position_ids if position_ids is not None else generate_positions(attention_mask))
        self.calls += 1
        return slab

    def _generate(self, pixel_values=None, input_ids=None, attention_mask=None, visual_features=None, **kw):
        if input_ids is None:
            raise ValueError("handoff.HipInternVLPrompt: generate() needs input_ids")
        return tuple(self.prompt(input_ids, attention_mask, pixel_values, visual_features).unbind(1))


class HipMiniCPMPrompt(_PromptHandoff):
    """The prompt pass of a MiniCPM-o model with the embedding merge and the decoder stack on the HIP path: prompt(**processor outputs) ->
    the [B, C, S, H] slab.  It does the work of get_vllm_embedding up to the scatter -- every image flattened to patch rows and padded to
    one batch, the patch mask and the target sizes, `model.vpm` in chunks of config.vision_batch_size and `model.resampler`, each whichever
    implementation is installed (the model's own, HipSiglip's, HipResampler's) -- takes the audio rows from `model.get_audio_embedding`
    (the model's own or HipAudio's), and then ONE launch writes token rows (times llm.config.scale_emb where the field exists), vision
    rows and audio rows into entry 0 of the slab the stack runs on (merge.MergePlan.from_bounds).  All bounds and target sizes of a call
    cross to the host in ONE read (none when they are on the CPU); the model's own path reads two ends per image bound.  Both forms of
    config.chunk_input are served: True lays a sample's concatenated audio rows over its bounds in order, False pairs audio i with bound
    i and raises the model's ValueError on a length mismatch.  A sample's bounds and its feature rows must agree in number (ValueError,
    before any launch).  install() makes `model.generate(**inputs)` return an object whose `hidden_states[0]` is the per-layer tuple of
    that slab: what the reference stacks."""

    def __init__(self, model, check_mask=True, check=True):
        for name in ("vpm", "resampler"):
            if not isinstance(getattr(model, name, None), nn.Module):
                raise RuntimeError("handoff: no model.%s found in %s" % (name, type(model).__name__))
        self._find(model, "llm")
        self.check_mask, self.check = check_mask, check
        self.scale = float(getattr(model.llm.config, "scale_emb", 1.0))

    def _vision_rows(self, pixel_values_list, tgt_sizes, dtype, device):
        """-> (bf16 [images, queries, H] or None, images per sample); tgt_sizes: host lists (merge.host_ints)"""
        import numpy as np
        flat, img_cnt = [], []
        for pixel_values in pixel_values_list:
            img_cnt.append(len(pixel_values))
            flat.extend(i.flatten(end_dim=1).permute(1, 0) for i in pixel_values)
        if not flat:
            return None, img_cnt
        sizes = [row for t in tgt_sizes if isinstance(t, list) and t for row in (t if isinstance(t[0], list) else [t])]
        if len(sizes) != len(flat):
            raise ValueError("handoff.HipMiniCPMPrompt: %d images and %d target sizes" % (len(flat), len(sizes)))
        patches = [int(h) * int(w) for h, w in sizes]
        x = torch.nn.utils.rnn.pad_sequence(flat, batch_first=True, padding_value=0.0)
        n, L, _ = x.shape
        x = x.permute(0, 2, 1).reshape(n, 3, -1, L).to(device=device, dtype=dtype)
        mask = np.zeros((n, 1, max(patches)), dtype=bool)
        for i, p in enumerate(patches):
            mask[i, 0, :p] = True
        mask = torch.from_numpy(mask).to(device)
        tgt = torch.tensor(sizes, dtype=torch.int32, device=device)
        step = int(self.model.config.vision_batch_size)
        hs = [self.model.vpm(x[i:i + step], patch_attention_mask=mask[i:i + step], tgt_sizes=tgt[i:i + step]).last_hidden_state
              for i in range(0, n, step)]
        return self.model.resampler(hs[0] if len(hs) == 1 else torch.cat(hs, dim=0), tgt).to(torch.bfloat16), img_cnt

    @torch.no_grad()
    def prompt(self, input_ids, pixel_values=None, tgt_sizes=None, image_bound=None, audio_features=(), audio_feature_lens=None,
               audio_bounds=None, attention_mask=None, position_ids=None, **ignored):
        from .merge import MergePlan, host_ints
        model, cfg = self.model, self.model.config
        B, S = input_ids.shape
        w = self.stack.embed_tokens.weight
        image_bound, audio_bounds, tgt_sizes = host_ints(image_bound, audio_bounds, tgt_sizes)        # the one host read
        image_bound = [list(b) for b in (image_bound or [])]
        vision, img_cnt = self._vision_rows(pixel_values if pixel_values is not None else [[]] * B, tgt_sizes or [], w.dtype, w.device)
        vision_rows = [n * (vision.shape[1] if vision is not None else 0) for n in img_cnt]
        audio, audio_rows = None, None
        if getattr(cfg, "init_audio", True) and audio_features is not None and len(audio_features) > 0:
            embs = model.get_audio_embedding(dict(audio_features=audio_features, audio_feature_lens=audio_feature_lens),
                                             chunk_length=getattr(cfg, "audio_chunk_length", -1))
            if len(embs) != B:
                raise ValueError("handoff.HipMiniCPMPrompt: audio embeddings for %d prompts, a batch of %d" % (len(embs), B))
            audio_bounds = [list(b) for b in (audio_bounds or [])] + [[]] * (B - len(audio_bounds or []))
            if not getattr(cfg, "chunk_input", False):
                for i in range(B):
                    for e, (s0, s1) in zip(embs[i], audio_bounds[i]):
                        if e.shape[0] != s1 - s0:
                            raise ValueError("Shape mismatch: Trying to assign embeddings of shape %s to input indices of length %d"
                                             % (tuple(e.shape), s1 - s0))
                    audio_bounds[i] = audio_bounds[i][:len(embs[i])]
                    embs[i] = embs[i][:len(audio_bounds[i])]
            else:
                audio_bounds = [b if embs[i] else [] for i, b in enumerate(audio_bounds)]      # (the model skips a sample without audio rows)
            audio_rows = [sum(int(e.shape[0]) for e in embs[i]) for i in range(B)]
            rows = [e for sample in embs for e in sample]
            if rows:
                audio = (rows[0] if len(rows) == 1 else torch.cat(rows, dim=0)).to(device=w.device, dtype=torch.bfloat16)
        else:
            audio_bounds = None
        plan = MergePlan.from_bounds(B, S, image_bound, audio_bounds, device=w.device, check=self.check, vision_rows=vision_rows,
                                     audio_rows=audio_rows).set_features(vision=vision, audio=audio)
        slab = self.stack(input_ids=input_ids, attention_mask=attention_mask, merge=plan, embed_scale=self.scale, check_mask=self.check_mask,
                          position_ids=position_ids if position_ids is not None else generate_positions(attention_mask))
        self.calls += 1
        return slab

    def _generate(self, input_ids=None, stream=False, vision_hidden_states=None, **inputs):
        if input_ids is None:
            raise ValueError("handoff.HipMiniCPMPrompt: generate() needs input_ids")
        if stream or vision_hidden_states is not None:
            raise ValueError("handoff.HipMiniCPMPrompt: stream=True and precomputed vision_hidden_states are not built; remove() the hand-off")
        for k in ("tokenizer", "max_new_tokens", "decode_text", "spk_bounds"):
            inputs.pop(k, None)
        from types import SimpleNamespace
        return SimpleNamespace(hidden_states=(tuple(self.prompt(input_ids, **inputs).unbind(1)),), sequences=None)


def prefill_hidden_states(model, dtype=torch.bfloat16, **inputs):
    """Convenience wrapper: [B, C, S, H] conditioning tensor of `inputs` from one forward of `model`."""
    return HiddenStateSlab(find_decoder(model), dtype).prefill(model, **inputs)
