#!/usr/bin/env python3
"""Interactive multi-turn Qwen2.5-VL -> image loop on the HIP path.  Counterpart of infer/inference_multi_turn.py: the
chat history grows each turn, the model answers with max_new_tokens=64, and the conditioning is the prompt-pass hidden
states concatenated along S with the generated-token hidden states (:132-141); 4 steps, 1024x1024, manual_seed(0).
With --hip_generate a turn is one handoff.HipGenerate.generate call (the decoder stack on the HIP path over the prompt and the answer),
with --hip_head its tokens are chosen on the HIP path too, and with --hip_keep_cache a turn's prompt pass runs only the tokens that the
history gained (HipGenerate(keep_cache=True): the key/value cache of the turns before stays)."""
import time

import torch

from .harness import Harness, SyntheticConditioner, build_parser, sample_seed, stack_hidden_states


class MultiTurnConditioner:
    """model / processor: hand in loaded ones (a test's tiny model and stub processor) and `path` is not read."""

    def __init__(self, path, device, hip_generate=False, hip_head=False, model=None, processor=None, hip_w8=False, keep_cache=False,
                 hip_sample=False, hip_sample_seed=0, hip_image=False):
        if hip_w8 and not hip_generate:         # (before the checkpoint is read)
            raise ValueError("--hip_w8 runs the decode steps of --hip_generate's loop on e4m3 weights: not without --hip_generate")
        if hip_sample and not (hip_generate and hip_head):
            raise ValueError("--hip_sample draws the tokens inside --hip_generate --hip_head's captured step: not without both")
        if keep_cache and not hip_generate:
            raise ValueError("--hip_keep_cache keeps the key/value cache of --hip_generate's loop between turns: not without --hip_generate")
        if model is None or processor is None:
            from transformers import AutoProcessor, Qwen2_5_VLForConditionalGeneration
            model = model if model is not None else Qwen2_5_VLForConditionalGeneration.from_pretrained(path, torch_dtype=torch.bfloat16).eval().to(device)
            processor = processor if processor is not None else AutoProcessor.from_pretrained(path)
        self.model, self.processor = model, processor
        self.device = device
        self.history = []
        self.generate = None
        if hip_head and not hip_generate:
            raise ValueError("--hip_head chooses the tokens of --hip_generate's loop: not without --hip_generate")
        if hip_generate:
            from ..handoff import HipGenerate
            if not hip_sample:
                HipGenerate.refuse_sampling(self.model.generation_config)
            self.generate = HipGenerate(self.model, hip_head=hip_head, w8=hip_w8, keep_cache=keep_cache, sample=hip_sample, seed=hip_sample_seed)
        # hip_image: the vision tower's input from the HIP path (handoff.HipQwenImage) in place of the processor's Qwen2VLImageProcessor;
        # the 256 x 256 resize of a turn's images stays on the host in front of it
        self.image = None
        if hip_image:
            from ..handoff import HipQwenImage
            self.image = HipQwenImage(self.processor, device).install()

    @torch.no_grad()
    def __call__(self, images=None, text_prompt=None, **_):
        from PIL import Image
        content, ims = [], []
        for p in images or []:
            im = Image.open(p).convert("RGB").resize((256, 256))  # :92
            content.append({"type": "image", "image": im})
            ims.append(im)
        content.append({"type": "text", "text": text_prompt})
        self.history.append({"role": "user", "content": content})
        prompt = self.processor.apply_chat_template(self.history, tokenize=False, add_generation_prompt=True)
        all_ims = [c["image"] for m in self.history if m["role"] == "user" for c in m["content"] if c["type"] == "image"]
        inputs = self.processor(text=[prompt], images=all_ims or None, return_tensors="pt").to(self.device)
        if self.generate is not None:
            gc = self.model.generation_config
            S = inputs["input_ids"].shape[1]
            out = self.generate.generate(self.model, max_new_tokens=64, eos_token_id=gc.eos_token_id, pad_token_id=gc.pad_token_id,
                                         logits_processor=self.model._get_logits_processor(gc, input_ids_seq_length=S, device=self.device), **inputs)
            answer = self.processor.batch_decode(out.sequences[:, S:], skip_special_tokens=True)[0]
            self.history.append({"role": "assistant", "content": [{"type": "text", "text": answer}]})
            if out.answer.shape[2] > 0:
                return torch.cat([out.prompt, out.answer], dim=2), answer
            return out.prompt, answer
        out = self.model.generate(**inputs, max_new_tokens=64, output_hidden_states=True, return_dict_in_generate=True)
        answer = self.processor.batch_decode(out.sequences[:, inputs.input_ids.shape[1]:], skip_special_tokens=True)[0]
        self.history.append({"role": "assistant", "content": [{"type": "text", "text": answer}]})
        prompt_hs = stack_hidden_states(out.hidden_states)
        if len(out.hidden_states) > 1:
            return torch.cat([prompt_hs, stack_hidden_states(out.hidden_states, use_answer=True)], dim=2), answer
        return prompt_hs, answer


def synthetic_turns(args, kind, device):
    """--synthetic: no checkpoints; the conversation is a list of text lengths (--turn_lengths, default: a history that grows by 37 tokens
    per turn, then the first two lengths again) and every turn prints its sampling latency -- a NEW length runs the eager launch sequence
    once (FluxPipeline's graph policy: no discarded warm-up pass), a length that comes back is captured and from then on replayed."""
    lengths = [int(x) for x in args.turn_lengths.split(",")] if args.turn_lengths else [96 + 37 * t for t in range(4)] + [96, 133, 96, 133]
    cond = SyntheticConditioner(kind, device)
    h = Harness(args, kind, cond, device)
    for turn, S in enumerate(lengths):
        cond.seq_len = S
        pooled, embeds = h.embeds(text_prompt="turn %d" % turn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.generate(pooled, embeds, "multi_turn", "turn_%d" % turn, seed=0)
        h.flush_outputs()              # (--hip_image_out: the turn's file is written before the turn is reported)
        torch.cuda.synchronize()
        st = h.pipeline.graph_stats
        print("turn %d: S_txt %4d  sampling %8.1f ms   (pipeline so far: %d eager, %d captures, %d replays)"
              % (turn, S, (time.perf_counter() - t0) * 1e3, st["eager"], st["captures"], st["replays"]), flush=True)


def main(argv=None):
    ap = build_parser("qwenvl")
    ap.add_argument("--turn_lengths", type=str, default=None, help="with --synthetic: comma-separated text lengths of the turns")
    ap.add_argument("--hip_keep_cache", action="store_true",
                    help="with --hip_generate: keep the key/value cache between turns and run only the tokens the history gained through the "
                         "prompt pass (HipGenerate(keep_cache=True), Qwen2DecoderStack.extend); the history's images must not change")
    args = ap.parse_args(argv)
    if args.hip_keep_cache and not args.hip_generate:      # (before a checkpoint is read)
        raise ValueError("--hip_keep_cache keeps the key/value cache of --hip_generate's loop between turns: not without --hip_generate")
    kind = "qwen" + args.qwen_size
    device = "cuda:0"
    torch.cuda.set_device(device)
    if args.synthetic:
        return synthetic_turns(args, kind, device)
    cond = MultiTurnConditioner(args.qwen_path, device, hip_generate=args.hip_generate, hip_head=args.hip_head, hip_w8=args.hip_w8,
                                keep_cache=args.hip_keep_cache, hip_sample=args.hip_sample, hip_sample_seed=sample_seed(args),
                                hip_image=args.hip_image)
    h = Harness(args, kind, lambda **kw: cond(**kw)[0], device)
    turn = 0
    while True:
        try:
            line = input("user (text [| image path ...], empty to quit)> ").strip()
        except EOFError:
            break
        if not line:
            break
        parts = [s.strip() for s in line.split("|")]
        pooled, embeds = h.embeds(text_prompt=parts[0], images=parts[1:] or None)
        h.generate(pooled, embeds, "multi_turn", "turn_%d" % turn, seed=0)
        h.flush_outputs()
        print("assistant>", cond.history[-1]["content"][0]["text"])
        turn += 1


if __name__ == "__main__":
    main()
