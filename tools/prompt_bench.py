#!/usr/bin/env python3
"""Time the prompt hand-offs of MiniCPM-o and InternVL2.5 (x2i_amd.handoff.HipMiniCPMPrompt / HipInternVLPrompt: one merge launch of
include/x2i_merge.h, then Qwen2DecoderStack called directly, no lm_head) against the same model's own generate(max_new_tokens=1) path
with hooks on its decoder (handoff.HiddenStateSlab, what the conditioners run without --hip_decoder), both in bf16 on the same GPU with
the same random weights at the real decoder configurations:
  minicpm     Qwen2.5-7B's decoder and vocabulary; a one-image prompt (64 query rows) and a 64-frame prompt (64 x 64 rows, about 4.3 k tokens)
  internvl1b  Qwen2-0.5B's (24 layers, hidden 896, 14 q / 2 kv heads of 64), S = 512 padded, with one tile (256 context tokens) and without
  internvl4b  Qwen2.5-3B's (36 layers, hidden 2048, 16 q / 2 kv heads of 128), the same two prompts
There are no checkpoints offline, so the models around the decoders are the model-like classes of tests/test_merge_gpu.py (the models'
own bounds, context tokens, scatter, slice and masked assignments, restated) with stub towers that cost next to nothing on either side:
what is timed is everything between the towers and the projector -- token lookup, merge, decoder, and on the model's side the lm_head
and the rest of generate().  Device events around each call, every prompt warmed up on both sides, REPS alternating repetitions (hand-off,
model, hand-off, ...), median and min .. max per side.  Output: stdout and, with --log, a file (profiles/prompt_decoder_bench.log)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd.handoff import HiddenStateSlab, HipInternVLPrompt, HipMiniCPMPrompt, find_decoder  # noqa: E402
from x2i_amd.qwen import Qwen2DecoderStack  # noqa: E402

VOCAB = 151680      # a multiple of 64 at the size of Qwen2.5's tables (151646 .. 152064 over the three checkpoints)
DECODERS = {
    "minicpm": dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, num_hidden_layers=28),
    "internvl1b": dict(hidden_size=896, num_attention_heads=14, num_key_value_heads=2, intermediate_size=4864, num_hidden_layers=24),
    "internvl4b": dict(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, intermediate_size=11008, num_hidden_layers=36),
}


def causal_lm(c):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(max_position_embeddings=32768, rms_norm_eps=1e-6, hidden_act="silu", use_cache=False, tie_word_embeddings=False,
                      bos_token_id=0, eos_token_id=1, pad_token_id=None, vocab_size=VOCAB,
                      rope_parameters=dict(rope_type="default", rope_theta=1000000.0), **c)
    cfg._attn_implementation = "sdpa"
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            torch.manual_seed(0)
            lm = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    finally:
        torch.set_default_dtype(old)
    # the decoder's weights as tools/qwen_bench.py draws them (linears N(0, 1 / fan_in), token table N(0, 1)): layers that move the residual stream
    lm.model.load_state_dict(Qwen2DecoderStack(device="cuda", vocab_size=VOCAB, **c).init_random_(0).state_dict(), strict=True)
    return lm


def minicpm_prompt(frames, Q=64, ps=14, grid=(32, 32)):
    """The processor's outputs for `frames` images of 32 x 32 patches in one unpadded prompt: per frame two marker tokens around Q rows"""
    g = torch.Generator().manual_seed(frames)
    S = 24 + frames * (Q + 3) + 8
    ids = torch.randint(0, VOCAB, (1, S), generator=g)
    bounds = [[25 + i * (Q + 3), 25 + i * (Q + 3) + Q] for i in range(frames)]
    images = [torch.randn((3, ps, grid[0] * grid[1] * ps), generator=g).bfloat16() for _ in range(frames)]
    return dict(input_ids=ids.cuda(), attention_mask=torch.ones((1, S), dtype=torch.long).cuda(), pixel_values=[[i.cuda() for i in images]],
                tgt_sizes=[torch.tensor([list(grid)] * frames).cuda()], image_bound=[torch.tensor(bounds).cuda()])


def internvl_prompt(tiles, ctx, S=512, valid=300, tokens_per_tile=256):
    g = torch.Generator().manual_seed(tiles)
    ids = torch.randint(0, ctx, (1, S), generator=g)
    mask = torch.zeros((1, S), dtype=torch.long)
    mask[:, :valid] = 1
    ids[:, valid:] = 0
    if tiles:
        ids[0, 20:20 + tiles * tokens_per_tile] = ctx
    return dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), pixel_values=torch.zeros((tiles, 3, 448, 448)).cuda() if tiles else None)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def main():
    from tests.test_merge_gpu import TinyInternVL as InternVLLike, TinyMiniCPM as MiniCPMLike
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="minicpm,internvl1b,internvl4b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prompt_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("prompt_bench: %s, torch %s, reps %d (alternating), warm-up %d per prompt and side" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.warmup))
    for name in a.configs.split(","):
        lm = causal_lm(DECODERS[name])
        if name == "minicpm":
            model = MiniCPMLike(lm=lm, queries=64, patch_size=14, vision_batch_size=16).cuda().bfloat16()
            handoff = HipMiniCPMPrompt(model)
            prompts = [("1 image", minicpm_prompt(1)), ("64 frames", minicpm_prompt(64))]
            run_hip = lambda p: handoff.prompt(**p)
        else:
            model = InternVLLike(lm=lm, ctx=VOCAB - 1, tokens_per_tile=256).cuda().bfloat16()
            handoff = HipInternVLPrompt(model)
            prompts = [("text only", internvl_prompt(0, VOCAB - 1)), ("1 tile", internvl_prompt(1, VOCAB - 1))]
            run_hip = lambda p: handoff.prompt(p["input_ids"], p["attention_mask"], p["pixel_values"])
        hooks = HiddenStateSlab(find_decoder(model))
        for label, p in prompts:
            S = p["input_ids"].shape[1]
            sides = [("hip", lambda: run_hip(p)), ("own", lambda: hooks.capture(lambda: model.generate(**p)))]
            with torch.no_grad():
                for _ in range(a.warmup):
                    for _, fn in sides:
                        fn()
                torch.cuda.synchronize()
                ms = {k: [] for k, _ in sides}
                out = {}
                for _ in range(a.reps):
                    for k, fn in sides:
                        t, out[k] = timed(fn)
                        ms[k].append(t)
            for k, _ in sides:
                say("%-10s %-9s S=%-4d %-3s: median %.3f ms (min %.3f .. max %.3f, %d reps)"
                    % (name, label, S, k, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k])))
            same0 = torch.equal(out["hip"][:, 0].view(torch.int16), out["own"][:, 0].view(torch.int16))
            valid = p["attention_mask"][0].bool()
            d = []
            for entry in (1, -1):      # layer 0's output, and the final norm's
                own = out["own"][:, entry][:, valid].float()
                d.append(float((out["hip"][:, entry][:, valid].float() - own).norm() / own.norm()))
            say("%-10s %-9s S=%-4d    : model's own path / hand-off time %.2f x; layer 0's input bit-equal: %s; the valid rows of the two bf16 paths "
                "differ by rel-L2 %.3e after layer 0, %.3e after the last norm" % (name, label, S, statistics.median(ms["own"]) / statistics.median(ms["hip"]), same0, d[0], d[1]))
            out.clear()
        del model, handoff, hooks, lm
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
