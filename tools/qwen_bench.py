#!/usr/bin/env python3
"""Time the Qwen2 decoder prefill on the HIP path (x2i_amd.qwen.Qwen2DecoderStack) against transformers' Qwen2Model, both in bf16 on the same
GPU with the same random weights, both as ONE prefill forward over `inputs_embeds` that returns every hidden state (the HIP side as the
[B, C, S, H] slab it writes in place; the library as its `hidden_states` tuple, without the stack / hook copies the hand-off adds to it):
  7b   Qwen2.5-7B's decoder (28 layers, hidden 3584, 28 q / 4 kv heads of 128, d_ff 18944) at B = 1 and 4, S = 512 -- Qwen2.5-VL 7B, MiniCPM-o
  3b   Qwen2.5-3B's decoder (36 layers, hidden 2048, 16 q / 2 kv heads of 128, d_ff 11008) at B = 1, S = 512 -- Qwen2.5-VL 3B, InternVL2.5-4B
The comparator is the library: the code this stage runs today.  Device events around each forward, every shape warmed up on both sides,
REPS alternating repetitions (HIP, library, HIP, ...), median and min .. max per side.  `--only hip` runs the HIP side alone (for a kernel
trace: rocprofv3 --kernel-trace --stats -- python tools/qwen_bench.py --only hip --reps 3 --configs 7b --batches 1).  Output: stdout and, with --log, a file
(profiles/qwen_decoder_bench.log)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd.qwen import Qwen2DecoderStack  # noqa: E402

# (the token table is not part of the timed forward: both sides take inputs_embeds; a small one keeps the two copies of the weights apart)
CONFIGS = {
    "7b": (dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, num_hidden_layers=28, vocab_size=1024),
           [(1, 512), (4, 512)]),
    "3b": (dict(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, intermediate_size=11008, num_hidden_layers=36, vocab_size=1024),
           [(1, 512)]),
}


def decoder_flops(c, B, S):
    """multiply-adds x 2 of one forward: the four projections, the causal half of the two score products and the three MLP linears per layer"""
    D, F = c["hidden_size"], c["intermediate_size"]
    dk = D // c["num_attention_heads"]
    nq, nkv = c["num_attention_heads"] * dk, c["num_key_value_heads"] * dk
    per_tok = 2 * (D * (nq + 2 * nkv) + nq * D + 3 * D * F) + 2 * S * nq
    return c["num_hidden_layers"] * B * S * per_tok


def library_decoder(c):
    from transformers import Qwen2Config, Qwen2Model
    cfg = Qwen2Config(max_position_embeddings=32768, rms_norm_eps=1e-6, hidden_act="silu", use_cache=False, tie_word_embeddings=False,
                      bos_token_id=0, eos_token_id=1, pad_token_id=None, rope_parameters=dict(rope_type="default", rope_theta=1000000.0), **c)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            return Qwen2Model(cfg).eval().requires_grad_(False)
    finally:
        torch.set_default_dtype(old)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="7b,3b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("both", "hip"), default="both")
    ap.add_argument("--batches", default=None, help="comma-separated batch sizes to keep of each configuration's shapes (default: all)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qwen_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("qwen_bench: %s, torch %s, reps %d (alternating), warm-up %d per shape and side" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.warmup))
    for name in a.configs.split(","):
        c, shapes = CONFIGS[name]
        hip = Qwen2DecoderStack(device="cuda", **c).init_random_(0)
        lib = None
        if a.only == "both":
            lib = library_decoder(c)
            lib.load_state_dict(hip.state_dict(), strict=True)
        for B, S in shapes:
            if a.batches is not None and str(B) not in a.batches.split(","):
                continue
            x = torch.randn((B, S, c["hidden_size"]), generator=torch.Generator().manual_seed(B * 1000 + S)).bfloat16().cuda()
            sides = [("hip", lambda: hip(inputs_embeds=x, check_mask=False))]
            if lib is not None:
                sides.append(("lib", lambda: lib(inputs_embeds=x, output_hidden_states=True, use_cache=False).hidden_states))
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
            fl = decoder_flops(c, B, S)
            for k, _ in sides:
                med = statistics.median(ms[k])
                say("%-3s B=%d S=%d %-3s: median %.3f ms (min %.3f .. max %.3f, %d reps), %.1f TFLOP/s whole forward"
                    % (name, B, S, k, med, min(ms[k]), max(ms[k]), len(ms[k]), fl / (med * 1e-3) / 1e12))
            if lib is not None:
                last = out["lib"][-1].float()
                d = (out["hip"][:, -1].float() - last).norm() / last.norm()
                say("%-3s B=%d S=%d    : library / HIP time %.2f x; last hidden states differ by rel-L2 %.3e (two bf16 paths)"
                    % (name, B, S, statistics.median(ms["lib"]) / statistics.median(ms["hip"]), float(d)))
            out.clear()
        del hip, lib
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
