#!/usr/bin/env python3
"""Time Qwen2 decoding with a key/value cache on the HIP path (x2i_amd.handoff.HipGenerate over Qwen2DecoderStack.prefill / decode_step)
against transformers' own cached `generate`, both in bf16 on the same GPU, in the same process, on the same random weights:
  7b   Qwen2.5-7B's decoder (28 layers, hidden 3584, 28 q / 4 kv heads of 128, d_ff 18944) -- Qwen2.5-VL 7B, MiniCPM-o
  3b   Qwen2.5-3B's decoder (36 layers, hidden 2048, 16 q / 2 kv heads of 128, d_ff 11008) -- Qwen2.5-VL 3B, InternVL2.5-4B
as a Qwen2ForCausalLM with a small vocabulary (the lm_head stays on PyTorch on both sides and is not what is measured), prompt 512, 128
greedy tokens, B = 1 and 4.  Three sides, interleaved (HIP eager, HIP graph-replayed, library, HIP eager, ...): each is timed as a whole
generate of T tokens and of 1 token, wall clock around a synchronised call; ms per token = (t(T) - t(1)) / (T - 1), medians over --reps.
The library runs generate(do_sample=False, use_cache=True, output_hidden_states=True), what the reference runs under --use_answer.

Then, per x2i_qwen_decode_linear_bf16 shape of a step, the achieved weight bytes per second beside a copy of the same number of bytes in the
same run.  A step streams every weight once, 15 GB for the 7B, so each launch is measured over a ring of distinct weights of over 1 GB
(nothing is served from the Infinity Cache), the whole ring captured in one graph and replayed (no launch gaps of the host in it).  The copy
is torch's vectorised copy kernel over the same ring: it reads AND writes, so its rate counts both directions.
With --vocab real the models carry their real vocabularies (152064 x 3584 and 151936 x 2048: the lm_head then streams 1.09 / 0.62 GB per token
on every side) and a fourth side joins the interleave: HipGenerate(hip_head=True), graph-replayed, the head kernels of
include/x2i_qwen_head.h inside the captured step; its comparator is `hip graph`, the same loop with the torch head.  --only head times one
x2i_qwen_head_logits_argmax_bf16 + x2i_qwen_head_select pair over a ring of distinct head weights, beside torch's lm_head call (bf16
logits) and torch's copy over the same bytes.
With --w8 the e4m3 weight-only decode steps join (include/x2i_qwen_decode_w8.h, Qwen2DecoderStack.pack_w8): per layer shape a `decode_linear_w8`
line beside each `decode_linear` line -- the two rings captured in a graph each and replayed alternately in the same run, us, TB/s of the
(halved) weight bytes, the ratio to the bf16 kernel and min .. max over the reps of both -- and in the generate table a `hip w8` side
(HipGenerate(w8=True), graph-replayed, torch head) next to `hip graph`, with `hip head + w8` under --vocab real
(profiles/qwen_decode_w8_bench.log).
With --vocab real --sample the sampled step joins (include/ext/sample/x2i_sample.h): HipGenerate(hip_head=True, sample=True) under a sampling
generation_config (temperature 0.7, top-k 50, top-p 0.8, penalty 1.05) against the greedy hip_head step under the same penalty, both
graph-replayed and alternating in the same run; then the select launch alone, x2i_sample_select_f32 beside x2i_qwen_head_select on the
same scores and workspace, a graph of 16 launches each, replayed alternately, for four settings of (top_k, top_p), and the step's tail --
the head launch with the scores written plus the sampled select against the greedy pair -- over a ring of distinct head weights.
--sample_step_batches limits the batch sizes whose whole generate loops run.  --only sample runs nothing else
(profiles/qwen_sample_bench.log).
Output: stdout and, with --log, a file (profiles/qwen_decode_bench.log, profiles/qwen_head_bench.log)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import ops  # noqa: E402
from x2i_amd import qwen_decode_ops as qd  # noqa: E402
from x2i_amd import qwen_decode_w8_ops as qd8  # noqa: E402
from x2i_amd import qwen_head_ops as qh  # noqa: E402
from x2i_amd import sample_binding as sb  # noqa: E402
from x2i_amd.handoff import HipGenerate  # noqa: E402

CONFIGS = {
    "7b": dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, num_hidden_layers=28, vocab_size=1024),
    "3b": dict(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, intermediate_size=11008, num_hidden_layers=36, vocab_size=1024),
}
REAL_VOCAB = {"7b": 152064, "3b": 151936}


def library_model(c, seed=0):
    """Qwen2ForCausalLM in bf16 on the GPU with Qwen2DecoderStack.init_random_'s kind of weights"""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(max_position_embeddings=32768, rms_norm_eps=1e-6, hidden_act="silu", use_cache=True, tie_word_embeddings=False,
                      bos_token_id=0, eos_token_id=None, pad_token_id=0, rope_parameters=dict(rope_type="default", rope_theta=1000000.0), **c)
    cfg._attn_implementation = "sdpa"
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            m = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    finally:
        torch.set_default_dtype(old)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            r = torch.randn(p.shape, device=p.device, generator=gen)
            if n.endswith("norm.weight"):
                p.copy_(1.0 + 0.1 * r)
            elif p.dim() == 1:
                p.copy_(0.1 * r)
            elif "embed_tokens" in n:
                p.copy_(r)
            else:
                p.copy_(r * p.shape[1] ** -0.5)
    m.generation_config.eos_token_id = None
    m.generation_config.pad_token_id = 0
    return m


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_generate(say, name, c, batches, S, T, reps, head=False, w8=False):
    model = library_model(c)
    hg = HipGenerate(model, check_mask=False)
    for B in batches:
        ids = torch.randint(0, c["vocab_size"], (B, S), generator=torch.Generator().manual_seed(B)).cuda()
        mask = torch.ones_like(ids)
        sides = {
            "hip eager": lambda n: hg.generate(model, max_new_tokens=n, graph=False, input_ids=ids, attention_mask=mask),
            "hip graph": lambda n: hg.generate(model, max_new_tokens=n, graph=True, input_ids=ids, attention_mask=mask),
            "library": lambda n: model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=n, min_new_tokens=n, do_sample=False, use_cache=True,
                                                output_hidden_states=True, return_dict_in_generate=True),
        }
        if head:
            sides["hip head"] = lambda n: hg.generate(model, max_new_tokens=n, graph=True, hip_head=True, input_ids=ids, attention_mask=mask)
        if w8:
            sides["hip w8"] = lambda n: hg.generate(model, max_new_tokens=n, graph=True, w8=True, input_ids=ids, attention_mask=mask)
            if head:
                sides["hip head + w8"] = lambda n: hg.generate(model, max_new_tokens=n, graph=True, hip_head=True, w8=True, input_ids=ids,
                                                               attention_mask=mask)
        for fn in sides.values():       # warm-up: every side once at both lengths
            fn(T)
            fn(1)
        per = {k: [] for k in sides}
        one = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():
                tT, _ = wall(lambda: fn(T))
                t1, _ = wall(lambda: fn(1))
                per[k].append((tT - t1) / (T - 1))
                one[k].append(t1)
        for k in sides:
            say("%-3s B=%d prompt %d, %d tokens, %-13s: %.3f ms per token (min %.3f .. max %.3f, %d reps); prompt pass + first token %.1f ms"
                % (name, B, S, T, k, statistics.median(per[k]), min(per[k]), max(per[k]), reps, statistics.median(one[k])))
        lib = statistics.median(per["library"])
        say("%-3s B=%d                              : library / HIP eager %.2f x, library / HIP graph %.2f x; weights %.2f GB per token -> %.2f TB/s at the graph's rate"
            % (name, B, lib / statistics.median(per["hip eager"]), lib / statistics.median(per["hip graph"]), decoder_bytes(c) / 1e9,
               decoder_bytes(c) / (statistics.median(per["hip graph"]) * 1e-3) / 1e12))
        if head:
            h, g = statistics.median(per["hip head"]), statistics.median(per["hip graph"])
            say("%-3s B=%d                              : hip head %.3f ms against hip graph (torch head) %.3f ms per token: %+.3f ms, %.3f x; "
                "lm_head %.2f GB per token" % (name, B, h, g, h - g, g / h, c["vocab_size"] * c["hidden_size"] * 2 / 1e9))
        if w8:
            for a, b in (("hip w8", "hip graph"),) + ((("hip head + w8", "hip head"),) if head else ()):
                ta, tb = statistics.median(per[a]), statistics.median(per[b])
                say("%-3s B=%d                              : %s %.3f ms against %s %.3f ms per token: %+.3f ms, %.3f x (min .. max of the two: "
                    "%.3f .. %.3f, %.3f .. %.3f); decoder weights %.2f -> %.2f GB per token"
                    % (name, B, a, ta, b, tb, ta - tb, tb / ta, min(per[a]), max(per[a]), min(per[b]), max(per[b]), decoder_bytes(c) / 1e9,
                       decoder_bytes(c) / 2e9))
    del hg, model
    torch.cuda.empty_cache()


def decoder_bytes(c):
    D, F = c["hidden_size"], c["intermediate_size"]
    dk = D // c["num_attention_heads"]
    nq, nkv = c["num_attention_heads"] * dk, c["num_key_value_heads"] * dk
    return 2 * c["num_hidden_layers"] * (D * (nq + 2 * nkv) + nq * D + 3 * D * F)


def graph_ms(body, reps):
    """median ms of one replay of `body` captured in a graph"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    g.replay()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        g.replay()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def graph_ms_interleaved(bodies, reps):
    """per body the list of ms of one replay, the bodies captured in a graph each and replayed in turn (a, b, a, b, ...)"""
    graphs = []
    for body in bodies:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        g.replay()
        graphs.append(g)
    ms = [[] for _ in bodies]
    for _ in range(reps):
        for i, g in enumerate(graphs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            g.replay()
            t1.record()
            torch.cuda.synchronize()
            ms[i].append(t0.elapsed_time(t1))
    return ms


def bench_linears(say, name, c, batches, reps, w8=False):
    D, F = c["hidden_size"], c["intermediate_size"]
    dk = D // c["num_attention_heads"]
    nq, nkv = c["num_attention_heads"] * dk, c["num_key_value_heads"] * dk
    shapes = [("qkv + bias", nq + 2 * nkv, D, False), ("o_proj + res", D, nq, False), ("gate|up gate", F, D, True), ("down + res", D, F, False)]
    for label, N, K, gate in shapes:
        rows = 2 * N if gate else N
        nbytes = rows * K * 2
        ring = max(4, -(-(1 << 30) // nbytes))
        W = (torch.randn((ring, rows, K), device="cuda", dtype=torch.bfloat16) * K ** -0.5)
        dst = torch.empty((rows, K), device="cuda", dtype=torch.bfloat16)
        t_copy = graph_ms(lambda: [dst.copy_(W[i]) for i in range(ring)], reps) / ring
        say("%-3s %-13s N=%-5d K=%-5d %6.1f MB: copy of the same bytes %.1f us = %.2f TB/s (read + write)"
            % (name, label, N, K, nbytes / 1e6, t_copy * 1e3, 2 * nbytes / (t_copy * 1e-3) / 1e12))
        if w8:      # the same ring, quantised as pack_w8() quantises a layer's weight: distinct memory per entry, half the bytes
            q = [ops.quantize_rows_fp8(W[i]) for i in range(ring)]
            W8, S8 = torch.stack([t[0].view(torch.uint8) for t in q]), torch.stack([t[1] for t in q])
            del q
        for B in batches:
            x = torch.randn((B, K), device="cuda").bfloat16()
            res = None if gate or label.startswith("qkv") else torch.randn((B, N), device="cuda").bfloat16()
            bias = torch.randn((rows,), device="cuda").bfloat16() if label.startswith("qkv") else None
            out = torch.empty((B, N), device="cuda", dtype=torch.bfloat16)
            if w8:
                ms16, ms8 = graph_ms_interleaved([lambda: [qd.linear(x, W[i], bias, res, out=out, gate=gate) for i in range(ring)],
                                                  lambda: [qd8.linear_w8(x, W8[i], S8[i], bias, res, out=out, gate=gate) for i in range(ring)]], reps)
                us16, us8 = [t / ring * 1e3 for t in ms16], [t / ring * 1e3 for t in ms8]
                m16, m8 = statistics.median(us16), statistics.median(us8)
                say("%-3s %-13s N=%-5d K=%-5d B=%d          : decode_linear    %.1f us (min %.1f .. max %.1f) = %.2f TB/s of weight (%.2f of the copy's time)"
                    % (name, label, N, K, B, m16, min(us16), max(us16), nbytes / (m16 * 1e-6) / 1e12, m16 * 1e-3 / t_copy))
                verdict = "faster by more than the spread" if max(us8) < min(us16) else ("NOT faster" if m8 >= m16 else "faster, within the spread")
                say("%-3s %-13s N=%-5d K=%-5d B=%d          : decode_linear_w8 %.1f us (min %.1f .. max %.1f) = %.2f TB/s of weight (%.1f MB); bf16 / w8 "
                    "%.2f x: %s" % (name, label, N, K, B, m8, min(us8), max(us8), nbytes / 2 / (m8 * 1e-6) / 1e12, nbytes / 2e6, m16 / m8, verdict))
                continue
            t = graph_ms(lambda: [qd.linear(x, W[i], bias, res, out=out, gate=gate) for i in range(ring)], reps) / ring
            say("%-3s %-13s N=%-5d K=%-5d B=%d          : decode_linear %.1f us = %.2f TB/s of weight (%.2f of the copy's time)"
                % (name, label, N, K, B, t * 1e3, nbytes / (t * 1e-3) / 1e12, t / t_copy))
        del W, dst
        if w8:
            del W8, S8
        torch.cuda.empty_cache()


def bench_head(say, name, c, batches, reps):
    """one logits_argmax + select pair (no logits written, penalty 1.05 over a seen mask) per head weight of a ring, beside torch's lm_head"""
    V, K = c["vocab_size"], c["hidden_size"]
    nbytes = V * K * 2
    ring = max(4, -(-(1 << 30) // nbytes))
    W = torch.randn((ring, V, K), device="cuda", dtype=torch.bfloat16) * K ** -0.5
    dst = torch.empty((V, K), device="cuda", dtype=torch.bfloat16)
    t_copy = graph_ms(lambda: [dst.copy_(W[i]) for i in range(ring)], reps) / ring
    say("%-3s lm_head       V=%-6d K=%-5d %6.1f MB: copy of the same bytes %.1f us = %.2f TB/s (read + write); the bytes alone at the guide's 6.3 TB/s: %.1f us"
        % (name, V, K, nbytes / 1e6, t_copy * 1e3, 2 * nbytes / (t_copy * 1e-3) / 1e12, nbytes / 6.3e12 * 1e6))
    del dst
    for B in batches:
        x = torch.randn((B, K), device="cuda").bfloat16()
        ws = torch.empty((qh.workspace_floats(B, V),), device="cuda", dtype=torch.float32)
        seen = (torch.rand((B, V), device="cuda") < 0.004).to(torch.uint8)       # about 600 ids: a 512-token prompt and its answer
        step, token = torch.zeros((1,), device="cuda", dtype=torch.int32), torch.zeros((B,), device="cuda", dtype=torch.long)
        seq, lengths = torch.zeros((B, 8 * ring), device="cuda", dtype=torch.long), torch.zeros((B,), device="cuda", dtype=torch.long)
        done = torch.zeros((B,), device="cuda", dtype=torch.uint8)

        def pair(i):
            qh.logits_argmax(x, W[i], ws, seen=seen, penalty=1.05, step=step)
            qh.select(ws, step, token, seq, lengths, done, 0, V, seen=seen)

        def body():
            step.zero_()
            for i in range(ring):
                pair(i)
        t = graph_ms(body, reps) / ring
        t_torch = graph_ms(lambda: [torch.nn.functional.linear(x, W[i]) for i in range(ring)], reps) / ring
        say("%-3s lm_head       V=%-6d K=%-5d B=%d          : head kernels %.1f us = %.2f TB/s of weight; torch lm_head (bf16 logits, no penalty, no "
            "argmax) %.1f us = %.2f TB/s; head / torch %.2f" % (name, V, K, B, t * 1e3, nbytes / (t * 1e-3) / 1e12, t_torch * 1e3,
                                                                nbytes / (t_torch * 1e-3) / 1e12, t / t_torch))
    del W
    torch.cuda.empty_cache()


def bench_sample(say, name, c, batches, step_batches, S, T, reps):
    """the sampled hip_head step against the greedy one, alternating (step_batches); then, per batch size, the two select launches alone on the
    same scores, and the head launch with each of them over a ring of distinct head weights"""
    from transformers import GenerationConfig
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    model = library_model(c)
    V, K = c["vocab_size"], c["hidden_size"]
    gc = GenerationConfig(do_sample=True, temperature=0.7, top_k=50, top_p=0.8, repetition_penalty=1.05, eos_token_id=None, pad_token_id=0)
    greedy = [RepetitionPenaltyLogitsProcessor(1.05)]
    sampled = greedy + [TemperatureLogitsWarper(0.7), TopKLogitsWarper(50), TopPLogitsWarper(0.8)]
    hg = HipGenerate(model, check_mask=False, hip_head=True)
    for B in step_batches:
        ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
        mask = torch.ones_like(ids)
        sides = {
            "hip head": lambda n: hg.generate(model, max_new_tokens=n, graph=True, logits_processor=greedy, input_ids=ids, attention_mask=mask),
            "hip sample": lambda n: hg.generate(model, max_new_tokens=n, graph=True, logits_processor=sampled, generation_config=gc, sample=True, seed=0,
                                                input_ids=ids, attention_mask=mask),
        }
        for fn in sides.values():
            fn(T)
            fn(1)
        per = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():
                tT, _ = wall(lambda: fn(T))
                t1, _ = wall(lambda: fn(1))
                per[k].append((tT - t1) / (T - 1))
        for k in sides:
            say("%-3s B=%d prompt %d, %d tokens, %-10s: %.3f ms per token (min %.3f .. max %.3f, %d reps)"
                % (name, B, S, T, k, statistics.median(per[k]), min(per[k]), max(per[k]), reps))
        h, m = statistics.median(per["hip head"]), statistics.median(per["hip sample"])
        say("%-3s B=%d                              : hip sample %.3f ms against hip head (greedy) %.3f ms per token: %+.3f ms, %.3f x"
            % (name, B, m, h, m - h, m / h))
    del hg, model
    torch.cuda.empty_cache()
    nbytes = V * K * 2
    ring = max(4, -(-(1 << 30) // nbytes))
    W = torch.randn((ring, V, K), device="cuda", dtype=torch.bfloat16) * K ** -0.5
    for B in batches:
        # the select launches alone, on the scores of one head launch
        x = torch.randn((B, K), device="cuda").bfloat16()
        ws = torch.empty((qh.workspace_floats(B, V),), device="cuda", dtype=torch.float32)
        logits = torch.empty((B, V), device="cuda", dtype=torch.float32)
        step, token = torch.zeros((1,), device="cuda", dtype=torch.int32), torch.zeros((B,), device="cuda", dtype=torch.long)
        seq, lengths = torch.zeros((B, 64), device="cuda", dtype=torch.long), torch.zeros((B,), device="cuda", dtype=torch.long)
        done = torch.zeros((B,), device="cuda", dtype=torch.uint8)
        rng = sb.rng_state(0, 0, "cuda")
        seen = (torch.rand((B, V), device="cuda") < 0.004).to(torch.uint8)       # about 600 ids: a 512-token prompt and its answer
        qh.logits_argmax(x, W[0], ws, step=step, logits=logits)
        n = 16
        for top_k, top_p in ((50, 0.8), (50, 1.0), (0, 0.8), (0, 1.0)):
            ms_s, ms_g = graph_ms_interleaved(
                [lambda: [sb.select(logits, ws, step, token, seq, lengths, done, 0, temperature=0.7, top_k=top_k, top_p=top_p, rng=rng) for _ in range(n)],
                 lambda: [qh.select(ws, step, token, seq, lengths, done, 0, V) for _ in range(n)]], 10)
            us_s, us_g = [t / n * 1e3 for t in ms_s], [t / n * 1e3 for t in ms_g]
            say("%-3s select        V=%-6d B=%d top_k=%-2d top_p=%.1f: x2i_sample_select_f32 %.1f us (min %.1f .. max %.1f); x2i_qwen_head_select %.1f us "
                "(min %.1f .. max %.1f)" % (name, V, B, top_k, top_p, statistics.median(us_s), min(us_s), max(us_s), statistics.median(us_g), min(us_g),
                                           max(us_g)))

        # the tail of a step: the head launch (penalty 1.05) with the scores written and the sampled select, against the greedy pair
        def pairs(sample):
            step.zero_()
            for i in range(ring):
                qh.logits_argmax(x, W[i], ws, seen=seen, penalty=1.05, step=step, logits=logits if sample else None)
                if sample:
                    sb.select(logits, ws, step, token, seq, lengths, done, 0, temperature=0.7, top_k=50, top_p=0.8, rng=rng, seen=seen)
                else:
                    qh.select(ws, step, token, seq, lengths, done, 0, V, seen=seen)
        ms_s, ms_g = graph_ms_interleaved([lambda: pairs(True), lambda: pairs(False)], 10)
        us_s, us_g = [t / ring * 1e3 for t in ms_s], [t / ring * 1e3 for t in ms_g]
        say("%-3s head + select V=%-6d B=%d top_k=50 top_p=0.8: scores written + sampled select %.1f us (min %.1f .. max %.1f); greedy pair %.1f us "
            "(min %.1f .. max %.1f): %+.1f us per token" % (name, V, B, statistics.median(us_s), min(us_s), max(us_s), statistics.median(us_g), min(us_g),
                                                            max(us_g), statistics.median(us_s) - statistics.median(us_g)))
    del W
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="7b,3b")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("all", "generate", "linears", "head", "sample"), default="all")
    ap.add_argument("--vocab", choices=("small", "real"), default="small",
                    help="real: the models' own vocabularies, and the hip_head side in the generate table")
    ap.add_argument("--w8", action="store_true", help="add the e4m3 weight-only sides: decode_linear_w8 per shape, hip w8 (and hip head + w8) per generate")
    ap.add_argument("--sample", action="store_true", help="with --vocab real: add the sampled hip_head step against the greedy one, and the select "
                                                          "launches alone")
    ap.add_argument("--sample_step_batches", default=None,
                    help="with --sample: the batch sizes whose whole generate loops are timed (default: --batches; the launches alone are timed at "
                         "every size of --batches)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if (a.sample or a.only == "sample") and a.vocab != "real":
        raise SystemExit("qwen_decode_bench: --sample times the step over the models' own vocabularies: it needs --vocab real")
    if not torch.cuda.is_available():
        raise SystemExit("qwen_decode_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    batches = [int(b) for b in a.batches.split(",")]
    say("qwen_decode_bench: %s, torch %s, prompt %d, %d tokens, %d reps, sides interleaved, vocabulary %s"
        % (torch.cuda.get_device_name(0), torch.__version__, a.prompt, a.tokens, a.reps, a.vocab))
    real = a.vocab == "real"
    for name in a.configs.split(","):
        c = dict(CONFIGS[name], vocab_size=REAL_VOCAB[name]) if real else CONFIGS[name]
        if a.only in ("all", "generate"):
            bench_generate(say, name, c, batches, a.prompt, a.tokens, a.reps, head=real, w8=a.w8)
        if a.only in ("all", "linears"):
            with torch.no_grad():
                bench_linears(say, name, c, batches, 10, w8=a.w8)
        if a.only == "head" or (a.only == "all" and real):
            with torch.no_grad():
                bench_head(say, name, dict(CONFIGS[name], vocab_size=REAL_VOCAB[name]), batches, 10)
        if a.sample or a.only == "sample":
            bench_sample(say, name, c, batches, [int(b) for b in a.sample_step_batches.split(",") if b] if a.sample_step_batches is not None
                         else batches, a.prompt, a.tokens, a.reps)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
