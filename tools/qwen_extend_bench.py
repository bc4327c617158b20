#!/usr/bin/env python3
"""Time the Qwen2 prompt extension (Qwen2DecoderStack.extend, include/x2i_qwen_extend.h) against a whole prefill of the same total length,
on the 7B decoder's shape (28 layers, hidden 3584, 28 q / 4 kv heads of 128, d_ff 18944) with random weights, B = 1: a cache that holds P
keys, P in {512, 2048, 4096}, and a chunk of n new rows, n in {64, 160, 512}.

Per point, in one process:
  stack      extend(cache, keep=P, the last n rows) and prefill(cache, all P + n rows), alternating, each call between two device events;
             both warmed up at the point's shapes first; median and min .. max over --reps.  The chunk's rows of the two are compared
             (rel-L2) before anything is timed: faster and different is not faster
  attention  one layer's launch alone: x2i_qwen_extend_attention_bf16 on rows P .. P + n - 1 and x2i_qwen_attention_bf16 on all P + n rows
             of the same cache, alternating, --inner launches between two events (a single launch is tens of microseconds)
The extension's attention has no split of the key axis: at n = 160 two query blocks per head walk every key tile of the cache, 56
workgroups on 256 compute units.  This tool is where that cost is read.
Output: stdout and, with --log, a file (profiles/qwen_extend_bench.log)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import qwen_extend_ops as qx  # noqa: E402
from x2i_amd import qwen_ops  # noqa: E402
from x2i_amd.qwen import Qwen2DecoderStack  # noqa: E402

CONFIG = dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, num_hidden_layers=28, vocab_size=1024)


def event_ms(fn, inner=1):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / inner


def alternate(a, b, reps, inner=1, warm=2):
    """(ms of a, ms of b): warm-up of both, then a, b, a, b, ... each between its own pair of device events"""
    for _ in range(warm):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(a, inner))
        tb.append(event_ms(b, inner))
    return ta, tb


def verdict(new, old):
    m_new, m_old = statistics.median(new), statistics.median(old)
    if max(new) < min(old):
        return "faster by more than the spread"
    return "NOT faster" if m_new >= m_old else "faster, within the spread"


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cached", default="512,2048,4096", help="cached lengths P")
    ap.add_argument("--chunks", default="64,160,512", help="chunk lengths n")
    ap.add_argument("--layers", type=int, default=CONFIG["num_hidden_layers"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="attention launches between two events")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qwen_extend_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    Ps, ns = [int(v) for v in a.cached.split(",")], [int(v) for v in a.chunks.split(",")]
    c = dict(CONFIG, num_hidden_layers=a.layers)
    say("qwen_extend_bench: %s, torch %s, 7B decoder shape with %d layers, random weights, B = 1, %d reps (attention: %d launches per event pair), "
        "extend and prefill alternating" % (torch.cuda.get_device_name(0), torch.__version__, a.layers, a.reps, a.inner))
    stack = Qwen2DecoderStack(**c, device="cuda").init_random_(0)
    D, Hq, Hkv, dk = c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], 128
    cache = stack.new_cache(1, max(Ps) + max(ns) + 1)
    cap = cache.cap
    g = torch.Generator(device="cuda").manual_seed(1)
    x_all = torch.randn((1, max(Ps) + max(ns), D), device="cuda", generator=g).bfloat16()
    ATT = torch.empty((max(Ps) + max(ns), Hq * dk), device="cuda", dtype=torch.bfloat16)
    for P in Ps:
        for n in ns:
            S = P + n
            x, pos = x_all[:, :S], torch.arange(S, device="cuda")[None]
            whole = lambda: stack.prefill(cache, inputs_embeds=x, position_ids=pos, check_mask=False)
            chunk = lambda: stack.extend(cache, P, inputs_embeds=x[:, P:], position_ids=pos[:, P:], check=False)
            want = whole()[:, :, P:].clone()
            got = chunk()
            e = rel_l2(got, want)
            if e > 0:      # two roundings of one function grow apart layer by layer; a wrong row would be far off after the first
                say("P=%-4d n=%-3d stack    : the chunk's rows of extend and prefill differ: rel-L2 %.2e after layer 1, %.2e after layer 2, %.2e at the "
                    "final norm" % (P, n, rel_l2(got[:, 1], want[:, 1]), rel_l2(got[:, 2], want[:, 2]), rel_l2(got[:, -1], want[:, -1])))
                # whose rounding moved?  Rows < P of a causal pass are a function of those rows alone, with or without the rows after them
                head = stack(inputs_embeds=x[:, :P], position_ids=pos[:, :P], check_mask=False)
                full = whole()
                say("P=%-4d n=%-3d stack    : ... and rows < %d of the prefill of %d against a prefill of those %d rows alone: rel-L2 %.2e after layer 1, "
                    "%.2e at the final norm (the GEMMs' summation order depends on M)" % (P, n, P, S, P, rel_l2(full[:, 1, :P], head[:, 1]),
                                                                                           rel_l2(full[:, -1, :P], head[:, -1])))
                del head, full
            t_ext, t_pre = alternate(chunk, whole, a.reps)
            m_ext, m_pre = statistics.median(t_ext), statistics.median(t_pre)
            say("P=%-4d n=%-3d stack    : extend %8.3f ms (min %.3f .. max %.3f)   prefill of %4d %8.3f ms (min %.3f .. max %.3f)   prefill / extend %.2f x: %s; "
                "the chunk's rows of the two differ by rel-L2 %.2e" % (P, n, m_ext, min(t_ext), max(t_ext), S, m_pre, min(t_pre), max(t_pre), m_pre / m_ext,
                                                                      verdict(t_ext, t_pre), e))
            Q, K, VT, scale = cache.Q, cache.K[0], cache.VT[0], dk ** -0.5
            att_ext = lambda: qx.attention(Q, K, VT, ATT, 1, Hq, Hkv, P, n, cap, dk, scale, Hq * dk, n * Hq * dk)
            att_all = lambda: qwen_ops.attention(Q, K, VT, ATT, 1, Hq, Hkv, S, cap, dk, scale, Hq * dk, S * Hq * dk)
            u_ext, u_all = alternate(att_ext, att_all, a.reps, a.inner)
            say("P=%-4d n=%-3d attention: extend %8.1f us (min %.1f .. max %.1f)   all %4d rows %8.1f us (min %.1f .. max %.1f)   all / extend %.2f x: %s; "
                "%d workgroups against %d" % (P, n, statistics.median(u_ext) * 1e3, min(u_ext) * 1e3, max(u_ext) * 1e3, S, statistics.median(u_all) * 1e3,
                                              min(u_all) * 1e3, max(u_all) * 1e3, statistics.median(u_all) / statistics.median(u_ext),
                                              verdict(u_ext, u_all), ((S + 127) // 128 - P // 128) * Hq, (S + 127) // 128 * Hq))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
