#!/usr/bin/env python3
"""Time the CLIP text encoder on the HIP path (x2i_amd.clip.CLIPTextModel) against transformers.CLIPTextModel, both in bf16 on the same GPU
with the same random weights, at the CLIP-L text shape (hidden 768, 12 heads x 64, 12 layers, intermediate 3072, S = 77) and B = 1, 4, 16 --
the first prompt encoder of the reference's sampling scripts and of its distillation teacher.

Per shape: device events around each forward, both sides warmed up, REPS alternating repetitions (HIP, library, HIP, ...), median and
min .. max per side.  Beside it, for the HIP side: the host time to enqueue one forward (a host clock around the call, no synchronise inside;
a forward whose enqueue takes as long as its device window is launch-bound) and the causal attention launch alone (device events around
ATT_REPS back-to-back launches on the forward's own buffers, divided by ATT_REPS).  `--only hip` runs the HIP side alone (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/clip_bench.py --only hip --reps 3).  Output: stdout and, with --log, a file
(profiles/clip_text_bench.log)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import clip_ops  # noqa: E402
from x2i_amd.clip import CLIPTextModel  # noqa: E402

CONFIG = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, vocab_size=49408, max_position_embeddings=77,
              eos_token_id=2)
SHAPES = [(1, 77), (4, 77), (16, 77)]
LAUNCHES_PER_LAYER = 9     # x2i_amd/clip.py: ln, gemm, head_split, attention, gemm, ln, gemm, quick_gelu, gemm


def forward_flops(c, B, S):
    """multiply-adds x 2 of one forward: the four projections, the two feed-forward linears and the causal half of the two score products"""
    D, F = c["hidden_size"], c["intermediate_size"]
    per_tok = 2 * (4 * D * D + 2 * D * F) + 2 * (S + 1) * D
    return c["num_hidden_layers"] * B * S * per_tok


def library_model(c):
    from transformers import CLIPTextConfig, CLIPTextModel as LibraryModel
    cfg = CLIPTextConfig(hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=0, pad_token_id=1, **c)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            return LibraryModel(cfg).eval().requires_grad_(False)
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--att-reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("both", "hip"), default="both")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    c = CONFIG
    say("clip_bench: %s, torch %s, reps %d (alternating), warm-up %d per shape and side; CLIP-L text: hidden %d, %d heads, %d layers, S 77"
        % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.warmup, c["hidden_size"], c["num_attention_heads"], c["num_hidden_layers"]))
    hip = CLIPTextModel(device="cuda", **c).init_random_(0)
    lib = None
    if a.only == "both":
        lib = library_model(c)
        # (the installed library may spell its keys with or without the `text_model.` prefix of the HIP module's)
        cut = 0 if any(n.startswith("text_model.") for n in lib.state_dict()) else len("text_model.")
        lib.load_state_dict({k[cut:]: v for k, v in hip.state_dict().items()}, strict=True)
    nlaunch = 3 + LAUNCHES_PER_LAYER * c["num_hidden_layers"]
    for B, S in SHAPES:
        ids = torch.randint(0, c["vocab_size"] - 1, (B, S), generator=torch.Generator().manual_seed(B * 1000 + S))
        ids[:, -1] = c["vocab_size"] - 1
        ids = ids.cuda()
        sides = [("hip", lambda: hip(ids).pooler_output)] + ([("lib", lambda: lib(ids).pooler_output)] if lib is not None else [])
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
            # host enqueue time of one HIP forward: the device idle before it, no synchronise inside the window
            enq = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hip(ids)
                enq.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            # the causal attention launch alone, on the forward's own buffers
            ws = hip._workspace(B, S)
            H, D = c["num_attention_heads"], c["hidden_size"]
            att = lambda: clip_ops.attention_causal(ws["Q"], ws["K"], ws["VT"], ws["ATT"], B, H, S, ws["Spad"], 64, 0.125, D, S * D)
            for _ in range(a.warmup):
                att()
            t_att, _ = timed(lambda: [att() for _ in range(a.att_reps)])
        fl = forward_flops(c, B, S)
        for k, _ in sides:
            med = statistics.median(ms[k])
            say("B=%-2d S=%d %-3s: median %.3f ms (min %.3f .. max %.3f, %d reps), %.2f TFLOP/s whole forward"
                % (B, S, k, med, min(ms[k]), max(ms[k]), len(ms[k]), fl / (med * 1e-3) / 1e12))
        med = statistics.median(ms["hip"])
        say("B=%-2d S=%d hip: %d launches, host enqueue median %.3f ms (%.1f us per launch) against the %.3f ms device window; "
            "attention alone %.1f us per launch back to back (%d workgroups), x %d layers = %.3f ms"
            % (B, S, nlaunch, statistics.median(enq), statistics.median(enq) * 1e3 / nlaunch, med, t_att * 1e3 / a.att_reps, B * H * ((S + 127) // 128),
               c["num_hidden_layers"], t_att / a.att_reps * c["num_hidden_layers"]))
        if lib is not None:
            d = (out["hip"].float() - out["lib"].float()).norm() / out["lib"].float().norm()
            say("B=%-2d S=%d    : library / HIP time %.2f x; pooled outputs differ by rel-L2 %.3e (two bf16 paths)"
                % (B, S, statistics.median(ms["lib"]) / statistics.median(ms["hip"]), float(d)))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
