#!/usr/bin/env python3
"""Time the T5 encoder on the HIP path (x2i_amd.t5.T5EncoderModel) against transformers.T5EncoderModel, both in bf16 on the same GPU with the
same random weights:
  xxl     the T5-XXL encoder (24 layers, d_model 4096, 64 heads x 64, d_ff 10240) at B = 1 and 4, S = 512 -- the distillation teacher's
          prompt encoder (train/train_qwenvl.py:666,778)
  legacy  the legacy projector heads' stack (4 layers, d_model 896, 12 heads x 64, d_ff 3584) on 29 sequences of 512 (model_internvl/proj.py)
Device events around each forward, every shape warmed up on both sides, REPS alternating repetitions (HIP, library, HIP, ...), median and
min .. max per side.  `--only hip` runs the HIP side alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/t5_bench.py
--only hip --reps 3).  Output: stdout and, with --log, a file (profiles/t5_encoder_bench.log)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd.t5 import T5EncoderModel  # noqa: E402

CONFIGS = {
    "xxl": (dict(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=24, vocab_size=32128), [(1, 512), (4, 512)]),
    "legacy": (dict(d_model=896, d_kv=64, num_heads=12, d_ff=3584, num_layers=4, vocab_size=32128), [(29, 512)]),
}


def encoder_flops(c, B, S):
    """multiply-adds x 2 of one forward: the four projections, the two score products and the three feed-forward linears per layer"""
    inner = c["num_heads"] * c["d_kv"]
    per_tok = 2 * (4 * c["d_model"] * inner + 3 * c["d_model"] * c["d_ff"]) + 4 * S * inner
    return c["num_layers"] * B * S * per_tok


def library_encoder(c):
    from transformers import T5Config, T5EncoderModel as LibraryEncoder
    cfg = T5Config(num_decoder_layers=0, layer_norm_epsilon=1e-6, is_encoder_decoder=False, is_decoder=False, dense_act_fn="gelu_new",
                   feed_forward_proj="gated-gelu", use_cache=False, **c)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            return LibraryEncoder(cfg).eval().requires_grad_(False)
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
    ap.add_argument("--configs", default="xxl,legacy")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("both", "hip"), default="both")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("t5_bench: no GPU visible; there is nothing to time on the CPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("t5_bench: %s, torch %s, reps %d (alternating), warm-up %d per shape and side" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.warmup))
    for name in a.configs.split(","):
        c, shapes = CONFIGS[name]
        hip = T5EncoderModel(device="cuda", **c)
        hip.encoder.init_random_(0)
        lib = None
        if a.only == "both":
            lib = library_encoder(c)
            sd = hip.state_dict()
            missing, unexpected = lib.load_state_dict(sd, strict=False)
            assert not unexpected and all("embed_tokens" in k or k == "shared.weight" for k in missing), (missing, unexpected)
        for B, S in shapes:
            ids = torch.randint(0, c["vocab_size"], (B, S), generator=torch.Generator().manual_seed(B * 1000 + S)).cuda()
            sides = [("hip", lambda: hip(ids)[0])] + ([("lib", lambda: lib(ids)[0])] if lib is not None else [])
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
            fl = encoder_flops(c, B, S)
            for k, _ in sides:
                med = statistics.median(ms[k])
                say("%-6s B=%d S=%d %-3s: median %.3f ms (min %.3f .. max %.3f, %d reps), %.1f TFLOP/s whole forward"
                    % (name, B, S, k, med, min(ms[k]), max(ms[k]), len(ms[k]), fl / (med * 1e-3) / 1e12))
            if lib is not None:
                d = (out["hip"].float() - out["lib"].float()).norm() / out["lib"].float().norm()
                say("%-6s B=%d S=%d    : library / HIP time %.2f x; outputs differ by rel-L2 %.3e (two bf16 paths)"
                    % (name, B, S, statistics.median(ms["lib"]) / statistics.median(ms["hip"]), float(d)))
        del hip, lib
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
