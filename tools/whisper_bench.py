#!/usr/bin/env python3
"""Time the MiniCPM-o Whisper audio tower with its projector and pooling tail on the HIP path (x2i_amd.whisper.WhisperAudioTower) against
the same computation composed from transformers' Whisper modules, both in bf16 on the same GPU with the same random weights, at full
width: 24 layers of 1024 / 16 heads of 64 / 4096, projector to 3584, pooling step 2, chunks of 50 tokens:
  T = 3000   thirty seconds of audio (S = 1500 tokens), B = 1 and B = 4
  T = 500    five seconds (S = 250), B = 1 and B = 4
The library's WhisperEncoder.forward ignores the attention mask and insists on all 1500 positions, so its own submodules are called in
the model's order (conv1, conv2, the position table, every WhisperEncoderLayer with the additive mask, layer_norm, linear / ReLU / linear,
AvgPool1d), under `sdpa` and under `eager`, with the mask get_audio_embedding builds (made once per case, outside the timed region).  The
HIP side runs a planned forward (the host work of the lengths done once).  The comparator is the library: the code this stage runs today.
Device events around each call, every shape warmed up on every side, REPS interleaved repetitions (HIP, sdpa, eager, HIP, ...), median
and min .. max per side; beside each HIP figure the number of launches it enqueues and the host time of enqueuing them.  Run it under a
time limit (timeout -k 10 600 python tools/whisper_bench.py --log profiles/whisper_audio_bench.log); --max_seconds stops it from starting
further cases itself.  `--only hip` runs the HIP side alone (for a kernel trace)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd.whisper import WhisperAudioTower, conv_rows, key_ranges  # noqa: E402

TOWER = dict(d_model=1024, encoder_attention_heads=16, encoder_ffn_dim=4096, encoder_layers=24, max_source_positions=1500, embed_dim=3584, pool_step=2)
CHUNK = 50
CASES = [("T=3000 B=1", 3000, 1), ("T=3000 B=4", 3000, 4), ("T=500 B=1", 500, 1), ("T=500 B=4", 500, 4)]      # (label, mel frames, spectrograms)


class Projector(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.linear1, self.relu, self.linear2 = nn.Linear(in_dim, out_dim), nn.ReLU(), nn.Linear(out_dim, out_dim)

    def forward(self, x):
        return self.linear2(self.relu(self.linear1(x)))


def library_modules(c, attn):
    from transformers.models.whisper.configuration_whisper import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    cfg = WhisperConfig(d_model=c["d_model"], encoder_attention_heads=c["encoder_attention_heads"], encoder_ffn_dim=c["encoder_ffn_dim"],
                        encoder_layers=c["encoder_layers"], max_source_positions=c["max_source_positions"], num_mel_bins=80,
                        activation_function="gelu", decoder_layers=1, decoder_ffn_dim=8, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    cfg._attn_implementation = attn
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            return WhisperEncoder(cfg).eval().requires_grad_(False), Projector(c["d_model"], c["embed_dim"]).eval().requires_grad_(False)
    finally:
        torch.set_default_dtype(old)


def library_forward(apm, proj, pool, mel, mask, S):
    h = nn.functional.gelu(apm.conv1(mel))
    h = nn.functional.gelu(apm.conv2(h))
    h = h.permute(0, 2, 1) + apm.embed_positions.weight[:S]
    for layer in apm.layers:
        h = layer(h, mask)
        h = h[0] if isinstance(h, tuple) else h
    h = apm.layer_norm(h)
    return pool(proj(h).transpose(1, 2)).transpose(1, 2)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    host = (time.perf_counter() - w0) * 1e3
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), host, out


def compare(say, label, sides, reps, warmup, launches):
    """sides: [(name, fn)]; interleaved repetitions -> the last outputs"""
    with torch.no_grad():
        for _ in range(warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        ms, host, out = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}, {}
        for _ in range(reps):
            for k, fn in sides:
                t, h, out[k] = timed(fn)
                ms[k].append(t)
                host[k].append(h)
    for k, _ in sides:
        extra = ", %d launches" % launches if k == "hip" else ""
        say("%-12s %-5s: median %.3f ms (min %.3f .. max %.3f, %d reps), host enqueue %.3f ms%s"
            % (label, k, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k]), statistics.median(host[k]), extra))
    for k in ("sdpa", "eager"):
        if k in ms:
            say("%-12s      : library (%s) / HIP time %.2f x" % (label, k, statistics.median(ms[k]) / statistics.median(ms["hip"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=TOWER["encoder_layers"])
    ap.add_argument("--only", choices=("all", "hip"), default="all")
    ap.add_argument("--max_seconds", type=float, default=480.0, help="start no further case after this many seconds")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("whisper_bench: no GPU visible; there is nothing to time on the CPU")
    lines, start = [], time.perf_counter()

    def say(s):
        print(s, flush=True)
        lines.append(s)

    c = dict(TOWER, encoder_layers=a.layers)
    say("whisper_bench: %s, torch %s, %d layers, chunks of %d, reps %d (interleaved), warm-up %d per case and side" % (
        torch.cuda.get_device_name(0), torch.__version__, a.layers, CHUNK, a.reps, a.warmup))
    hip = WhisperAudioTower(device="cuda", **c).init_random_(0)
    libs = {}
    if a.only == "all":
        sd = hip.state_dict()
        for attn in ("sdpa", "eager"):
            apm, proj = library_modules(c, attn)
            apm.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("apm.")}, strict=True)
            proj.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("audio_projection_layer.")}, strict=True)
            libs[attn] = (apm, proj)
    pool = nn.AvgPool1d(c["pool_step"], stride=c["pool_step"])
    for label, T, B in CASES:
        if time.perf_counter() - start > a.max_seconds:
            say("%s: skipped, %.0f s have passed (--max_seconds %.0f)" % (label, time.perf_counter() - start, a.max_seconds))
            continue
        g = torch.Generator().manual_seed(T + B)
        mel = torch.randn((B, 80, T), generator=g).bfloat16().cuda()
        S, lens = conv_rows(T), [T] * B
        hi = key_ranges(lens, S, CHUNK)
        mask = torch.zeros((B, 1, S, S), dtype=torch.bfloat16)
        mask.masked_fill_(torch.arange(S)[None, None, None, :] >= hi[:, None, :, None], float("-inf"))
        mask = mask.cuda()
        plan = hip.plan(lens, T, CHUNK)
        sides = [("hip", lambda: hip(mel, plan=plan)[0])]
        for attn, (apm, proj) in libs.items():
            sides.append((attn, lambda apm=apm, proj=proj: library_forward(apm, proj, pool, mel, mask, S)))
        out = compare(say, label, sides, a.reps, a.warmup, 4 + 8 * a.layers + 4)
        if "sdpa" in out:
            d = (out["hip"].float() - out["sdpa"].float()).norm() / out["sdpa"].float().norm()
            say("%-12s      : HIP against library (sdpa) rel-L2 %.3e" % (label, float(d)))
        del out, mel, mask, plan
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
