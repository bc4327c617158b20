#!/usr/bin/env python3
"""Time the Whisper log-mel front end on the HIP path (x2i_amd.logmel.LogMel) against what runs without it for the same input:
transformers' WhisperFeatureExtractor called as the MiniCPM-o processor calls it (sampling_rate=16000, padding="max_length",
return_attention_mask=True, return_tensors="pt": float32 on the host, torch.stft on the CPU's threads) followed by .to(device).
  5 s       one waveform of 80000 samples
  30 s      one chunk of 480000 samples
  4 x 30 s  four chunks
Three sides per case, each a host clock around work that ends in a device synchronise: `hip` (host waveforms: the pinned copy, the one
transfer, the two launches), `hip_dev` (the waveforms already on the device: no transfer) and `host` (the extractor and the copy of its
features to the device).  Every side is warmed up, then REPS interleaved repetitions (hip, hip_dev, host, hip, ...); median and
min .. max per side.  Beside them the two kernels' device times from device events around each launch, and the outputs' agreement.
No speed target: the result is stated as it falls.  Run it under a time limit (timeout -k 10 300 python tools/logmel_bench.py --log
profiles/logmel_bench.log)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd import logmel_binding as lb  # noqa: E402
from x2i_amd.logmel import LogMel  # noqa: E402

CASES = [("5 s", 80000, 1), ("30 s", 480000, 1), ("4 x 30 s", 480000, 4)]      # (label, samples, waveforms)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def fmt(xs):
    return "%8.3f ms  (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("logmel_bench: needs a GPU")
    from transformers import WhisperFeatureExtractor
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fe = WhisperFeatureExtractor()
    lm = LogMel.from_hf(fe, "cuda")
    say("logmel_bench: %s, torch %s, %d CPU threads for the host side, reps %d, warm-up %d"
        % (torch.cuda.get_device_name(0), torch.__version__, torch.get_num_threads(), args.reps, args.warmup))
    for label, n, B in CASES:
        rng = np.random.default_rng(n + B)
        waves = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(B)]
        dev_waves = [torch.from_numpy(w).cuda() for w in waves]
        plan_h, plan_d = lm.plan(B, n), lm.plan(B, n)
        sides = [
            ("hip", lambda: lm(waves, plan=plan_h)[0]),
            ("hip_dev", lambda: lm(dev_waves, plan=plan_d)[0]),
            ("host", lambda: fe(waves, sampling_rate=16000, return_attention_mask=True, padding="max_length",
                                return_tensors="pt")["input_features"].to("cuda")),
        ]
        times, outs = {k: [] for k, _ in sides}, {}
        for _ in range(args.warmup):
            for k, fn in sides:
                wall(fn)
        for _ in range(args.reps):
            for k, fn in sides:
                ms, outs[k] = wall(fn)
                times[k].append(ms)
        L = lm.lengths([n])[0]
        say()
        say("%s: B = %d, %d samples each (%.2f MB of waveform, %.2f MB of float32 features [%d, 80, 3000])"
            % (label, B, n, 4e-6 * n * B, 4e-6 * B * 80 * 3000, B))
        for k, _ in sides:
            say("  %-8s %s" % (k, fmt(times[k])))
        say("  host / hip = %.1fx, host / hip_dev = %.1fx (medians)"
            % (statistics.median(times["host"]) / statistics.median(times["hip"]), statistics.median(times["host"]) / statistics.median(times["hip_dev"])))
        say("  largest difference hip - host over the %d kept frames: %.3g; hip == hip_dev bit for bit: %s"
            % (L, float((outs["hip"][:, :, :L] - outs["host"][:, :, :L]).abs().max()), torch.equal(outs["hip"], outs["hip_dev"])))
        # the two kernels alone, device events around each launch
        out = torch.empty((B, lm.n_mels, L), dtype=torch.float32, device="cuda")
        spec = lambda: lb.spectrum(plan_d.wave, plan_d.n, lm.dft, lm.fbank, plan_d.lg, plan_d.part, lm.n_samples, lm.n_mels)   # noqa: E731
        fin = lambda: lb.finish(plan_d.lg, plan_d.part, plan_d.n, out, lm.n_samples, lm.n_mels)                              # noqa: E731
        for _ in range(args.warmup):
            spec(), fin()
        ks, kf = [], []
        for _ in range(args.reps):
            ks.append(device_ms(spec))
            kf.append(device_ms(fin))
        frames = B * lb.seen_frames(n, lm.n_samples)
        flop = frames * 2.0 * (400 * 402 + 201 * lm.n_mels)
        say("  logmel_spectrum_kernel %s   %.2f GFLOP of DFT and filter bank needed -> %.1f TFLOP/s" % (fmt(ks), flop * 1e-9, flop / statistics.median(ks) * 1e-9))
        say("  logmel_finish_kernel   %s" % fmt(kf))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
