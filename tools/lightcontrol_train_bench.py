"""LightControlTrainStep at the reference's shape (lightcontrol/train_lightcontrol.py:672-775): FLUX.1-dev-sized transformer (19 + 38 blocks, guidance
embedder, frozen), 19 control nets, 1024^2 image and hint (4096 image + 512 text tokens), random weights and inputs, B = 1 and 2.  HIP-event time of
every phase of the step -- forward (conditioning, noising, control nets with saves, transformer with saves), loss head, transformer backward
(activation gradients down to injection 0), control backward (the 19 backward_net calls at their injections), optimizer (clip + AdamW) -- and
peak memory.  Prints one JSON line per batch size.

    python tools/lightcontrol_train_bench.py [--nets 19] [--layers 19] [--single 38] [--size 1024] [--text 512] [--batches 1,2] [--iters 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("forward", "loss head", "transformer backward", "control backward", "optimizer")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", type=int, default=19)
    ap.add_argument("--layers", type=int, default=19)
    ap.add_argument("--single", type=int, default=38)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--text", type=int, default=512)
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--use_8bit_adam", action="store_true", help="block-wise 8-bit AdamW moments (stands where the reference selects bnb.optim.AdamW8bit; here x2i_amd.optim.FlatAdamW8bit on HIP)")
    a = ap.parse_args()
    from oracle import flux as OF
    from x2i_amd.flux import FluxTransformer2DModel
    from x2i_amd.lightcontrol import ControlNeXtModel
    from x2i_amd.lightcontrol_step import LightControlTrainStep, sample_timesteps, sigmas_for
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    from x2i_amd.pipeline import FlowMatchEulerDiscreteScheduler
    dev = "cuda"
    m = FluxTransformer2DModel(num_layers=a.layers, num_single_layers=a.single, guidance_embeds=True, device=dev).init_random_(seed=1)
    nets = []
    for i in range(a.nets):
        n = ControlNeXtModel(device=dev)
        n.load_state_dict({k: v.to(torch.bfloat16) for k, v in OF.random_controlnext_state_dict(seed=i).items()}, strict=True)
        nets.append(n)
    tr = ControlNeXtTrainer(nets, use_8bit_adam=a.use_8bit_adam)
    step = LightControlTrainStep(m, tr)
    sched = FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=True)
    lat = a.size // 8
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(3)
        rn = lambda *s: torch.randn(s, device=dev, generator=g).bfloat16()  # noqa: E731
        ts = sample_timesteps(sched, B, torch.Generator().manual_seed(4))
        batch = dict(latents=rn(B, 16, lat, lat), noise=rn(B, 16, lat, lat), timesteps=ts, sigmas=sigmas_for(sched, ts),
                     prompt_embeds=rn(B, a.text, 4096), pooled_prompt_embeds=rn(B, 768),
                     guided_hint=torch.rand((B, 3, a.size, a.size), device=dev, generator=g) * 2 - 1)
        times = []
        torch.cuda.reset_peak_memory_stats()
        for it in range(a.iters + 1):
            marks = []

            def mark(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))
            step.mark = mark
            mark("start")
            loss = step(**batch)
            torch.cuda.synchronize()
            dt = dict.fromkeys(PHASES, 0.0)
            for (_, e0), (name, e1) in zip(marks, marks[1:]):
                dt[name] += e0.elapsed_time(e1)
            print("B = %d step %d: loss %.4f  grad norm %.4e  " % (B, it, float(loss), float(tr.last_norm[1]))
                  + "  ".join("%s %.1f" % (k, v) for k, v in dt.items()) + "  total %.1f ms" % sum(dt.values())
                  + ("  (first step: weight transposes, allocations)" if it == 0 else ""), flush=True)
            if it:
                times.append([dt[k] for k in PHASES])
        med = [sorted(c)[len(c) // 2] for c in zip(*times)]
        out = dict(nets=a.nets, layers=a.layers, single=a.single, size=a.size, text_tokens=a.text, B=B)
        out.update({k.replace(" ", "_") + "_ms": round(v, 2) for k, v in zip(PHASES, med)})
        out.update(step_ms=round(sum(med), 2), samples_per_s=round(B / (sum(med) * 1e-3), 3),
                   peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
