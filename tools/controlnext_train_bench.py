"""ControlNeXtTrainer at the reference's shape: 19 control nets (train_lightcontrol.py:572-577) on a 1024^2 hint, B = 1 and 2.  HIP-event times of
forward-with-saves, backward and step, peak memory, and the achieved rate against the algorithmic FLOPs: forward 437 GFLOP per net per image
(SURVEY.md section 2a), backward counted as 2 x 437 minus the stem's data gradient (the hint takes none: 2 * 64 * 27 MACs per output pixel of the
stem, 0.057 GFLOP per net per image at 1024^2) = 873.9 GFLOP.  Prints one JSON line per batch size.

    python tools/controlnext_train_bench.py [--nets 19] [--size 1024] [--batches 1,2] [--iters 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FWD_GFLOP = 437.0
STEM_DGRAD_GFLOP = 2 * 64 * 27 * 512 * 512 / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", type=int, default=19)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--use_8bit_adam", action="store_true", help="block-wise 8-bit AdamW moments (stands where the reference selects bnb.optim.AdamW8bit; here x2i_amd.optim.FlatAdamW8bit on HIP)")
    a = ap.parse_args()
    from oracle import flux as OF
    from x2i_amd.lightcontrol import ControlNeXtModel
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    nets = []
    for i in range(a.nets):
        m = ControlNeXtModel(device="cuda")
        m.load_state_dict({k: v.to(torch.bfloat16) for k, v in OF.random_controlnext_state_dict(seed=i).items()}, strict=True)
        m.compose = False
        nets.append(m)
    tr = ControlNeXtTrainer(nets, use_8bit_adam=a.use_8bit_adam)
    scale = (a.size / 1024) ** 2
    for B in [int(b) for b in a.batches.split(",")]:
        hint = torch.rand((B, 3, a.size, a.size), device="cuda") * 2 - 1
        t = torch.tensor([500.0], device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        times = []
        torch.cuda.reset_peak_memory_stats()
        for it in range(a.iters + 1):
            ev[0].record()
            outs = tr.forward(hint, t)
            ev[1].record()
            tr.backward([torch.randn_like(o, dtype=torch.float32).to(torch.bfloat16) * 1e-3 for o in outs])
            ev[2].record()
            tr.step()
            ev[3].record()
            torch.cuda.synchronize()
            if it:
                times.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
        med = [sorted(c)[len(c) // 2] for c in zip(*times)]
        fwd = FWD_GFLOP * scale * a.nets * B
        bwd = (2 * FWD_GFLOP - STEM_DGRAD_GFLOP) * scale * a.nets * B
        print(json.dumps(dict(nets=a.nets, size=a.size, B=B, forward_ms=round(med[0], 2), backward_ms=round(med[1], 2), step_ms=round(med[2], 2),
                              forward_tflops=round(fwd / med[0], 1), backward_tflops=round(bwd / med[1], 1),
                              peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), gflop_forward=round(fwd, 1),
                              gflop_backward=round(bwd, 1))), flush=True)


if __name__ == "__main__":
    main()
