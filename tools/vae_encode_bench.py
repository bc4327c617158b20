#!/usr/bin/env python3
"""Time the FLUX VAE encode (AutoencoderKL.encode(x).latent_dist.sample(), lightcontrol/train_lightcontrol.py:678) at 1024 x 1024 on the HIP
path: random-init encoder, B = 1 and 4 (X2I_BS="1,4"), HIP-event timing, ms per image, encode_flops and the fraction of the 2.5 PF dense bf16 peak."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x2i_amd.vae import AutoencoderKL, encode_flops  # noqa: E402

PEAK = 2.5e15
RES = int(os.environ.get("X2I_RES", "1024"))
ITERS = int(os.environ.get("X2I_ITERS", "5"))
vae = AutoencoderKL(device="cuda", with_encoder=True).init_random_(0)
fl = encode_flops(vae.config, RES, RES)
for B in [int(b) for b in os.environ.get("X2I_BS", "1,4").split(",")]:
    x = (torch.rand(B, 3, RES, RES, device="cuda") * 2 - 1).bfloat16()
    g = torch.Generator(device="cuda")
    for _ in range(2):
        z = vae.encode(x).latent_dist.sample(generator=g.manual_seed(0))
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(ITERS):
        z = vae.encode(x).latent_dist.sample(generator=g.manual_seed(0))
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / ITERS
    pf = fl * B / (ms * 1e-3) / 1e15
    print(f"vae encode B={B} {RES}^2: {ms:.2f} ms ({ms / B:.2f} ms/image), {fl / 1e12:.2f} TFLOP/image, {pf:.3f} PF = {pf * 1e15 / PEAK:.1%} of "
          f"2.5 PF; latent {tuple(z.shape)} finite={bool(torch.isfinite(z.float()).all())}")
