#!/usr/bin/env python3
"""AutoencoderKL.decode of this tree against decode of another revision's x2i_amd/vae.py on the same device: same random weights, same
latents, the outputs compared bit for bit (shape, strides and values).  The other file is loaded as a module of this package, so it runs on
this tree's library and ops.
  git show HEAD~1:x2i_amd/vae.py > /tmp/parent_vae.py && python tools/vae_decode_ab.py --other /tmp/parent_vae.py"""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (((128, 128), 1, [(2, 16, 16), (2, 24, 16)]), ((128, 256, 512, 512), 2, [(1, 16, 16), (2, 32, 32)]))   # block_out_channels, layers, [B, h, w]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other", required=True, help="the other revision's vae.py")
    args = ap.parse_args()
    import torch

    from x2i_amd import vae as new
    spec = importlib.util.spec_from_file_location("x2i_amd._other_vae", args.other)
    old = importlib.util.module_from_spec(spec)
    sys.modules["x2i_amd._other_vae"] = old
    spec.loader.exec_module(old)
    ok = True
    for boc, lpb, shapes in CASES:
        a = new.AutoencoderKL(block_out_channels=boc, layers_per_block=lpb, device="cuda").init_random_(11)
        b = old.AutoencoderKL(block_out_channels=boc, layers_per_block=lpb, device="cuda").init_random_(11)
        for B, h, w in shapes:
            z = (torch.randn((B, 16, h, w), generator=torch.Generator().manual_seed(h + w)) * 1.5).to(torch.bfloat16).cuda()
            ya, yb = a.decode(z, return_dict=False)[0], b.decode(z, return_dict=False)[0]
            same = ya.shape == yb.shape and ya.stride() == yb.stride() and bool(torch.equal(ya, yb))
            ok &= same
            print("decode %s layers %d z %s: this tree == other: %s (std %.3f)" % (boc, lpb, (B, 16, h, w), same, float(ya.float().std())), flush=True)
    torch.cuda.synchronize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
