#!/usr/bin/env python3
"""Generator of tests/golden/resampler_tiny.safetensors: the MiniCPM-o Resampler of the reference tree, run on the CPU in float64.

Runs only where the reference tree is (--reference DIR, the tree make_golden.py reads); the fixture it writes is data only: a random state
dict, an input, the grids, the reference module's output and the slices of its float32 position table that the grids index.  Nothing of
the reference's source text is written anywhere.  tests/test_resampler_ref_cpu.py reads the fixture; tests/resampler_ref.py restates the
module in float64 and must meet the recorded output to 1e-10 (both sides float64, other summation order).

Configuration: embed 256, 2 heads, kv_dim 64, 8 queries, a padded batch of grids (3, 5) and (2, 2).
"""
import argparse
import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import resampler_ref as RR  # noqa: E402

EMBED, HEADS, KV_DIM, NQ, GRIDS, SEED = 256, 2, 64, 8, [(3, 5), (2, 2)], 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("X2I_REFERENCE"), help="root of the reference tree (or $X2I_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(HERE, "resampler_tiny.safetensors"))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "minicpm")):
        raise SystemExit("make_resampler_golden: give the reference tree with --reference DIR (it holds minicpm/resampler.py)")
    sys.path.insert(0, os.path.join(args.reference, "minicpm"))
    # the reference module takes names from `from torch.nn.functional import *` that newer torch no longer re-exports there; lend it
    # the ones it misses, from where they live now, before it is imported
    import builtins
    import typing
    import torch.nn.functional as F
    import torch.overrides
    lent = dict(List=typing.List, has_torch_function=torch.overrides.has_torch_function, handle_torch_function=torch.overrides.handle_torch_function)
    for name in ("_mha_shape_check", "_canonical_mask", "_none_or_dtype", "_in_projection", "_check_key_padding_mask"):
        if hasattr(F, name):
            lent[name] = getattr(F, name)
    for name, obj in lent.items():
        if not hasattr(builtins, name):
            setattr(builtins, name, obj)
    from resampler import Resampler
    ref = Resampler(num_queries=NQ, embed_dim=EMBED, num_heads=HEADS, kv_dim=KV_DIM, adaptive=True)
    sd = RR.random_state_dict(NQ, EMBED, KV_DIM, SEED)
    ref.load_state_dict(sd, strict=True)
    table = ref.pos_embed.clone()          # float32 [70, 70, D], before .double() touches the buffer
    assert table.dtype == torch.float32
    ref = ref.double().eval()
    L = max(h * w for h, w in GRIDS)
    x = RR.random_input(GRIDS, L, KV_DIM, SEED + 1)
    with torch.no_grad():
        out = ref(x.double(), torch.tensor(GRIDS, dtype=torch.int32))
    assert out.dtype == torch.float64 and out.shape == (len(GRIDS), NQ, EMBED) and bool(torch.isfinite(out).all())
    tensors = {"sd." + k: v.bfloat16().contiguous() for k, v in sd.items()}      # (exactly representable: half the bytes, the same values)
    tensors.update({"x": x, "tgt_sizes": torch.tensor(GRIDS, dtype=torch.int32), "out": out.contiguous(),
                    "pos_3x5": table[:3, :5].contiguous(), "pos_2x2": table[:2, :2].contiguous()})
    save_file(tensors, args.out, metadata=dict(embed=str(EMBED), heads=str(HEADS), kv_dim=str(KV_DIM), queries=str(NQ)))
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
