#!/usr/bin/env python3
"""Generator of tests/golden/internvit_tiny.safetensors: InternVisionModel and the chat model's extract_feature of the reference tree, run on
the CPU in float64.

Runs only where the reference tree is (--reference DIR, the tree make_golden.py reads); the fixture it writes is data only: a random state
dict, an input, and what the reference's modules make of them.  Nothing of the reference's source text is written anywhere.
tests/test_internvit_ref_cpu.py reads the fixture; tests/internvit_ref.py restates the modules and must meet the recorded outputs to 1e-10
(both sides float64, other summation order).

Configuration (tests/internvit_ref.py: TINY): hidden 128, 2 heads, 2 layers, intermediate 256, image 56 / patch 14 (grid 4 x 4, 17 tokens),
H_llm 192, B = 2, random ls1 / ls2, ps_version v2, select_layer -1.  Recorded: the state dict (the matrices as one byte per weight and a
power-of-two step, tests/internvit_ref.py: pack_state_dict), the input, last_hidden_state, hidden_states[-2] and the extract_feature
output at the native grid; and for one 84 x 84 input (grid 6 x 6) the interpolated position table and last_hidden_state.  The
restatement's pixel_shuffle index expression is compared with the reference's function here, under v1 and v2, bit for bit.
"""
import argparse
import os
import sys
import types

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import internvit_ref as IR  # noqa: E402

SEED, B = 30, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("X2I_REFERENCE"), help="root of the reference tree (or $X2I_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(HERE, "internvit_tiny.safetensors"))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "model_internvl", "internvl")):
        raise SystemExit("make_internvit_golden: give the reference tree with --reference DIR (it holds model_internvl/internvl/)")
    sys.path.insert(0, args.reference)
    # the reference module imports timm's DropPath, which it never builds at drop_path_rate 0, and einops' rearrange, which only its
    # flash-attention branch calls; lend it stand-ins for whichever of the two is not installed, before it is imported
    import importlib.machinery
    import transformers  # noqa: F401  (before the stand-ins: it probes for timm while it loads)
    for name, attr in (("timm.models.layers", "DropPath"), ("einops", "rearrange")):
        try:
            __import__(name)
        except ImportError:
            parts = name.split(".")
            for i in range(1, len(parts) + 1):
                sub = ".".join(parts[:i])
                if sub not in sys.modules:
                    sys.modules[sub] = types.ModuleType(sub)
                    sys.modules[sub].__spec__ = importlib.machinery.ModuleSpec(sub, None)
            setattr(sys.modules[name], attr, torch.nn.Identity)
    from model_internvl.internvl.configuration_intern_vit import InternVisionConfig
    from model_internvl.internvl.modeling_intern_vit import InternVisionModel
    from model_internvl.internvl.modeling_internvl_chat import InternVLChatModel
    c = IR.TINY
    cfg = InternVisionConfig(hidden_size=c["hidden_size"], num_attention_heads=c["num_attention_heads"], num_hidden_layers=c["num_hidden_layers"],
                             intermediate_size=c["intermediate_size"], image_size=c["image_size"], patch_size=c["patch_size"],
                             layer_norm_eps=c["layer_norm_eps"], hidden_act=c["hidden_act"], norm_type=c["norm_type"],
                             qk_normalization=c["qk_normalization"], qkv_bias=c["qkv_bias"], use_flash_attn=False, drop_path_rate=0.0)
    sd = IR.fixture_state_dict(c, IR.TINY_LLM, SEED)
    vit = InternVisionModel(cfg)
    vit.load_state_dict({k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}, strict=True)
    vit = vit.double().eval()
    D = c["hidden_size"]
    mlp1 = torch.nn.Sequential(torch.nn.LayerNorm(4 * D), torch.nn.Linear(4 * D, IR.TINY_LLM), torch.nn.GELU(), torch.nn.Linear(IR.TINY_LLM, IR.TINY_LLM))
    mlp1.load_state_dict({k[len("mlp1."):]: v for k, v in sd.items() if k.startswith("mlp1.")}, strict=True)
    mlp1 = mlp1.double().eval()

    def chat(ps_version, select_layer):
        """the chat model's own pixel_shuffle / extract_feature on a stand-in for `self` that holds what they read"""
        me = types.SimpleNamespace(ps_version=ps_version, select_layer=select_layer, downsample_ratio=0.5, vision_model=vit, mlp1=mlp1)
        me.pixel_shuffle = lambda x, scale_factor=0.5: InternVLChatModel.pixel_shuffle(me, x, scale_factor=scale_factor)
        return me

    x = IR.random_pixels(B, c["image_size"], SEED + 1)
    x6 = IR.random_pixels(1, 84, SEED + 2)
    with torch.no_grad():
        out = vit(pixel_values=x.double(), output_hidden_states=True, return_dict=True)
        feat = InternVLChatModel.extract_feature(chat("v2", -1), x.double())
        g = c["image_size"] // c["patch_size"]
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            shuffled_v1 = chat("v1", -1).pixel_shuffle(out.last_hidden_state[:, 1:, :].reshape(B, g, g, -1), scale_factor=0.5)
        pos6 = vit.embeddings._get_pos_embed(vit.embeddings.position_embedding[:, 1:, :], 6, 6)
        last6 = vit(pixel_values=x6.double(), return_dict=True).last_hidden_state
    assert out.last_hidden_state.dtype == torch.float64 and out.last_hidden_state.shape == (B, 1 + g * g, D)
    assert feat.shape == (B, (g // 2) ** 2, IR.TINY_LLM) and bool(torch.isfinite(feat).all()) and last6.shape == (1, 37, D)
    # ps_version v1 is a pure permutation: the restatement's index expression is checked here, against the reference's function, bit for bit
    # (and v2 with it), so nothing of it needs recording
    tokens = out.last_hidden_state[:, 1:, :]
    assert torch.equal(IR.shuffle_gather(tokens, g, v1=True), shuffled_v1.reshape(B, -1, 4 * D))
    assert torch.equal(IR.shuffle_gather(tokens, g), chat("v2", -1).pixel_shuffle(tokens.reshape(B, g, g, -1), scale_factor=0.5).reshape(B, -1, 4 * D))
    assert pos6.dtype == torch.float64 and torch.equal(pos6.float().double(), pos6)      # (float32 values: the interpolation runs in float32)
    tensors = IR.pack_state_dict(sd)
    tensors.update({"x": x.bfloat16(), "x6": x6.bfloat16(), "last_hidden_state": out.last_hidden_state.contiguous(),
                    "hidden_m2": out.hidden_states[-2].contiguous(), "extract_feature": feat.contiguous(),
                    "pos_6x6": pos6.float().contiguous(), "last_hidden_state_6x6": last6.contiguous()})
    save_file(tensors, args.out, metadata=dict(llm=str(IR.TINY_LLM), seed=str(SEED), ps_version="v2", select_layer="-1"))
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
