"""float64 references and helpers for the MiniCPM-o SigLIP vision tower's kernels and host module (include/x2i_siglip.h, x2i_amd/siglip.py).
No GPU-only code here: the CPU tests import it too.

  position ids  the bucketised ids of SiglipVisionEmbeddings restated as a loop over the images
  strips        an image of h x w patches <-> the one-patch-high strip the tower is called with
  tower         the whole tower restated in float64 from a state dict with the library's key names, on a padded batch of strips
  library       `transformers`' Idefics2VisionTransformer, the same module under another name, which sees each image in its 2-D form
"""
import torch

from tests.t5_ref import rel_l2  # noqa: F401  (for the tests that import this module)

SIDE = 70       # image_size 980 // patch_size 14


# ---------------------------------------------------------------------------------------------------------------- position ids
def position_ids(tgt_sizes, L, side=SIDE):
    """int64 [B, L]: for image b of (h, w) patches the first h * w entries are bucket_h * side + bucket_w of the patch's fractional
    coordinates i / h and j / w among `side` float32 boundaries, the rest (padding) 0.  The coordinates and the boundaries are float32
    aranges and the comparison is bucketize(right=True), as in the model's own code: the float rounding decides the edges."""
    out = torch.zeros((len(tgt_sizes), L), dtype=torch.int64)
    boundaries = torch.arange(1 / side, 1.0, 1 / side)
    for b, (h, w) in enumerate(tgt_sizes):
        h, w = torch.tensor(int(h), dtype=torch.int32), torch.tensor(int(w), dtype=torch.int32)
        ch, cw = torch.arange(0, 1 - 1e-6, 1 / h), torch.arange(0, 1 - 1e-6, 1 / w)
        bh, bw = torch.bucketize(ch, boundaries, right=True), torch.bucketize(cw, boundaries, right=True)
        out[b, :int(h) * int(w)] = (bh[:, None] * side + bw).flatten()
    return out


def library_position_ids(h, w, side=SIDE, patch=14):
    """The ids Idefics2VisionEmbeddings derives from an all-ones 2-D patch mask [1, h, w]: what its position table is indexed with"""
    from transformers.models.idefics2.configuration_idefics2 import Idefics2VisionConfig
    from transformers.models.idefics2.modeling_idefics2 import Idefics2VisionEmbeddings
    emb = Idefics2VisionEmbeddings(Idefics2VisionConfig(hidden_size=8, image_size=side * patch, patch_size=patch))
    seen = []
    hook = emb.position_embedding.register_forward_hook(lambda m, args, out: seen.append(args[0].clone()))
    with torch.no_grad():
        emb(torch.zeros((1, 3, h * patch, w * patch)), torch.ones((1, h, w), dtype=torch.bool))
    hook.remove()
    return seen[0].reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- strips
def strip_to_image(strip, h, w):
    """[3, P, P * n] with n >= h * w (patch p = i * w + j at columns P*p .. P*p + P-1) -> the image [3, h * P, w * P]"""
    P = strip.shape[1]
    return strip[:, :, :P * h * w].reshape(3, P, h, w, P).permute(0, 2, 1, 3, 4).reshape(3, h * P, w * P)


def image_to_strip(image, P, L=None):
    """[3, h * P, w * P] -> [3, P, P * L], the patches row by row and zeros beyond h * w (L defaults to h * w)"""
    h, w = image.shape[1] // P, image.shape[2] // P
    strip = image.reshape(3, h, P, w, P).permute(0, 2, 1, 3, 4).reshape(3, P, P * h * w)
    if L is None or L == h * w:
        return strip.contiguous()
    out = torch.zeros((3, P, P * L), dtype=image.dtype)
    out[:, :, :P * h * w] = strip
    return out


def random_strips(grids, L, P=14, seed=0):
    """(strips [B, 3, P, P * L] of N(0, 1) pixels holding bf16 values, zero in the padding patches; the 2-D images they are strips of)"""
    g = torch.Generator().manual_seed(seed)
    images = [torch.randn((3, h * P, w * P), generator=g).bfloat16().float() for h, w in grids]
    return torch.stack([image_to_strip(im, P, L) for im in images]), images


def patch_rows(strips, Kp=None):
    """[B, 3, P, P * L] -> [B * L, 3 * P * P] in the Conv2d weight's column order, with a zero tail up to Kp"""
    B, _, P, W = strips.shape
    L = W // P
    rows = strips.reshape(B, 3, P, L, P).permute(0, 3, 1, 2, 4).reshape(B * L, 3 * P * P)
    if Kp is None:
        return rows
    return torch.cat((rows, torch.zeros((B * L, Kp - 3 * P * P), dtype=strips.dtype, device=strips.device)), 1)


# ---------------------------------------------------------------------------------------------------------------- the whole tower
def gelu_tanh_f64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def tower_reference(sd, strips, tgt_sizes, *, num_heads, side=SIDE, eps=1e-6, scale_dim=None):
    """float64 restatement of the SigLIP tower from the state dict `sd` (the library's key names) on a padded batch: strips
    [B, 3, P, P * L], tgt_sizes rows (h, w).  Every row of image b attends to the keys [0, h * w).  -> last_hidden_state [B, L, D]; rows
    >= h * w of an image mean nothing.
    The head width is read off q_proj's shape, so head-padded weights (pad_heads) run as they are; scale_dim is the REAL head width of
    such weights (the softmax scale is scale_dim ** -0.5)."""
    f = torch.float64
    w = lambda k: sd[k].to(f)
    B, _, P, W = strips.shape
    L, H = W // P, num_heads
    pe = w("embeddings.patch_embedding.weight")
    D = pe.shape[0]
    x = patch_rows(strips.to(f)) @ pe.reshape(D, -1).t() + w("embeddings.patch_embedding.bias")
    x = x + w("embeddings.position_embedding.weight")[position_ids(tgt_sizes, L, side).reshape(-1)]
    dkw = sd["encoder.layers.0.self_attn.q_proj.weight"].shape[0] // H
    scale = (scale_dim or dkw) ** -0.5
    dead = torch.arange(L)[None, :] >= torch.tensor([int(h) * int(v) for h, v in tgt_sizes])[:, None]       # [B, L] keys that do not count
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (D,), w(p + ".weight"), w(p + ".bias"), eps)
    n = 0
    while "encoder.layers.%d.layer_norm1.weight" % n in sd:
        n += 1
    for i in range(n):
        p = "encoder.layers.%d." % i
        lin = lambda t, nm: t @ w(p + nm + ".weight").t() + w(p + nm + ".bias")
        h = ln(x, p + "layer_norm1")
        q, k, v = (lin(h, "self_attn." + nm).reshape(B, L, H, dkw).transpose(1, 2) for nm in ("q_proj", "k_proj", "v_proj"))
        s = (q @ k.transpose(-1, -2) * scale).masked_fill(dead[:, None, None, :], float("-inf"))
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, H * dkw)
        x = x + lin(a, "self_attn.out_proj")
        h = ln(x, p + "layer_norm2")
        x = x + lin(gelu_tanh_f64(lin(h, "mlp.fc1")), "mlp.fc2")
    return ln(x, "post_layernorm").reshape(B, L, D)


def library_tower(hidden, heads, inter, layers, attn="sdpa", image_size=980, patch_size=14):
    """(config, `transformers` Idefics2VisionTransformer in float32 on the CPU, its own initialisation under a fixed seed)"""
    from transformers.models.idefics2.configuration_idefics2 import Idefics2VisionConfig
    from transformers.models.idefics2.modeling_idefics2 import Idefics2VisionTransformer
    cfg = Idefics2VisionConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter, num_hidden_layers=layers,
                               image_size=image_size, patch_size=patch_size, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
    cfg._attn_implementation = attn
    torch.manual_seed(0)
    return cfg, Idefics2VisionTransformer(cfg).eval().requires_grad_(False)


def library_forward(lib, images, P=14):
    """The library tower on each image alone, in its 2-D form with an all-ones mask -> a list of last_hidden_state [h * w, D]"""
    out = []
    for im in images:
        h, w = im.shape[1] // P, im.shape[2] // P
        x = im.to(device=lib.post_layernorm.weight.device, dtype=lib.post_layernorm.weight.dtype)[None]
        mask = torch.ones((1, h, w), dtype=torch.bool, device=x.device)
        out.append(lib(x, patch_attention_mask=mask).last_hidden_state[0])
    return out


def random_state_dict(tower, seed):
    """The test weights of a library tower: every matrix (the Conv2d kernel included) N(0, 1 / fan_in), the position table N(0, 0.02^2) as
    the library draws it; every 1-D tensor -- the norm weights and the biases, whose defaults are one and zero and would hide a missing
    bias -- its default plus 0.1 N(0, 1); float32 tensors that hold bf16 values"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in tower.state_dict().items():
        v = v.detach().float().clone()
        if v.dim() == 1:
            v = (torch.ones_like(v) if "norm" in k and k.endswith("weight") else torch.zeros_like(v)) + 0.1 * torch.randn(v.shape, generator=g)
        elif "position_embedding" in k:
            v = 0.02 * torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * (v.numel() // v.shape[0]) ** -0.5
        sd[k] = v.bfloat16().float()
    return sd


def pad_heads(sd, heads, dk=72, dkp=80):
    """A copy of sd whose q_proj / k_proj / v_proj gain zero rows (and zero bias entries) dk .. dkp-1 in every head and whose out_proj gains
    the matching zero columns: what the tower's packed weights hold"""
    out = dict(sd)
    for k, v in sd.items():
        if ".self_attn." not in k:
            continue
        if "out_proj" in k:
            if k.endswith("weight"):
                D = v.shape[0]
                t = torch.zeros((D, heads, dkp), dtype=v.dtype)
                t[:, :, :dk] = v.reshape(D, heads, dk)
                out[k] = t.reshape(D, heads * dkp)
        else:
            t = torch.zeros((heads, dkp) + tuple(v.shape[1:]), dtype=v.dtype)
            t[:, :dk] = v.reshape((heads, dk) + tuple(v.shape[1:]))
            out[k] = t.reshape((heads * dkp,) + tuple(v.shape[1:]))
    return out


def pad_mlp(sd, Fp):
    """A copy of sd whose fc1 gains zero rows (and zero bias) up to Fp and whose fc2 gains the matching zero columns"""
    out = dict(sd)
    for k, v in sd.items():
        if ".mlp.fc1." in k:
            t = torch.zeros((Fp,) + tuple(v.shape[1:]), dtype=v.dtype)
            t[:v.shape[0]] = v
            out[k] = t
        elif k.endswith(".mlp.fc2.weight"):
            t = torch.zeros((v.shape[0], Fp), dtype=v.dtype)
            t[:, :v.shape[1]] = v
            out[k] = t
    return out
