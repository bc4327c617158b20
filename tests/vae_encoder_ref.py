"""CPU restatement of the FLUX VAE ENCODER (diffusers AutoencoderKL.encode, as lightcontrol/train_lightcontrol.py:678-679 calls it), for the
tests of x2i_amd.vae's opt-in encoder half.  Composed in fp32 from oracle.vae's building blocks (`_conv`, `_gn`, `resnet`, `mid_attention`)
plus F.pad for Downsample2D.

PARITY UNPINNED, as for the decoder: diffusers is third-party and not installed here.  The structure below is the published FLUX
`vae/config.json` (block_out_channels [128, 256, 512, 512], layers_per_block 2, norm_num_groups 32, latent_channels 16, in_channels 3,
use_quant_conv false) with diffusers' Encoder(double_z=True) / DownEncoderBlock2D / Downsample2D(use_conv=True, padding=0: F.pad(x, (0, 1, 0, 1))
then a stride-2 conv) / UNetMidBlock2D(attention, eps 1e-6) / DiagonalGaussianDistribution semantics.
"""
import torch
import torch.nn.functional as F

from oracle.vae import FLUX_VAE_CFG, _conv, _gn, mid_attention, resnet


def vae_encode_params(sd, x, cfg=FLUX_VAE_CFG):
    """x: [B, 3, H, W] images in [-1, 1] -> the encoder's conv_out [B, 2 latent_channels, H / 8, W / 8] (mean channels, then logvar)."""
    G = cfg["norm_num_groups"]
    boc = cfg["block_out_channels"]
    h = _conv(sd, "encoder.conv_in", x, padding=1)
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"]):
            h = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", h, G)
        if i != len(boc) - 1:
            h = _conv(sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", F.pad(h, (0, 1, 0, 1)), stride=2)
    h = resnet(sd, "encoder.mid_block.resnets.0", h, G)
    h = mid_attention(sd, "encoder.mid_block.attentions.0", h, G)
    h = resnet(sd, "encoder.mid_block.resnets.1", h, G)
    h = F.silu(_gn(sd, "encoder.conv_norm_out", h, G))
    return _conv(sd, "encoder.conv_out", h, padding=1)


def posterior(params, latent_channels=16):
    """DiagonalGaussianDistribution: (mean, clamped logvar, std)."""
    mean, logvar = torch.chunk(params, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return mean, logvar, torch.exp(0.5 * logvar)


def vae_encoder_param_shapes(cfg=FLUX_VAE_CFG, in_channels=3):
    s = {}

    def conv(n, co, ci, k):
        s[n + ".weight"] = (co, ci, k, k)
        s[n + ".bias"] = (co,)

    def vec(n, c):
        s[n + ".weight"] = (c,)
        s[n + ".bias"] = (c,)

    def res(n, ci, co):
        vec(n + ".norm1", ci)
        conv(n + ".conv1", co, ci, 3)
        vec(n + ".norm2", co)
        conv(n + ".conv2", co, co, 3)
        if ci != co:
            conv(n + ".conv_shortcut", co, ci, 1)

    boc = cfg["block_out_channels"]
    conv("encoder.conv_in", boc[0], in_channels, 3)
    prev = boc[0]
    for i, co in enumerate(boc):
        for j in range(cfg["layers_per_block"]):
            res(f"encoder.down_blocks.{i}.resnets.{j}", prev if j == 0 else co, co)
        prev = co
        if i != len(boc) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", co, co, 3)
    top = boc[-1]
    res("encoder.mid_block.resnets.0", top, top)
    a = "encoder.mid_block.attentions.0"
    vec(a + ".group_norm", top)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        s[a + "." + n + ".weight"] = (top, top)
        s[a + "." + n + ".bias"] = (top,)
    res("encoder.mid_block.resnets.1", top, top)
    vec("encoder.conv_norm_out", top)
    conv("encoder.conv_out", 2 * cfg["latent_channels"], top, 3)
    return s


def random_vae_encoder_state_dict(cfg=FLUX_VAE_CFG, seed=0, dtype=torch.float32):
    """Fan-in-scaled random weights (the scheme of oracle.vae.random_vae_decoder_state_dict), so activations stay O(1) through the encoder."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, shp in vae_encoder_param_shapes(cfg).items():
        if len(shp) == 4:
            t = torch.randn(shp, generator=g) / (shp[1] * shp[2] * shp[3]) ** 0.5
        elif len(shp) == 2:
            t = torch.randn(shp, generator=g) / shp[1] ** 0.5
        elif n.endswith("weight"):
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            t = 0.02 * torch.randn(shp, generator=g)
        sd[n] = t.to(dtype)
    return sd
