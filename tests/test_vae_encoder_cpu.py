"""The VAE encoder half without a GPU: parameter tree and key names against the restatement's table, the opt-in default, checkpoint
loading, known answers of the fp32 restatement, and argument validation of the two new entry points."""
import json
import math
import os

import pytest
import torch

from oracle import vae as OV
from tests import vae_encoder_ref as ER

X2I_ERR_ARG, X2I_ERR_SHAPE = -1, -2


def test_encoder_parameter_tree_is_the_flux_table():
    from x2i_amd.vae import AutoencoderKL
    vae = AutoencoderKL(device="meta", with_encoder=True)
    got = {k: tuple(v.shape) for k, v in vae.state_dict().items()}
    enc = ER.vae_encoder_param_shapes()
    assert got == {**{k: tuple(v) for k, v in OV.vae_decoder_param_shapes().items()}, **enc}
    assert len(enc) == 106
    n = sum(math.prod(s) for s in enc.values())
    assert round(n / 1e6, 3) == 34.274
    assert round((n + sum(math.prod(s) for s in OV.vae_decoder_param_shapes().values())) / 1e6, 1) == 83.8


def test_encoder_is_opt_in():
    from x2i_amd.vae import AutoencoderKL
    vae = AutoencoderKL(device="meta")
    assert not any(k.startswith("encoder.") for k in vae.state_dict()) and not hasattr(vae, "encoder")
    assert {k: tuple(v.shape) for k, v in vae.state_dict().items()} == {k: tuple(v) for k, v in OV.vae_decoder_param_shapes().items()}
    with pytest.raises(RuntimeError, match="with_encoder=True"):
        vae.encode(torch.zeros(1, 3, 64, 64, device="meta"))
    with pytest.raises(NotImplementedError):
        AutoencoderKL(device="meta", with_encoder=True, use_quant_conv=True)


def test_encode_flops():
    from x2i_amd.vae import AutoencoderKL, encode_flops
    cfg = AutoencoderKL(device="meta", with_encoder=True).config
    assert abs(encode_flops(cfg, 1024, 1024) / 1e12 - 4.88) < 0.01
    # conv_in alone at 8 x 8 with one-block widths: 2 * 3 * 128 * 9 per pixel
    small = dict(cfg, block_out_channels=(128,), layers_per_block=0)
    T = 64
    assert encode_flops(type(cfg)(small), 8, 8) == 2.0 * 3 * 128 * 9 * T + 4 * 2.0 * T * 128 * 128 + 2 * 2.0 * T * T * 128 + \
        2 * 2 * (2.0 * 128 * 128 * 9 * T) + 2.0 * 128 * 32 * 9 * T


def _write_vae_dir(path, sd, **cfg):
    from safetensors.torch import save_file
    os.makedirs(path)
    json.dump(dict(dict(latent_channels=16, out_channels=3, in_channels=3, block_out_channels=[64, 64], layers_per_block=1, norm_num_groups=16,
                        scaling_factor=0.3611, shift_factor=0.1159), **cfg), open(os.path.join(path, "config.json"), "w"))
    save_file({k: v.detach().contiguous() for k, v in sd.items()}, os.path.join(path, "diffusion_pytorch_model.safetensors"))


def test_from_pretrained_with_encoder(tmp_path):
    from x2i_amd.vae import AutoencoderKL
    cfg = dict(OV.FLUX_VAE_CFG, block_out_channels=(64, 64), layers_per_block=1, norm_num_groups=16)
    sd = {k: v.bfloat16() for k, v in {**OV.random_vae_decoder_state_dict(cfg, seed=3), **ER.random_vae_encoder_state_dict(cfg, seed=4)}.items()}
    d = str(tmp_path / "vae")
    _write_vae_dir(d, sd)
    vae = AutoencoderKL.from_pretrained(d, device="cpu", with_encoder=True)
    got = vae.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    # the default still takes the decoder only from the same full checkpoint
    dec = AutoencoderKL.from_pretrained(d, device="cpu")
    assert not any(k.startswith("encoder.") for k in dec.state_dict())
    # missing encoder keys
    d2 = str(tmp_path / "vae_dec_only")
    _write_vae_dir(d2, {k: v for k, v in sd.items() if not k.startswith("encoder.down_blocks.1")})
    with pytest.raises(KeyError):
        AutoencoderKL.from_pretrained(d2, device="cpu", with_encoder=True)
    AutoencoderKL.from_pretrained(d2, device="cpu")   # (decoder-only: fine)
    # quant_conv
    d3 = str(tmp_path / "vae_quant")
    _write_vae_dir(d3, sd, use_quant_conv=True)
    with pytest.raises(NotImplementedError):
        AutoencoderKL.from_pretrained(d3, device="cpu", with_encoder=True)
    # load_state_dict: with the encoder, encoder.* keys are taken (strictly)
    vae2 = AutoencoderKL(**{k: cfg[k] for k in ("block_out_channels", "layers_per_block", "norm_num_groups")}, device="cpu", with_encoder=True)
    vae2.load_state_dict(sd)
    assert torch.equal(vae2.encoder.conv_out.weight, sd["encoder.conv_out.weight"])
    with pytest.raises(RuntimeError):
        vae2.load_state_dict({k: v for k, v in sd.items() if k != "encoder.conv_in.bias"})


def test_restatement_known_answers():
    cfg = dict(OV.FLUX_VAE_CFG, block_out_channels=(32, 32), layers_per_block=1, norm_num_groups=8)
    sd = ER.random_vae_encoder_state_dict(cfg, seed=1)
    x = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(2)) * 2 - 1
    # zero conv_out weight: the posterior parameters are the bias at every pixel
    sd["encoder.conv_out.weight"].zero_()
    p = ER.vae_encode_params(sd, x, cfg)
    assert p.shape == (1, 32, 8, 8)
    assert torch.equal(p, sd["encoder.conv_out.bias"].view(1, 32, 1, 1).expand_as(p))
    # logvar above 20 clamps: std == exp(10); below -30: std == exp(-15)
    sd["encoder.conv_out.bias"][16:24] = 25.0
    sd["encoder.conv_out.bias"][24:] = -40.0
    mean, logvar, std = ER.posterior(ER.vae_encode_params(sd, x, cfg))
    assert torch.equal(std[:, :8], torch.full_like(std[:, :8], math.exp(10.0)))
    assert torch.equal(logvar[:, 8:], torch.full_like(logvar[:, 8:], -30.0))
    assert torch.equal(mean, sd["encoder.conv_out.bias"][:16].view(1, 16, 1, 1).expand_as(mean))


def test_new_entry_points_validate_without_a_gpu():
    from x2i_amd import _lib
    lib = _lib.load()
    fake = 0x1000
    # x2i_conv3x3_image_bf16(x, w, bias, y, B, Cin, H, W, Cout, moments, moments_scratch, stream)
    assert lib.x2i_conv3x3_image_bf16(None, fake, None, fake, 1, 3, 8, 8, 128, None, None, None) == X2I_ERR_ARG
    assert lib.x2i_conv3x3_image_bf16(fake, fake, None, fake, 1, 3, 8, 8, 128, fake, None, None) == X2I_ERR_ARG
    assert b"moments_scratch" in lib.x2i_last_error()
    assert lib.x2i_conv3x3_image_bf16(fake, fake, None, fake, 1, 5, 8, 8, 128, None, None, None) == X2I_ERR_SHAPE
    assert lib.x2i_conv3x3_image_bf16(fake, fake, None, fake, 1, 3, 8, 8, 136, None, None, None) == X2I_ERR_SHAPE
    assert lib.x2i_conv3x3_image_bf16(fake, fake, None, fake, 1, 3, 8, 8, 24, None, None, None) == X2I_ERR_SHAPE
    assert lib.x2i_conv3x3_image_bf16(fake, fake, None, fake, 0, 3, 8, 8, 128, None, None, None) == X2I_ERR_SHAPE
    assert b"Cout a multiple of 16" in lib.x2i_last_error()
    # x2i_vae_posterior_bf16(params, ldp, eps, out_nchw, out_packed, B, C, h, w, scale_shift, shift, scale, stream)
    assert lib.x2i_vae_posterior_bf16(None, 32, None, fake, None, 1, 16, 8, 8, 0, 0.0, 1.0, None) == X2I_ERR_ARG
    assert lib.x2i_vae_posterior_bf16(fake, 32, None, None, None, 1, 16, 8, 8, 0, 0.0, 1.0, None) == X2I_ERR_ARG
    assert lib.x2i_vae_posterior_bf16(fake, 32, None, fake, None, 1, 16, 8, 8, 2, 0.0, 1.0, None) == X2I_ERR_ARG
    assert lib.x2i_vae_posterior_bf16(fake, 30, None, fake, None, 1, 16, 8, 8, 0, 0.0, 1.0, None) == X2I_ERR_SHAPE
    assert b"ldp" in lib.x2i_last_error()
    assert lib.x2i_vae_posterior_bf16(fake, 32, None, None, fake, 1, 16, 7, 8, 0, 0.0, 1.0, None) == X2I_ERR_SHAPE
    assert b"even" in lib.x2i_last_error()
