"""The VAE encoder half on the HIP path: the image-stem kernel and the posterior kernel against their fp32 formulas, `encode` against the fp32
restatement (tests/vae_encoder_ref.py; diffusers is absent, so parity with it stays unpinned), repeatability and the argument errors."""
import pytest
import torch
import torch.nn.functional as F

from oracle import vae as OV
from tests import vae_encoder_ref as ER
from tests.util import rel_l2, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bf(x):
    return x.to(torch.bfloat16)


def bf16_ulp(ref):
    """Spacing of bf16 numbers at |ref| (8 significant bits), floored at the smallest normal's."""
    a = ref.abs().double().clamp_min(torch.finfo(torch.bfloat16).tiny)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def pack_latents(z):
    """FluxPipeline._pack_latents: [B, C, h, w] -> [B, (h/2)(w/2), 4 C]."""
    B, C, h, w = z.shape
    return z.view(B, C, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (h // 2) * (w // 2), C * 4)


@pytest.mark.parametrize("B,Cin,H,W,Cout", [(1, 3, 8, 8, 16), (2, 3, 24, 40, 128), (1, 4, 16, 24, 48), (1, 3, 1024, 1024, 128)])
def test_image_stem_conv(B, Cin, H, W, Cout):
    """x2i_conv3x3_image_bf16 vs F.conv2d in fp32 on the bf16 inputs: every output within one bf16 ulp of the reference (plus the fp32 summation
    allowance 2^-20 sum |w x|, which matters only where the 28 terms cancel); its moments vs fp64 sums of its own bf16 outputs; two calls
    bit-identical."""
    from x2i_amd import ops
    x = bf(seeded((B, Cin, H, W), 11).clamp(-1, 1))
    w = bf(seeded((Cout, Cin, 3, 3), 12) / (9 * Cin) ** 0.5)
    b = bf(seeded((Cout,), 13) * 0.1)
    mom = torch.empty((B, Cout, 2), device=DEV, dtype=torch.float32)
    y = ops.conv3x3_image(x.to(DEV), w.to(DEV), b.to(DEV), moments=mom)
    mom2 = torch.empty_like(mom)
    y2 = ops.conv3x3_image(x.to(DEV), w.to(DEV), b.to(DEV), moments=mom2)
    y3 = ops.conv3x3_image(x.to(DEV), w.to(DEV), b.to(DEV))          # (the form without moments writes the same tensor)
    torch.cuda.synchronize()
    assert y.shape == (B, H, W, Cout)
    assert torch.equal(y, y2) and torch.equal(mom, mom2) and torch.equal(y, y3)
    yc = y.cpu()
    for c0 in range(0, Cout, 32):   # (in channel slices: the 1024^2 reference would otherwise hold several GiB)
        ws = w[c0:c0 + 32].float()
        ref = F.conv2d(x.float(), ws, b[c0:c0 + 32].float(), padding=1).permute(0, 2, 3, 1)
        mag = F.conv2d(x.float().abs(), ws.abs(), b[c0:c0 + 32].float().abs(), padding=1).permute(0, 2, 3, 1)
        err = (yc[..., c0:c0 + 32].double() - ref.double()).abs()
        tol = bf16_ulp(ref) + mag.double() * 2.0 ** -20
        assert bool((err <= tol).all()), (c0, float((err - tol).max()))
    # moments: channel-quad sums at c % 4 == 0, zeros elsewhere (x2i_conv_desc.moments)
    v = yc.double().reshape(B, H * W, Cout // 4, 4)
    s1, s2, sa = v.sum((1, 3)), (v * v).sum((1, 3)), v.abs().sum((1, 3))
    m = mom.cpu().double().reshape(B, Cout // 4, 4, 2)
    assert bool((m[:, :, 1:] == 0).all())
    assert bool(((m[:, :, 0, 0] - s1).abs() <= 1e-5 * sa).all())
    assert bool(((m[:, :, 0, 1] - s2).abs() <= 1e-5 * s2).all())


def _params(B, C, h, w, ldp, seed):
    p = seeded((B, h, w, ldp), seed)
    p[..., :C] *= 2.0
    p[..., C:2 * C] = p[..., C:2 * C] * 20.0 - 5.0    # logvar well outside [-30, 20] at both ends, too
    return bf(p)


def test_posterior_kernel():
    from x2i_amd import ops
    B, C, h, w = 2, 16, 12, 20
    for ldp in (2 * C, 40):
        p = _params(B, C, h, w, ldp, 21)
        pd = p.to(DEV)
        eps = bf(seeded((B, C, h, w), 22))
        mean = p[..., :C].permute(0, 3, 1, 2).float()
        lv = p[..., C:2 * C].permute(0, 3, 1, 2).float()
        assert float(lv.min()) < -30 and float(lv.max()) > 20
        # mode: the mean channels, bit-exact
        assert torch.equal(ops.vae_posterior(pd, C).cpu(), bf(mean))
        # sample with a given eps
        ref = mean + torch.exp(0.5 * lv.clamp(-30, 20)) * eps.float()
        z = ops.vae_posterior(pd, C, eps=eps.to(DEV)).cpu()
        assert bool(((z.double() - ref.double()).abs() <= bf16_ulp(ref)).all())
        # (z - shift) * scale, on both
        sh, sc = 0.1159, 0.3611
        for e, r in ((None, mean), (eps, ref)):
            rs = (r - sh) * sc
            zs = ops.vae_posterior(pd, C, eps=None if e is None else e.to(DEV), scale_shift=(sh, sc)).cpu()
            assert bool(((zs.double() - rs.double()).abs() <= bf16_ulp(rs)).all())
            # packed tokens: FluxPipeline._pack_latents of the NCHW output, bit-exact
            zp = ops.vae_posterior(pd, C, eps=None if e is None else e.to(DEV), scale_shift=(sh, sc), packed=True).cpu()
            assert zp.shape == (B, (h // 2) * (w // 2), 4 * C) and torch.equal(zp, pack_latents(zs))
    # deterministic
    a = ops.vae_posterior(pd, C, eps=eps.to(DEV), packed=True)
    assert torch.equal(a, ops.vae_posterior(pd, C, eps=eps.to(DEV), packed=True))


def _vae(cfg, seed):
    from x2i_amd.vae import AutoencoderKL
    sd = {**OV.random_vae_decoder_state_dict(cfg, seed=seed), **ER.random_vae_encoder_state_dict(cfg, seed=seed + 1)}
    sd = {k: bf(v) for k, v in sd.items()}
    vae = AutoencoderKL(**{k: cfg[k] for k in ("block_out_channels", "layers_per_block", "norm_num_groups", "latent_channels")}, device=DEV,
                        with_encoder=True)
    vae.load_state_dict(sd, strict=True)
    return vae, {k: v.float() for k, v in sd.items()}


def _image(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1)


def test_sample_with_generator_draws_the_diffusers_noise():
    cfg = dict(OV.FLUX_VAE_CFG, block_out_channels=(128, 128), layers_per_block=1)
    vae, _ = _vae(cfg, 30)
    x = _image((2, 3, 32, 48), 31).to(DEV)
    dist = vae.encode(x).latent_dist
    mean, lv = dist.mean.float().cpu(), dist.logvar.float().cpu()
    assert dist.mean.shape == (2, 16, 16, 24)
    for gdev in ("cuda", "cpu"):
        z = dist.sample(generator=torch.Generator(device=gdev).manual_seed(5)).cpu()
        eps = torch.randn(mean.shape, generator=torch.Generator(device=gdev).manual_seed(5), device=gdev, dtype=torch.bfloat16).float().cpu()
        ref = mean + torch.exp(0.5 * lv) * eps
        assert bool(((z.double() - ref.double()).abs() <= bf16_ulp(ref)).all()), gdev
        zs = dist.sample(generator=torch.Generator(device=gdev).manual_seed(5), scale_shift=True).cpu()
        rs = (ref - vae.config.shift_factor) * vae.config.scaling_factor
        assert bool(((zs.double() - rs.double()).abs() <= bf16_ulp(rs)).all()), gdev
    assert torch.equal(dist.mode().cpu(), dist.mean.cpu())
    assert torch.equal(dist.mode(scale_shift=True, packed=True).cpu(), pack_latents(dist.mode(scale_shift=True).cpu()))
    with pytest.raises(NotImplementedError):
        dist.kl()
    with pytest.raises(NotImplementedError):
        dist.nll(z)


@pytest.mark.parametrize("widths,shape", [((128, 128, 256, 256), (2, 3, 64, 96)), ((128, 256, 512, 512), (1, 3, 128, 128)),
                                          ((128, 256, 512, 512), (1, 3, 512, 512))])
def test_encode_vs_restatement(widths, shape):
    cfg = dict(OV.FLUX_VAE_CFG, block_out_channels=widths)
    vae, sd = _vae(cfg, 40)
    x = _image(shape, 41)
    out = vae.encode(x.to(DEV))
    dist = out.latent_dist
    (dist2,) = vae.encode(x.to(DEV), return_dict=False)
    assert torch.equal(dist.parameters.cpu(), dist2.parameters.cpu())   # repeatable, bit for bit
    with torch.no_grad():
        ref = ER.vae_encode_params(sd, bf(x).float(), cfg)
    mean, logvar, _ = ER.posterior(ref)
    e_mean, e_lv = rel_l2(dist.mean, mean), rel_l2(dist.logvar, logvar)
    print("encode %s %s: rel L2 mean %.3e, logvar %.3e" % (widths, shape, e_mean, e_lv))
    assert e_mean <= 3e-2 and e_lv <= 3e-2


def test_encode_batch_consistency_and_errors():
    cfg = dict(OV.FLUX_VAE_CFG, block_out_channels=(128, 128, 256, 256))
    vae, _ = _vae(cfg, 50)
    x = _image((2, 3, 64, 64), 51).to(DEV)
    p2 = vae.encode(x).latent_dist.parameters
    p1 = vae.encode(x[:1]).latent_dist.parameters
    e = rel_l2(p2[:1], p1)
    print("batch-2 sample 0 vs batch-1: rel L2 %.3e, bit-identical: %s" % (e, torch.equal(p2[:1], p1)))
    assert e < 1e-3
    # fp32 / fp16 input is cast to bf16 first: same result as a bf16 input
    assert torch.equal(vae.encode(x.to(torch.bfloat16)).latent_dist.parameters, p2)
    with pytest.raises(ValueError, match="multiples of 8"):
        vae.encode(x[..., :60])
    with pytest.raises(ValueError, match="multiple of 8"):
        vae.encode(x[..., :24, :24])                  # 3 x 3 = 9 mid-block tokens
    with pytest.raises(ValueError):
        vae.encode(x[:, :2])
    from x2i_amd.vae import AutoencoderKL
    dec = AutoencoderKL(block_out_channels=(128, 128, 256, 256), device=DEV)
    with pytest.raises(RuntimeError, match="with_encoder=True"):
        dec.encode(x)
