"""The numpy restatements of the image back end's kernels (tests/image_out_ref.py) against the code they replace, on the CPU:
VaeImageProcessor.postprocess and harness.generate's torch expression for the uint8 pixels, FluxPipeline._unpack_latents + divide + add +
AutoencoderKL.decode's pad / permute for the decoder's input -- for all 65536 bf16 bit patterns -- and the planted faults those checks
must catch.

The scalars: on the GPU torch multiplies by the float32 reciprocal of scaling_factor and adds float32(shift_factor); on the CPU it
divides by float32(scaling_factor) and rounds shift_factor to bf16 before it adds.  The kernel follows the GPU (the restatement's
device=True).  Here the CPU expression is compared with device=False, bit for bit, and tests/golden/image_out_scalar_forms.json lists
every input on which the two forms give different bits (1236 of the 65536 at the FLUX constants, all of magnitude below 0.14: the sum
lies near a tie there and the shift's own rounding, 0.1159 -> 0.11572, decides it).  Taken alone, the quotient and the product with
the reciprocal round to the same bf16 for every input at both pairs of constants.

A NaN: the restatement writes 0x7FC0, what torch's scalar conversion (the GPU's) gives; torch's vectorised CPU conversion may write another
NaN pattern, so NaNs are compared here as NaNs, everything else bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import image_out_ref as R

FLUX = (0.3611, 0.1159)
OTHER = (0.13025, 0.0609)


def _forms_differ(consts):
    """the recorded inputs on which the CPU and the GPU form differ, as a sorted list"""
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "image_out_scalar_forms.json")) as fh:
        rec = json.load(fh)["pairs"]["%g,%g" % consts]
    pats = [p for a, b in rec["runs"] for p in range(a, b + 1)]
    assert len(pats) == rec["count"]
    return pats


def _bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _all_patterns_image(ldy=4):
    """[2, 96, 128, ldy] whose first three channels walk all 65536 patterns (and the first 8192 a second time)"""
    bits = np.zeros((2 * 96 * 128, ldy), dtype=np.uint16)
    bits[:, :3] = np.resize(R.ALL_BF16, (2 * 96 * 128, 3))
    assert set(bits[:, :3].ravel().tolist()) == set(range(65536))
    return bits.reshape(2, 96, 128, ldy)


def test_u8_restatement_equals_postprocess_for_every_bf16_pattern():
    from x2i_amd.pipeline import VaeImageProcessor
    bits = _all_patterns_image()
    nan = R.is_nan_bf16(bits[..., :3])
    img = _bf16_tensor(np.where(R.is_nan_bf16(bits), 0, bits))[..., :3].permute(0, 3, 1, 2).contiguous()      # NCHW, as decode returns it
    pil = VaeImageProcessor(vae_scale_factor=16).postprocess(img, output_type="pil")
    want = np.stack([np.asarray(p) for p in pil])
    got = R.image_to_u8(bits)
    assert got.shape == want.shape == (2, 96, 128, 3) and got.dtype == np.uint8
    assert np.array_equal(got[~nan], want[~nan])
    assert nan.sum() == 254                                    # the patterns hold every NaN ...
    assert (got[nan] == 0).all()                               # ... and each gives 0, the defined extension


def test_u8_restatement_equals_the_harness_expression():
    bits = _all_patterns_image(8)
    nan = R.is_nan_bf16(bits[..., :3])
    image = _bf16_tensor(np.where(R.is_nan_bf16(bits), 0, bits))[..., :3].permute(0, 3, 1, 2).contiguous()
    want = ((image.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()   # harness.generate's line
    got = R.image_to_u8(bits)
    assert np.array_equal(got[~nan], want[~nan])
    # float32 values beyond bf16: postprocess takes any float image; the probes are the exact halves (image_out_ref.half_probes)
    from x2i_amd.pipeline import VaeImageProcessor
    x = np.concatenate([R.half_probes(), np.linspace(-1.5, 1.5, 4099, dtype=np.float32), np.float32([np.inf, -np.inf, -0.0, 1.0, -1.0])])
    x = np.resize(x, (1, 3, 40, 140)).astype(np.float32)
    pil = VaeImageProcessor().postprocess(torch.from_numpy(x), output_type="pil")
    assert np.array_equal(R.u8_of_f32(x.transpose(0, 2, 3, 1))[0], np.asarray(pil[0]))


def _packed_all_patterns():
    """packed latents [2, 512, 64]: every bf16 pattern once, h = 32, w = 64"""
    return R.ALL_BF16.reshape(2, 512, 64).copy(), 32, 64


def _torch_decoder_input(bits, h, w, Cz, sf, shift):
    """the parent's path on torch CPU: _unpack_latents, / scaling_factor + shift_factor, decode's zero pad and NHWC copy"""
    from x2i_amd.pipeline import FluxPipeline
    lat = _bf16_tensor(bits[:, :, :4 * Cz])
    z = FluxPipeline._unpack_latents(lat, 8 * h, 8 * w, 16)          # vae_scale_factor 16: 2 * (8 h // 16) = h latent rows
    z = (z / sf) + shift
    B = z.shape[0]
    x = torch.zeros((B, h, w, 64), dtype=torch.bfloat16)
    x[..., :Cz] = z.to(torch.bfloat16).permute(0, 2, 3, 1)
    return _bits(x)


@pytest.mark.parametrize("consts", [FLUX, OTHER])
@pytest.mark.parametrize("Cz", [16, 4])
def test_latents_restatement_equals_the_torch_path_for_every_bf16_pattern(consts, Cz):
    sf, shift = consts
    bits, h, w = _packed_all_patterns()
    if Cz == 4:         # rows of 16 values: the same patterns, four times the rows
        bits, h, w = bits.reshape(2, 2048, 16), 64, 128
    want = _torch_decoder_input(bits, h, w, Cz, sf, shift)
    got = R.latents_to_vae(bits, h, w, Cz, sf, shift, device=False)             # torch's CPU form: divides, shift rounded to bf16
    nan = R.is_nan_bf16(want)
    assert np.array_equal(nan, R.is_nan_bf16(got)) and nan.sum() == 254
    assert (got[nan] == 0x7FC0).all()
    assert np.array_equal(got[~nan], want[~nan])
    assert (got[..., Cz:] == 0).all() and (want[..., Cz:] == 0).all()
    # the device's form: the inputs on which it gives other bits are the recorded ones, and the divide alone is none of the reason
    a, b = R.scale_shift(R.ALL_BF16, sf, shift, False), R.scale_shift(R.ALL_BF16, sf, shift, True)
    differ = np.nonzero(a != b)[0].tolist()
    assert differ == _forms_differ(consts) and 0 < len(differ) < 2048
    assert np.abs(R.bf16_to_f32(np.array(differ, dtype=np.uint16))).max() < 0.14
    v, s = R.bf16_to_f32(R.ALL_BF16), np.float32(sf)
    with np.errstate(all="ignore"):
        assert np.array_equal(R.f32_to_bf16(v / s), R.f32_to_bf16(v * (np.float32(1.0) / s)))
    dev = R.latents_to_vae(bits, h, w, Cz, sf, shift, device=True)
    assert int((dev != got).sum()) == len(differ)          # every pattern stands once in the layout


def test_latents_restatement_layout_on_a_ragged_row_width():
    """ld = 64 with Cz = 4: the values behind 4 Cz of a packed row are never read"""
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 0x7F80, size=(2, 3 * 5, 64), dtype=np.uint16)
    a = R.latents_to_vae(bits, 6, 10, 4, *FLUX)
    junk = bits.copy()
    junk[:, :, 16:] = 0x7FC0
    assert np.array_equal(a, R.latents_to_vae(junk, 6, 10, 4, *FLUX))
    # one element by hand: channel 3 of pixel (2 * 2 + 1, 2 * 4 + 0) of item 1 is element 3 * 4 + 1 * 2 + 0 of packed row 2 * 5 + 4
    assert a[1, 5, 8, 3] == R.scale_shift(bits[1, 14, 14], *FLUX)
    assert np.array_equal(R.latents_to_vae(bits, 6, 10, 4, *FLUX, device=False), _torch_decoder_input(bits, 6, 10, 4, *FLUX))


def test_planted_faults_are_caught():
    from x2i_amd.pipeline import VaeImageProcessor
    post = lambda x: np.asarray(VaeImageProcessor().postprocess(torch.from_numpy(x.reshape(1, 1, 1, -1).repeat(3, 1)), output_type="pil")[0])[0, :, 0]   # noqa: E731
    # round half up: only a product that is exactly k + 0.5 with k even tells it from half to even; such float32 inputs exist
    probes = R.half_probes()
    assert len(probes) >= 8
    want = post(probes)
    assert np.array_equal(R.u8_of_f32(probes), want)
    assert not np.array_equal(R.u8_of_f32(probes, _fault="half_up"), want)
    assert (R.u8_of_f32(probes, _fault="half_up") != want).sum() >= 4
    # the clamp moved behind the * 255 (bounds 0 and 1 as they stand in the source): caught by every value above 1 / 255.  (With the bounds
    # scaled as well, clamp(x * 255, 0, 255), the function is the same for every float32 -- the product is monotone -- so that is no fault.)
    bits = _all_patterns_image()
    ok = ~R.is_nan_bf16(bits[..., :3])
    assert not np.array_equal(R.image_to_u8(bits, _fault="clamp_after_scale")[ok], R.image_to_u8(bits)[ok])
    grid = np.linspace(-1.0, 1.0, 511, dtype=np.float32)
    assert not np.array_equal(R.u8_of_f32(grid, _fault="clamp_after_scale"), post(grid)) and np.array_equal(R.u8_of_f32(grid), post(grid))
    # swapped a / b in the unpack, a non-zero pad channel: against the torch path
    pk, h, w = _packed_all_patterns()
    want = _torch_decoder_input(pk, h, w, 16, *FLUX)
    ok = ~R.is_nan_bf16(want)
    assert np.array_equal(R.latents_to_vae(pk, h, w, 16, *FLUX, device=False)[ok], want[ok])
    for fault in ("swap_ab", "pad"):
        assert not np.array_equal(R.latents_to_vae(pk, h, w, 16, *FLUX, device=False, _fault=fault)[ok], want[ok]), fault
