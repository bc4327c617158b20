"""numpy restatements of the image back end's two kernels (abi/backend/x2i_image_out.h, csrc/image_out.hip); a helper of the image_out
tests, it holds no tests.  bf16 values travel as their uint16 bit patterns, every float32 operation is one numpy float32 operation.

`latents / scaling_factor + shift_factor` on a bf16 tensor is not one function in PyTorch.  On the GPU (device=True, what the kernel
computes, and the default here) both host scalars reach the kernel as float32: the divide multiplies by the float32 reciprocal
1.0f / scaling_factor, the add adds float32(shift_factor).  On the CPU (device=False) the divide divides by float32(scaling_factor), and
the add's scalar is first rounded to bf16, the tensor's dtype.  The device's value is the contract.
tests/test_image_out_ref_cpu.py lists the inputs on which the two differ.

The `_fault` arguments plant one wrong step each, for the tests that show that the checks would catch it.
"""
import numpy as np

F32 = np.float32
ALL_BF16 = np.arange(65536, dtype=np.uint16)
PAD = 64


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def f32_to_bf16(f):
    """round to nearest even on the bits, every NaN 0x7FC0: c10::BFloat16's round_to_nearest_even, torch's scalar .to(bfloat16)"""
    f = np.ascontiguousarray(f, dtype=F32)
    u = f.view(np.uint32)
    out = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)   # (wraps for NaNs only, which are replaced)
    out[np.isnan(f)] = 0x7FC0
    return out


def is_nan_bf16(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return (bits & 0x7FFF) > 0x7F80


def scale_shift(bits, scaling_factor, shift_factor, device=True):
    """bf16 bits of `x / scaling_factor + shift_factor` on a bf16 tensor: two roundings to bf16"""
    v, s, t = bf16_to_f32(bits), F32(scaling_factor), F32(shift_factor)
    with np.errstate(all="ignore"):
        q = v * (F32(1.0) / s) if device else v / s
        if not device:
            t = bf16_to_f32(f32_to_bf16(np.array([t])))[0]
        return f32_to_bf16(bf16_to_f32(f32_to_bf16(q)) + t)


def latents_to_vae(bits, h, w, Cz, scaling_factor, shift_factor, device=True, _fault=None):
    """bits uint16 [B, (h / 2)(w / 2), ld >= 4 Cz] -> uint16 [B, h, w, 64]: x2i_latents_to_vae"""
    bits = np.asarray(bits, dtype=np.uint16)
    B, rows, ld = bits.shape
    assert h % 2 == 0 and w % 2 == 0 and rows == (h // 2) * (w // 2) and 1 <= Cz <= 16 and ld >= 4 * Cz
    val = scale_shift(bits[:, :, :4 * Cz], scaling_factor, shift_factor, device).reshape(B, h // 2, w // 2, Cz, 2, 2)   # (i, j, c, a, b)
    out = np.zeros((B, h, w, PAD), dtype=np.uint16)
    for a in (0, 1):
        for b in (0, 1):
            src = val[..., b, a] if _fault == "swap_ab" else val[..., a, b]
            out[:, a::2, b::2, :Cz] = src
    if _fault == "pad" and Cz < PAD:
        out[:, h - 1, w - 1, PAD - 1] = 0x3F80
    return out


def u8_of_f32(x, _fault=None):
    """float32 image values -> uint8: rint(clamp(x * 0.5 + 0.5, 0, 1) * 255), NaN -> 0 (the kernel's arithmetic; postprocess's for
    everything but a NaN, which it leaves undefined)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        f = x * F32(0.5) + F32(0.5)
        if _fault == "clamp_after_scale":                       # the clamp line moved behind the * 255 line
            s = np.fmin(np.fmax(f * F32(255.0), F32(0.0)), F32(1.0))
        else:
            s = np.fmin(np.fmax(f, F32(0.0)), F32(1.0)) * F32(255.0)    # fmax / fmin drop a NaN: fmax(NaN, 0) = 0
        r = np.floor(s + F32(0.5)) if _fault == "half_up" else np.rint(s)
    return r.astype(np.uint8)


def image_to_u8(bits, _fault=None):
    """bits uint16 [B, H, W, ldy >= 3] -> uint8 [B, H, W, 3]: x2i_image_to_u8 with dense pitches"""
    bits = np.asarray(bits, dtype=np.uint16)
    return u8_of_f32(bf16_to_f32(bits[..., :3]), _fault)


def half_probes():
    """float32 image values x in [0, 1) whose x * 0.5 + 0.5 is exact and whose product with 255 is exactly k + 0.5 in float32: the only
    inputs on which rounding half up and half to even can differ (no bf16 value but 0 is one, and 127.5 rounds to 128 either way)"""
    out = []
    for k in range(128, 255):
        centre = F32((k + 0.5) / 255.0)
        f = centre
        for _ in range(4):
            f = np.nextafter(f, F32(0.0))
        for _ in range(9):
            if F32(f * F32(255.0)) == F32(k + 0.5):
                out.append(F32(F32(2.0) * f - F32(1.0)))
            f = np.nextafter(f, F32(2.0))
    return np.array(out, dtype=F32)
