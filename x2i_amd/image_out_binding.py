"""ctypes binding and torch-tensor wrappers of the extension header abi/backend/x2i_image_out.h: the image back end's two kernels
(csrc/image_out.hip), packed latents to the VAE decoder's conv_in input and the decoder's output to uint8 pixels.

Like image_rows_binding.py: the entry points are not in _lib._EXPORTS, _lib.extension binds them; PyTorch supplies device memory and the
current stream, every computation happens in libx2i_hip.so, nothing here synchronises, and there is no fallback.  (Not called *_ops.py,
for image_binding.py's reason.)
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of abi/backend/x2i_image_out.h: name -> argtypes (all return int).  tests/test_image_out_boundary_cpu.py checks it against
# the header's prototypes.
_EXPORTS = {
    "x2i_latents_to_vae": [_vp, _i64, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp],
    "x2i_image_to_u8": [_vp, _i32, _vp, _i64, _i64, _i32, _i32, _i32, _vp],
}

PAD = 64            # channels of the decoder's conv_in input (csrc/image_out.hip: eight 16-byte pieces a pixel)

load = _lib.extension("backend/x2i_image_out.h", _EXPORTS, root="abi")


def _latents_args(latents, h, w, Cz, scaling_factor, shift_factor, out):
    """The one place the arguments of x2i_latents_to_vae are put together (field order of abi/backend/x2i_image_out.h)"""
    ops._req_dense(latents, torch.bfloat16, "latents")
    ops._req_dense(out, torch.bfloat16, "out")
    if latents.dim() != 3:
        raise X2IError("x2i_amd: latents must be [B, (h / 2)(w / 2), 4 Cz] packed rows, got shape %s" % (tuple(latents.shape),))
    B, rows, ld = latents.shape
    if h < 2 or w < 2 or h % 2 or w % 2 or rows != (h // 2) * (w // 2):
        raise X2IError("x2i_amd: latents holds %d packed rows per item; h=%d and w=%d must be even and (h / 2)(w / 2) that many" % (rows, h, w))
    if not 1 <= Cz <= 16 or ld < 4 * Cz:
        raise X2IError("x2i_amd: Cz=%d must lie in 1..16 and a packed row (%d elements) hold 4 Cz values" % (Cz, ld))
    if tuple(out.shape) != (B, h, w, PAD):
        raise X2IError("x2i_amd: out must be [%d, %d, %d, %d], got %s" % (B, h, w, PAD, tuple(out.shape)))
    return ops._p(latents), ld, ops._p(out), B, h, w, Cz, float(scaling_factor), float(shift_factor)


def latents_to_vae(latents, h, w, Cz, scaling_factor, shift_factor, out=None):
    """packed latents bf16 [B, (h / 2)(w / 2), >= 4 Cz] -> bf16 [B, h, w, 64] NHWC: the unpacked latents / scaling_factor + shift_factor
    as torch computes it on the device, channels Cz .. 63 zero (abi/backend/x2i_image_out.h)"""
    if out is None:
        out = torch.empty((latents.shape[0], h, w, PAD), device=latents.device, dtype=torch.bfloat16)
    args = _latents_args(latents, h, w, Cz, scaling_factor, shift_factor, out)
    ops._req(latents, torch.bfloat16, "latents")
    ops._req(out, torch.bfloat16, "out")
    check(load().x2i_latents_to_vae(*args, ops._stream()), "latents_to_vae")
    return out


def _u8_args(y, out, image_pitch, row_pitch, offset):
    """The one place the arguments of x2i_image_to_u8 are put together (field order of abi/backend/x2i_image_out.h)"""
    ops._req_dense(y, torch.bfloat16, "y")
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise X2IError("x2i_amd: out must be a contiguous uint8 buffer (got %s, strides %s)" % (out.dtype, tuple(out.stride())))
    if y.dim() != 4 or y.shape[3] not in (4, 8):
        raise X2IError("x2i_amd: y must be [B, H, W, 4 or 8] NHWC, got shape %s" % (tuple(y.shape),))
    B, H, W, ldy = y.shape
    if B < 1 or H < 1 or W < 1:
        raise X2IError("x2i_amd: y must hold at least one pixel, got shape %s" % (tuple(y.shape),))
    if row_pitch < 3 * W or image_pitch < (H - 1) * row_pitch + 3 * W or offset < 0:
        raise X2IError("x2i_amd: row_pitch=%d must be at least 3 W = %d, image_pitch=%d at least (H - 1) row_pitch + 3 W, offset=%d not negative"
                       % (row_pitch, 3 * W, image_pitch, offset))
    need = offset + (B - 1) * image_pitch + (H - 1) * row_pitch + 3 * W
    if out.numel() < need:
        raise X2IError("x2i_amd: out holds %d bytes; %d images of %d rows of %d pixels at offset %d with pitches %d and %d need %d"
                       % (out.numel(), B, H, W, offset, image_pitch, row_pitch, need))
    return ops._p(y), ldy, C.c_void_p(out.data_ptr() + offset), image_pitch, row_pitch, B, H, W


def image_to_u8(y, out=None, image_pitch=None, row_pitch=None, offset=0):
    """the decoder's output y bf16 [B, H, W, 4 or 8] NHWC -> uint8 pixels, VaeImageProcessor.postprocess's values: without `out` a new
    [B, H, W, 3] tensor; with it a flat uint8 device buffer that receives pixel (n, r, x) at offset + n * image_pitch + r * row_pitch + 3 x
    (bytes; the pitches default to the dense ones), nothing else of it written (abi/backend/x2i_image_out.h)"""
    B, H, W = y.shape[:3]
    ret = out
    if out is None:
        ret = torch.empty((B, H, W, 3), device=y.device, dtype=torch.uint8)
        out = ret.view(-1)
    row_pitch = 3 * W if row_pitch is None else row_pitch
    image_pitch = H * row_pitch if image_pitch is None else image_pitch
    args = _u8_args(y, out, image_pitch, row_pitch, offset)
    ops._req(y, torch.bfloat16, "y")
    ops._req(out, torch.uint8, "out")
    check(load().x2i_image_to_u8(*args, ops._stream()), "image_to_u8")
    return ret
