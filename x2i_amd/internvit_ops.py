"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_internvit.h: the InternVL2.5 InternViT vision tower's kernels (csrc/internvit.hip).

The three entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like
ops.py and the other *_ops.py modules: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so,
nothing here allocates behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_internvit.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_internvit_patch_rows_bf16": [_vp, _i64, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp],
    "x2i_internvit_embed_bf16": [_vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "x2i_internvit_shuffle_ln_bf16": [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp],
}

pad64 = _lib.pad64

load = _lib.extension("x2i_internvit.h", _EXPORTS)


def patch_rows(img, Xp, P, Kp, ldx=None):
    """img bf16 [B, 3, gh*P, gw*P] (unit stride along an image row; any row, channel and sample strides) -> Xp rows [B*gh*gw]: columns
    ci*P*P + y*P + x < 3*P*P hold img[b][ci][r*P + y][q*P + x] for row b*gh*gw + r*gw + q, columns up to Kp are zero; nothing at or beyond
    column Kp is written."""
    ops._req(img, torch.bfloat16, "img")
    ops._req(Xp, torch.bfloat16, "Xp")
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] % P or img.shape[3] % P or not img.shape[2] or not img.shape[3]:
        raise X2IError("x2i_amd: img must be [B, 3, gh*P, gw*P] with P = %d (got %s)" % (P, tuple(img.shape)))
    B, gh, gw = img.shape[0], img.shape[2] // P, img.shape[3] // P
    if img.stride(3) != 1:
        raise X2IError("x2i_amd: img must have unit stride along an image row (strides %s)" % (img.stride(),))
    ldx = Xp.stride(-2) if ldx is None else ldx
    if Xp.numel() and (Xp.shape[-1] < Kp or Xp.numel() // Xp.shape[-1] < B * gh * gw):
        raise X2IError("x2i_amd: Xp must hold B*gh*gw = %d rows of at least Kp = %d columns (got %s)" % (B * gh * gw, Kp, tuple(Xp.shape)))
    check(load().x2i_internvit_patch_rows_bf16(ops._p(img), img.stride(0) if B > 1 else 3 * img.stride(1), img.stride(1), img.stride(2), ops._p(Xp),
                                               ldx, B, gh, gw, P, Kp, ops._stream()), "internvit_patch_rows")
    return Xp


def embed(X, cls, pos):
    """X bf16 [B, 1+L, D] contiguous, rows 1.. holding the patch embedding's output, in place: row 0 = bf16(cls + pos[0]), row 1+p += pos[1+p]
    (one f32 add, one rounding).  cls bf16 [D] (any shape of D elements), pos bf16 [1+L, D] contiguous (a leading 1 allowed)."""
    ops._req(X, torch.bfloat16, "X")
    ops._req(cls, torch.bfloat16, "cls")
    ops._req(pos, torch.bfloat16, "pos")
    if X.dim() != 3 or not X.is_contiguous() or X.shape[1] < 2:
        raise X2IError("x2i_amd: X must be a contiguous [B, 1+L, D] tensor (got %s, strides %s)" % (tuple(X.shape), X.stride()))
    B, S, D = X.shape
    if cls.numel() != D or not cls.is_contiguous() or pos.numel() != S * D or pos.shape[-1] != D or not pos.is_contiguous():
        raise X2IError("x2i_amd: cls must hold D = %d elements and pos be a contiguous [1+L, D] = [%d, %d] table (got cls %s, pos %s)"
                       % (D, S, D, tuple(cls.shape), tuple(pos.shape)))
    check(load().x2i_internvit_embed_bf16(ops._p(X), ops._p(cls), ops._p(pos), B, S - 1, D, ops._stream()), "internvit_embed")
    return X


def shuffle_ln(X, weight, bias, eps, out, g, v1=False, ldy=None):
    """X bf16 [B, 1+g*g, D] (unit stride along a row) -> out rows [B*(g/2)^2] of 4*D: class token dropped, pixel_shuffle(0.5) ('v2', or 'v1'
    with v1=True), LayerNorm(4*D) with weight / bias bf16 [4*D]; x2i_ln_affine_bf16 of the gathered row bit for bit.  Columns >= 4*D of out
    are not written."""
    ops._req(X, torch.bfloat16, "X")
    ops._req(out, torch.bfloat16, "out")
    ops._req(weight, torch.bfloat16, "weight")
    ops._req(bias, torch.bfloat16, "bias")
    if X.dim() != 3 or X.shape[1] != 1 + g * g or X.stride(2) != 1:
        raise X2IError("x2i_amd: X must be [B, 1 + g*g, D] with g = %d and unit stride along a row (got %s, strides %s)" % (g, tuple(X.shape), X.stride()))
    B, _, D = X.shape
    rows = B * (g // 2) ** 2
    if weight.numel() != 4 * D or bias.numel() != 4 * D or not weight.is_contiguous() or not bias.is_contiguous():
        raise X2IError("x2i_amd: weight and bias must hold 4*D = %d elements (got %s, %s)" % (4 * D, tuple(weight.shape), tuple(bias.shape)))
    ldy = out.stride(-2) if ldy is None else ldy
    if out.shape[-1] < 4 * D or out.numel() // out.shape[-1] < rows:
        raise X2IError("x2i_amd: out must hold B*(g/2)^2 = %d rows of at least 4*D = %d columns (got %s)" % (rows, 4 * D, tuple(out.shape)))
    check(load().x2i_internvit_shuffle_ln_bf16(ops._p(X), X.stride(0) if B > 1 else X.shape[1] * X.stride(1), X.stride(1), ops._p(out), ldy,
                                               ops._p(weight), ops._p(bias), B, g, D, eps, 1 if v1 else 0, ops._stream()), "internvit_shuffle_ln")
    return out
