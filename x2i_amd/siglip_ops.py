"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_siglip.h: the MiniCPM-o SigLIP vision tower's kernels (csrc/siglip.hip).

The three entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like
ops.py, t5_ops.py, clip_ops.py, qwen_ops.py and vit_ops.py: PyTorch supplies device memory and the current stream, every computation happens
in libx2i_hip.so, nothing here allocates behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops, vit_ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/x2i_siglip.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_siglip_patch_rows_bf16": [_vp, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
    "x2i_siglip_add_positions_bf16": [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _vp],
    "x2i_siglip_head_split_bf16": [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
}

pad64 = _lib.pad64
stored_width = vit_ops.stored_width      # heads of 80 are stored 128 wide (include/x2i_vit.h)


load = _lib.extension("x2i_siglip.h", _EXPORTS)


def patch_rows(strips, Xp, P, Kp, ldx=None):
    """strips bf16 [B, 3, P, P*L] (unit stride along the strip, channel stride P times the row stride) -> Xp rows [B*L]: columns
    ci*P*P + r*P + c < 3*P*P hold strips[b][ci][r][P*p + c], columns up to Kp are zero; nothing at or beyond column Kp is written."""
    ops._req(strips, torch.bfloat16, "strips")
    ops._req(Xp, torch.bfloat16, "Xp")
    if strips.dim() != 4 or strips.shape[1] != 3 or strips.shape[2] != P or strips.shape[3] % P:
        raise X2IError("x2i_amd: strips must be [B, 3, P, P*L] with P = %d (got %s)" % (P, tuple(strips.shape)))
    B, L = strips.shape[0], strips.shape[3] // P
    ld = strips.stride(2)
    if strips.stride(3) != 1 or strips.stride(1) != P * ld:
        raise X2IError("x2i_amd: strips must have unit stride along the strip and channels P rows apart (strides %s)" % (strips.stride(),))
    ldx = Xp.stride(-2) if ldx is None else ldx
    if Xp.numel() and (Xp.shape[-1] < Kp or Xp.numel() // Xp.shape[-1] < B * L):
        raise X2IError("x2i_amd: Xp must hold B*L = %d rows of at least Kp = %d columns (got %s)" % (B * L, Kp, tuple(Xp.shape)))
    check(load().x2i_siglip_patch_rows_bf16(ops._p(strips), strips.stride(0) if B > 1 else 3 * P * ld, ld, ops._p(Xp), ldx, B, L, P, Kp,
                                            ops._stream()), "siglip_patch_rows")
    return Xp


def add_positions(X, ids, pos, rows=None, ldx=None):
    """X[r] = bf16(X[r] + pos[ids[r]]) in place (one f32 add, one rounding); ids int32 [rows] on the device, clamped into the table."""
    ops._req(X, torch.bfloat16, "X")
    ops._req(pos, torch.bfloat16, "pos")
    ops._req(ids, torch.int32, "ids")
    D = pos.shape[-1]
    rows = X.numel() // X.shape[-1] if rows is None else rows
    if pos.dim() != 2 or not pos.is_contiguous() or not ids.is_contiguous() or ids.numel() != rows or X.shape[-1] < D:
        raise X2IError("x2i_amd: pos must be a contiguous [n_pos, D] table, ids a contiguous int32 [rows] = [%d] tensor and X at least D wide "
                       "(got pos %s, ids %s, X %s)" % (rows, tuple(pos.shape), tuple(ids.shape), tuple(X.shape)))
    check(load().x2i_siglip_add_positions_bf16(ops._p(X), X.stride(-2) if ldx is None else ldx, ops._p(ids), ops._p(pos), pos.shape[0], rows, D,
                                               ops._stream()), "siglip_add_positions")
    return X


def head_split(qkv, Q, K, VT, B, S, Spad, H, dk, ld=None):
    """Rows [B*S, q|k|v] of the fused projection -> Q, K [B,H,Spad,dkp] and VT [B,H,dkp,Spad], dkp = stored_width(dk); only rows / columns
    s < S, d < dk are written."""
    ops._req(qkv, torch.bfloat16, "qkv")
    need = B * H * Spad * stored_width(dk)
    if min(Q.numel(), K.numel(), VT.numel()) < need:
        raise X2IError("x2i_amd: Q, K, VT must hold B*H*Spad*%d = %d elements each" % (stored_width(dk), need))
    check(load().x2i_siglip_head_split_bf16(ops._p(qkv), qkv.stride(-2) if ld is None else ld, ops._p(Q), ops._p(K), ops._p(VT), B, S, Spad, H, dk,
                                            ops._stream()), "siglip_head_split")
