"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_vit.h: the Qwen2.5-VL vision tower's kernels (csrc/vit.hip, csrc/encoder_attention.hip).

The two entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like ops.py,
t5_ops.py, clip_ops.py and qwen_ops.py: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so,
nothing here allocates behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_vit.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_vit_attention_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i64, _vp],
    "x2i_vit_rope_split_bf16": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
}

pad64 = _lib.pad64


def stored_width(dk):
    """The width heads of dk are stored at in Q, K (columns) and VT (rows): heads of 80 are stored 128 wide (include/x2i_vit.h)"""
    return 128 if dk == 80 else dk


load = _lib.extension("x2i_vit.h", _EXPORTS)


def _rows(t, B, S, name):
    if t is None:
        return None
    ops._req(t, torch.int32, name)
    if tuple(t.shape) != (B, S) or not t.is_contiguous():
        raise X2IError("x2i_amd: %s must be a contiguous int32 [B, S] = [%d, %d] tensor (got %s)" % (name, B, S, tuple(t.shape)))
    return t


def attention(Q, K, VT, out, B, H, S, Spad, dk, scale, ldo, o_batch_stride, row_lo=None, row_hi=None, o_offset=0):
    """O = softmax(scale Q K^T) V over the keys row_lo[b, i] <= j < row_hi[b, i], masked by index; a row with an empty range is exactly 0
    (x2i_vit_attention_bf16).  Q, K bf16 [B,H,Spad,dkp]; VT bf16 [B,H,dkp,Spad], dkp = stored_width(dk), finite in rows / columns < dk;
    row_lo, row_hi int32 [B, S] on the device or both None ([0, S)); out token-major (offset, ldo, batch stride), head h at column h * dk."""
    ops._req(Q, torch.bfloat16, "Q")
    ops._req(K, torch.bfloat16, "K")
    ops._req(VT, torch.bfloat16, "VT")
    need = B * H * Spad * stored_width(dk)
    if min(Q.numel(), K.numel(), VT.numel()) < need:
        raise X2IError("x2i_amd: Q, K, VT must hold B*H*Spad*%d = %d elements each" % (stored_width(dk), need))
    check(load().x2i_vit_attention_bf16(ops._p(Q), ops._p(K), ops._p(VT), ops._p(_rows(row_lo, B, S, "row_lo")), ops._p(_rows(row_hi, B, S, "row_hi")),
                                        ops._off(out, o_offset), B, H, S, Spad, dk, scale, ldo, o_batch_stride, ops._stream()), "vit_attention")
    return out


def rope_split(qkv, cos, sin, Q, K, VT, B, S, Spad, H, dk, ld=None):
    """Rows [B*S, q|k|v] of the qkv projection (biases added) -> rotate-half RoPE on q and k -> Q, K [B,H,Spad,dkp] and VT [B,H,dkp,Spad],
    dkp = stored_width(dk); cos, sin f32 [B,S,dk/2] (half tables); only rows / columns s < S, d < dk are written."""
    ops._req(qkv, torch.bfloat16, "qkv")
    for t, name in ((cos, "cos"), (sin, "sin")):
        ops._req(t, torch.float32, name)
        if tuple(t.shape) != (B, S, dk // 2) or not t.is_contiguous():
            raise X2IError("x2i_amd: %s must be a contiguous f32 [B, S, dk/2] = [%d, %d, %d] tensor (got %s)" % (name, B, S, dk // 2, tuple(t.shape)))
    need = B * H * Spad * stored_width(dk)
    if min(Q.numel(), K.numel(), VT.numel()) < need:
        raise X2IError("x2i_amd: Q, K, VT must hold B*H*Spad*%d = %d elements each" % (stored_width(dk), need))
    check(load().x2i_vit_rope_split_bf16(ops._p(qkv), qkv.stride(-2) if ld is None else ld, ops._p(cos), ops._p(sin), ops._p(Q), ops._p(K),
                                         ops._p(VT), B, S, Spad, H, dk, ops._stream()), "vit_rope_split")
