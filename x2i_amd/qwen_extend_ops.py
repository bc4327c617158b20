"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_qwen_extend.h: the Qwen2 prompt extension's kernels
(csrc/qwen_extend.hip, csrc/encoder_attention.hip's CAUSAL_EXT mode).

Like qwen_decode_w8_ops.py: the entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension
binds them.  PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind
the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_qwen_extend.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_qwen_extend_rope_split_bf16": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "x2i_qwen_extend_attention_bf16": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i64, _vp],
}

load = _lib.extension("x2i_qwen_extend.h", _EXPORTS)


def rope_split(qkv, cos, sin, Q, K, VT, B, row0, n, cap, Hq, Hkv, dk, ld=None):
    """Rows [B*n, q|k|v] of the fused projection (biases added) -> rotate-half RoPE on q and k -> rows row0 .. row0+n-1 of Q [B,Hq,cap,dk]
    and K [B,Hkv,cap,dk], columns row0 .. row0+n-1 of VT [B,Hkv,dk,cap]; cos, sin f32 [B,n,dk/2] (the half tables of the chunk's positions);
    nothing else of Q, K, VT is written (x2i_qwen_extend_rope_split_bf16)."""
    ops._req(qkv, torch.bfloat16, "qkv")
    for t, name in ((Q, "Q"), (K, "K"), (VT, "VT")):
        ops._req(t, torch.bfloat16, name)
    for t, name in ((cos, "cos"), (sin, "sin")):
        ops._req(t, torch.float32, name)
        if tuple(t.shape) != (B, n, dk // 2) or not t.is_contiguous():
            raise X2IError("x2i_amd: %s must be a contiguous f32 [B, n, dk/2] = [%d, %d, %d] tensor (got %s)" % (name, B, n, dk // 2, tuple(t.shape)))
    check(load().x2i_qwen_extend_rope_split_bf16(ops._p(qkv), qkv.stride(-2) if ld is None else ld, ops._p(cos), ops._p(sin), ops._p(Q), ops._p(K),
                                                 ops._p(VT), B, row0, n, cap, Hq, Hkv, dk, ops._stream()), "qwen_extend_rope_split")


def attention(Q, K, VT, out, B, Hq, Hkv, row0, n, cap, dk, scale, ldo, o_batch_stride, k_lo=None, o_offset=0):
    """Rows row0 .. row0+n-1 of O = softmax(scale Q K^T) V over the keys k_lo[b] <= j <= i of a cache of cap slots, masked by index; query head
    h reads key/value head h // (Hq // Hkv); output row i - row0; rows with no counted key are exactly 0 (x2i_qwen_extend_attention_bf16).
    Q bf16 [B,Hq,cap,dk]; K bf16 [B,Hkv,cap,dk]; VT bf16 [B,Hkv,dk,cap], finite everywhere; k_lo int32 [B] on the device or None (0); out
    token-major (offset, ldo, batch stride)."""
    ops._req(Q, torch.bfloat16, "Q")
    ops._req(K, torch.bfloat16, "K")
    ops._req(VT, torch.bfloat16, "VT")
    if k_lo is not None:
        ops._req(k_lo, torch.int32, "k_lo")
        if tuple(k_lo.shape) != (B,) or not k_lo.is_contiguous():
            raise X2IError("x2i_amd: k_lo must be a contiguous int32 [%d] tensor (got %s)" % (B, tuple(k_lo.shape)))
    check(load().x2i_qwen_extend_attention_bf16(ops._p(Q), ops._p(K), ops._p(VT), ops._p(k_lo), ops._off(out, o_offset), B, Hq, Hkv, row0, n, cap, dk,
                                                scale, ldo, o_batch_stride, ops._stream()), "qwen_extend_attention")
    return out
