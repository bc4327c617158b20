"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_qwen.h: the Qwen2 decoder prefill's kernels (csrc/qwen.hip, csrc/encoder_attention.hip).

The three entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like
ops.py, t5_ops.py and clip_ops.py: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so,
nothing here allocates behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_qwen.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_qwen_attention_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i64, _vp],
    "x2i_qwen_rope_split_bf16": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "x2i_qwen_swiglu_bf16": [_vp, _i64, _vp, _i64, _i64, _i32, _vp],
}

pad64 = _lib.pad64


load = _lib.extension("x2i_qwen.h", _EXPORTS)


def _range(t, B, name):
    if t is None:
        return None
    ops._req(t, torch.int32, name)
    if tuple(t.shape) != (B,) or not t.is_contiguous():
        raise X2IError("x2i_amd: %s must be a contiguous int32 [%d] tensor (got %s)" % (name, B, tuple(t.shape)))
    return t


def attention(Q, K, VT, out, B, Hq, Hkv, S, Spad, dk, scale, ldo, o_batch_stride, k_lo=None, k_hi=None, o_offset=0):
    """O = softmax(scale Q K^T) V over the keys k_lo[b] <= j < k_hi[b], j <= i, masked by index; query head h reads key/value head
    h // (Hq // Hkv); rows with no counted key are exactly 0 (x2i_qwen_attention_bf16).  Q bf16 [B,Hq,Spad,dk]; K bf16 [B,Hkv,Spad,dk];
    VT bf16 [B,Hkv,dk,Spad], finite everywhere; k_lo, k_hi int32 [B] on the device or both None ([0, S)); out token-major (offset, ldo,
    batch stride)."""
    ops._req(Q, torch.bfloat16, "Q")
    ops._req(K, torch.bfloat16, "K")
    ops._req(VT, torch.bfloat16, "VT")
    check(load().x2i_qwen_attention_bf16(ops._p(Q), ops._p(K), ops._p(VT), ops._p(_range(k_lo, B, "k_lo")), ops._p(_range(k_hi, B, "k_hi")),
                                         ops._off(out, o_offset), B, Hq, Hkv, S, Spad, dk, scale, ldo, o_batch_stride, ops._stream()),
          "qwen_attention")
    return out


def rope_split(qkv, cos, sin, Q, K, VT, B, S, Spad, Hq, Hkv, dk, ld=None):
    """Rows [B*S, q|k|v] of the fused projection (biases added) -> rotate-half RoPE on q and k -> Q [B,Hq,Spad,dk], K [B,Hkv,Spad,dk], and
    VT [B,Hkv,dk,Spad]; cos, sin f32 [B,S,dk/2] (half tables); only rows / columns < S are written."""
    ops._req(qkv, torch.bfloat16, "qkv")
    for t, name in ((cos, "cos"), (sin, "sin")):
        ops._req(t, torch.float32, name)
        if tuple(t.shape) != (B, S, dk // 2) or not t.is_contiguous():
            raise X2IError("x2i_amd: %s must be a contiguous f32 [B, S, dk/2] = [%d, %d, %d] tensor (got %s)" % (name, B, S, dk // 2, tuple(t.shape)))
    check(load().x2i_qwen_rope_split_bf16(ops._p(qkv), qkv.stride(-2) if ld is None else ld, ops._p(cos), ops._p(sin), ops._p(Q), ops._p(K),
                                          ops._p(VT), B, S, Spad, Hq, Hkv, dk, ops._stream()), "qwen_rope_split")


def swiglu(AB, out=None, rows=None, ld_in=None, ldy=None):
    """Rows [a (F) | b (F)] -> y = bf16(silu(a) * b) (one rounding), [rows, F]."""
    ops._req(AB, torch.bfloat16, "AB")
    F = AB.shape[-1] // 2
    rows = AB.numel() // (2 * F) if rows is None else rows
    out = torch.empty(AB.shape[:-1] + (F,), device=AB.device, dtype=torch.bfloat16) if out is None else out
    check(load().x2i_qwen_swiglu_bf16(ops._p(AB), 2 * F if ld_in is None else ld_in, ops._p(out), F if ldy is None else ldy, rows, F,
                                      ops._stream()), "qwen_swiglu")
    return out
