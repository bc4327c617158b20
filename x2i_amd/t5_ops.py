"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_t5.h: the T5 encoder's kernels (csrc/t5.hip, csrc/encoder_attention.hip).

The four entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like
ops.py: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind the
caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_t5.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_t5_attention_bf16": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i64, _vp],
    "x2i_t5_head_split_bf16": [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "x2i_t5_rms_rows_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _f32, _vp],
    "x2i_t5_gated_gelu_bf16": [_vp, _i64, _vp, _i64, _i64, _i32, _vp],
}

pad64 = _lib.pad64


load = _lib.extension("x2i_t5.h", _EXPORTS)


def attention_relbias(Q, K, VT, bias_tab, out, B, H, S, Spad, dk, R, ldo, o_batch_stride, o_offset=0):
    """O = softmax(Q K^T + bias_tab[h][clamp(j - i, -R, R) + R]) V, no scale, keys >= S masked by index (x2i_t5_attention_bf16).
    Q, K bf16 [B,H,Spad,dk]; VT bf16 [B,H,dk,Spad], zero beyond S; bias_tab f32 [H, 2R+1]; out token-major (offset, ldo, batch stride)."""
    ops._req(Q, torch.bfloat16, "Q")
    ops._req(bias_tab, torch.float32, "bias_tab")
    if tuple(bias_tab.shape) != (H, 2 * R + 1) or not bias_tab.is_contiguous():
        raise X2IError("x2i_amd: bias_tab must be a contiguous f32 [H, 2R+1] = [%d, %d] tensor (got %s)" % (H, 2 * R + 1, tuple(bias_tab.shape)))
    check(load().x2i_t5_attention_bf16(ops._p(Q), ops._p(K), ops._p(VT), ops._p(bias_tab), ops._off(out, o_offset), B, H, S, Spad, dk, R, ldo,
                                       o_batch_stride, ops._stream()), "t5_attention")
    return out


def head_split(qkv, Q, K, VT, B, S, Spad, H, dk, ld=None):
    """Rows [B*S, q|k|v] of the fused projection -> Q, K [B,H,Spad,dk] and VT [B,H,dk,Spad]; only rows / columns < S are written."""
    ops._req(qkv, torch.bfloat16, "qkv")
    check(load().x2i_t5_head_split_bf16(ops._p(qkv), qkv.stride(-2) if ld is None else ld, ops._p(Q), ops._p(K), ops._p(VT), B, S, Spad, H, dk,
                                        ops._stream()), "t5_head_split")


def rms_rows(X, weight, eps, out=None, rows=None, ldx=None, ldy=None):
    """T5LayerNorm: y = bf16(w * x * rsqrt(mean(x^2) + eps)), f32 throughout and one rounding, over the last dimension of X (rows addressed by ldx / ldy)."""
    ops._req(X, torch.bfloat16, "X")
    ops._req(weight, torch.bfloat16, "weight")
    D = X.shape[-1]
    out = torch.empty_like(X) if out is None else out
    rows = X.numel() // D if rows is None else rows
    check(load().x2i_t5_rms_rows_bf16(ops._p(X), D if ldx is None else ldx, ops._p(out), D if ldy is None else ldy, ops._p(weight), rows, D, eps,
                                      ops._stream()), "t5_rms_rows")
    return out


def gated_gelu(AB, out=None, rows=None, ld_in=None, ldy=None):
    """Rows [a (F) | b (F)] -> y = bf16(gelu_tanh(a) * b) (one rounding), [rows, F]."""
    ops._req(AB, torch.bfloat16, "AB")
    F = AB.shape[-1] // 2
    rows = AB.numel() // (2 * F) if rows is None else rows
    out = torch.empty(AB.shape[:-1] + (F,), device=AB.device, dtype=torch.bfloat16) if out is None else out
    check(load().x2i_t5_gated_gelu_bf16(ops._p(AB), 2 * F if ld_in is None else ld_in, ops._p(out), F if ldy is None else ldy, rows, F,
                                        ops._stream()), "t5_gated_gelu")
    return out
