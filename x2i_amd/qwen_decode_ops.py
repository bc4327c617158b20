"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_qwen_decode.h: the kernels of Qwen2 decoding with a key/value
cache (csrc/qwen_decode.hip).

Like qwen_ops.py: the entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds
them.  PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind the
caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_qwen_decode.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_qwen_decode_rope_append_bf16": [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "x2i_qwen_decode_attention_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp],
    "x2i_qwen_decode_linear_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
}

CHUNK = 256   # X2I_QWEN_DECODE_CHUNK of the header

load = _lib.extension("x2i_qwen_decode.h", _EXPORTS)


def workspace_floats(B, Hq, cap, dk):
    """X2I_QWEN_DECODE_WS_FLOATS of the header: f32 elements of attention's workspace"""
    return B * Hq * ((cap + CHUNK - 1) // CHUNK) * (dk + 2)


def _vec(t, B, name):
    ops._req(t, torch.int32, name)
    if tuple(t.shape) != (B,) or not t.is_contiguous():
        raise X2IError("x2i_amd: %s must be a contiguous int32 [%d] tensor (got %s)" % (name, B, tuple(t.shape)))
    return t


def rope_append(qkv, cos, sin, slot, Qd, K, VT, B, Hq, Hkv, cap, dk, ld=None):
    """One row per sample of the fused q|k|v projection -> rotate-half RoPE on q and k -> Qd [B,Hq,dk], row slot[b] of K [B,Hkv,cap,dk] and
    column slot[b] of VT [B,Hkv,dk,cap]; cos, sin f32 [B, dk/2]; slot int32 [B] on the device (outside [0, cap): nothing is written)."""
    ops._req(qkv, torch.bfloat16, "qkv")
    for t, name in ((Qd, "Qd"), (K, "K"), (VT, "VT")):
        ops._req(t, torch.bfloat16, name)
    for t, name in ((cos, "cos"), (sin, "sin")):
        ops._req(t, torch.float32, name)
        if tuple(t.shape) != (B, dk // 2) or not t.is_contiguous():
            raise X2IError("x2i_amd: %s must be a contiguous f32 [B, dk/2] = [%d, %d] tensor (got %s)" % (name, B, dk // 2, tuple(t.shape)))
    check(load().x2i_qwen_decode_rope_append_bf16(ops._p(qkv), qkv.stride(-2) if ld is None else ld, ops._p(cos), ops._p(sin),
                                                  ops._p(_vec(slot, B, "slot")), ops._p(Qd), ops._p(K), ops._p(VT), B, Hq, Hkv, cap, dk,
                                                  ops._stream()), "qwen_decode_rope_append")


def attention(Qd, K, VT, k_lo, k_hi, out, ws, B, Hq, Hkv, cap, dk, scale, ldo=None, o_offset=0):
    """O[b] = softmax(scale q k^T) v of one query per head over the keys k_lo[b] <= j < k_hi[b] (int32 [B] on the device), masked by index;
    query head h reads key/value head h // (Hq // Hkv); an empty range gives exactly 0.  Qd bf16 [B,Hq,dk]; K bf16 [B,Hkv,cap,dk]; VT bf16
    [B,Hkv,dk,cap], finite everywhere; ws f32, at least workspace_floats(B, Hq, cap, dk) elements; out bf16 rows of ldo elements."""
    ops._req(Qd, torch.bfloat16, "Qd")
    ops._req(K, torch.bfloat16, "K")
    ops._req(VT, torch.bfloat16, "VT")
    ops._req(out, torch.bfloat16, "out")
    ops._req(ws, torch.float32, "ws")
    check(load().x2i_qwen_decode_attention_bf16(ops._p(Qd), ops._p(K), ops._p(VT), ops._p(_vec(k_lo, B, "k_lo")), ops._p(_vec(k_hi, B, "k_hi")),
                                                ops._off(out, o_offset), ops._p(ws), ws.numel(), B, Hq, Hkv, cap, dk, scale,
                                                out.stride(-2) if ldo is None else ldo, ops._stream()), "qwen_decode_attention")
    return out


def linear(X, W, bias=None, res=None, out=None, gate=False, B=None, N=None, ldx=None, ldw=None, ldr=None, ldy=None, y_offset=0, res_offset=0):
    """Y = bf16(X W^T + bias (+ res)) for 1..8 rows X [B, K], W bf16 [N, K]; gate=True: W is the stacked [gate_proj; up_proj] weight [2N, K]
    and Y = bf16(silu(a) * b).  f32 sums, one rounding; a row's result does not depend on B (x2i_qwen_decode_linear_bf16)."""
    ops._req(X, torch.bfloat16, "X")
    ops._req(W, torch.bfloat16, "W")
    for t, name in ((bias, "bias"), (res, "res"), (out, "out")):
        if t is not None:
            ops._req(t, torch.bfloat16, name)
    K = X.shape[-1]
    B = X.numel() // K if B is None else B
    N = (W.shape[0] // 2 if gate else W.shape[0]) if N is None else N
    if out is None:
        out = torch.empty((B, N), device=X.device, dtype=torch.bfloat16)
    check(load().x2i_qwen_decode_linear_bf16(ops._p(X), X.stride(-2) if ldx is None else ldx, ops._p(W), W.stride(0) if ldw is None else ldw,
                                             ops._p(bias), ops._off(res, res_offset), (res.stride(-2) if res is not None else 0) if ldr is None else ldr,
                                             ops._off(out, y_offset), out.stride(-2) if ldy is None else ldy, B, N, K, 1 if gate else 0,
                                             ops._stream()), "qwen_decode_linear")
    return out
