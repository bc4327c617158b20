"""ctypes binding and torch-tensor wrapper of the extension header include/x2i_qwen_decode_w8.h: the decode-step linear with an e4m3 weight
(csrc/qwen_decode_w8.hip).

Like qwen_decode_ops.py: the entry point is not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds
it.  PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind the
caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/x2i_qwen_decode_w8.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_qwen_decode_linear_w8_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
}

load = _lib.extension("x2i_qwen_decode_w8.h", _EXPORTS)


def linear_w8(X, W8, w_scale, bias=None, res=None, out=None, gate=False, B=None, N=None, ldx=None, ldw=None, ldr=None, ldy=None, y_offset=0,
              res_offset=0):
    """qwen_decode_ops.linear with the weight w_scale[n] * e4m3(W8[n][k]): Y = bf16(w_scale * (X e4m3(W8)^T) + bias (+ res)) for 1..8 rows
    X bf16 [B, K]; W8 torch.float8_e4m3fn or uint8 [N, K] (OCP e4m3fn codes; ldw in bytes), w_scale f32 [N]; gate=True: W8 and w_scale are
    those of the stacked [gate_proj; up_proj] weight [2N, K] and Y = bf16(silu(a) * b).  f32 sums, one rounding; a row's result does not
    depend on B (x2i_qwen_decode_linear_w8_bf16)."""
    ops._req(X, torch.bfloat16, "X")
    if W8.dtype not in (ops.FP8, torch.uint8):
        raise X2IError("x2i_amd: W8 must be %s or torch.uint8 (got %s)" % (ops.FP8, W8.dtype))
    ops._req(W8, W8.dtype, "W8")
    ops._req(w_scale, torch.float32, "w_scale")
    for t, name in ((bias, "bias"), (res, "res"), (out, "out")):
        if t is not None:
            ops._req(t, torch.bfloat16, name)
    K = X.shape[-1]
    B = X.numel() // K if B is None else B
    N = (W8.shape[0] // 2 if gate else W8.shape[0]) if N is None else N
    if w_scale.numel() < (2 * N if gate else N) or not w_scale.is_contiguous():
        raise X2IError("x2i_amd: w_scale must be a contiguous f32 tensor of %d elements (got %s)" % (2 * N if gate else N, tuple(w_scale.shape)))
    if out is None:
        out = torch.empty((B, N), device=X.device, dtype=torch.bfloat16)
    check(load().x2i_qwen_decode_linear_w8_bf16(ops._p(X), X.stride(-2) if ldx is None else ldx, ops._p(W8), W8.stride(0) if ldw is None else ldw,
                                                ops._p(w_scale), ops._p(bias), ops._off(res, res_offset),
                                                (res.stride(-2) if res is not None else 0) if ldr is None else ldr, ops._off(out, y_offset),
                                                out.stride(-2) if ldy is None else ldy, B, N, K, 1 if gate else 0, ops._stream()),
          "qwen_decode_linear_w8")
    return out
