"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_whisper.h: the MiniCPM-o Whisper audio tower's kernels (csrc/whisper.hip).

The two entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like ops.py
and the other *_ops.py modules: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing
here allocates behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/x2i_whisper.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_whisper_mel_rows_bf16": [_vp, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
    "x2i_whisper_pool_rows_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp],
}

pad64 = _lib.pad64


load = _lib.extension("x2i_whisper.h", _EXPORTS)


def pooled_rows(S, k):
    """Rows AvgPool1d(k, stride=k) makes of S: (S - k) // k + 1, and 0 where S < k"""
    return (S - k) // k + 1 if 1 <= k <= S else 0


def _mel_rows_args(mel, Xr, Kp, ldx=None):
    """The one place the arguments of x2i_whisper_mel_rows_bf16 are put together (field order of include/x2i_whisper.h)"""
    ops._req(mel, torch.bfloat16, "mel")
    ops._req(Xr, torch.bfloat16, "Xr")
    if mel.dim() != 3 or not mel.numel():
        raise X2IError("x2i_amd: mel must be a non-empty [B, Cin, T] tensor (got %s)" % (tuple(mel.shape),))
    B, Cin, T = mel.shape
    if T > 1 and mel.stride(2) != 1:
        raise X2IError("x2i_amd: mel must have unit stride along time (strides %s)" % (mel.stride(),))
    ld = mel.stride(1) if Cin > 1 else T
    ldx = Xr.stride(-2) if ldx is None else ldx
    if Xr.shape[-1] < Kp or Xr.numel() // Xr.shape[-1] < B * T:
        raise X2IError("x2i_amd: Xr must hold B*T = %d rows of at least Kp = %d columns (got %s)" % (B * T, Kp, tuple(Xr.shape)))
    return (ops._p(mel), mel.stride(0) if B > 1 else Cin * ld, ld, ops._p(Xr), ldx, B, Cin, T, Kp)


def mel_rows(mel, Xr, Kp, ldx=None):
    """mel bf16 [B, Cin, T] (unit stride along time) -> Xr rows [B*T]: column ci*3 + k < 3*Cin holds mel[b][ci][t + k - 1] (zero outside
    [0, T)), columns up to Kp are zero; nothing at or beyond column Kp is written."""
    check(load().x2i_whisper_mel_rows_bf16(*_mel_rows_args(mel, Xr, Kp, ldx), ops._stream()), "whisper_mel_rows")
    return Xr


def _pool_rows_args(X, Y, B, S, D, k, x_batch_stride=None, ldx=None, y_batch_stride=None, ldy=None):
    """The one place the arguments of x2i_whisper_pool_rows_bf16 are put together"""
    ops._req(X, torch.bfloat16, "X")
    ops._req(Y, torch.bfloat16, "Y")
    ldx = X.stride(-2) if ldx is None else ldx
    ldy = Y.stride(-2) if ldy is None else ldy
    n = pooled_rows(S, k)
    xbs = S * ldx if x_batch_stride is None else x_batch_stride
    ybs = n * ldy if y_batch_stride is None else y_batch_stride
    if ldx > 0 and X.numel() < (B - 1) * xbs + (S - 1) * ldx + D or ldy > 0 and n > 0 and Y.numel() < (B - 1) * ybs + (n - 1) * ldy + D:
        raise X2IError("x2i_amd: X must hold B = %d samples of S = %d rows and Y of %d rows of D = %d columns (got X %s, Y %s)"
                       % (B, S, n, D, tuple(X.shape), tuple(Y.shape)))
    return (ops._p(X), xbs, ldx, ops._p(Y), ybs, ldy, B, S, D, k)


def pool_rows(X, Y, B, S, D, k, **kw):
    """Y[b][j] = bf16(sum_{i<k} float(X[b][k*j + i]) / k) for j < (S - k) // k + 1: AvgPool1d(k, stride=k) over the time axis of token-major
    rows (the f32 sum in index order, one division, one rounding).  X: B samples of S rows (row stride ldx, batch stride S * ldx unless
    given); Y likewise with the pooled row count."""
    check(load().x2i_whisper_pool_rows_bf16(*_pool_rows_args(X, Y, B, S, D, k, **kw), ops._stream()), "whisper_pool_rows")
    return Y
