"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_qwen_head.h: token selection of greedy Qwen2 decoding
(csrc/qwen_head.hip).

Like qwen_decode_ops.py: the entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension
binds them.  PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind
the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_qwen_head.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_qwen_head_logits_argmax_bf16": [_vp, _i64, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp],
    "x2i_qwen_head_select": [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _i32, _i32, _vp],
}

ROWS = 16   # X2I_QWEN_HEAD_ROWS of the header

load = _lib.extension("x2i_qwen_head.h", _EXPORTS)


def workspace_floats(B, V):
    """X2I_QWEN_HEAD_WS_FLOATS of the header: f32 elements of the workspace the two calls share"""
    return 4 + 2 * B * ((V + ROWS - 1) // ROWS)


def _opt(t, dtype, name):
    if t is not None:
        ops._req(t, dtype, name)
    return t


def logits_argmax(X, W, ws, seen=None, penalty=1.0, logits=None, step=None, B=None, V=None, ldx=None, ldw=None, ld_seen=None, ldl=None):
    """The argmax partials of p = penalty(X W^T) for 1..8 rows X bf16 [B, K], W bf16 [V, K], into ws (f32, at least workspace_floats(B, V)
    elements); seen uint8 [B, V] or None; logits f32 [B, V] or None receives p; step int32 [1] or None is the column counter that
    select() advances (x2i_qwen_head_logits_argmax_bf16)."""
    ops._req(X, torch.bfloat16, "X")
    ops._req(W, torch.bfloat16, "W")
    ops._req(ws, torch.float32, "ws")
    _opt(seen, torch.uint8, "seen")
    _opt(logits, torch.float32, "logits")
    _opt(step, torch.int32, "step")
    K = X.shape[-1]
    B = X.numel() // K if B is None else B
    V = W.shape[0] if V is None else V
    check(load().x2i_qwen_head_logits_argmax_bf16(
        ops._p(X), X.stride(-2) if ldx is None else ldx, ops._p(W), W.stride(0) if ldw is None else ldw, ops._p(seen),
        (seen.stride(-2) if seen is not None else 0) if ld_seen is None else ld_seen, penalty, ops._p(logits),
        (logits.stride(-2) if logits is not None else 0) if ldl is None else ldl, ops._p(step), ops._p(ws), ws.numel(), B, V, K, ops._stream()),
        "qwen_head_logits_argmax")
    return ws


def select(ws, step, token, sequences, lengths, done, pad, V, eos=None, seen=None, B=None, ncols=None, ld_seq=None, ld_seen=None, n_eos=None):
    """The next token of every sample from the partials logits_argmax left in ws, and the bookkeeping of one generated token: token int64
    [B], sequences int64 [B, ncols] at column step[0], lengths int64 [B], done uint8 or bool [B], eos int64 [n_eos] or None, seen uint8
    [B, V] or None; step int32 [1] advances by one (x2i_qwen_head_select)."""
    ops._req(ws, torch.float32, "ws")
    ops._req(step, torch.int32, "step")
    for t, name in ((token, "token"), (sequences, "sequences"), (lengths, "lengths")):
        ops._req(t, torch.int64, name)
    _opt(eos, torch.int64, "eos")
    _opt(seen, torch.uint8, "seen")
    if done.dtype not in (torch.uint8, torch.bool):
        raise X2IError("x2i_amd: done must be a uint8 or bool tensor (got %s)" % done.dtype)
    ops._req(done, done.dtype, "done")
    B = token.numel() if B is None else B
    if done.numel() < B or lengths.numel() < B or not done.is_contiguous() or not lengths.is_contiguous() or not token.is_contiguous():
        raise X2IError("x2i_amd: token, lengths and done must be contiguous [B] = [%d] tensors" % B)
    check(load().x2i_qwen_head_select(
        ops._p(ws), ws.numel(), ops._p(step), ops._p(token), ops._p(sequences), sequences.stride(-2) if ld_seq is None else ld_seq,
        sequences.shape[-1] if ncols is None else ncols, ops._p(lengths), ops._p(done), ops._p(eos),
        (eos.numel() if eos is not None else 0) if n_eos is None else n_eos, pad, ops._p(seen),
        (seen.stride(-2) if seen is not None else 0) if ld_seen is None else ld_seen, B, V, ops._stream()), "qwen_head_select")
    return token
