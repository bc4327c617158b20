"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_merge.h: the prompt merge in front of the Qwen2 decoder
stack (csrc/merge.hip).

Like qwen_head_ops.py: the entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds
them.  PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind the
caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_merge.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_merge_rank_i32": [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp],
    "x2i_embed_merge_bf16": [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _vp],
}

RANK_CHUNK = 2048          # X2I_MERGE_RANK_CHUNK of the header: rows per workgroup of the rank launches
SRC_ARRAY_BIT = 30         # X2I_MERGE_SRC_ARRAY_BIT: bit 30 of a non-negative src picks the feature array
SRC_ROW_MASK = 0x3fffffff  # X2I_MERGE_SRC_ROW_MASK: bits 0..29 are the row inside it

load = _lib.extension("x2i_merge.h", _EXPORTS)


def rank_workspace_ints(n):
    """X2I_MERGE_RANK_WS_INTS of the header: int32 elements of the rank's workspace"""
    return (n + RANK_CHUNK - 1) // RANK_CHUNK


def rank(ids, placeholder, src, total, ws):
    """src int32 [n] <- the exclusive rank of every row of ids (int64, contiguous, n elements in all) that equals placeholder, -1 elsewhere;
    total int32 [1] <- their number; ws int32, at least rank_workspace_ints(n) elements (x2i_merge_rank_i32)."""
    ops._req(ids, torch.int64, "ids")
    for t, name in ((src, "src"), (total, "total"), (ws, "ws")):
        ops._req(t, torch.int32, name)
    n = ids.numel()
    if not ids.is_contiguous() or not src.is_contiguous() or src.numel() != n:
        raise X2IError("x2i_amd: ids and src must be contiguous and of one size (got %d and %d elements)" % (n, src.numel()))
    check(load().x2i_merge_rank_i32(ops._p(ids), n, int(placeholder), ops._p(src), ops._p(total), ops._p(ws), ws.numel(), ops._stream()), "merge_rank")
    return src


def _rows(t, name):
    """(tensor, row stride, rows) of a bf16 [rows, H] array whose rows are contiguous; (None, 0, 0) for None"""
    if t is None:
        return None, 0, 0
    ops._req(t, torch.bfloat16, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise X2IError("x2i_amd: %s must be a [rows, H] tensor with contiguous rows (got shape %s, strides %s)" % (name, tuple(t.shape), t.stride()))
    return t, t.stride(0), t.shape[0]


def embed_merge(out, err, ids=None, src=None, table=None, scale=1.0, feat0=None, feat1=None, V=None, n0=None, n1=None):
    """out bf16 [B, S, H] (a view: last stride 1, a row stride and a batch stride, e.g. slab[:, 0] of a [B, C, S, H] slab) <- per row r = b * S
    + s: feat_a[k] when src[r] >= 0 (a = bit 30, k = bits 0..29), else bf16(scale * table[ids[r]]); with table None those rows are not touched.
    ids int64 [B, S] contiguous; src int32 [B * S] or None (every row a table row); table bf16 [V, H]; feat0 / feat1 bf16 [n, H] or None;
    err int32 [1]: 1 is stored when an id or a feature row is out of range, and that row is zeros (x2i_embed_merge_bf16).  V, n0, n1
    override the tensors' row counts."""
    ops._req(out, torch.bfloat16, "out")
    ops._req(err, torch.int32, "err")
    if out.dim() != 3 or out.stride(2) != 1:
        raise X2IError("x2i_amd: out must be a [B, S, H] view with contiguous rows (got shape %s, strides %s)" % (tuple(out.shape), out.stride()))
    B, S, H = out.shape
    if ids is not None:
        ops._req(ids, torch.int64, "ids")
        if ids.numel() != B * S or not ids.is_contiguous():
            raise X2IError("x2i_amd: ids must be a contiguous [B, S] = [%d, %d] tensor (got %s)" % (B, S, tuple(ids.shape)))
    if src is not None:
        ops._req(src, torch.int32, "src")
        if src.numel() != B * S or not src.is_contiguous():
            raise X2IError("x2i_amd: src must be a contiguous tensor of B * S = %d elements (got %s)" % (B * S, tuple(src.shape)))
    table, ldt, vt = _rows(table, "table")
    feat0, ldf0, c0 = _rows(feat0, "feat0")
    feat1, ldf1, c1 = _rows(feat1, "feat1")
    for t, name in ((table, "table"), (feat0, "feat0"), (feat1, "feat1")):
        if t is not None and t.shape[1] != H:
            raise X2IError("x2i_amd: %s has rows of %d elements, out of %d" % (name, t.shape[1], H))
    check(load().x2i_embed_merge_bf16(
        ops._p(ids), ops._p(src), ops._p(table), ldt, vt if V is None else V, float(scale), ops._p(feat0), ldf0, c0 if n0 is None else n0,
        ops._p(feat1), ldf1, c1 if n1 is None else n1, ops._p(out), out.stride(1), out.stride(0) if B > 1 else 0, ops._p(err), B, S, H,
        ops._stream()), "embed_merge")
    return out
