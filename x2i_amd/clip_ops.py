"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_clip.h: the CLIP text encoder's kernels (csrc/clip.hip, csrc/encoder_attention.hip).

The four entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like ops.py
and t5_ops.py: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates
behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_clip.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_clip_attention_bf16": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i64, _vp],
    "x2i_clip_embed_bf16": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "x2i_clip_quick_gelu_bf16": [_vp, _i64, _vp, _i64, _i64, _i32, _vp],
    "x2i_clip_pool_bf16": [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
}

pad64 = _lib.pad64


load = _lib.extension("x2i_clip.h", _EXPORTS)


def attention_causal(Q, K, VT, out, B, H, S, Spad, dk, scale, ldo, o_batch_stride, o_offset=0):
    """O = softmax_{j <= i}(scale Q K^T) V, keys after a row's own index masked by index (x2i_clip_attention_bf16).
    Q, K bf16 [B,H,Spad,dk]; VT bf16 [B,H,dk,Spad], finite beyond S; out token-major (offset, ldo, batch stride)."""
    ops._req(Q, torch.bfloat16, "Q")
    ops._req(K, torch.bfloat16, "K")
    ops._req(VT, torch.bfloat16, "VT")
    check(load().x2i_clip_attention_bf16(ops._p(Q), ops._p(K), ops._p(VT), ops._off(out, o_offset), B, H, S, Spad, dk, scale, ldo,
                                         o_batch_stride, ops._stream()), "clip_attention")
    return out


def _ids(ids, B, S):
    if ids.device.type != "cuda":
        raise X2IError("x2i_amd: ids must live on the GPU (got %s); the HIP path has no CPU fallback" % ids.device)
    if ids.dtype != torch.int64 or tuple(ids.shape) != (B, S) or not ids.is_contiguous():
        raise X2IError("x2i_amd: ids must be a contiguous int64 [%d, %d] tensor (got %s %s)" % (B, S, ids.dtype, tuple(ids.shape)))
    return ids


def embed(ids, tok, pos, out=None):
    """CLIPTextEmbeddings: X[b*S+s] = bf16(float(tok[ids[b][s]]) + float(pos[s])), [B*S, D].  ids int64 [B, S]; an id outside the table is clamped."""
    ops._req(tok, torch.bfloat16, "tok")
    ops._req(pos, torch.bfloat16, "pos")
    B, S = ids.shape
    vocab, D = tok.shape
    if pos.shape[0] < S or pos.shape[1] != D or not tok.is_contiguous() or not pos.is_contiguous():
        raise X2IError("x2i_amd: pos must be a contiguous [>= %d, %d] table beside a contiguous tok (got %s)" % (S, D, tuple(pos.shape)))
    out = torch.empty((B * S, D), device=tok.device, dtype=torch.bfloat16) if out is None else out
    check(load().x2i_clip_embed_bf16(ops._p(_ids(ids, B, S)), ops._p(tok), ops._p(pos), ops._p(out), B, S, D, vocab, ops._stream()), "clip_embed")
    return out


def quick_gelu(X, out=None, rows=None, ldx=None, ldy=None):
    """y = bf16(x * sigmoid(1.702 x)) (one rounding) over the last dimension of X (rows addressed by ldx / ldy)."""
    ops._req(X, torch.bfloat16, "X")
    F = X.shape[-1]
    rows = X.numel() // F if rows is None else rows
    out = torch.empty_like(X) if out is None else out
    check(load().x2i_clip_quick_gelu_bf16(ops._p(X), F if ldx is None else ldx, ops._p(out), F if ldy is None else ldy, rows, F, ops._stream()),
          "clip_quick_gelu")
    return out


def pool(ids, Hs, eos_token_id, out=None, ldh=None, ldp=None):
    """pooled[b] = Hs[b*S + idx_b]: idx_b the first maximum of ids[b] (eos_token_id == 2) or the first eos_token_id (0 when there is none).
    ids int64 [B, S]; Hs bf16 [B*S, D] (or [B, S, D]); -> [B, D]."""
    ops._req(Hs, torch.bfloat16, "Hs")
    B, S = ids.shape
    D = Hs.shape[-1]
    out = torch.empty((B, D), device=Hs.device, dtype=torch.bfloat16) if out is None else out
    check(load().x2i_clip_pool_bf16(ops._p(_ids(ids, B, S)), ops._p(Hs), D if ldh is None else ldh, ops._p(out), D if ldp is None else ldp, B, S, D,
                                    eos_token_id, ops._stream()), "clip_pool")
    return out
