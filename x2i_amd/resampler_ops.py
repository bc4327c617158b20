"""ctypes binding and torch-tensor wrappers of the extension header include/x2i_resampler.h: the MiniCPM-o Resampler's kernels (csrc/resampler.hip).

The three entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like
ops.py and the other *_ops.py: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing
here allocates behind the caller's back or synchronises, and there is no fallback.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/x2i_resampler.h: name -> argtypes (all return int).  tests/test_extension_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_resampler_attention_bf16": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i64, _i64, _vp],
    "x2i_resampler_ln_pos_bf16": [_vp, _i64, _vp, _vp, _f32, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _i64, _i32, _vp],
    "x2i_resampler_kv_split_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
}

DK = 128                 # the one head width (embed_dim // 128 heads by construction in the model's init_resampler)
NQ_MAX = 64
pad64 = _lib.pad64


def pad32(n):
    """NQpad: the rows a head of Q holds"""
    return (n + 31) // 32 * 32


load = _lib.extension("x2i_resampler.h", _EXPORTS)


def attention(Q, K, VT, out, B, H, NQ, L, Lpad, scale, ldo, o_batch_stride, n_keys=None):
    """Q [H, NQpad, 128] (shared by the B samples), K [B, H, Lpad, 128], VT [B, H, 128, Lpad] -> out rows i < NQ of sample b at
    b * o_batch_stride + i * ldo, head h at columns 128h ..; n_keys: int32 [B] on the device (None: L keys everywhere)."""
    for t, name in ((Q, "Q"), (K, "K"), (VT, "VT"), (out, "out")):
        ops._req(t, torch.bfloat16, name)
    if n_keys is not None:
        ops._req(n_keys, torch.int32, "n_keys")
        if not n_keys.is_contiguous() or n_keys.numel() < B:
            raise X2IError("x2i_amd: n_keys must be a contiguous int32 [B] = [%d] tensor (got %s)" % (B, tuple(n_keys.shape)))
    if 1 <= NQ <= NQ_MAX and B >= 1 and H >= 1 and Lpad >= 1:
        if Q.numel() < H * pad32(NQ) * DK or min(K.numel(), VT.numel()) < B * H * Lpad * DK:
            raise X2IError("x2i_amd: Q must hold H*NQpad*128 = %d elements and K, VT B*H*Lpad*128 = %d each" % (H * pad32(NQ) * DK, B * H * Lpad * DK))
        if ldo >= H * DK and out.numel() < (B - 1) * o_batch_stride + (NQ - 1) * ldo + H * DK:
            raise X2IError("x2i_amd: out is too small for B=%d samples of NQ=%d rows (ldo=%d, o_batch_stride=%d)" % (B, NQ, ldo, o_batch_stride))
    check(load().x2i_resampler_attention_bf16(ops._p(Q), ops._p(K), ops._p(VT), ops._p(n_keys), ops._p(out), B, H, NQ, L, Lpad, scale, ldo,
                                              o_batch_stride, ops._stream()), "resampler_attention")
    return out


def ln_pos(X, weight, bias, eps, ids, pos, XV, XK, rows=None, ldx=None, ldv=None, ldk=None):
    """XV[r] = ln_affine(X[r]); XK[r] = bf16(XV[r] + pos[ids[r]]), XK[r] = XV[r] where ids[r] < 0; ids int32 [rows] on the device, ids beyond
    the table clamped into it.  D = pos.shape[-1]; columns >= D of the three row buffers are untouched."""
    for t, name in ((X, "X"), (weight, "weight"), (bias, "bias"), (pos, "pos"), (XV, "XV"), (XK, "XK")):
        ops._req(t, torch.bfloat16, name)
    ops._req(ids, torch.int32, "ids")
    D = pos.shape[-1]
    rows = X.numel() // X.shape[-1] if rows is None else rows
    if pos.dim() != 2 or not pos.is_contiguous() or not ids.is_contiguous() or ids.numel() != rows or weight.numel() != D or bias.numel() != D:
        raise X2IError("x2i_amd: pos must be a contiguous [n_pos, D] table, weight and bias [D] and ids a contiguous int32 [rows] = [%d] tensor "
                       "(got pos %s, weight %s, ids %s)" % (rows, tuple(pos.shape), tuple(weight.shape), tuple(ids.shape)))
    for t, name in ((X, "X"), (XV, "XV"), (XK, "XK")):
        if t.shape[-1] < D or t.numel() // t.shape[-1] < rows:
            raise X2IError("x2i_amd: %s must hold rows = %d rows of at least D = %d columns (got %s)" % (name, rows, D, tuple(t.shape)))
    check(load().x2i_resampler_ln_pos_bf16(ops._p(X), X.stride(-2) if ldx is None else ldx, ops._p(weight), ops._p(bias), eps, ops._p(ids), ops._p(pos),
                                           pos.shape[0], ops._p(XV), XV.stride(-2) if ldv is None else ldv, ops._p(XK),
                                           XK.stride(-2) if ldk is None else ldk, rows, D, ops._stream()), "resampler_ln_pos")
    return XV, XK


def kv_split(Kr, Vr, K, VT, B, L, Lpad, H, ldk=None, ldv=None):
    """Rows [B*L, H*128] of the k and of the v projection (views into one buffer are fine) -> K [B,H,Lpad,128] and VT [B,H,128,Lpad]; only
    rows / columns s < L are written."""
    ops._req(Kr, torch.bfloat16, "Kr")
    ops._req(Vr, torch.bfloat16, "Vr")
    ops._req(K, torch.bfloat16, "K")
    ops._req(VT, torch.bfloat16, "VT")
    if B >= 1 and H >= 1 and Lpad >= 1 and L >= 1:
        if min(K.numel(), VT.numel()) < B * H * Lpad * DK:
            raise X2IError("x2i_amd: K, VT must hold B*H*Lpad*128 = %d elements each" % (B * H * Lpad * DK))
        if min(Kr.shape[-1], Vr.shape[-1]) < H * DK or min(Kr.numel() // Kr.shape[-1], Vr.numel() // Vr.shape[-1]) < B * L:
            raise X2IError("x2i_amd: Kr, Vr must hold B*L = %d rows of H*128 = %d columns (got %s, %s)" % (B * L, H * DK, tuple(Kr.shape), tuple(Vr.shape)))
    check(load().x2i_resampler_kv_split_bf16(ops._p(Kr), Kr.stride(-2) if ldk is None else ldk, ops._p(Vr), Vr.stride(-2) if ldv is None else ldv,
                                             ops._p(K), ops._p(VT), B, L, Lpad, H, ops._stream()), "resampler_kv_split")
