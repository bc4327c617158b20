"""ctypes binding and torch-tensor wrapper of the extension header include/ext/sample/x2i_sample.h: sampled token selection of Qwen2
decoding (csrc/qwen_sample.hip).

The entry point is not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds it.  Like ops.py and
the *_ops.py modules: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here
allocates behind the caller's back or synchronises, and there is no fallback.  (The module is not called sample_ops.py: the set of
*_ops.py modules mirrors the closed set of include/x2i_*.h headers.)
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# Every export of include/ext/sample/x2i_sample.h: name -> argtypes (all return int).  tests/test_sample_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_sample_select_f32": [_vp, _i64, _vp, _i64, _f32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i64, _vp,
                              _i64, _i32, _i32, _vp],
}

DIAG_FLOATS = 4     # X2I_SAMPLE_DIAG_FLOATS of the header
MASS_BITS = 34      # X2I_SAMPLE_MASS_BITS of the header

load = _lib.extension("ext/sample/x2i_sample.h", _EXPORTS)


def head_workspace_floats(B, V):
    """X2I_SAMPLE_HEAD_WS_FLOATS of the header: the head launch's workspace, which this entry point reads"""
    return 4 + 2 * B * ((V + 15) // 16)


def _opt(t, dtype, name):
    if t is not None:
        ops._req(t, dtype, name)
    return t


def select(logits, ws, step, token, sequences, lengths, done, pad, temperature=1.0, top_k=0, top_p=1.0, rng=None, u=None, diag=None, eos=None,
           seen=None, B=None, V=None, ncols=None, ldl=None, ld_seq=None, ld_seen=None, n_eos=None):
    """The sampled next token of every sample from the f32 scores [B, V] and the partials that qwen_head_ops.logits_argmax(..., logits=logits)
    left, and the bookkeeping of one generated token as qwen_head_ops.select does it.  rng int64 [2] = (seed, offset) on the device, or u
    f32 [B] in [0, 1); diag f32 [B, 4] or None (x2i_sample_select_f32)."""
    ops._req(logits, torch.float32, "logits")
    ops._req(ws, torch.float32, "ws")
    ops._req(step, torch.int32, "step")
    for t, name in ((token, "token"), (sequences, "sequences"), (lengths, "lengths")):
        ops._req(t, torch.int64, name)
    _opt(rng, torch.int64, "rng")
    _opt(u, torch.float32, "u")
    _opt(diag, torch.float32, "diag")
    _opt(eos, torch.int64, "eos")
    _opt(seen, torch.uint8, "seen")
    if done.dtype not in (torch.uint8, torch.bool):
        raise X2IError("x2i_amd: done must be a uint8 or bool tensor (got %s)" % done.dtype)
    ops._req(done, done.dtype, "done")
    B = token.numel() if B is None else B
    V = logits.shape[-1] if V is None else V
    if done.numel() < B or lengths.numel() < B or not done.is_contiguous() or not lengths.is_contiguous() or not token.is_contiguous():
        raise X2IError("x2i_amd: token, lengths and done must be contiguous [B] = [%d] tensors" % B)
    if (rng is not None and (rng.numel() < 2 or not rng.is_contiguous())) or (u is not None and (u.numel() < B or not u.is_contiguous())) or (
            diag is not None and (diag.numel() < DIAG_FLOATS * B or not diag.is_contiguous())):
        raise X2IError("x2i_amd: rng must hold 2, u B = %d and diag 4 B contiguous elements" % B)
    if logits.dim() < 2 or logits.stride(-1) != 1:
        raise X2IError("x2i_amd: logits must be a [B, V] tensor with unit stride along the vocabulary (got %s)" % (tuple(logits.shape),))
    check(load().x2i_sample_select_f32(
        ops._p(logits), logits.stride(-2) if ldl is None else ldl, ops._p(ws), ws.numel(), temperature, top_k, top_p, ops._p(rng), ops._p(u),
        ops._p(diag), ops._p(step), ops._p(token), ops._p(sequences), sequences.stride(-2) if ld_seq is None else ld_seq,
        sequences.shape[-1] if ncols is None else ncols, ops._p(lengths), ops._p(done), ops._p(eos),
        (eos.numel() if eos is not None else 0) if n_eos is None else n_eos, pad, ops._p(seen),
        (seen.stride(-2) if seen is not None else 0) if ld_seen is None else ld_seen, B, V, ops._stream()), "sample_select")
    return token


def rng_state(seed, offset, device):
    """(seed, offset) as the int64 [2] the kernel reads as uint64: values of 2^63 and above wrap to their two's complement"""
    wrap = lambda v: (int(v) & (2 ** 64 - 1)) - (2 ** 64 if int(v) & (1 << 63) else 0)
    return torch.tensor([wrap(seed), wrap(offset)], device=device, dtype=torch.int64)

