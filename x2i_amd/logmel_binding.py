"""ctypes binding and torch-tensor wrappers of the extension header include/ext/x2i_logmel.h: the Whisper log-mel front end's kernels
(csrc/logmel.hip).

The two entry points are not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds them.  Like ops.py
and the *_ops.py modules: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing
here allocates behind the caller's back or synchronises, and there is no fallback.  (The module is not called logmel_ops.py: the set of
*_ops.py modules mirrors the closed set of include/x2i_*.h headers.)
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/ext/x2i_logmel.h: name -> argtypes (all return int).  tests/test_logmel_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_logmel_spectrum_f32": [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp],
    "x2i_logmel_finish": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp],
}

N_FFT, HOP, BINS = 400, 160, 201        # the compile-time constants of csrc/logmel.hip
FRAMES_PER_WG = 32
DFT_SHAPE, FBANK_SHAPE = (400, 448), (224, 128)
MAX_MELS = 128


load = _lib.extension("ext/x2i_logmel.h", _EXPORTS)


def frames(N_max):
    """T: frames of a chunk of N_max samples"""
    return N_max // HOP


def workspace_floats(B, N_max, n_mels):
    """(floats of lg, floats of part) that B samples need"""
    T = frames(N_max)
    return B * n_mels * T, B * ((T + FRAMES_PER_WG - 1) // FRAMES_PER_WG)


def kept_frames(n, N_max):
    """L: the frames the processor keeps of n samples, ceil(n / 160), at most T"""
    return min((n + HOP - 1) // HOP, frames(N_max))


def seen_frames(n, N_max):
    """A: the frames that can see one of n samples, all of which take part in the chunk's maximum"""
    return min(frames(N_max), (n + 199) // HOP + 1)


def _tables(dft, fbank):
    ops._req(dft, torch.float32, "dft")
    ops._req(fbank, torch.float32, "fbank")
    if tuple(dft.shape) != DFT_SHAPE or tuple(fbank.shape) != FBANK_SHAPE or not dft.is_contiguous() or not fbank.is_contiguous():
        raise X2IError("x2i_amd: dft must be a contiguous %s and fbank a contiguous %s tensor (got %s, %s)"
                       % (DFT_SHAPE, FBANK_SHAPE, tuple(dft.shape), tuple(fbank.shape)))


def _workspaces(lg, part):
    ops._req(lg, torch.float32, "lg")
    ops._req(part, torch.float32, "part")
    if not lg.is_contiguous() or not part.is_contiguous():
        raise X2IError("x2i_amd: the workspaces lg and part must be contiguous")


def _spectrum_args(wave, n, dft, fbank, lg, part, N_max, n_mels):
    """The one place the arguments of x2i_logmel_spectrum_f32 are put together (field order of include/ext/x2i_logmel.h)"""
    ops._req(wave, torch.float32, "wave")
    ops._req(n, torch.int32, "n")
    _tables(dft, fbank)
    _workspaces(lg, part)
    if wave.dim() != 2 or not wave.numel() or wave.stride(1) != 1:
        raise X2IError("x2i_amd: wave must be a non-empty [B, ldw] tensor with unit stride along the samples (got %s)" % (tuple(wave.shape),))
    B = wave.shape[0]
    if n.numel() != B or not n.is_contiguous():
        raise X2IError("x2i_amd: n must hold B = %d contiguous sample counts (got %s)" % (B, tuple(n.shape)))
    ldw = wave.stride(0) if B > 1 else wave.shape[1]
    if ldw < wave.shape[1]:
        raise X2IError("x2i_amd: the rows of wave overlap (strides %s)" % (wave.stride(),))
    return (ops._p(wave), ldw, ops._p(n), ops._p(dft), ops._p(fbank), ops._p(lg), lg.numel(), ops._p(part), part.numel(), B, N_max, n_mels)


def spectrum(wave, n, dft, fbank, lg, part, N_max, n_mels):
    """wave f32 [B, ldw], n int32 [B] (device) -> lg[b][m][t] = log10(max(mel power, 1e-10)) for the frames that can see a sample, and the
    per-workgroup maxima in part (include/ext/x2i_logmel.h)"""
    check(load().x2i_logmel_spectrum_f32(*_spectrum_args(wave, n, dft, fbank, lg, part, N_max, n_mels), ops._stream()), "logmel_spectrum")


def _finish_args(lg, part, n, out, N_max, n_mels, T_out=None):
    """The one place the arguments of x2i_logmel_finish are put together"""
    _workspaces(lg, part)
    ops._req(n, torch.int32, "n")
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise X2IError("x2i_amd: out must be float32 or bfloat16 (got %s)" % out.dtype)
    ops._req(out, out.dtype, "out")
    if out.dim() != 3 or not out.numel() or out.shape[1] != n_mels or (out.shape[2] > 1 and out.stride(2) != 1):
        raise X2IError("x2i_amd: out must be a non-empty [B, n_mels = %d, T_out] tensor with unit stride along time (got %s)" % (n_mels, tuple(out.shape)))
    B = out.shape[0]
    T_out = out.shape[2] if T_out is None else T_out
    if T_out > out.shape[2] or n.numel() != B or not n.is_contiguous():
        raise X2IError("x2i_amd: out holds %d columns for T_out = %d, n %s counts for B = %d" % (out.shape[2], T_out, tuple(n.shape), B))
    ld = out.stride(1) if n_mels > 1 else out.shape[2]
    return (ops._p(lg), lg.numel(), ops._p(part), part.numel(), ops._p(n), ops._p(out), out.stride(0) if B > 1 else n_mels * ld, ld, B, N_max, n_mels,
            T_out, int(out.dtype == torch.bfloat16))


def finish(lg, part, n, out, N_max, n_mels, T_out=None):
    """out[b][m][t] = (max(lg, mx_b - 8) + 4) / 4 for t < L_b and 0 up to T_out (default: out's columns); float32 or bf16 by out's dtype"""
    check(load().x2i_logmel_finish(*_finish_args(lg, part, n, out, N_max, n_mels, T_out), ops._stream()), "logmel_finish")
    return out
