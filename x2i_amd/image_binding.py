"""ctypes binding and torch-tensor wrapper of the extension header include/frontend/x2i_image.h: the MiniCPM-o image front end's kernel
(csrc/image.hip).

The entry point is not in _lib._EXPORTS (include/x2i.h's table is closed under ABI version 5); _lib.extension binds it.  Like ops.py and the
other bindings: PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates
behind the caller's back or synchronises, and there is no fallback.  (The module is not called image_ops.py: the set of *_ops.py modules
mirrors the closed set of include/x2i_*.h headers.)
"""
import ctypes as C
import math

import torch

from . import _lib, ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/frontend/x2i_image.h: name -> argtypes (all return int).  tests/test_image_boundary_cpu.py checks it against the header's prototypes.
_EXPORTS = {
    "x2i_image_frontend": [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _vp],
}

PATCH, MAX_PATCHES, MAX_IN, LDS_BYTES = 14, 70, 65535, 65536       # the compile-time constants of csrc/image.hip
PRECISION_BITS = 22


load = _lib.extension("frontend/x2i_image.h", _EXPORTS)


def ksize(n_in, n_out):
    """Taps per output of one axis (Pillow's ksize for BICUBIC); 0 where the axis does not resize"""
    return 0 if n_in == n_out else int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def window(n_in, n_out, xx):
    """(xmin, xmax) of output xx: Pillow's tap window, cut at the image's borders"""
    scale = n_in / n_out
    support = 2.0 * max(scale, 1.0)
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    return xmin, min(int(center + support + 0.5), n_in) - xmin


def lds_plan(in_h, out_h):
    """(rows, tile, pitch): the input rows a patch row's vertical taps reach at most, the patches of columns per workgroup (4, 2 or 1) and
    the bytes of an LDS row; X2IError where one patch of columns does not fit in 64 KiB -- the launcher's own plan and refusal"""
    rows = PATCH
    if in_h != out_h:
        rows = 0
        for p in range(out_h // PATCH):
            lo, _ = window(in_h, out_h, PATCH * p)
            lo2, cnt2 = window(in_h, out_h, PATCH * p + PATCH - 1)
            rows = max(rows, lo2 + cnt2 - lo)
    pitch = lambda t: (3 * PATCH * t + 3) // 4 * 4   # noqa: E731
    tile = 4
    while tile > 1 and rows * pitch(tile) > LDS_BYTES:
        tile //= 2
    if rows * pitch(tile) > LDS_BYTES:
        raise X2IError("x2i_amd: the image front end's LDS plan does not fit: in_h=%d -> out_h=%d needs %d rows of %d bytes, at most %d bytes"
                       % (in_h, out_h, rows, pitch(tile), LDS_BYTES))
    return rows, tile, pitch(tile)


def check_input_size(in_w, in_h):
    """X2IError for an input size that none of the three image entry points serves"""
    if not (1 <= in_w <= MAX_IN and 1 <= in_h <= MAX_IN):
        raise X2IError("x2i_amd: in_w=%d and in_h=%d must be in 1..65535" % (in_w, in_h))


def check_sizes(in_w, in_h, out_w, out_h):
    """X2IError for sizes the kernel does not serve (what the launcher refuses for the same sizes)"""
    check_input_size(in_w, in_h)
    for name, v in (("out_w", out_w), ("out_h", out_h)):
        if v < PATCH or v % PATCH or v > PATCH * MAX_PATCHES:
            raise X2IError("x2i_amd: %s=%d must be a multiple of 14 in 14..980" % (name, v))
    return lds_plan(in_h, out_h)


def _table(bound, coef, n_out, k, name):
    if k == 0:
        if bound is not None or coef is not None:
            raise X2IError("x2i_amd: the %s tables must be None where the axis does not resize" % name)
        return
    if bound is None or coef is None:
        raise X2IError("x2i_amd: the %s tables are missing" % name)
    ops._req(bound, torch.int32, name + " bound")
    ops._req(coef, torch.int32, name + " coef")
    if tuple(bound.shape) != (n_out, 2) or tuple(coef.shape) != (n_out, k) or not bound.is_contiguous() or not coef.is_contiguous():
        raise X2IError("x2i_amd: the %s tables must be contiguous [%d, 2] and [%d, %d] (got %s, %s)"
                       % (name, n_out, n_out, k, tuple(bound.shape), tuple(coef.shape)))


def _shared_args(frames, lut, out, sizes, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, hbound, hcoef, vbound, vcoef):
    """What x2i_image_frontend, x2i_image_tiles and x2i_image_rows check alike about their arguments, in the order their refusals fire: the
    dtypes; sizes(), the entry point's own size rules; the tables of both axes; lut; contiguity; the n frames within `frames`.
    -> (hk, vk, what sizes() returned)"""
    ops._req(frames, torch.uint8, "frames")
    ops._req(lut, torch.float32, "lut")
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise X2IError("x2i_amd: out must be float32 or bfloat16 (got %s)" % out.dtype)
    ops._req(out, out.dtype, "out")
    own = sizes()
    hk, vk = ksize(in_w, out_w), ksize(in_h, out_h)
    _table(hbound, hcoef, out_w, hk, "horizontal")
    _table(vbound, vcoef, out_h, vk, "vertical")
    if tuple(lut.shape) != (3, 256) or not lut.is_contiguous():
        raise X2IError("x2i_amd: lut must be a contiguous [3, 256] tensor (got %s)" % (tuple(lut.shape),))
    if not frames.is_contiguous() or not out.is_contiguous():
        raise X2IError("x2i_amd: frames and out are flat buffers and must be contiguous")
    if n < 1 or row_pitch < 3 * in_w or frame_pitch < (in_h - 1) * row_pitch + 3 * in_w or frames.numel() < (n - 1) * frame_pitch + (in_h - 1) * row_pitch + 3 * in_w:
        raise X2IError("x2i_amd: frames holds %d bytes; %d frames of %d x %d with row_pitch %d and frame_pitch %d do not fit"
                       % (frames.numel(), n, in_w, in_h, row_pitch, frame_pitch))
    return hk, vk, own


def _frontend_args(frames, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, hbound, hcoef, vbound, vcoef, lut, out, out_frame_stride,
                   out_row_stride):
    """The one place the arguments of x2i_image_frontend are put together (field order of include/frontend/x2i_image.h)"""
    hk, vk, _ = _shared_args(frames, lut, out, lambda: check_sizes(in_w, in_h, out_w, out_h), in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h,
                             hbound, hcoef, vbound, vcoef)
    L14 = out_h // PATCH * out_w
    if out_row_stride < L14 or out_frame_stride < 3 * PATCH * out_row_stride or out.numel() < (n - 1) * out_frame_stride + (3 * PATCH - 1) * out_row_stride + L14:
        raise X2IError("x2i_amd: out holds %d elements; %d frames of [3, 14, %d] with row stride %d and frame stride %d do not fit"
                       % (out.numel(), n, L14, out_row_stride, out_frame_stride))
    return (ops._p(frames), frame_pitch, row_pitch, n, in_w, in_h, out_w, out_h, ops._p(hbound), ops._p(hcoef), hk, ops._p(vbound), ops._p(vcoef), vk,
            ops._p(lut), ops._p(out), out_frame_stride, out_row_stride, int(out.dtype == torch.bfloat16))


def frontend(frames, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, hbound, hcoef, vbound, vcoef, lut, out, out_frame_stride, out_row_stride):
    """frames: a flat uint8 device buffer, n frames of in_h rows of in_w RGB pixels with the given pitches in bytes -> out, a flat float32 or
    bf16 device buffer: frame f as [3][14][14 L] at f * out_frame_stride with rows out_row_stride apart (elements); only the 14 L columns of
    each row are written (include/frontend/x2i_image.h)"""
    args = _frontend_args(frames, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, hbound, hcoef, vbound, vcoef, lut, out, out_frame_stride,
                          out_row_stride)
    check(load().x2i_image_frontend(*args, ops._stream()), "image_frontend")
    return out
