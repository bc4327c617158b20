"""ctypes binding and torch-tensor wrapper of the extension header include/frontend/rows/qwen/x2i_image_rows.h: the Qwen2.5-VL image
front end's kernel (csrc/image_rows.hip), raw frames to the patch rows [S, 1176] of Qwen2VLImageProcessor.

Like image_tiles_binding.py, whose tables, windows and LDS plan (image_binding.py) it shares: the entry point is not in _lib._EXPORTS,
_lib.extension binds it; PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here
allocates behind the caller's back or synchronises, and there is no fallback.  (Not called *_ops.py, for image_binding.py's reason.)
"""
import ctypes as C

import torch

from . import _lib, image_binding as ib, ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/frontend/rows/qwen/x2i_image_rows.h: name -> argtypes (all return int).  tests/test_image_rows_boundary_cpu.py
# checks it against the header's prototypes.
_EXPORTS = {
    "x2i_image_rows": [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _vp],
}

PATCH, UNIT, MAX_OUT, ROW, MAX_FRAMES = ib.PATCH, 28, 11760, 1176, 65535       # the compile-time constants of csrc/image_rows.hip

load = _lib.extension("frontend/rows/qwen/x2i_image_rows.h", _EXPORTS)


def check_sizes(in_w, in_h, out_w, out_h, n_items=1, t_in=1):
    """(grid_t, gh, gw) of an item; X2IError for sizes the kernel does not serve (what the launcher refuses for the same sizes)"""
    if n_items < 1 or t_in < 1 or n_items * t_in > MAX_FRAMES:
        raise X2IError("x2i_amd: n_items=%d and t_in=%d must be at least 1 and n_items * t_in in 1..65535" % (n_items, t_in))
    ib.check_input_size(in_w, in_h)
    for name, v in (("out_w", out_w), ("out_h", out_h)):
        if v < UNIT or v % UNIT or v > MAX_OUT:
            raise X2IError("x2i_amd: %s=%d must be a multiple of 28 in 28..11760" % (name, v))
    ib.lds_plan(in_h, out_h)
    return (t_in + 1) // 2, out_h // PATCH, out_w // PATCH


def _rows_args(frames, in_w, in_h, row_pitch, frame_pitch, n_items, t_in, out_w, out_h, hbound, hcoef, vbound, vcoef, lut, out,
               out_item_stride, out_row_stride):
    """The one place the arguments of x2i_image_rows are put together (field order of include/frontend/rows/qwen/x2i_image_rows.h)"""
    hk, vk, (grid_t, gh, gw) = ib._shared_args(frames, lut, out, lambda: check_sizes(in_w, in_h, out_w, out_h, n_items, t_in), in_w, in_h, row_pitch,
                                               frame_pitch, n_items * t_in, out_w, out_h, hbound, hcoef, vbound, vcoef)
    rows = grid_t * gh * gw
    if (out_row_stride < ROW or out_item_stride < rows * out_row_stride
            or out.numel() < (n_items - 1) * out_item_stride + (rows - 1) * out_row_stride + ROW):
        raise X2IError("x2i_amd: out holds %d elements; %d items of %d rows of 1176 with row stride %d and item stride %d do not fit"
                       % (out.numel(), n_items, rows, out_row_stride, out_item_stride))
    return (ops._p(frames), frame_pitch, row_pitch, n_items, t_in, in_w, in_h, out_w, out_h, ops._p(hbound), ops._p(hcoef), hk, ops._p(vbound),
            ops._p(vcoef), vk, ops._p(lut), ops._p(out), out_item_stride, out_row_stride, int(out.dtype == torch.bfloat16))


def rows(frames, in_w, in_h, row_pitch, frame_pitch, n_items, t_in, out_w, out_h, hbound, hcoef, vbound, vcoef, lut, out, out_item_stride,
         out_row_stride):
    """frames: a flat uint8 device buffer, n_items * t_in frames of in_h rows of in_w RGB pixels with the given pitches in bytes -> out, a
    flat float32 or bf16 device buffer: item i as (t_in + 1) / 2 * gh * gw patch rows of 1176 values at i * out_item_stride, rows
    out_row_stride apart (elements), in the order and layout of Qwen2VLImageProcessor; nothing else is written
    (include/frontend/rows/qwen/x2i_image_rows.h)"""
    args = _rows_args(frames, in_w, in_h, row_pitch, frame_pitch, n_items, t_in, out_w, out_h, hbound, hcoef, vbound, vcoef, lut, out,
                      out_item_stride, out_row_stride)
    check(load().x2i_image_rows(*args, ops._stream()), "image_rows")
    return out
