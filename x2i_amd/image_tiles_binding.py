"""ctypes binding and torch-tensor wrapper of the extension header include/frontend/tiles/x2i_image_tiles.h: the image front end for a
resized image cut into a grid of crops (csrc/image_tiles.hip).

Like image_binding.py, whose tables, windows and LDS plan it shares: the entry point is not in _lib._EXPORTS, _lib.extension binds it;
PyTorch supplies device memory and the current stream, every computation happens in libx2i_hip.so, nothing here allocates behind the
caller's back or synchronises, and there is no fallback.  (Not called *_ops.py, for image_binding.py's reason.)
"""
import ctypes as C

import torch

from . import _lib, image_binding as ib, ops
from ._lib import X2IError, check

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# Every export of include/frontend/tiles/x2i_image_tiles.h: name -> argtypes (all return int).  tests/test_image_tiles_boundary_cpu.py
# checks it against the header's prototypes.
_EXPORTS = {
    "x2i_image_tiles": [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i64,
                        _i32, _i32, _vp],
}

PATCH, MAX_PATCHES, MAX_GRID = ib.PATCH, ib.MAX_PATCHES, 12       # the compile-time constants of csrc/image_tiles.hip
STRIP, PLANAR = 0, 1

load = _lib.extension("frontend/tiles/x2i_image_tiles.h", _EXPORTS)


def check_sizes(in_w, in_h, out_w, out_h, tile_w, tile_h):
    """(gx, gy) of the grid; X2IError for sizes the kernel does not serve (what the launcher refuses for the same sizes)"""
    ib.check_input_size(in_w, in_h)
    for name, v in (("tile_w", tile_w), ("tile_h", tile_h)):
        if v < PATCH or v % PATCH or v > PATCH * MAX_PATCHES:
            raise X2IError("x2i_amd: %s=%d must be a multiple of 14 in 14..980" % (name, v))
    for name, v, t, tn in (("out_w", out_w, tile_w, "tile_w"), ("out_h", out_h, tile_h, "tile_h")):
        if v < t or v % t or v // t > MAX_GRID:
            raise X2IError("x2i_amd: %s=%d must be 1..12 times %s=%d" % (name, v, tn, t))
    ib.lds_plan(in_h, out_h)
    return out_w // tile_w, out_h // tile_h


def tile_extent(tile_w, tile_h, layout, out_row_stride):
    """(the least row stride, the rows of a crop, the elements from a crop's first to one past its last) of a layout"""
    if layout == PLANAR:
        return tile_w, 3 * tile_h, (3 * tile_h - 1) * out_row_stride + tile_w
    L14 = tile_h // PATCH * tile_w
    return L14, 3 * PATCH, (3 * PATCH - 1) * out_row_stride + L14


def _tiles_args(frames, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, tile_w, tile_h, hbound, hcoef, vbound, vcoef, lut, out,
                out_frame_stride, out_tile_stride, out_row_stride, layout):
    """The one place the arguments of x2i_image_tiles are put together (field order of include/frontend/tiles/x2i_image_tiles.h)"""
    def sizes():
        if layout not in (STRIP, PLANAR):
            raise X2IError("x2i_amd: layout=%r must be 0 (strip) or 1 (planar)" % (layout,))
        return check_sizes(in_w, in_h, out_w, out_h, tile_w, tile_h)
    hk, vk, (gx, gy) = ib._shared_args(frames, lut, out, sizes, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, hbound, hcoef, vbound, vcoef)
    row_min, rows, extent = tile_extent(tile_w, tile_h, layout, out_row_stride)
    if (out_row_stride < row_min or out_tile_stride < rows * out_row_stride or out_frame_stride < gx * gy * out_tile_stride
            or out.numel() < (n - 1) * out_frame_stride + (gx * gy - 1) * out_tile_stride + extent):
        raise X2IError("x2i_amd: out holds %d elements; %d frames of %d x %d crops of %d rows of %d with row stride %d, tile stride %d and "
                       "frame stride %d do not fit" % (out.numel(), n, gy, gx, rows, row_min, out_row_stride, out_tile_stride, out_frame_stride))
    return (ops._p(frames), frame_pitch, row_pitch, n, in_w, in_h, out_w, out_h, tile_w, tile_h, ops._p(hbound), ops._p(hcoef), hk,
            ops._p(vbound), ops._p(vcoef), vk, ops._p(lut), ops._p(out), out_frame_stride, out_tile_stride, out_row_stride, layout,
            int(out.dtype == torch.bfloat16))


def tiles(frames, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, tile_w, tile_h, hbound, hcoef, vbound, vcoef, lut, out,
          out_frame_stride, out_tile_stride, out_row_stride, layout):
    """frames: a flat uint8 device buffer, n frames of in_h rows of in_w RGB pixels with the given pitches in bytes -> out, a flat float32
    or bf16 device buffer: the resize to out_w x out_h cut into crops of tile_w x tile_h, crop (i, j) of frame f at
    f * out_frame_stride + (i * gx + j) * out_tile_stride as the strip [3][14][14 L] (layout 0) or planar [3][tile_h][tile_w] (layout 1)
    with rows out_row_stride apart (elements); nothing else is written (include/frontend/tiles/x2i_image_tiles.h)"""
    args = _tiles_args(frames, in_w, in_h, row_pitch, frame_pitch, n, out_w, out_h, tile_w, tile_h, hbound, hcoef, vbound, vcoef, lut, out,
                       out_frame_stride, out_tile_stride, out_row_stride, layout)
    check(load().x2i_image_tiles(*args, ops._stream()), "image_tiles")
    return out
