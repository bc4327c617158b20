/* x2i_image_tiles.h -- extension header of libx2i_hip.so: the image front end for a resized image that is cut into a uniform grid of crops
 * (csrc/image_tiles.hip).  Two host computations have this form: the slices of MiniCPMVImageProcessor.preprocess for an image over
 * 448 x 448 pixels under max_slice_nums > 1 (strip layout, the input of the SigLIP tower, x2i_siglip.h), and the 448 x 448 tiles of
 * InternVL2.5's load_image (planar layout, the input of InternViT, x2i_internvit.h).  Bit for bit what the host computes.
 *
 * Everything x2i_image.h says holds here: the conventions (device pointers owned by the caller, `stream` a hipStream_t passed as void* and
 * the last argument, work enqueued and never synchronised, no allocation, no atomics, 0 or a negative X2I_ERR_* code with the message in
 * x2i_last_error(); every argument is validated before any launch), Pillow's integer arithmetic with the uint8 image between the passes,
 * the per-axis `bound` / `coef` tables and `lut`, the kernel's clamping of what it reads of `bound`, and the LDS plan, which is computed
 * for the whole resize in_h -> out_h.  The header stands in a directory of its own because the set of include/frontend/ *.h headers is
 * closed too (x2i_image.h declares x2i_image_frontend and nothing else); the binding is x2i_amd/image_tiles_binding.py, the host modules
 * x2i_amd/image.py (ImageFrontEnd, sliced images) and x2i_amd/internvl_image.py (InternVLImageFrontEnd).
 *
 * The resize target (out_w, out_h) is cut into gy rows of gx crops of tile_w x tile_h pixels, gx = out_w / tile_w, gy = out_h / tile_h.
 * A crop is a WINDOW OF THE RESIZED WHOLE IMAGE: the tables are those of in_w -> out_w and in_h -> out_h, and the tap windows of rows and
 * columns near a crop's edge reach input pixels that belong to the neighbouring crop.  (Resizing each crop from its own box of the input
 * gives other values at every edge.)
 *
 * One workgroup owns the 14 output rows of one patch row of one crop and a tile of 4, 2 or 1 patches of columns of that crop; the column
 * tiles are laid out per crop, so the last tile of a crop is partial at the crop's edge and no workgroup straddles two crops.  Crop heights
 * are multiples of 14, so no patch row straddles two crops either.
 */
#ifndef X2I_IMAGE_TILES_H
#define X2I_IMAGE_TILES_H
#include "../../x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* frames, frame_pitch, row_pitch, n, in_w, in_h, hbound, hcoef, hk, vbound, vcoef, vk, lut: as in x2i_image_frontend, the tables those of
 * in_w -> out_w and in_h -> out_h (all of an axis 0 / null exactly where it does not resize).
 * out: float32, or bf16 (one rounding of the float32 value, to nearest even) where out_bf16 != 0.  Crop (i, j), i the row of the grid, of
 * frame f starts at  base = f * out_frame_stride + (i * gx + j) * out_tile_stride  (strides in elements), and with
 * v(y, x, c) = lut[c][resized[i * tile_h + y][j * tile_w + x][c]]:
 *   layout 0, strip  [3][14][14 L], L = (tile_h / 14) * (tile_w / 14):
 *     out[base + (c * 14 + r) * out_row_stride + (ph * (tile_w / 14) + pw) * 14 + q] = v(14 ph + r, 14 pw + q, c)
 *   layout 1, planar [3][tile_h][tile_w]:
 *     out[base + (c * tile_h + y) * out_row_stride + x] = v(y, x, c)
 * Nothing but these elements is written: not the columns at and beyond 14 L (layout 0) or tile_w (layout 1) of a row, and nothing between
 * the crops or the frames.  A relaunch gives the same bits.
 * Needs n in 1..65535, in_w and in_h in 1..65535, tile_w and tile_h multiples of 14 in 14..980, out_w = gx * tile_w and out_h = gy * tile_h
 * with gx and gy in 1..12 (so out_w and out_h up to 11760; 9 x 980 = 8820 is MiniCPM-o's largest, 12 x 448 = 5376 InternVL2.5's),
 * row_pitch >= 3 in_w, frame_pitch >= (in_h - 1) * row_pitch + 3 in_w, layout 0 or 1,
 *   layout 0: out_row_stride >= 14 L and out_tile_stride >= 42 * out_row_stride,
 *   layout 1: out_row_stride >= tile_w and out_tile_stride >= 3 * tile_h * out_row_stride,
 * out_frame_stride >= gx * gy * out_tile_stride, the tables and lut 4-byte aligned, out aligned to its element size, and an LDS plan
 * (x2i_image.h, for in_h -> out_h) that fits. */
int x2i_image_tiles(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n, int32_t in_w, int32_t in_h, int32_t out_w,
                    int32_t out_h, int32_t tile_w, int32_t tile_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound,
                    const void* vcoef, int32_t vk, const void* lut, void* out, int64_t out_frame_stride, int64_t out_tile_stride,
                    int64_t out_row_stride, int32_t layout, int32_t out_bf16, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
