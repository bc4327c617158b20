/* x2i_image_rows.h -- extension header of libx2i_hip.so: the Qwen2.5-VL image front end (csrc/image_rows.hip), raw uint8 RGB frames to the
 * patch rows `pixel_values` [S, 1176] that Qwen2VLImageProcessor computes on the host and the vision tower (x2i_vit.h,
 * x2i_amd/qwen_vision.py) reads: Pillow's BICUBIC resize on 8 bits per channel, the normalisation, the temporal duplicate and the
 * flattening in merge-unit order, bit for bit.
 *
 * Everything x2i_image.h says holds here: the conventions (device pointers owned by the caller, `stream` a hipStream_t passed as void* and
 * the last argument, work enqueued and never synchronised, no allocation, no atomics, 0 or a negative X2I_ERR_* code with the message in
 * x2i_last_error(); every argument is validated before any launch), Pillow's integer arithmetic with the uint8 image between the passes,
 * the per-axis `bound` / `coef` tables and `lut`, the kernel's clamping of what it reads of `bound`, and the LDS plan of in_h -> out_h.
 * The header stands in a directory of its own because the sets of include/frontend/ *.h and include/frontend/<dir>/ *.h headers are closed
 * too; the binding is x2i_amd/image_rows_binding.py, the host module x2i_amd/qwen_image.py (QwenImageFrontEnd).
 *
 * An ITEM is an image (t_in = 1) or a clip of t_in frames of one size; frame f of item i starts at frames + (i * t_in + f) * frame_pitch.
 * With gh = out_h / 14 and gw = out_w / 14 (both even: the merge size is 2) an item has grid_t = (t_in + 1) / 2 temporal steps of gh * gw
 * rows of 1176 = 3 * 2 * 14 * 14 values.  Temporal slot tp (0 or 1) of step t reads frame min(2 t + tp, t_in - 1): an image fills both slots
 * with the same values, and the last frame of an odd clip is repeated.
 *
 * One workgroup owns one patch row of one FRAME and a tile of 4, 2 or 1 patches of columns: the two passes are those of x2i_image.h, and
 * the store walks (patch, channel, row of the patch, column of the patch) with the column fastest, so that consecutive lanes store
 * consecutive elements of the 196-element channel plane of a patch.  A frame that fills both slots of its step is computed once and stored
 * twice.
 */
#ifndef X2I_IMAGE_ROWS_H
#define X2I_IMAGE_ROWS_H
#include "../../../x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* frames, frame_pitch, row_pitch, in_w, in_h, hbound, hcoef, hk, vbound, vcoef, vk, lut: as in x2i_image_frontend, over n_items * t_in
 * frames, the tables those of in_w -> out_w and in_h -> out_h (all of an axis 0 / null exactly where it does not resize).
 * out: float32, or bf16 (one rounding of the float32 value, to nearest even) where out_bf16 != 0.  With
 * v(t, tp, y, x, c) = lut[c][resized[frame min(2 t + tp, t_in - 1) of item i][y][x][c]] (strides in elements):
 *   out[i * out_item_stride + row * out_row_stride + c * 392 + tp * 196 + r * 14 + q] = v(t, tp, 14 ph + r, 14 pw + q, c)
 *   row = t * gh * gw + ((ph / 2) * (gw / 2) + pw / 2) * 4 + (ph % 2) * 2 + (pw % 2)
 * the library's order (grid_t, gh / 2, gw / 2, 2, 2, C, tp, 14, 14).  Nothing but these elements is written: not the columns at and beyond
 * 1176 of a row, and nothing between the items.  A relaunch gives the same bits.
 * Needs n_items >= 1, t_in >= 1 and n_items * t_in in 1..65535, in_w and in_h in 1..65535, out_w and out_h multiples of 28 in 28..11760,
 * row_pitch >= 3 in_w, frame_pitch >= (in_h - 1) * row_pitch + 3 in_w, out_row_stride >= 1176,
 * out_item_stride >= grid_t * gh * gw * out_row_stride, the tables and lut 4-byte aligned, out aligned to its element size, and an LDS
 * plan (x2i_image.h) that fits. */
int x2i_image_rows(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_items, int32_t t_in, int32_t in_w, int32_t in_h,
                   int32_t out_w, int32_t out_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound, const void* vcoef,
                   int32_t vk, const void* lut, void* out, int64_t out_item_stride, int64_t out_row_stride, int32_t out_bf16,
                   x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
