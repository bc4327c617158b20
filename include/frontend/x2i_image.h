/* x2i_image.h -- extension header of libx2i_hip.so: the MiniCPM-o image front end (csrc/image.hip), raw uint8 RGB frames to the
 * `pixel_values` that MiniCPMVImageProcessor.preprocess computes on the host for an unsliced image and the SigLIP tower (x2i_siglip.h)
 * reads: Pillow's BICUBIC resize on 8 bits per channel, the normalisation, and the strip layout of reshape_by_patch, bit for bit.
 *
 * The conventions are those of x2i.h and of the other extension headers (device pointers owned by the caller, `stream` a hipStream_t passed
 * as void* and the last argument, work enqueued and never synchronised, no allocation, no atomics, 0 or a negative X2I_ERR_* code with the
 * message in x2i_last_error(); every argument is validated before any launch).  The header stands under include/frontend/ because the sets
 * of include/x2i_*.h, include/ext/*.h and include/ext/<dir>/*.h headers are closed; the binding is x2i_amd/image_binding.py, the host module
 * x2i_amd/image.py (ImageFrontEnd).
 *
 * The arithmetic is Pillow's ImagingResample for 8-bit channels.  Per axis, for n_in -> n_out, in float64 on the host:
 *   scale = n_in / n_out, fs = max(scale, 1), support = 2 fs, ksize = ceil(support) * 2 + 1
 *   output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), n_in) - xmin
 *              w_x = cubic((x + xmin - center + 0.5) / fs) for x < xmax (a = -0.5), k_x = w_x / sum w,
 *              K_x = int(k_x 2^22 + 0.5) for k_x >= 0, int(k_x 2^22 - 0.5) otherwise (int truncates toward zero)
 *   one output = clip(((1 << 21) + sum_x pixel[xmin + x] K_x) >> 22, 0, 255), an arithmetic shift of an int32 accumulator
 * The horizontal pass runs first, only where in_w != out_w, and its result is a uint8 image; the vertical pass reads that image, only where
 * in_h != out_h.  No wider intermediate exists.  The accumulator: sum |K_x| 255 + 2^21 must stay below 2^31, that is sum |K_x| below
 * 2.0059 * 2^22; over the scales swept by tests/test_image_ref_cpu.py the largest sum |K_x| is 1.2686 * 2^22 (sum |K_x| 255 = 1.36e9), and
 * the host module checks every table it builds.  The kernel adds in uint32 (the same bits), so a table that broke the bound would give
 * wrong pixels and nothing worse.
 *
 * Tables per axis that resizes (int32, device memory, 4-byte aligned):
 *   bound [n_out][2]      (xmin, xmax)
 *   coef  [n_out][ksize]  K_x for x < xmax; the rest is not read
 * The kernel clamps what it reads of `bound` to the image and to ksize, so no table content can make it read or write out of bounds.
 *   lut   f32 [3][256]    lut[c][v] = (float32(v) / 255 - mean[c]) / std[c], the processor's own float32 expressions, computed by the host
 *
 * One workgroup owns the 14 output rows of one patch row and a tile of 4, 2 or 1 patches of columns: it runs the horizontal pass for the
 * input rows its vertical taps reach (at most `rows`, below) into LDS as uint8, then the vertical pass from LDS, clips, looks up lut and
 * stores.  The LDS plan: rows * pitch bytes with pitch = 3 * 14 * tile rounded up to 4, at most 65536; the largest tile of 4, 2, 1 patches
 * that fits is taken, and a scale for which one patch does not fit is refused (X2I_ERR_SHAPE).  rows = 14 where in_h == out_h, otherwise the
 * largest of ymin(14 p + 13) + ymax(14 p + 13) - ymin(14 p) over the patch rows p, which the launcher computes from the formula above.
 */
#ifndef X2I_IMAGE_H
#define X2I_IMAGE_H
#include "../x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* frames: uint8, n frames of in_h rows of in_w RGB pixels; pixel (f, y, x) channel c at frames + f * frame_pitch + y * row_pitch + 3 x + c
 * (pitches in bytes, any alignment).
 * hbound, hcoef, hk: the horizontal tables and their ksize; all of them 0 / null exactly where in_w == out_w.  vbound, vcoef, vk: the same
 * for the vertical axis.  hk and vk must equal the ksize of the formula above.
 * out: n frames [3][14][14 L] with L = (out_h / 14) * (out_w / 14), float32, or bf16 (one rounding of the float32 value, to nearest even)
 * where out_bf16 != 0:
 *   out[f * out_frame_stride + (c * 14 + r) * out_row_stride + (ph * (out_w / 14) + pw) * 14 + q] = lut[c][resized[14 ph + r][14 pw + q][c]]
 * (strides in elements).  Columns at and beyond 14 L of a row, and everything between the frames, are not written.  A relaunch gives
 * the same bits.
 * Needs n in 1..65535, in_w and in_h in 1..65535, out_w and out_h multiples of 14 in 14..980, row_pitch >= 3 in_w,
 * frame_pitch >= (in_h - 1) * row_pitch + 3 in_w, out_row_stride >= 14 L, out_frame_stride >= 42 * out_row_stride, the tables and lut 4-byte
 * aligned, out aligned to its element size, and an LDS plan that fits. */
int x2i_image_frontend(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n, int32_t in_w, int32_t in_h, int32_t out_w,
                       int32_t out_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound, const void* vcoef, int32_t vk,
                       const void* lut, void* out, int64_t out_frame_stride, int64_t out_row_stride, int32_t out_bf16, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
