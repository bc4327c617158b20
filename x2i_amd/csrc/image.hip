// The MiniCPM-o image front end (include/frontend/x2i_image.h): raw uint8 RGB frames to the float pixel_values of
// MiniCPMVImageProcessor.preprocess for an unsliced image -- Pillow's 8-bit BICUBIC resize (two integer passes with a uint8 image between
// them), the normalisation as a table lookup, the strip layout [3][14][14 L].  One launch for n frames of one input and one output size;
// integer arithmetic and a lookup only, so the result equals the host's bit for bit.  The launcher enqueues on the caller's stream and returns.
#include "image_passes.h"
#include "../../include/frontend/x2i_image.h"

extern "C" {

int x2i_image_frontend(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n, int32_t in_w, int32_t in_h, int32_t out_w,
                       int32_t out_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound, const void* vcoef, int32_t vk,
                       const void* lut, void* out, int64_t out_frame_stride, int64_t out_row_stride, int32_t out_bf16, x2i_stream_t stream) {
  const char* what = "image_frontend";
  if (!frames || !lut || !out) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer (frames, lut or out)", what);
  if (n < 1 || n > 65535) return x2i_set_error(X2I_ERR_SHAPE, "%s: n=%d must be in 1..65535", what, n);
  if (in_w < 1 || in_w > MAX_IN || in_h < 1 || in_h > MAX_IN)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: in_w=%d and in_h=%d must be in 1..65535", what, in_w, in_h);
  if (out_w < PATCH || out_w % PATCH || out_w > PATCH * MAX_PATCHES)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_w=%d must be a multiple of 14 in 14..980", what, out_w);
  if (out_h < PATCH || out_h % PATCH || out_h > PATCH * MAX_PATCHES)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_h=%d must be a multiple of 14 in 14..980", what, out_h);
  if (row_pitch < 3LL * in_w || frame_pitch < (long long)(in_h - 1) * row_pitch + 3LL * in_w)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: row_pitch=%lld must be at least 3 * in_w and frame_pitch=%lld at least (in_h - 1) * row_pitch + 3 * in_w",
                         what, (long long)row_pitch, (long long)frame_pitch);
  const int want_hk = in_w != out_w ? Axis(in_w, out_w).ksize : 0, want_vk = in_h != out_h ? Axis(in_h, out_h).ksize : 0;
  if (hk != want_hk) return x2i_set_error(X2I_ERR_SHAPE, "%s: hk=%d, the tables of in_w=%d -> out_w=%d have ksize %d", what, hk, in_w, out_w, want_hk);
  if (vk != want_vk) return x2i_set_error(X2I_ERR_SHAPE, "%s: vk=%d, the tables of in_h=%d -> out_h=%d have ksize %d", what, vk, in_h, out_h, want_vk);
  if ((hk != 0) != (hbound != nullptr) || (hk != 0) != (hcoef != nullptr))
    return x2i_set_error(X2I_ERR_ARG, "%s: hbound and hcoef must be given exactly where in_w != out_w", what);
  if ((vk != 0) != (vbound != nullptr) || (vk != 0) != (vcoef != nullptr))
    return x2i_set_error(X2I_ERR_ARG, "%s: vbound and vcoef must be given exactly where in_h != out_h", what);
  const long long L14 = (long long)(out_h / PATCH) * out_w;
  if (out_row_stride < L14 || out_frame_stride < 3LL * PATCH * out_row_stride)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_row_stride=%lld must be at least 14 L = %lld and out_frame_stride=%lld at least 42 * out_row_stride", what,
                         (long long)out_row_stride, L14, (long long)out_frame_stride);
  // the LDS plan (checked before the alignment, so that a refused scale is reported as such whatever the pointers are)
  int rows, tile, ld;
  if (!image_lds_plan(in_h, out_h, vk, &rows, &tile, &ld))
    return x2i_set_error(X2I_ERR_SHAPE, "%s: the LDS plan does not fit: in_h=%d -> out_h=%d needs %d rows of %d bytes for one patch of columns, at most %d bytes",
                         what, in_h, out_h, rows, ld, LDS_BYTES);
  const uintptr_t tabs = (uintptr_t)hbound | (uintptr_t)hcoef | (uintptr_t)vbound | (uintptr_t)vcoef | (uintptr_t)lut;
  if ((tabs & 3) || (((uintptr_t)out) & (out_bf16 ? 1 : 3)))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: the tables and lut must be 4-byte aligned, out aligned to its element size", what);
  ImageArgs a;
  a.frames = (const uint8_t*)frames;
  a.frame_pitch = frame_pitch;
  a.row_pitch = row_pitch;
  a.hb = (const int*)hbound;
  a.hc = (const int*)hcoef;
  a.vb = (const int*)vbound;
  a.vc = (const int*)vcoef;
  a.lut = (const float*)lut;
  a.out = out;
  a.ofs = out_frame_stride;
  a.ors = out_row_stride;
  a.in_w = in_w, a.in_h = in_h, a.out_w = out_w, a.out_h = out_h, a.hk = hk, a.vk = vk;
  a.tile = tile, a.rows = rows, a.ld = ld;
  a.crop_w = out_w, a.crop_h = out_h, a.gx = 1, a.ots = 0;     // the whole image is the one crop of a 1 x 1 grid
  image_passes_launch(a, n, 1, false, out_bf16 != 0, (hipStream_t)stream);
  return x2i_check_launch(what);
}

}  // extern "C"
