// The image front end for a resized image cut into a uniform grid of crops (include/frontend/tiles/x2i_image_tiles.h): the slices of
// MiniCPMVImageProcessor.preprocess (strip layout) and the 448 x 448 tiles of InternVL2.5's load_image (planar layout).  The kernel is
// csrc/image.hip's image_passes_kernel, reached through image_passes_launch (image_passes.h): its workgroup map per crop, per-crop output
// base and planar store serve this entry point, which keeps its own size, layout and stride rules.  One launch for n frames of one input
// size, one resize target and one grid; the launcher enqueues on the caller's stream and returns.
#include "image_passes.h"
#include "../../include/frontend/tiles/x2i_image_tiles.h"

namespace {
constexpr int MAX_GRID = 12;
}

extern "C" {

int x2i_image_tiles(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n, int32_t in_w, int32_t in_h, int32_t out_w,
                    int32_t out_h, int32_t tile_w, int32_t tile_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound,
                    const void* vcoef, int32_t vk, const void* lut, void* out, int64_t out_frame_stride, int64_t out_tile_stride,
                    int64_t out_row_stride, int32_t layout, int32_t out_bf16, x2i_stream_t stream) {
  const char* what = "image_tiles";
  const ImageCall c = {frames, frame_pitch, row_pitch, in_w, in_h, out_w, out_h, hbound, hcoef, hk, vbound, vcoef, vk, lut, out, out_bf16};
  if (int rc = image_check_pointers(what, c)) return rc;
  if (n < 1 || n > 65535) return x2i_set_error(X2I_ERR_SHAPE, "%s: n=%d must be in 1..65535", what, n);
  if (int rc = image_check_input_size(what, c)) return rc;
  if (tile_w < PATCH || tile_w % PATCH || tile_w > PATCH * MAX_PATCHES)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: tile_w=%d must be a multiple of 14 in 14..980", what, tile_w);
  if (tile_h < PATCH || tile_h % PATCH || tile_h > PATCH * MAX_PATCHES)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: tile_h=%d must be a multiple of 14 in 14..980", what, tile_h);
  if (out_w < tile_w || out_w % tile_w || out_w / tile_w > MAX_GRID)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_w=%d must be 1..12 times tile_w=%d", what, out_w, tile_w);
  if (out_h < tile_h || out_h % tile_h || out_h / tile_h > MAX_GRID)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_h=%d must be 1..12 times tile_h=%d", what, out_h, tile_h);
  const int gx = out_w / tile_w, gy = out_h / tile_h;
  if (layout != 0 && layout != 1) return x2i_set_error(X2I_ERR_ARG, "%s: layout=%d must be 0 (strip) or 1 (planar)", what, layout);
  if (int rc = image_check_tables(what, c)) return rc;
  const long long row_min = layout ? tile_w : (long long)(tile_h / PATCH) * tile_w, rows_per_tile = layout ? 3LL * tile_h : 3LL * PATCH;
  if (out_row_stride < row_min || out_tile_stride < rows_per_tile * out_row_stride || out_frame_stride < (long long)gx * gy * out_tile_stride)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: layout %d needs out_row_stride=%lld at least %lld, out_tile_stride=%lld at least %lld * out_row_stride and "
                         "out_frame_stride=%lld at least %d * out_tile_stride", what, layout, (long long)out_row_stride, row_min,
                         (long long)out_tile_stride, rows_per_tile, (long long)out_frame_stride, gx * gy);
  ImageArgs a;      // the LDS plan is that of the whole resize
  if (int rc = image_plan_args(what, c, &a)) return rc;
  a.ofs = out_frame_stride, a.ors = out_row_stride, a.ots = out_tile_stride;
  a.crop_w = tile_w, a.crop_h = tile_h, a.gx = gx;
  image_passes_launch(a, n, gy, layout == 1, out_bf16 != 0, (hipStream_t)stream);
  return x2i_check_launch(what);
}

}  // extern "C"
