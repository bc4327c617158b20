// The Qwen2.5-VL image front end (include/frontend/rows/qwen/x2i_image_rows.h): raw uint8 RGB frames to the patch rows [S, 1176] of
// Qwen2VLImageProcessor -- the two passes of csrc/image.hip (image_passes.h), then the library's flattening
// (grid_t, gh / 2, gw / 2, 2, 2, C, tp, 14, 14) with the temporal duplicate.  New here are the workgroup map per frame, the store order
// and the second store of a frame that fills both temporal slots.  One launch for n_items items of t_in frames of one input size and one
// resize target; the launcher enqueues on the caller's stream and returns.
#include "image_passes.h"
#include "../../include/frontend/rows/qwen/x2i_image_rows.h"

namespace {

constexpr int UNIT = 28, MAX_OUT = 11760, PLANE = PATCH * PATCH, ROW = 3 * 2 * PLANE;   // 196 values per channel plane, 1176 per row

struct RowsArgs {
  ImageArgs im;    // ofs, ots, crop_w, crop_h, gx and tpc are not used; ors is the stride between patch rows of the output
  long long ois;   // elements between items
  int t_in;
};

// grid (column tiles, patch rows gh, n_items * t_in frames), 256 threads.  Phase 1 is horizontal_pass_to_lds.  Phase 2 walks
// (patch, channel, r, q) with q fastest: a channel plane of a patch is 196 consecutive output elements, so consecutive lanes store
// consecutive elements (the strip's order would store runs of 14).  Frame f of an item is slot f % 2 of step f / 2; the last frame of an
// odd t_in (an image: t_in = 1) fills slot 1 too, 196 elements further on: one value, two stores.
template <bool BF16>
__global__ __launch_bounds__(256) void image_rows_kernel(const RowsArgs ra) {
  extern __shared__ uint8_t img[];
  const ImageArgs& a = ra.im;
  const int tid = threadIdx.x, ph = blockIdx.y;
  const long long z = blockIdx.z;                            // the frame among all frames
  const int item = (int)(z / ra.t_in), f = (int)(z - (long long)item * ra.t_in);
  const int c0 = blockIdx.x * a.tile * PATCH;
  const int cw = min(a.tile * PATCH, a.out_w - c0);
  int row0, nrows;
  patch_row_span(a, ph, &row0, &nrows);
  horizontal_pass_to_lds(a, a.frames + z * a.frame_pitch + (long long)row0 * a.row_pitch, nrows, c0, cw, img);
  __syncthreads();
  const int gw = a.out_w / PATCH, gh = a.out_h / PATCH, t = f >> 1, tp = f & 1;
  const bool both = tp == 0 && f == ra.t_in - 1;
  // the row of patch column 0 of this patch row; patch column pw adds (pw / 2) * 4 + (pw % 2)
  const long long row_ph = (long long)t * gh * gw + (long long)(ph >> 1) * (gw >> 1) * 4 + (ph & 1) * 2;
  const long long base = item * ra.ois + tp * PLANE;
  const int pw0 = c0 / PATCH, total = (cw / PATCH) * 3 * PLANE;
  for (int i = tid; i < total; i += 256) {
    const int p = i / (3 * PLANE), pc = i - p * 3 * PLANE, c = pc / PLANE, rq = pc - c * PLANE, r = rq / PATCH, q = rq - r * PATCH;
    const float val = a.lut[c * 256 + vertical_tap_value(a, img, ph, r, PATCH * p + q, c, row0, nrows)];
    const int pw = pw0 + p;
    const long long o = base + (row_ph + (pw >> 1) * 4 + (pw & 1)) * a.ors + c * 2 * PLANE + rq;
    if (BF16) {
      const bf16_t h = f32_to_bf16(val);
      ((bf16_t*)a.out)[o] = h;
      if (both) ((bf16_t*)a.out)[o + PLANE] = h;
    } else {
      ((float*)a.out)[o] = val;
      if (both) ((float*)a.out)[o + PLANE] = val;
    }
  }
}

}  // namespace

extern "C" {

int x2i_image_rows(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_items, int32_t t_in, int32_t in_w, int32_t in_h,
                   int32_t out_w, int32_t out_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound, const void* vcoef,
                   int32_t vk, const void* lut, void* out, int64_t out_item_stride, int64_t out_row_stride, int32_t out_bf16,
                   x2i_stream_t stream) {
  const char* what = "image_rows";
  const ImageCall c = {frames, frame_pitch, row_pitch, in_w, in_h, out_w, out_h, hbound, hcoef, hk, vbound, vcoef, vk, lut, out, out_bf16};
  if (int rc = image_check_pointers(what, c)) return rc;
  if (n_items < 1 || t_in < 1 || (long long)n_items * t_in > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: n_items=%d and t_in=%d must be at least 1 and n_items * t_in in 1..65535", what, n_items, t_in);
  if (int rc = image_check_input_size(what, c)) return rc;
  if (out_w < UNIT || out_w % UNIT || out_w > MAX_OUT)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_w=%d must be a multiple of 28 in 28..11760", what, out_w);
  if (out_h < UNIT || out_h % UNIT || out_h > MAX_OUT)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_h=%d must be a multiple of 28 in 28..11760", what, out_h);
  if (int rc = image_check_tables(what, c)) return rc;
  // rows of an item: at most 32768 * 840 * 840; the product with out_row_stride is never formed (it could pass 2^63)
  const long long item_rows = (long long)((t_in + 1) / 2) * (out_h / PATCH) * (out_w / PATCH);
  if (out_row_stride < ROW || out_item_stride / out_row_stride < item_rows)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_row_stride=%lld must be at least 1176 and out_item_stride=%lld at least grid_t * gh * gw = %lld times "
                         "out_row_stride", what, (long long)out_row_stride, (long long)out_item_stride, item_rows);
  RowsArgs ra;
  ImageArgs& a = ra.im;
  if (int rc = image_plan_args(what, c, &a)) return rc;
  a.ors = out_row_stride;
  const int gw = out_w / PATCH;
  a.tpc = (gw + a.tile - 1) / a.tile;
  ra.ois = out_item_stride;
  ra.t_in = t_in;
  const dim3 grid(a.tpc, out_h / PATCH, n_items * t_in);
  const size_t lds = (size_t)a.rows * a.ld;
  if (out_bf16)
    hipLaunchKernelGGL((image_rows_kernel<true>), grid, dim3(256), lds, (hipStream_t)stream, ra);
  else
    hipLaunchKernelGGL((image_rows_kernel<false>), grid, dim3(256), lds, (hipStream_t)stream, ra);
  return x2i_check_launch(what);
}

}  // extern "C"
