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
  if (!frames || !lut || !out) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer (frames, lut or out)", what);
  if (n_items < 1 || t_in < 1 || (long long)n_items * t_in > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: n_items=%d and t_in=%d must be at least 1 and n_items * t_in in 1..65535", what, n_items, t_in);
  if (in_w < 1 || in_w > MAX_IN || in_h < 1 || in_h > MAX_IN)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: in_w=%d and in_h=%d must be in 1..65535", what, in_w, in_h);
  if (out_w < UNIT || out_w % UNIT || out_w > MAX_OUT)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_w=%d must be a multiple of 28 in 28..11760", what, out_w);
  if (out_h < UNIT || out_h % UNIT || out_h > MAX_OUT)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_h=%d must be a multiple of 28 in 28..11760", what, out_h);
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
  // rows of an item: at most 32768 * 840 * 840; the product with out_row_stride is never formed (it could pass 2^63)
  const long long item_rows = (long long)((t_in + 1) / 2) * (out_h / PATCH) * (out_w / PATCH);
  if (out_row_stride < ROW || out_item_stride / out_row_stride < item_rows)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_row_stride=%lld must be at least 1176 and out_item_stride=%lld at least grid_t * gh * gw = %lld times "
                         "out_row_stride", what, (long long)out_row_stride, (long long)out_item_stride, item_rows);
  // the LDS plan (checked before the alignment, so that a refused scale is reported as such whatever the pointers are)
  int rows, tile, ld;
  if (!image_lds_plan(in_h, out_h, vk, &rows, &tile, &ld))
    return x2i_set_error(X2I_ERR_SHAPE, "%s: the LDS plan does not fit: in_h=%d -> out_h=%d needs %d rows of %d bytes for one patch of columns, at most %d bytes",
                         what, in_h, out_h, rows, ld, LDS_BYTES);
  const uintptr_t tabs = (uintptr_t)hbound | (uintptr_t)hcoef | (uintptr_t)vbound | (uintptr_t)vcoef | (uintptr_t)lut;
  if ((tabs & 3) || (((uintptr_t)out) & (out_bf16 ? 1 : 3)))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: the tables and lut must be 4-byte aligned, out aligned to its element size", what);
  RowsArgs ra;
  ImageArgs& a = ra.im;
  a.frames = (const uint8_t*)frames;
  a.frame_pitch = frame_pitch;
  a.row_pitch = row_pitch;
  a.hb = (const int*)hbound;
  a.hc = (const int*)hcoef;
  a.vb = (const int*)vbound;
  a.vc = (const int*)vcoef;
  a.lut = (const float*)lut;
  a.out = out;
  a.ofs = 0, a.ots = 0;
  a.ors = out_row_stride;
  a.in_w = in_w, a.in_h = in_h, a.out_w = out_w, a.out_h = out_h, a.hk = hk, a.vk = vk;
  a.tile = tile, a.rows = rows, a.ld = ld;
  a.crop_w = out_w, a.crop_h = out_h, a.gx = 1;
  const int gw = out_w / PATCH;
  a.tpc = (gw + tile - 1) / tile;
  ra.ois = out_item_stride;
  ra.t_in = t_in;
  const dim3 grid(a.tpc, out_h / PATCH, n_items * t_in);
  const size_t lds = (size_t)rows * ld;
  if (out_bf16)
    hipLaunchKernelGGL((image_rows_kernel<true>), grid, dim3(256), lds, (hipStream_t)stream, ra);
  else
    hipLaunchKernelGGL((image_rows_kernel<false>), grid, dim3(256), lds, (hipStream_t)stream, ra);
  return x2i_check_launch(what);
}

}  // extern "C"
