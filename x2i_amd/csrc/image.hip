// The MiniCPM-o image front end (include/frontend/x2i_image.h): raw uint8 RGB frames to the float pixel_values of
// MiniCPMVImageProcessor.preprocess for an unsliced image -- Pillow's 8-bit BICUBIC resize (two integer passes with a uint8 image between
// them), the normalisation as a table lookup, the strip layout [3][14][14 L].  One launch for n frames of one input and one output size;
// integer arithmetic and a lookup only, so the result equals the host's bit for bit.  The launcher enqueues on the caller's stream and returns.
// The kernel stores a resized image as a grid of crops and is compiled here alone: csrc/image_tiles.hip (x2i_image_tiles) launches it
// through image_passes_launch (image_passes.h), and a whole image is the grid of one crop.
#include "image_passes.h"
#include "../../include/frontend/x2i_image.h"

namespace {

// grid (crops per row * column tiles per crop, patch rows of the resized image, frames), 256 threads.  Phase 1: the horizontal pass (or a
// copy) of input rows row0 .. row0 + nrows for the tile's columns, uint8 [nrows][ld] in LDS (horizontal_pass_to_lds).  Phase 2: the
// vertical pass (or a copy) from LDS, one thread per (channel, row, column) with the column fastest, so that a wave stores consecutive
// elements of one output row.  The tables are those of the whole resized image: a crop's edge columns and rows take their taps from input
// pixels on either side of the edge.  PLANAR: a crop is stored as [3][crop_h][crop_w], else as the strip [3][14][14 L].
template <bool BF16, bool PLANAR>
__global__ __launch_bounds__(256) void image_passes_kernel(const ImageArgs a) {
  extern __shared__ uint8_t img[];
  const int tid = threadIdx.x, ph = blockIdx.y;
  const long long f = blockIdx.z;
  const int cj = blockIdx.x / a.tpc;                         // the crop's column in the grid
  const int cc = (blockIdx.x - cj * a.tpc) * a.tile * PATCH; // the tile's first column within the crop
  const int c0 = cj * a.crop_w + cc;                         // ... and within the resized image
  const int cw = min(a.tile * PATCH, a.crop_w - cc);
  int row0, nrows;
  patch_row_span(a, ph, &row0, &nrows);
  horizontal_pass_to_lds(a, a.frames + f * a.frame_pitch + (long long)row0 * a.row_pitch, nrows, c0, cw, img);
  __syncthreads();
  const int pr = a.crop_h / PATCH, ci = ph / pr, pc = ph - ci * pr;   // the crop's row in the grid, the patch row within the crop
  const long long base = f * a.ofs + (long long)(ci * a.gx + cj) * a.ots;
  for (int i = tid; i < 3 * PATCH * cw; i += 256) {
    const int cr = i / cw, col = i - cr * cw, c = cr / PATCH, r = cr - c * PATCH;
    const float val = a.lut[c * 256 + vertical_tap_value(a, img, ph, r, col, c, row0, nrows)];
    const long long o = PLANAR ? base + ((long long)c * a.crop_h + PATCH * pc + r) * a.ors + cc + col
                               : base + (long long)(c * PATCH + r) * a.ors + (long long)pc * a.crop_w + cc + col;
    if (BF16)
      ((bf16_t*)a.out)[o] = f32_to_bf16(val);
    else
      ((float*)a.out)[o] = val;
  }
}

}  // namespace

// a: everything but tpc set.  One launch for n frames, gx * gy crops each.
void image_passes_launch(ImageArgs a, int n, int gy, bool planar, bool bf16, hipStream_t stream) {
  const int cp = a.crop_w / PATCH;
  a.tpc = (cp + a.tile - 1) / a.tile;
  const dim3 grid(a.gx * a.tpc, gy * (a.crop_h / PATCH), n);
  const size_t lds = (size_t)a.rows * a.ld;
  if (planar) {
    if (bf16)
      hipLaunchKernelGGL((image_passes_kernel<true, true>), grid, dim3(256), lds, stream, a);
    else
      hipLaunchKernelGGL((image_passes_kernel<false, true>), grid, dim3(256), lds, stream, a);
  } else {
    if (bf16)
      hipLaunchKernelGGL((image_passes_kernel<true, false>), grid, dim3(256), lds, stream, a);
    else
      hipLaunchKernelGGL((image_passes_kernel<false, false>), grid, dim3(256), lds, stream, a);
  }
}

extern "C" {

int x2i_image_frontend(const void* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n, int32_t in_w, int32_t in_h, int32_t out_w,
                       int32_t out_h, const void* hbound, const void* hcoef, int32_t hk, const void* vbound, const void* vcoef, int32_t vk,
                       const void* lut, void* out, int64_t out_frame_stride, int64_t out_row_stride, int32_t out_bf16, x2i_stream_t stream) {
  const char* what = "image_frontend";
  const ImageCall c = {frames, frame_pitch, row_pitch, in_w, in_h, out_w, out_h, hbound, hcoef, hk, vbound, vcoef, vk, lut, out, out_bf16};
  if (int rc = image_check_pointers(what, c)) return rc;
  if (n < 1 || n > 65535) return x2i_set_error(X2I_ERR_SHAPE, "%s: n=%d must be in 1..65535", what, n);
  if (int rc = image_check_input_size(what, c)) return rc;
  if (out_w < PATCH || out_w % PATCH || out_w > PATCH * MAX_PATCHES)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_w=%d must be a multiple of 14 in 14..980", what, out_w);
  if (out_h < PATCH || out_h % PATCH || out_h > PATCH * MAX_PATCHES)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_h=%d must be a multiple of 14 in 14..980", what, out_h);
  if (int rc = image_check_tables(what, c)) return rc;
  const long long L14 = (long long)(out_h / PATCH) * out_w;
  if (out_row_stride < L14 || out_frame_stride < 3LL * PATCH * out_row_stride)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: out_row_stride=%lld must be at least 14 L = %lld and out_frame_stride=%lld at least 42 * out_row_stride", what,
                         (long long)out_row_stride, L14, (long long)out_frame_stride);
  ImageArgs a;
  if (int rc = image_plan_args(what, c, &a)) return rc;
  a.ofs = out_frame_stride, a.ors = out_row_stride;
  image_passes_launch(a, n, 1, false, out_bf16 != 0, (hipStream_t)stream);     // the whole image is the one crop of a 1 x 1 grid
  return x2i_check_launch(what);
}

}  // extern "C"
