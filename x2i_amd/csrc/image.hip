// The MiniCPM-o image front end (include/frontend/x2i_image.h): raw uint8 RGB frames to the float pixel_values of
// MiniCPMVImageProcessor.preprocess for an unsliced image -- Pillow's 8-bit BICUBIC resize (two integer passes with a uint8 image between
// them), the normalisation as a table lookup, the strip layout [3][14][14 L].  One launch for n frames of one input and one output size;
// integer arithmetic and a lookup only, so the result equals the host's bit for bit.  The launcher enqueues on the caller's stream and returns.
#include "x2i_common.h"
#include "../../include/frontend/x2i_image.h"

#include <math.h>

namespace {

constexpr int PATCH = 14, PREC = 22, MAX_PATCHES = 70, LDS_BYTES = 65536, MAX_IN = 65535;

struct ImageArgs {
  const uint8_t* frames;
  long long frame_pitch, row_pitch;
  const int *hb, *hc, *vb, *vc;
  const float* lut;
  void* out;
  long long ofs, ors;
  int in_w, in_h, out_w, out_h, hk, vk;
  int tile;   // patches of columns per workgroup
  int rows;   // input rows a patch row's vertical taps reach, at most
  int ld;     // bytes of an LDS row
};

__device__ __forceinline__ int clip8(unsigned acc) {
  const int v = ((int)acc) >> PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (column tiles, patch rows, frames), 256 threads.  Phase 1: the horizontal pass (or a copy) of input rows row0 .. row0 + nrows for the
// tile's columns, uint8 [nrows][ld] in LDS, a thread per pixel with consecutive lanes on consecutive output columns.  Phase 2: the vertical
// pass (or a copy) from LDS, one thread per (channel, row, column) with the column fastest, so that a wave stores consecutive elements of
// one output row.  Every value read from a bound table is clamped to the image, to ksize and to the LDS rows before it is used.
template <bool BF16>
__global__ __launch_bounds__(256) void image_frontend_kernel(const ImageArgs a) {
  extern __shared__ uint8_t img[];
  const int tid = threadIdx.x, ph = blockIdx.y;
  const long long f = blockIdx.z;
  const int c0 = blockIdx.x * a.tile * PATCH;
  const int cw = min(a.tile * PATCH, a.out_w - c0);
  int row0 = PATCH * ph, nrows = PATCH;                    // in_h == out_h: the patch row's own 14 rows
  if (a.vk) {
    const int last = PATCH * ph + PATCH - 1;
    row0 = clampi(a.vb[2 * PATCH * ph], 0, a.in_h - 1);
    const int hi = clampi(a.vb[2 * last] + a.vb[2 * last + 1], row0, a.in_h);
    nrows = min(hi - row0, a.rows);
  }
  const uint8_t* src = a.frames + f * a.frame_pitch + (long long)row0 * a.row_pitch;
  for (int i = tid; i < nrows * cw; i += 256) {
    const int r = i / cw, col = i - r * cw, oc = c0 + col;
    const uint8_t* rowp = src + (long long)r * a.row_pitch;
    uint8_t* dst = img + r * a.ld + 3 * col;
    if (a.hk) {
      const int xmin = clampi(a.hb[2 * oc], 0, a.in_w - 1);
      const int cnt = clampi(a.hb[2 * oc + 1], 0, min(a.hk, a.in_w - xmin));
      const int* k = a.hc + (long long)oc * a.hk;
      const uint8_t* px = rowp + 3 * xmin;
      unsigned s0 = 1u << (PREC - 1), s1 = s0, s2 = s0;
      for (int x = 0; x < cnt; ++x) {
        const unsigned kk = (unsigned)k[x];
        s0 += px[3 * x] * kk;
        s1 += px[3 * x + 1] * kk;
        s2 += px[3 * x + 2] * kk;
      }
      dst[0] = (uint8_t)clip8(s0);
      dst[1] = (uint8_t)clip8(s1);
      dst[2] = (uint8_t)clip8(s2);
    } else {
      const uint8_t* px = rowp + 3 * oc;
      dst[0] = px[0];
      dst[1] = px[1];
      dst[2] = px[2];
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * PATCH * cw; i += 256) {
    const int cr = i / cw, col = i - cr * cw, c = cr / PATCH, r = cr - c * PATCH;
    int v;
    if (a.vk) {
      const int oy = PATCH * ph + r;
      const int y0 = clampi(a.vb[2 * oy] - row0, 0, nrows);
      const int cnt = clampi(a.vb[2 * oy + 1], 0, min(a.vk, nrows - y0));
      const int* k = a.vc + (long long)oy * a.vk;
      const uint8_t* q = img + y0 * a.ld + 3 * col + c;
      unsigned s = 1u << (PREC - 1);
      for (int y = 0; y < cnt; ++y) s += q[y * a.ld] * (unsigned)k[y];
      v = clip8(s);
    } else {
      v = img[r * a.ld + 3 * col + c];
    }
    const float val = a.lut[c * 256 + v];
    const long long o = f * a.ofs + (long long)(c * PATCH + r) * a.ors + (long long)ph * a.out_w + c0 + col;
    if (BF16)
      ((bf16_t*)a.out)[o] = f32_to_bf16(val);
    else
      ((float*)a.out)[o] = val;
  }
}

// Pillow's window of output xx: (xmin, xmax), and the axis's ksize
struct Axis {
  double scale, support;
  int n_in, ksize;
  Axis(int n_in_, int n_out) : n_in(n_in_) {
    scale = (double)n_in_ / n_out;
    support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    ksize = (int)ceil(support) * 2 + 1;
  }
  void window(int xx, int* xmin, int* xmax) const {
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
    *xmin = lo;
    *xmax = hi - lo;
  }
};

}  // namespace

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
  int rows = PATCH;
  if (vk) {
    const Axis ax(in_h, out_h);
    rows = 0;
    for (int p = 0; p < out_h / PATCH; ++p) {
      int lo, cnt, lo2, cnt2;
      ax.window(PATCH * p, &lo, &cnt);
      ax.window(PATCH * p + PATCH - 1, &lo2, &cnt2);
      if (lo2 + cnt2 - lo > rows) rows = lo2 + cnt2 - lo;
    }
  }
  int tile = 4;
  while (tile > 1 && (long long)rows * ((3 * PATCH * tile + 3) & ~3) > LDS_BYTES) tile >>= 1;
  const int ld = (3 * PATCH * tile + 3) & ~3;
  if ((long long)rows * ld > LDS_BYTES)
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
  const int gw = out_w / PATCH;
  const dim3 grid((gw + tile - 1) / tile, out_h / PATCH, n);
  const size_t lds = (size_t)rows * ld;
  if (out_bf16)
    hipLaunchKernelGGL(image_frontend_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(image_frontend_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, a);
  return x2i_check_launch(what);
}

}  // extern "C"
