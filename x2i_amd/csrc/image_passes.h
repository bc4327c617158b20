// The two passes of the image front ends (Pillow's 8-bit BICUBIC resize, the normalisation as a table lookup) as one kernel, shared by
// csrc/image.hip (x2i_image_frontend: the resized image is the output) and csrc/image_tiles.hip (x2i_image_tiles: the resized image is cut
// into a grid of crops).  The arithmetic stands in include/frontend/x2i_image.h; what differs between the two entry points is the workgroup
// map and the store, and a whole image is the grid of one crop.  The passes themselves are device functions, which csrc/image_rows.hip
// (x2i_image_rows: Qwen2.5-VL's patch rows) calls from a kernel of its own with another store order.  Included by those three files only.
#pragma once
#include "x2i_common.h"

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
  long long ots;   // elements between the crops of a frame (0 for a whole image)
  int in_w, in_h, out_w, out_h, hk, vk;
  int tile;   // patches of columns per workgroup
  int rows;   // input rows a patch row's vertical taps reach, at most
  int ld;     // bytes of an LDS row
  int crop_w, crop_h;   // a crop's size in pixels (out_w, out_h for a whole image)
  int gx;               // crops per row of crops
  int tpc;              // column tiles per crop: the last one of a crop is partial at the crop's edge
};

__device__ __forceinline__ int clip8(unsigned acc) {
  const int v = ((int)acc) >> PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The input rows a patch row's vertical taps reach: rows row0 .. row0 + nrows of the frame (the patch row's own 14 where in_h == out_h)
__device__ __forceinline__ void patch_row_span(const ImageArgs& a, int ph, int* row0_, int* nrows_) {
  int row0 = PATCH * ph, nrows = PATCH;
  if (a.vk) {
    const int last = PATCH * ph + PATCH - 1;
    row0 = clampi(a.vb[2 * PATCH * ph], 0, a.in_h - 1);
    const int hi = clampi(a.vb[2 * last] + a.vb[2 * last + 1], row0, a.in_h);
    nrows = min(hi - row0, a.rows);
  }
  *row0_ = row0, *nrows_ = nrows;
}

// Phase 1 of a workgroup of 256 threads: the horizontal pass (or a copy) of the input rows src, src + row_pitch, ... (nrows of them) for
// the cw output columns from c0 of the resized image, uint8 [nrows][ld] in LDS, a thread per pixel with consecutive lanes on consecutive
// output columns.  Every value read from a bound table is clamped to the image and to ksize before it is used.
__device__ __forceinline__ void horizontal_pass_to_lds(const ImageArgs& a, const uint8_t* src, int nrows, int c0, int cw, uint8_t* img) {
  for (int i = threadIdx.x; i < nrows * cw; i += 256) {
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
}

// The vertical pass (or a copy) from LDS for one output value: row r of patch row ph, column col of the tile, channel c -> the uint8 of
// the resized image.  What is read of the bound table is clamped to the LDS rows and to ksize.
__device__ __forceinline__ int vertical_tap_value(const ImageArgs& a, const uint8_t* img, int ph, int r, int col, int c, int row0, int nrows) {
  if (!a.vk) return img[r * a.ld + 3 * col + c];
  const int oy = PATCH * ph + r;
  const int y0 = clampi(a.vb[2 * oy] - row0, 0, nrows);
  const int cnt = clampi(a.vb[2 * oy + 1], 0, min(a.vk, nrows - y0));
  const int* k = a.vc + (long long)oy * a.vk;
  const uint8_t* q = img + y0 * a.ld + 3 * col + c;
  unsigned s = 1u << (PREC - 1);
  for (int y = 0; y < cnt; ++y) s += q[y * a.ld] * (unsigned)k[y];
  return clip8(s);
}

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

// The LDS plan of in_h -> out_h (include/frontend/x2i_image.h): rows, the patches of columns per workgroup and the bytes of an LDS row;
// false where one patch of columns does not fit
inline bool image_lds_plan(int in_h, int out_h, int vk, int* rows_, int* tile_, int* ld_) {
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
  *rows_ = rows, *tile_ = tile, *ld_ = (3 * PATCH * tile + 3) & ~3;
  return (long long)rows * *ld_ <= LDS_BYTES;
}

// a: everything but tpc set.  One launch for n frames, gx * gy crops each.
inline void image_passes_launch(ImageArgs a, int n, int gy, bool planar, bool bf16, hipStream_t stream) {
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

}  // namespace
