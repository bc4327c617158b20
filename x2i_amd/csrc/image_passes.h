// What the three image front ends share.  The two passes (Pillow's 8-bit BICUBIC resize, the normalisation as a table lookup) are device
// functions here; image_passes_kernel, which stores a resized image as a grid of crops, lives in csrc/image.hip alone and is reached
// through image_passes_launch by csrc/image.hip (x2i_image_frontend: a whole image is the grid of one crop) and csrc/image_tiles.hip
// (x2i_image_tiles); csrc/image_rows.hip (x2i_image_rows: Qwen2.5-VL's patch rows) calls the passes from a kernel of its own with another
// store order.  The arithmetic stands in include/frontend/x2i_image.h.  The checks the three entry points make alike, and the fill of
// ImageArgs, are host functions at the end.  Included by those three files only.
#pragma once
#include "x2i_common.h"

#include <math.h>

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

// csrc/image.hip: one launch of image_passes_kernel for n frames, gx * gy crops each.  a: everything but tpc set.
void image_passes_launch(ImageArgs a, int n, int gy, bool planar, bool bf16, hipStream_t stream);

namespace {

constexpr int PATCH = 14, PREC = 22, MAX_PATCHES = 70, LDS_BYTES = 65536, MAX_IN = 65535;

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

// The arguments the three entry points take alike, under the names of include/frontend/x2i_image.h
struct ImageCall {
  const void* frames;
  long long frame_pitch, row_pitch;
  int in_w, in_h, out_w, out_h;
  const void *hbound, *hcoef;
  int hk;
  const void *vbound, *vcoef;
  int vk;
  const void* lut;
  void* out;
  int out_bf16;
};

// The checks of an entry point `what`, in the order every entry point makes them: image_check_pointers, its own count,
// image_check_input_size, its own output sizes, image_check_tables, its own output strides, image_plan_args.  X2I_OK or the error recorded.
inline int image_check_pointers(const char* what, const ImageCall& c) {
  if (!c.frames || !c.lut || !c.out) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer (frames, lut or out)", what);
  return X2I_OK;
}

inline int image_check_input_size(const char* what, const ImageCall& c) {
  if (c.in_w < 1 || c.in_w > MAX_IN || c.in_h < 1 || c.in_h > MAX_IN)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: in_w=%d and in_h=%d must be in 1..65535", what, c.in_w, c.in_h);
  return X2I_OK;
}

// The pitches, hk / vk against the axes' ksize, the tables exactly where an axis resizes
inline int image_check_tables(const char* what, const ImageCall& c) {
  if (c.row_pitch < 3LL * c.in_w || c.frame_pitch < (long long)(c.in_h - 1) * c.row_pitch + 3LL * c.in_w)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: row_pitch=%lld must be at least 3 * in_w and frame_pitch=%lld at least (in_h - 1) * row_pitch + 3 * in_w",
                         what, c.row_pitch, c.frame_pitch);
  const int want_hk = c.in_w != c.out_w ? Axis(c.in_w, c.out_w).ksize : 0, want_vk = c.in_h != c.out_h ? Axis(c.in_h, c.out_h).ksize : 0;
  if (c.hk != want_hk)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: hk=%d, the tables of in_w=%d -> out_w=%d have ksize %d", what, c.hk, c.in_w, c.out_w, want_hk);
  if (c.vk != want_vk)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: vk=%d, the tables of in_h=%d -> out_h=%d have ksize %d", what, c.vk, c.in_h, c.out_h, want_vk);
  if ((c.hk != 0) != (c.hbound != nullptr) || (c.hk != 0) != (c.hcoef != nullptr))
    return x2i_set_error(X2I_ERR_ARG, "%s: hbound and hcoef must be given exactly where in_w != out_w", what);
  if ((c.vk != 0) != (c.vbound != nullptr) || (c.vk != 0) != (c.vcoef != nullptr))
    return x2i_set_error(X2I_ERR_ARG, "%s: vbound and vcoef must be given exactly where in_h != out_h", what);
  return X2I_OK;
}

// The LDS plan (checked before the alignment, so that a refused scale is reported as such whatever the pointers are), the alignment, and
// *a filled for a whole image stored as the one crop of a 1 x 1 grid: all but the output strides ofs and ors, which are the entry point's
// own, and tpc, which belongs to the launch
inline int image_plan_args(const char* what, const ImageCall& c, ImageArgs* a) {
  int rows, tile, ld;
  if (!image_lds_plan(c.in_h, c.out_h, c.vk, &rows, &tile, &ld))
    return x2i_set_error(X2I_ERR_SHAPE, "%s: the LDS plan does not fit: in_h=%d -> out_h=%d needs %d rows of %d bytes for one patch of columns, at most %d bytes",
                         what, c.in_h, c.out_h, rows, ld, LDS_BYTES);
  const uintptr_t tabs = (uintptr_t)c.hbound | (uintptr_t)c.hcoef | (uintptr_t)c.vbound | (uintptr_t)c.vcoef | (uintptr_t)c.lut;
  if ((tabs & 3) || (((uintptr_t)c.out) & (c.out_bf16 ? 1 : 3)))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: the tables and lut must be 4-byte aligned, out aligned to its element size", what);
  a->frames = (const uint8_t*)c.frames;
  a->frame_pitch = c.frame_pitch;
  a->row_pitch = c.row_pitch;
  a->hb = (const int*)c.hbound;
  a->hc = (const int*)c.hcoef;
  a->vb = (const int*)c.vbound;
  a->vc = (const int*)c.vcoef;
  a->lut = (const float*)c.lut;
  a->out = c.out;
  a->ofs = 0, a->ots = 0;
  a->in_w = c.in_w, a->in_h = c.in_h, a->out_w = c.out_w, a->out_h = c.out_h, a->hk = c.hk, a->vk = c.vk;
  a->tile = tile, a->rows = rows, a->ld = ld;
  a->crop_w = c.out_w, a->crop_h = c.out_h, a->gx = 1;
  return X2I_OK;
}

}  // namespace
