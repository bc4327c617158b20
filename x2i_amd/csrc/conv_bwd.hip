// Backward kernels of the ControlNeXt control nets (x2i_amd/lightcontrol_train.py: ControlNeXtTrainer; include/x2i.h "ControlNeXt backward"):
//   conv_wgrad        dW[co][ci][ky][kx] (+)= sum over (b, oy, ox) of dY[b,oy,ox,co] * X[b, s oy + ky - p, s ox + kx - p, ci] and db[co] (+)= sum dY:
//                     a GEMM whose K axis is the pixels.  Both operands arrive pixel-major (NHWC); each step stages a [32 pixels][64 channels]
//                     tile of dY and of the tap-shifted X into LDS as it comes from HBM, and the MFMA operands are read back with gfx950's
//                     ds_read_b64_tr_b16, which delivers four pixels of one channel per lane -- no im2col, no transpose pass
//   conv_stem_wgrad   the same for Conv2d(3 -> Cout, k3, s2, p1) on the hint (embedding.0), 27 taps per output channel, plain FMAs
//   groupnorm_bwd     the backward of x2i_groupnorm_nhwc_bf16's y = act(w GN(x + pre_add) + b) (+ post_add): dx, d weight, d bias, d pre_add
//   linear_wgrad      dW (+)= dY^T act(X) of the time-embedding linears (B rows, f32)
// Every reduction is two-stage: per-split partials into the caller's workspace, then x2i_launch_reduce_rows in a fixed order.  No atomics:
// two launches on the same inputs are bit-identical.
#include "x2i_common.h"
#include "x2i_kernels.h"

namespace {

constexpr int WG_PX = 32;      // pixels (the GEMM's K) per step = the K of one 16 x 16 x 32 MFMA
constexpr int WG_CH = 64;      // output channels x input channels of a workgroup's tile (one tap)
constexpr int LDS_PITCH = 72;  // bf16 per LDS row: 144-byte rows keep the 16-byte stores aligned and every transposed read 8-byte aligned
constexpr int WG_TARGET = 1024;

typedef __attribute__((ext_vector_type(8))) __bf16 mbf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

// gfx950 ds_read_b64_tr_b16: lane 4q + p of a 16-lane group names row q, columns 4p .. 4p + 3 of a 4 x 16 block; lane i receives column i
// of the four rows (row q in element q).  Needs every lane of the wave active and an 8-byte-aligned address.
__device__ __forceinline__ s16x4_t lds_read_tr(const bf16_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p));
}

// The 16 x 16 x 32 operand of lane l: column (l & 15) of the tile's 16-column block at `col` (a channel), pixels 8 (l >> 4) .. + 7 (its K run):
// two transposed reads of four pixels each.
__device__ __forceinline__ mbf16x8_t tr_operand(const bf16_t* tile, int lane, int col) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const bf16_t* a = tile + (8 * g + q) * LDS_PITCH + col + 4 * p;
  const s16x4_t lo = lds_read_tr(a), hi = lds_read_tr(a + 4 * LDS_PITCH);
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(mbf16x8_t, v);
}

// grid: x = (tap, ci tile, co tile) with the co tile fastest, y = pixel split.  Four waves, each a 32 x 32 quarter of the 64 x 64 tile.
// part[split][co][ci][ky][kx] (the parameter's own layout) and, from the (tap 0, ci tile 0) workgroups when with_bias, part[split][Cout Cin KK + co].
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, long long dy_bs, int ldy,
                                                         float* __restrict__ part, long long part_stride, int H, int W, int Cin, int OH, int OW,
                                                         int Cout, int KH, int KW, int stride, int pad, long long P, long long chunk, int with_bias) {
  __shared__ __attribute__((aligned(16))) bf16_t sA[WG_PX * LDS_PITCH];  // dY tile [pixel][co]
  __shared__ __attribute__((aligned(16))) bf16_t sB[WG_PX * LDS_PITCH];  // X tile  [pixel][ci] at the tap's offset (zero outside the image)
  __shared__ float sBias[4][WG_CH];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nco = Cout / WG_CH, nci = Cin / WG_CH, KK = KH * KW;
  int blk = blockIdx.x;
  const int cot = blk % nco;
  blk /= nco;
  const int cit = blk % nci;
  const int tap = blk / nci;
  const int ky = tap / KW, kx = tap - ky * KW;
  const int co0 = cot * WG_CH, ci0 = cit * WG_CH;
  const long long p_begin = (long long)blockIdx.y * chunk;
  const long long p_end = p_begin + chunk < P ? p_begin + chunk : P;
  const long long OHW = (long long)OH * OW;
  const int lp = t >> 3, lc = t & 7;  // loader: pixel row of the tile, 16-byte piece of it
  const int wm = wave >> 1, wn = wave & 1;
  const bool bias_blk = with_bias && cit == 0 && tap == 0;
  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  for (long long p0 = p_begin; p0 < p_end; p0 += WG_PX) {
    const long long p = p0 + lp;
    bf16x8_t va = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0}, vb = va;
    if (p < p_end) {
      const long long b = p / OHW;
      const long long r = p - b * OHW;
      const int oy = (int)(r / OW), ox = (int)(r - (long long)oy * OW);
      va = *(const bf16x8_t*)(dy + b * dy_bs + r * ldy + co0 + lc * 8);
      const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) vb = *(const bf16x8_t*)(x + ((b * H + iy) * W + ix) * Cin + ci0 + lc * 8);
    }
    __syncthreads();  // the previous step's reads of the tiles are done
    *(bf16x8_t*)(sA + lp * LDS_PITCH + lc * 8) = va;
    *(bf16x8_t*)(sB + lp * LDS_PITCH + lc * 8) = vb;
    __syncthreads();
    mbf16x8_t fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = tr_operand(sA, lane, 32 * wm + 16 * i);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = tr_operand(sB, lane, 32 * wn + 16 * j);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    if (bias_blk) {  // column sums of the dY tile: wave w takes pixels 8w .. 8w + 7 (rows past p_end were stored as zeros)
#pragma unroll
      for (int r = 0; r < 8; ++r) bsum += bf16_to_f32(sA[(8 * wave + r) * LDS_PITCH + lane]);
    }
  }
  // C/D map of the 16 x 16 x 32 MFMA: column = lane & 15 (input channel), row = 4 (lane >> 4) + e (output channel)
  float* pp = part + (long long)blockIdx.y * part_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = co0 + 32 * wm + 16 * i + 4 * (lane >> 4) + e;
        const int ci = ci0 + 32 * wn + 16 * j + (lane & 15);
        pp[((long long)co * Cin + ci) * KK + tap] = acc[i][j][e];
      }
  if (bias_blk) {
    sBias[wave][lane] = bsum;
    __syncthreads();
    if (t < WG_CH) pp[(long long)Cout * Cin * KK + co0 + t] = ((sBias[0][t] + sBias[1][t]) + sBias[2][t]) + sBias[3][t];
  }
}

struct WgradPlan {
  long long P, chunk, part_stride;
  int nsplit, nblk;
};

bool wgrad_plan(int B, int OH, int OW, int Cin, int Cout, int KH, int KW, WgradPlan* pl) {
  if (B <= 0 || OH <= 0 || OW <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || Cin % WG_CH || Cout % WG_CH) return false;
  pl->P = (long long)B * OH * OW;
  pl->nblk = (Cout / WG_CH) * (Cin / WG_CH) * KH * KW;
  const long long steps = (pl->P + WG_PX - 1) / WG_PX;
  long long ns = (WG_TARGET + pl->nblk - 1) / pl->nblk;
  const long long max_ns = (steps + 7) / 8;  // at least eight steps per split
  if (ns > max_ns) ns = max_ns;
  if (ns < 1) ns = 1;
  const long long per = (steps + ns - 1) / ns;
  pl->chunk = per * WG_PX;
  pl->nsplit = (int)((steps + per - 1) / per);  // no empty split
  pl->part_stride = (long long)Cout * Cin * KH * KW + Cout;
  return true;
}

// ---------------------------------------------------------------------------------------------------- stem weight gradient
constexpr int STEM_BLOCKS = 1024;

// block: a run of output pixels; thread (sub, co): every fourth pixel of the run, one output channel, 27 taps + the bias.  The 27 input values
// of a pixel are the same for all lanes of a wave (broadcast loads).  part[blk][co][ci][ky][kx], then part[blk][Cout * 27 + co].
__global__ __launch_bounds__(256) void conv_stem_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part,
                                                              int H, int W, int OH, int OW, int Cout, long long P, long long chunk) {
  __shared__ float red[4][64][29];
  const int co = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const long long p_begin = (long long)blockIdx.x * chunk;
  const long long p_end = p_begin + chunk < P ? p_begin + chunk : P;
  const long long OHW = (long long)OH * OW;
  float acc[28];
#pragma unroll
  for (int i = 0; i < 28; ++i) acc[i] = 0.f;
  if (co < Cout) {
    for (long long p = p_begin + sub; p < p_end; p += 4) {
      const long long b = p / OHW;
      const long long r = p - b * OHW;
      const int oy = (int)(r / OW), ox = (int)(r - (long long)oy * OW);
      const float g = bf16_to_f32(dy[p * Cout + co]);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = 2 * ox + kx - 1;
          const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
          const bf16_t* px = x + ((b * H + (in ? iy : 0)) * W + (in ? ix : 0)) * 3;
#pragma unroll
          for (int ci = 0; ci < 3; ++ci) {
            const float v = in ? bf16_to_f32(px[ci]) : 0.f;
            acc[ci * 9 + ky * 3 + kx] = __builtin_fmaf(g, v, acc[ci * 9 + ky * 3 + kx]);
          }
        }
      }
      acc[27] += g;
    }
  }
#pragma unroll
  for (int i = 0; i < 28; ++i) red[sub][co][i] = acc[i];
  __syncthreads();
  float* pp = part + (long long)blockIdx.x * ((long long)Cout * 28);
  for (int i = threadIdx.x; i < Cout * 28; i += 256) {
    const int c = i / 28, e = i - c * 28;
    const float s = ((red[0][c][e] + red[1][c][e]) + red[2][c][e]) + red[3][c][e];
    pp[e < 27 ? c * 27 + e : Cout * 27 + c] = s;
  }
}

void stem_plan(int B, int OH, int OW, long long* P, long long* chunk, int* nblk) {
  *P = (long long)B * OH * OW;
  long long n = (*P + 255) / 256;  // at least 256 pixels per block
  if (n > STEM_BLOCKS) n = STEM_BLOCKS;
  if (n < 1) n = 1;
  *chunk = (*P + n - 1) / n;
  *nblk = (int)((*P + *chunk - 1) / *chunk);
}

// ---------------------------------------------------------------------------------------------------- GroupNorm backward
// y = act(z) (+ post_add), z = w[c] xhat + b[c], xhat = (x + pre_add[b][c] - mean_g) rstd_g.  The pass kernels run on grid (chunk, sample),
// 256 threads; thread t handles the 8-channel piece (t % (C / 8)) of every (256 / (C / 8))-th pixel of the chunk.
constexpr int GN_TARGET = 1024;

__device__ __forceinline__ float act_grad(float z, int act) {
  if (act == X2I_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == X2I_ACT_SILU) {
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
  }
  return 1.f;
}

__device__ __forceinline__ void load8(const bf16_t* p, float (&f)[8]) {
  const bf16x8_t v = *(const bf16x8_t*)p;
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = bf16_to_f32((bf16_t)v[i]);
}

// per-thread sums of 8 channels -> out[C][2] (a fixed-order sum over the block's pixel rows)
__device__ __forceinline__ void gn_block_store(const float (&s0)[8], const float (&s1)[8], float* red, float* out, int C) {
  const int cv = C / 8, rows = 256 / cv, t = threadIdx.x, vec = t % cv, r = t / cv;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    red[(r * C + vec * 8 + i) * 2] = s0[i];
    red[(r * C + vec * 8 + i) * 2 + 1] = s1[i];
  }
  __syncthreads();
  for (int i = t; i < 2 * C; i += 256) {
    float s = 0.f;
    for (int k = 0; k < rows; ++k) s += red[k * 2 * C + i];
    out[i] = s;
  }
}

// part[b][chunk][C][2] = (sum (x + pre_add), sum (x + pre_add)^2)
__global__ __launch_bounds__(256) void gn_bwd_stats_kernel(const bf16_t* __restrict__ x, const float* __restrict__ pre_add, long long HW, int C,
                                                           long long chunk, float* __restrict__ part, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float gn_red[];
  const int b = blockIdx.y, cv = C / 8, rows = 256 / cv, vec = threadIdx.x % cv, r = threadIdx.x / cv;
  const long long p_begin = (long long)blockIdx.x * chunk;
  const long long p_end = p_begin + chunk < HW ? p_begin + chunk : HW;
  float pa[8], s0[8], s1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    pa[i] = pre_add ? pre_add[(long long)b * C + vec * 8 + i] : 0.f;
    s0[i] = s1[i] = 0.f;
  }
  const bf16_t* xb = x + (long long)b * HW * C + vec * 8;
  for (long long p = p_begin + r; p < p_end; p += rows) {
    float v[8];
    load8(xb + p * C, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float u = v[i] + pa[i];
      s0[i] += u;
      s1[i] = __builtin_fmaf(u, u, s1[i]);
    }
  }
  gn_block_store(s0, s1, gn_red, part + ((long long)b * nchunk + blockIdx.x) * 2 * C, C);
}

// group statistics of one sample from its per-channel moments mom[C][2] (fixed order over the group's channels) -> st[G][2] = (mean, rstd)
__device__ __forceinline__ void gn_group_stats(const float* mom, int C, int G, long long HW, float eps, float* st) {
  const int cg = C / G;
  for (int g = threadIdx.x; g < G; g += 256) {
    float a = 0.f, q = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
      a += mom[2 * c];
      q += mom[2 * c + 1];
    }
    const float n = (float)HW * cg;
    const float mean = a / n;
    const float var = fmaxf(q / n - mean * mean, 0.f);
    st[2 * g] = mean;
    st[2 * g + 1] = rsqrtf(var + eps);
  }
}

// part[b][chunk][C][2] = (sum dz, sum dz xhat), dz = dy act'(z)
__global__ __launch_bounds__(256) void gn_bwd_dz_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
                                                        const bf16_t* __restrict__ bias, const float* __restrict__ pre_add, const float* __restrict__ mom,
                                                        long long HW, int C, int G, float eps, int act, long long chunk, float* __restrict__ part,
                                                        int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float gn_red[];
  const int b = blockIdx.y, cv = C / 8, rows = 256 / cv, vec = threadIdx.x % cv, r = threadIdx.x / cv;
  float* st = gn_red + rows * 2 * C;
  gn_group_stats(mom + (long long)b * C * 2, C, G, HW, eps, st);
  __syncthreads();
  const int cg = C / G;
  float pa[8], mean[8], rstd[8], gw[8], gb[8], s0[8], s1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = vec * 8 + i;
    pa[i] = pre_add ? pre_add[(long long)b * C + c] : 0.f;
    mean[i] = st[2 * (c / cg)];
    rstd[i] = st[2 * (c / cg) + 1];
    gw[i] = bf16_to_f32(w[c]);
    gb[i] = bf16_to_f32(bias[c]);
    s0[i] = s1[i] = 0.f;
  }
  const long long p_begin = (long long)blockIdx.x * chunk;
  const long long p_end = p_begin + chunk < HW ? p_begin + chunk : HW;
  const long long off = (long long)b * HW * C + vec * 8;
  for (long long p = p_begin + r; p < p_end; p += rows) {
    float v[8], g[8];
    load8(x + off + p * C, v);
    load8(dy + off + p * C, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float xh = (v[i] + pa[i] - mean[i]) * rstd[i];
      const float dz = g[i] * act_grad(__builtin_fmaf(gw[i], xh, gb[i]), act);
      s0[i] += dz;
      s1[i] = __builtin_fmaf(dz, xh, s1[i]);
    }
  }
  gn_block_store(s0, s1, gn_red, part + ((long long)b * nchunk + blockIdx.x) * 2 * C, C);
}

// per sample b: coef[b][G][4] = (mean, rstd, mean_g(w dz), mean_g(w dz xhat)) and d pre_add[b][c] = sum over the pixels of dx (closed form);
// block 0 also finishes d weight / d bias (the samples summed in order)
__global__ __launch_bounds__(256) void gn_bwd_finish_kernel(const bf16_t* __restrict__ w, const float* __restrict__ mom, const float* __restrict__ sdz,
                                                            long long HW, int B, int C, int G, float eps, float* __restrict__ coef,
                                                            float* __restrict__ dpre, float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  __shared__ float st[4 * 1024];
  const int b = blockIdx.x, cg = C / G;
  gn_group_stats(mom + (long long)b * C * 2, C, G, HW, eps, st);
  __syncthreads();
  const float* s = sdz + (long long)b * C * 2;
  const float n = (float)HW * cg;
  for (int g = threadIdx.x; g < G; g += 256) {
    float a = 0.f, q = 0.f;
    for (int c = g * cg; c < (g + 1) * cg; ++c) {
      const float wc = bf16_to_f32(w[c]);
      a = __builtin_fmaf(wc, s[2 * c], a);
      q = __builtin_fmaf(wc, s[2 * c + 1], q);
    }
    float* cf = coef + ((long long)b * G + g) * 4;
    cf[0] = st[2 * g];
    cf[1] = st[2 * g + 1];
    cf[2] = a / n;
    cf[3] = q / n;
    st[2 * G + 2 * g] = a / n;
    st[2 * G + 2 * g + 1] = q / n;
  }
  __syncthreads();
  if (dpre) {
    const float* m = mom + (long long)b * C * 2;
    for (int c = threadIdx.x; c < C; c += 256) {
      const int g = c / cg;
      const float mean = st[2 * g], rstd = st[2 * g + 1], A = st[2 * G + 2 * g], Q = st[2 * G + 2 * g + 1];
      const float sxh = (m[2 * c] - (float)HW * mean) * rstd;  // sum over the pixels of xhat
      dpre[(long long)b * C + c] = rstd * (bf16_to_f32(w[c]) * s[2 * c] - (float)HW * A - Q * sxh);
    }
  }
  if (b == 0 && dw) {
    for (int c = threadIdx.x; c < C; c += 256) {
      float a = 0.f, q = 0.f;
      for (int k = 0; k < B; ++k) {
        a += sdz[((long long)k * C + c) * 2];
        q += sdz[((long long)k * C + c) * 2 + 1];
      }
      dw[c] = accumulate ? dw[c] + q : q;
      db[c] = accumulate ? db[c] + a : a;
    }
  }
}

// dx = rstd (w dz - mean_g(w dz) - xhat mean_g(w dz xhat)), zeroed where x <= 0 with in_relu, plus dx_in; one bf16 rounding
__global__ __launch_bounds__(256) void gn_bwd_dx_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
                                                        const bf16_t* __restrict__ bias, const float* __restrict__ pre_add, const float* __restrict__ coef,
                                                        const bf16_t* dx_in, bf16_t* dx, long long HW, int C, int G, int act, int in_relu,
                                                        long long chunk) {
  const int b = blockIdx.y, cv = C / 8, rows = 256 / cv, vec = threadIdx.x % cv, r = threadIdx.x / cv;
  const int cg = C / G;
  float pa[8], mean[8], rstd[8], A[8], Q[8], gw[8], gb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = vec * 8 + i;
    const float* cf = coef + ((long long)b * G + c / cg) * 4;
    pa[i] = pre_add ? pre_add[(long long)b * C + c] : 0.f;
    mean[i] = cf[0];
    rstd[i] = cf[1];
    A[i] = cf[2];
    Q[i] = cf[3];
    gw[i] = bf16_to_f32(w[c]);
    gb[i] = bf16_to_f32(bias[c]);
  }
  const long long p_begin = (long long)blockIdx.x * chunk;
  const long long p_end = p_begin + chunk < HW ? p_begin + chunk : HW;
  const long long off = (long long)b * HW * C + vec * 8;
  for (long long p = p_begin + r; p < p_end; p += rows) {
    float v[8], g[8], d0[8], o[8];
    load8(x + off + p * C, v);
    load8(dy + off + p * C, g);
    if (dx_in) load8(dx_in + off + p * C, d0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float xh = (v[i] + pa[i] - mean[i]) * rstd[i];
      const float dz = g[i] * act_grad(__builtin_fmaf(gw[i], xh, gb[i]), act);
      float d = rstd[i] * (gw[i] * dz - A[i] - xh * Q[i]);
      if (in_relu && !(v[i] > 0.f)) d = 0.f;
      o[i] = dx_in ? d + d0[i] : d;
    }
    bf16x8_t ov;
#pragma unroll
    for (int i = 0; i < 8; ++i) ov[i] = (short)f32_to_bf16(o[i]);
    *(bf16x8_t*)(dx + off + p * C) = ov;
  }
}

struct GnPlan {
  int nchunk, red_floats;
  long long chunk, part, mom, sdz, coef, total;
};

bool gn_plan(int B, long long HW, int C, int G, GnPlan* pl) {
  if (B <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % 8 || C % G || 256 % (C / 8) || C > 1024) return false;
  const int rows = 256 / (C / 8);
  long long n = (GN_TARGET + B - 1) / B;
  const long long max_n = (HW + 63) / 64;
  if (n > max_n) n = max_n;
  if (n < 1) n = 1;
  pl->chunk = (HW + n - 1) / n;
  pl->nchunk = (int)((HW + pl->chunk - 1) / pl->chunk);
  pl->red_floats = rows * 2 * C + 2 * G;
  pl->part = 0;
  pl->mom = (long long)B * pl->nchunk * 2 * C;
  pl->sdz = pl->mom + (long long)B * 2 * C;
  pl->coef = pl->sdz + (long long)B * 2 * C;
  pl->total = pl->coef + (long long)B * G * 4;
  return true;
}

// dw[n][k] (+)= sum_b dy[b][n] act(x[b][k]); the threads past N K: db[n] (+)= sum_b dy[b][n].  The samples are summed in order.
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dw,
                                                           float* __restrict__ db, int B, int N, int K, int act_in, int accumulate) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nk = (long long)N * K;
  if (i < nk) {
    const int n = (int)(i / K), k = (int)(i - (long long)n * K);
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
      const float xv = x[(long long)b * K + k];
      s = __builtin_fmaf(dy[(long long)b * N + n], act_in == X2I_ACT_SILU ? xv / (1.f + expf(-xv)) : xv, s);
    }
    dw[i] = accumulate ? dw[i] + s : s;
  } else if (db && i < nk + N) {
    const int n = (int)(i - nk);
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dy[(long long)b * N + n];
    db[n] = accumulate ? db[n] + s : s;
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ---------------------------------------------------------------------------------------------------- launchers
long long x2i_conv_wgrad_workspace(int B, int OH, int OW, int Cin, int Cout, int KH, int KW) {
  WgradPlan pl;
  if (!wgrad_plan(B, OH, OW, Cin, Cout, KH, KW, &pl)) return -1;
  return (long long)pl.nsplit * pl.part_stride;
}

int x2i_launch_conv_wgrad(const void* x, const void* dy, long long dy_bs, int ldy, float* dw, float* db, int B, int H, int W, int Cin, int OH, int OW,
                          int Cout, int KH, int KW, int stride, int pad, int accumulate, float* ws, long long ws_floats, hipStream_t stream) {
  if (!x || !dy || !dw || !ws) return x2i_set_error(X2I_ERR_ARG, "conv_wgrad: null pointer");
  WgradPlan pl;
  if (!wgrad_plan(B, OH, OW, Cin, Cout, KH, KW, &pl) || H <= 0 || W <= 0 || stride <= 0 || pad < 0)
    return x2i_set_error(X2I_ERR_SHAPE, "conv_wgrad: need Cin, Cout multiples of 64 and positive sizes (B=%d OH=%d OW=%d Cin=%d Cout=%d KH=%d KW=%d)", B, OH,
                         OW, Cin, Cout, KH, KW);
  if ((OH - 1) * stride + KH - pad > H + pad || (OW - 1) * stride + KW - pad > W + pad)
    return x2i_set_error(X2I_ERR_SHAPE, "conv_wgrad: %d x %d outputs of a %d x %d / stride %d / pad %d window leave the padded %d x %d input", OH, OW, KH,
                         KW, stride, pad, H, W);
  if (ldy < Cout || ldy % 8 || dy_bs % 8 || !al16(x) || !al16(dy))
    return x2i_set_error(X2I_ERR_ALIGN, "conv_wgrad: need ldy >= Cout, ldy and the batch stride of dy multiples of 8, 16-byte aligned x and dy");
  const long long need = (long long)pl.nsplit * pl.part_stride;
  if (ws_floats < need) return x2i_set_error(X2I_ERR_ARG, "conv_wgrad: workspace of %lld floats, need %lld (x2i_conv_wgrad_workspace_floats)", ws_floats, need);
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3(pl.nblk, pl.nsplit), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)dy, dy_bs, ldy, ws,
                     pl.part_stride, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, pl.P, pl.chunk, db ? 1 : 0);
  int rc = x2i_check_launch("conv_wgrad");
  if (rc) return rc;
  const long long len = (long long)Cout * Cin * KH * KW;
  rc = x2i_launch_reduce_rows(ws, 0, pl.nsplit, pl.part_stride, dw, 0, 1, (int)len, accumulate, 1.f, stream);
  if (rc || !db) return rc;
  return x2i_launch_reduce_rows(ws + len, 0, pl.nsplit, pl.part_stride, db, 0, 1, Cout, accumulate, 1.f, stream);
}

long long x2i_conv_stem_wgrad_workspace(int B, int H, int W, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > 64) return -1;
  long long P, chunk;
  int nblk;
  stem_plan(B, (H + 1) / 2, (W + 1) / 2, &P, &chunk, &nblk);
  return (long long)nblk * Cout * 28;
}

int x2i_launch_conv_stem_wgrad(const void* x, const void* dy, float* dw, float* db, int B, int H, int W, int Cout, int accumulate, float* ws,
                               long long ws_floats, hipStream_t stream) {
  if (!x || !dy || !dw || !ws) return x2i_set_error(X2I_ERR_ARG, "conv_stem_wgrad: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout > 64) return x2i_set_error(X2I_ERR_SHAPE, "conv_stem_wgrad: need positive sizes and Cout <= 64");
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  long long P, chunk;
  int nblk;
  stem_plan(B, OH, OW, &P, &chunk, &nblk);
  if (ws_floats < (long long)nblk * Cout * 28)
    return x2i_set_error(X2I_ERR_ARG, "conv_stem_wgrad: workspace of %lld floats, need %lld (x2i_conv_stem_wgrad_workspace_floats)", ws_floats,
                         (long long)nblk * Cout * 28);
  hipLaunchKernelGGL(conv_stem_wgrad_kernel, dim3(nblk), dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)dy, ws, H, W, OH, OW, Cout, P, chunk);
  int rc = x2i_check_launch("conv_stem_wgrad");
  if (rc) return rc;
  rc = x2i_launch_reduce_rows(ws, 0, nblk, (long long)Cout * 28, dw, 0, 1, Cout * 27, accumulate, 1.f, stream);
  if (rc || !db) return rc;
  return x2i_launch_reduce_rows(ws + (long long)Cout * 27, 0, nblk, (long long)Cout * 28, db, 0, 1, Cout, accumulate, 1.f, stream);
}

long long x2i_groupnorm_bwd_workspace(int B, long long HW, int C, int G) {
  GnPlan pl;
  return gn_plan(B, HW, C, G, &pl) ? pl.total : -1;
}

int x2i_launch_groupnorm_bwd(const void* x, const void* dy, const void* w, const void* b, const float* pre_add, void* dx, const void* dx_in, float* dw,
                             float* db, float* dpre, int B, long long HW, int C, int G, float eps, int act, int in_relu, int accumulate, float* ws,
                             long long ws_floats, hipStream_t stream) {
  if (!x || !dy || !w || !b || !dx || !ws) return x2i_set_error(X2I_ERR_ARG, "groupnorm_bwd: null pointer");
  if ((dw == nullptr) != (db == nullptr)) return x2i_set_error(X2I_ERR_ARG, "groupnorm_bwd: d weight and d bias go together");
  if (act != X2I_ACT_NONE && act != X2I_ACT_RELU && act != X2I_ACT_SILU) return x2i_set_error(X2I_ERR_ARG, "groupnorm_bwd: activation %d (none, ReLU, SiLU)", act);
  if (in_relu && pre_add) return x2i_set_error(X2I_ERR_ARG, "groupnorm_bwd: in_relu and pre_add do not go together");
  if (dpre && !pre_add) return x2i_set_error(X2I_ERR_ARG, "groupnorm_bwd: d pre_add needs pre_add");
  GnPlan pl;
  if (!gn_plan(B, HW, C, G, &pl))
    return x2i_set_error(X2I_ERR_SHAPE, "groupnorm_bwd: need C %% 8 == 0, C %% G == 0, 256 %% (C / 8) == 0, C <= 1024 (B=%d C=%d G=%d)", B, C, G);
  if (!al16(x) || !al16(dy) || !al16(dx) || (dx_in && !al16(dx_in))) return x2i_set_error(X2I_ERR_ALIGN, "groupnorm_bwd: tensors must be 16-byte aligned");
  if (ws_floats < pl.total)
    return x2i_set_error(X2I_ERR_ARG, "groupnorm_bwd: workspace of %lld floats, need %lld (x2i_groupnorm_bwd_workspace_floats)", ws_floats, pl.total);
  const dim3 grid(pl.nchunk, B);
  const size_t lds = (size_t)pl.red_floats * 4;
  hipLaunchKernelGGL(gn_bwd_stats_kernel, grid, dim3(256), lds, stream, (const bf16_t*)x, pre_add, HW, C, pl.chunk, ws + pl.part, pl.nchunk);
  int rc = x2i_check_launch("groupnorm_bwd");
  if (rc) return rc;
  if ((rc = x2i_launch_reduce_rows(ws + pl.part, (long long)pl.nchunk * 2 * C, pl.nchunk, 2 * C, ws + pl.mom, 2 * C, B, 2 * C, 0, 1.f, stream))) return rc;
  hipLaunchKernelGGL(gn_bwd_dz_kernel, grid, dim3(256), lds, stream, (const bf16_t*)x, (const bf16_t*)dy, (const bf16_t*)w, (const bf16_t*)b, pre_add,
                     ws + pl.mom, HW, C, G, eps, act, pl.chunk, ws + pl.part, pl.nchunk);
  if ((rc = x2i_check_launch("groupnorm_bwd"))) return rc;
  if ((rc = x2i_launch_reduce_rows(ws + pl.part, (long long)pl.nchunk * 2 * C, pl.nchunk, 2 * C, ws + pl.sdz, 2 * C, B, 2 * C, 0, 1.f, stream))) return rc;
  hipLaunchKernelGGL(gn_bwd_finish_kernel, dim3(B), dim3(256), 0, stream, (const bf16_t*)w, ws + pl.mom, ws + pl.sdz, HW, B, C, G, eps, ws + pl.coef,
                     dpre, dw, db, accumulate);
  if ((rc = x2i_check_launch("groupnorm_bwd"))) return rc;
  hipLaunchKernelGGL(gn_bwd_dx_kernel, grid, dim3(256), 0, stream, (const bf16_t*)x, (const bf16_t*)dy, (const bf16_t*)w, (const bf16_t*)b, pre_add,
                     ws + pl.coef, (const bf16_t*)dx_in, (bf16_t*)dx, HW, C, G, act, in_relu, pl.chunk);
  return x2i_check_launch("groupnorm_bwd");
}

int x2i_launch_linear_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int N, int K, int act_in, int accumulate, hipStream_t stream) {
  if (!dy || !x || !dw) return x2i_set_error(X2I_ERR_ARG, "linear_wgrad: null pointer");
  if (B <= 0 || N <= 0 || K <= 0) return x2i_set_error(X2I_ERR_SHAPE, "linear_wgrad: need positive sizes");
  if (act_in != X2I_ACT_NONE && act_in != X2I_ACT_SILU) return x2i_set_error(X2I_ERR_ARG, "linear_wgrad: act_in %d (none, SiLU)", act_in);
  const long long n = (long long)N * K + N;
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dy, x, dw, db, B, N, K, act_in, accumulate);
  return x2i_check_launch("linear_wgrad");
}
