// Pieces the encoder extension files share (t5.hip, clip.hip, qwen.hip, qwen_extend.hip, vit.hip, siglip.hip, internvit.hip, whisper.hip, encoder_attention.hip): the
// attention kernel's constants and its LDS-DMA load, the bf16 chunk unpacker, the stored head width and the grid of the row-chunk kernels, the V -> V^T tile transposer of the
// head-split kernels, the plain head split of t5.hip and siglip.hip, the rotate-half RoPE head split of qwen.hip and vit.hip, the patch rows of siglip.hip and internvit.hip and the
// row-chunk activation kernel behind the gated GELU, SwiGLU and quick-GELU entry points.  Other .hip files keep private helpers of the same names in their own anonymous
// namespaces, so these stay out of x2i_common.h and stand in the anonymous namespace too: every includer gets its own copy, and a file that has
// both this header and a helper of its own of one of these names does not compile.
#pragma once
#include "x2i_common.h"

namespace {

constexpr int KVB = 64;               // keys per attention tile
constexpr float NEG_BIG = -1.0e30f;   // a masked score
constexpr float M_FLOOR = -1.0e15f;   // where the causal mode's running maximum starts (encoder_attention.hip)
constexpr float LOG2E = 1.4426950408889634f;
constexpr int RELBIAS_RMAX = 2047;   // largest clamp distance of the relative-bias mode: the table region of the LDS image is 16 KiB

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ void unpack8(const uint4& p, float (&v)[8]) {
  v[0] = __uint_as_float(p.x << 16); v[1] = __uint_as_float(p.x & 0xffff0000u);
  v[2] = __uint_as_float(p.y << 16); v[3] = __uint_as_float(p.y & 0xffff0000u);
  v[4] = __uint_as_float(p.z << 16); v[5] = __uint_as_float(p.z & 0xffff0000u);
  v[6] = __uint_as_float(p.w << 16); v[7] = __uint_as_float(p.w & 0xffff0000u);
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

inline int stored_width(int dk) { return dk == 80 ? 128 : dk; }   // heads of 80 are stored 128 wide (include/x2i_vit.h)

// Workgroups of 256 threads for a grid-stride kernel with one thread per 16-byte chunk
inline unsigned chunk_blocks(long long chunks) { return (unsigned)((chunks + 255) / 256 < 8192 ? (chunks + 255) / 256 : 8192); }

// ------------------------------------------------------------------------------------------------------------------- V -> V^T
// The whole workgroup (256 threads) transposes tokens s0 .. s0+63 of one head: v points at the head's dk columns of token 0 (row stride
// ld), vt at the head's VT rows [dk][Spad].  V goes through an LDS tile [64 tokens][dk + 2] and leaves as 16-byte pieces of VT rows
// (scalar stores in the one piece that straddles S: columns >= S stay untouched).  dk <= 128.
__device__ __forceinline__ void v_tile_to_vt(const bf16_t* __restrict__ v, long long ld, bf16_t* __restrict__ vt, int s0, int S, int Spad, int dk) {
  __shared__ uint32_t tile[64 * (128 + 2) / 2];
  const int tid = threadIdx.x;
  const int ck = dk >> 3;           // 16-byte chunks per head row
  const int pitch = (dk + 2) >> 1;  // LDS row pitch in dwords
  for (int c = tid; c < 64 * ck; c += 256) {
    const int tok = c / ck, ch = c - tok * ck;
    const int s = s0 + tok;
    uint4 p = make_uint4(0u, 0u, 0u, 0u);
    if (s < S) p = *(const uint4*)(v + s * ld + ch * 8);
    uint32_t* t = tile + tok * pitch + ch * 4;
    t[0] = p.x; t[1] = p.y; t[2] = p.z; t[3] = p.w;
  }
  __syncthreads();
  const bf16_t* tb = (const bf16_t*)tile;
  for (int i = tid; i < dk * 8; i += 256) {
    const int tc = i & 7, d = i >> 3;
    const int s = s0 + tc * 8;
    if (s >= S) continue;
    bf16_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = tb[(tc * 8 + j) * (2 * pitch) + d];
    bf16_t* dst = vt + (long long)d * Spad + s;
    if (s + 8 <= S) {
      *(uint4*)dst = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (s + j < S) dst[j] = e[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- head split
// The body of the kernels behind x2i_t5_head_split_bf16 (dkp = dk) and x2i_siglip_head_split_bf16 (dkp = stored_width(dk)), 256 threads,
// grid (64-token tiles, H, B): one workgroup per (64-token tile, head, sample); Q and K rows are 16-byte copies into rows of dkp >= dk
// elements, V goes through v_tile_to_vt into the head's dkp V^T rows.  Only d < dk and s < S are written.  dk % 8 == 0.
__device__ __forceinline__ void head_split_body(const bf16_t* __restrict__ qkv, long long ld, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                bf16_t* __restrict__ VT, int S, int Spad, int H, int dk, int dkp) {
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int ck = dk >> 3;           // 16-byte chunks per head row
  const long long bh = (long long)b * H + h;
  const int inner = H * dk;
  for (int c = tid; c < 64 * ck; c += 256) {
    const int tok = c / ck, ch = c - tok * ck;
    const int s = s0 + tok;
    if (s >= S) continue;
    const bf16_t* src = qkv + ((long long)b * S + s) * ld + h * dk + ch * 8;
    const long long dst = (bh * Spad + s) * dkp + ch * 8;
    *(uint4*)(Q + dst) = *(const uint4*)src;
    *(uint4*)(K + dst) = *(const uint4*)(src + inner);
  }
  v_tile_to_vt(qkv + (long long)b * S * ld + 2 * inner + h * dk, ld, VT + bh * dkp * Spad, s0, S, Spad, dk);
}

// ------------------------------------------------------------------------------------------------------------------- RoPE + head split
// Eight rotate-half pairs (x[d], x[d + half]), d = 0 .. 7 from src, against eight entries of the half tables: lo = x1 cos - x2 sin, up = x2 cos + x1 sin,
// packed bf16 pairs.  One rounding: both products and their sum stay f32 (the library rounds each product and the sum to bf16).
__device__ __forceinline__ void rope_rotate8(const bf16_t* __restrict__ src, int half, const float* __restrict__ cp, const float* __restrict__ sp,
                                             uint32_t (&lo)[4], uint32_t (&up)[4]) {
  float x1[8], x2[8];
  unpack8(*(const uint4*)src, x1);
  unpack8(*(const uint4*)(src + half), x2);
  const float4 c0 = *(const float4*)cp, c1 = *(const float4*)(cp + 4), t0 = *(const float4*)sp, t1 = *(const float4*)(sp + 4);
  const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float ss[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    lo[j >> 1] = pack_bf16x2(__fsub_rn(__fmul_rn(x1[j], cc[j]), __fmul_rn(x2[j], ss[j])),
                             __fsub_rn(__fmul_rn(x1[j + 1], cc[j + 1]), __fmul_rn(x2[j + 1], ss[j + 1])));
    up[j >> 1] = pack_bf16x2(__fadd_rn(__fmul_rn(x2[j], cc[j]), __fmul_rn(x1[j], ss[j])),
                             __fadd_rn(__fmul_rn(x2[j + 1], cc[j + 1]), __fmul_rn(x1[j + 1], ss[j + 1])));
  }
}

// The body of the kernels behind x2i_qwen_rope_split_bf16 and x2i_vit_rope_split_bf16, 256 threads, grid (64-token tiles, Hq + Hkv, B).
// One workgroup per (64-token tile, head, sample); heads 0 .. Hq-1 are query heads, Hq .. Hq+Hkv-1 key/value heads.  A work item rotates
// eight pairs (x[d], x[d + dk/2]), d = 8c .. 8c+7: two 16-byte loads of the row, two 32-byte pieces of each half table, two 16-byte stores.
// A key/value head's V goes through v_tile_to_vt, as head_split_body's does.  dkp >= dk: the width the heads are STORED at (Q / K rows of
// dkp elements, dkp V^T rows per head); only columns / rows d < dk are written.  dk % 16 == 0.
__device__ __forceinline__ void rope_split_body(const bf16_t* __restrict__ qkv, long long ld, const float* __restrict__ cs,
                                                const float* __restrict__ sn, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                bf16_t* __restrict__ VT, int S, int Spad, int Hq, int Hkv, int dk, int dkp) {
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, hh = blockIdx.y, b = blockIdx.z;
  const bool is_q = hh < Hq;
  const int g = hh - Hq;            // key/value head (when !is_q)
  const int half = dk >> 1;
  const int cr = dk >> 4;           // work items per token: 16-byte chunks of one half
  const int col = is_q ? hh * dk : (Hq + g) * dk;   // the head's first column in q | k
  bf16_t* dst_base = is_q ? Q + ((long long)b * Hq + hh) * Spad * dkp : K + ((long long)b * Hkv + g) * Spad * dkp;
  for (int c = tid; c < 64 * cr; c += 256) {
    const int tok = c / cr, ch = c - tok * cr;
    const int s = s0 + tok;
    if (s >= S) continue;
    const bf16_t* src = qkv + ((long long)b * S + s) * ld + col + ch * 8;
    const float* cp = cs + ((long long)b * S + s) * half + ch * 8;
    const float* sp = sn + ((long long)b * S + s) * half + ch * 8;
    uint32_t lo[4], up[4];
    rope_rotate8(src, half, cp, sp, lo, up);
    bf16_t* dst = dst_base + (long long)s * dkp + ch * 8;
    *(uint4*)dst = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *(uint4*)(dst + half) = make_uint4(up[0], up[1], up[2], up[3]);
  }
  if (is_q) return;   // (uniform across the workgroup)

  v_tile_to_vt(qkv + (long long)b * S * ld + (Hq + Hkv + g) * dk, ld, VT + ((long long)b * Hkv + g) * dkp * Spad, s0, S, Spad, dk);
}

// ------------------------------------------------------------------------------------------------------------------- patch rows
// The body of the kernels behind x2i_internvit_patch_rows_bf16 and x2i_siglip_patch_rows_bf16 (a strip is a grid of one row: gw = L, channel
// stride P * strip_ld), grid-stride, one thread per 16-byte chunk of Xp.  Column col = ci*P*P + y*P + x of row b*L + r*gw + q is
// img[b][ci][r*P + y][q*P + x]: (ci, y, x) is divided out once per chunk and then carried.  A patch row starts at a multiple of P elements
// (28 bytes for P = 14), so the image is read element by element (consecutive lanes read consecutive 16-byte runs of one image row most
// of the time); columns >= 3*P*P are zero.
__device__ __forceinline__ void patch_rows_body(const bf16_t* __restrict__ img, long long ibs, long long ics, long long ild,
                                                bf16_t* __restrict__ Xp, long long ldx, long long rows, int L, int gw, int P, int Kp) {
  const int nc = Kp >> 3, PP = P * P, K3 = 3 * PP;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int ch = (int)(i - row * nc);
    const long long b = row / L;
    const int p = (int)(row - b * L);
    const int r = p / gw, q = p - r * gw;
    const bf16_t* src = img + b * ibs + (long long)r * P * ild + (long long)q * P;
    int col = ch * 8;
    int ci = col / PP;
    int y = (col - ci * PP) / P;
    int x = col - ci * PP - y * P;
    bf16_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j, ++col) {
      e[j] = col < K3 ? src[ci * ics + y * ild + x] : (bf16_t)0;
      if (++x == P) {
        x = 0;
        if (++y == P) { y = 0; ++ci; }
      }
    }
    *(uint4*)(Xp + row * ldx + ch * 8) = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16),
                                                   e[6] | ((uint32_t)e[7] << 16));
  }
}

// ------------------------------------------------------------------------------------------------------------------- row activations
// One thread per 16-byte chunk of Y: y = bf16(act(a)), or with GATED, rows [a (F) | b (F)] -> y = bf16(act(a) * b).
struct GeluTanhAct { __device__ __forceinline__ float operator()(float x) const { return gelu_tanh_f(x); } };
struct SiluAct { __device__ __forceinline__ float operator()(float x) const { return silu_f(x); } };
struct QuickGeluAct { __device__ __forceinline__ float operator()(float x) const { return quick_gelu_f(x); } };

template <class Act, bool GATED>
__global__ __launch_bounds__(256) void row_act_kernel(const bf16_t* __restrict__ X, long long ldx, bf16_t* __restrict__ Y, long long ldy,
                                                      long long rows, int F) {
  const Act act;
  const int nc = F >> 3;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    const bf16_t* src = X + row * ldx + c * 8;
    float a[8], g[8];
    unpack8(*(const uint4*)src, a);
    if constexpr (GATED) unpack8(*(const uint4*)(src + F), g);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // one rounding: the activation stays f32 until the gate has multiplied it (the library rounds it to bf16 in between)
      if constexpr (GATED) o[j >> 1] = pack_bf16x2(__fmul_rn(act(a[j]), g[j]), __fmul_rn(act(a[j + 1]), g[j + 1]));
      else o[j >> 1] = pack_bf16x2(act(a[j]), act(a[j + 1]));
    }
    *(uint4*)(Y + row * ldy + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

template <class Act, bool GATED>
int launch_row_act(const char* what, const void* X, long long ldx, void* Y, long long ldy, long long rows, int F, hipStream_t stream) {
  hipLaunchKernelGGL((row_act_kernel<Act, GATED>), dim3(chunk_blocks(rows * (F / 8))), dim3(256), 0, stream, (const bf16_t*)X, ldx, (bf16_t*)Y, ldy, rows, F);
  return x2i_check_launch(what);
}

}  // namespace
