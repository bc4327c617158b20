// The Qwen2 prompt extension's kernels (include/x2i_qwen_extend.h): a chunk of n new rows run against a key/value cache that already holds
// the keys before them.  Rotate-half RoPE with the head split into the cache at an arbitrary first slot, here; the causal attention of the
// chunk's rows over the cache is encoder_attention.hip's CAUSAL_EXT mode.  All coordinates are physical cache slots: row s of the chunk
// lives at slot row0 + s.  bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_qwen_extend.h"

namespace {

// 256 threads, grid (64-slot tiles of the cache that meet [row0, row0 + n), Hq + Hkv, B).  A workgroup owns the slots a0 .. a0 + 63 (a0 a
// multiple of 64) of one head of one sample, so that a V^T column group of eight slots is one aligned 16 bytes whatever row0 is.
//   * q / k: rope_split_body's work item (rope_rotate8, two 16-byte stores), the row written at slot a instead of s = a - row0
//   * v: through an LDS tile [64 slots][dk + 2] into V^T columns.  A group wholly inside [row0, row0 + n) is one 16-byte store; the two
//     groups that the chunk's ends cut are written from the outside in with 2-, 4- and 8-byte stores at their natural alignment, so that
//     no column outside the chunk is touched
__global__ __launch_bounds__(256) void qwen_extend_rope_split_kernel(const bf16_t* __restrict__ qkv, long long ld, const float* __restrict__ cs,
                                                                     const float* __restrict__ sn, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                                     bf16_t* __restrict__ VT, int row0, int n, int cap, int Hq, int Hkv, int dk) {
  __shared__ uint32_t tile[64 * (128 + 2) / 2];
  const int tid = threadIdx.x;
  const int a0 = (row0 / 64 + blockIdx.x) * 64, hh = blockIdx.y, b = blockIdx.z;
  const int end = row0 + n;
  const bool is_q = hh < Hq;
  const int g = hh - Hq;            // key/value head (when !is_q)
  const int half = dk >> 1;
  const int cr = dk >> 4;           // work items per token: 16-byte chunks of one half
  const int col = is_q ? hh * dk : (Hq + g) * dk;   // the head's first column in q | k
  bf16_t* dst_base = is_q ? Q + ((long long)b * Hq + hh) * cap * dk : K + ((long long)b * Hkv + g) * cap * dk;
  for (int c = tid; c < 64 * cr; c += 256) {
    const int tok = c / cr, ch = c - tok * cr;
    const int a = a0 + tok;
    if (a < row0 || a >= end) continue;
    const long long r = (long long)b * n + (a - row0);   // the chunk's row
    uint32_t lo[4], up[4];
    rope_rotate8(qkv + r * ld + col + ch * 8, half, cs + r * half + ch * 8, sn + r * half + ch * 8, lo, up);
    bf16_t* dst = dst_base + (long long)a * dk + ch * 8;
    *(uint4*)dst = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *(uint4*)(dst + half) = make_uint4(up[0], up[1], up[2], up[3]);
  }
  if (is_q) return;   // (uniform across the workgroup)

  const bf16_t* v = qkv + (long long)b * n * ld + (Hq + Hkv + g) * dk;
  bf16_t* vt = VT + ((long long)b * Hkv + g) * dk * cap;
  const int ck = dk >> 3;           // 16-byte chunks per head row
  const int pitch = (dk + 2) >> 1;  // LDS row pitch in dwords
  for (int c = tid; c < 64 * ck; c += 256) {
    const int tok = c / ck, ch = c - tok * ck;
    const int a = a0 + tok;
    uint4 p = make_uint4(0u, 0u, 0u, 0u);
    if (a >= row0 && a < end) p = *(const uint4*)(v + (long long)(a - row0) * ld + ch * 8);
    uint32_t* t = tile + tok * pitch + ch * 4;
    t[0] = p.x; t[1] = p.y; t[2] = p.z; t[3] = p.w;
  }
  __syncthreads();
  const bf16_t* tb = (const bf16_t*)tile;
  for (int i = tid; i < dk * 8; i += 256) {
    const int tc = i & 7, d = i >> 3;
    const int a = a0 + tc * 8;
    int j0 = max(row0 - a, 0), j1 = min(end - a, 8);   // the group's columns [j0, j1) belong to the chunk
    if (j0 >= j1) continue;
    const bf16_t* src = tb + (tc * 8) * (2 * pitch) + d;
    auto pair = [&](int j) { return (uint32_t)src[j * (2 * pitch)] | ((uint32_t)src[(j + 1) * (2 * pitch)] << 16); };
    bf16_t* dst = vt + (long long)d * cap + a;   // 16-byte aligned: cap % 64 == 0, a % 8 == 0
    if (j1 - j0 == 8) {
      *(uint4*)dst = make_uint4(pair(0), pair(2), pair(4), pair(6));
      continue;
    }
    if ((j0 & 1) && j0 < j1) { dst[j0] = src[j0 * (2 * pitch)]; ++j0; }
    if ((j1 & 1) && j0 < j1) { --j1; dst[j1] = src[j1 * (2 * pitch)]; }
    if ((j0 & 2) && j0 < j1) { *(uint32_t*)(dst + j0) = pair(j0); j0 += 2; }
    if ((j1 & 2) && j0 < j1) { j1 -= 2; *(uint32_t*)(dst + j1) = pair(j1); }
    if (j0 < j1) *(uint2*)(dst + j0) = make_uint2(pair(j0), pair(j0 + 2));   // [0, 4) or [4, 8): all eight is the store above
  }
}

// what the two entry points refuse alike: the chunk's place in the cache
int refuse_window(const char* name, int row0, int n, int cap) {
  if (row0 < 0) return x2i_set_error(X2I_ERR_SHAPE, "%s: row0=%d is negative", name, row0);
  if (n < 1) return x2i_set_error(X2I_ERR_SHAPE, "%s: n=%d rows is not a chunk (n >= 1)", name, n);
  if (cap <= 0 || cap % 64) return x2i_set_error(X2I_ERR_SHAPE, "%s: cap=%d is not a positive multiple of 64", name, cap);
  if ((long long)row0 + n > cap) return x2i_set_error(X2I_ERR_SHAPE, "%s: rows row0=%d .. row0 + n=%d - 1 do not fit cap=%d", name, row0, n, cap);
  return X2I_OK;
}

}  // namespace

extern "C" {

int x2i_qwen_extend_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                                    int32_t row0, int32_t n, int32_t cap, int32_t Hq, int32_t Hkv, int32_t dk, x2i_stream_t stream) {
  const char* name = "qwen_extend_rope_split";
  if (!qkv || !cos || !sin || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", name);
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "%s: head width dk=%d is not one of 64, 128", name, dk);
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq + Hkv > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: bad shape (B=%d Hq=%d Hkv=%d)", name, B, Hq, Hkv);
  if (const int rc = refuse_window(name, row0, n, cap)) return rc;
  if (ld < ((long long)Hq + 2LL * Hkv) * dk || ld % 8)
    return x2i_set_error(X2I_ERR_ALIGN, "%s: ld=%lld must be a multiple of 8 and >= (Hq+2*Hkv)*dk", name, (long long)ld);
  if (!al16(qkv) || !al16(cos) || !al16(sin) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: pointers must be 16-byte aligned (qkv=%p cos=%p sin=%p Q=%p K=%p VT=%p)", name, qkv, (const void*)cos,
                         (const void*)sin, Q, K, VT);
  const int tiles = (row0 + n - 1) / 64 - row0 / 64 + 1;
  hipLaunchKernelGGL(qwen_extend_rope_split_kernel, dim3(tiles, Hq + Hkv, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld,
                     cos, sin, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, row0, n, cap, Hq, Hkv, dk);
  return x2i_check_launch(name);
}

int x2i_qwen_extend_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* k_lo, void* O, int32_t B, int32_t Hq, int32_t Hkv,
                                   int32_t row0, int32_t n, int32_t cap, int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride,
                                   x2i_stream_t stream) {
  const char* name = "qwen_extend_attention";
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", name);
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "%s: head width dk=%d is not one of 64, 128", name, dk);
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: need Hq %% Hkv == 0 (B=%d Hq=%d Hkv=%d)", name, B, Hq, Hkv);
  if (const int rc = refuse_window(name, row0, n, cap)) return rc;
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "%s: scale=%g must be positive and finite", name, (double)scale);
  if ((long long)((n + 254) / 128) * Hq * B > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "%s: too many work items", name);
  if (ldo < (long long)Hq * dk || ldo % 4 || o_batch_stride % 4)
    return x2i_set_error(X2I_ERR_ALIGN, "%s: output rows must hold Hq*dk elements and be 8-byte aligned (ldo=%d o_batch_stride=%lld)", name, ldo,
                         (long long)o_batch_stride);
  if (!al16(Q) || !al16(K) || !al16(VT) || (((uintptr_t)O) & 7) || (((uintptr_t)k_lo) & 3))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: Q, K, VT must be 16-byte, O 8-byte and k_lo 4-byte aligned (Q=%p K=%p VT=%p O=%p k_lo=%p)", name, Q, K, VT, O,
                         (const void*)k_lo);
  return x2i_launch_encoder_attention_causal_ext(Q, K, VT, k_lo, O, B, Hq, Hkv, row0, n, cap, dk, scale, ldo, o_batch_stride, (hipStream_t)stream);
}

}  // extern "C"
