// The decode-step linear with an e4m3 weight (include/x2i_qwen_decode_w8.h): decode_linear_kernel of qwen_decode.hip (decode_linear_core.h)
// reading half the bytes.  The weight is OCP e4m3fn codes with one f32 scale per output row; a lane's 16-byte load is 16 weights, so a wave's
// k-step is 1024 columns; the codes are decoded with the packed conversion (v_cvt_pk_f32_fp8, OCP on gfx950), X stays bf16 in LDS, the sum f32.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_qwen_decode_w8.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 16 bytes that are read once: do not keep them in the caches
__device__ __forceinline__ uint4 load_stream16(const uint8_t* p) {
  return __builtin_bit_cast(uint4, __builtin_nontemporal_load((const bf16x8_t*)p));
}

// 16 e4m3 codes -> f32, byte order = k order: the low half of a dword (word select 0) is its bytes 0 and 1
__device__ __forceinline__ void decode16(const uint4& p, float (&f)[16]) {
  const uint32_t d[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[i], true);
    f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
  }
}

// Y[b][n] from sum_k e4m3(W8[n][k]) X[b][k] for NB rows b.  The shape of decode_linear_dot: a wave owns R weight rows and streams them once,
// 16 bytes per lane and row, straight to registers; the loads of 8 / R k-steps are issued together before their arithmetic, so eight loads
// (128 bytes) per lane are in flight.  X is staged once per workgroup in LDS as bf16 [NB][KC] (KC = K when that fits 64 KiB, else a multiple
// of 1024 that does) and read back 32 bytes per lane.
// The arithmetic of one (row, sample): lane l sums k = 16 l + 1024 i + j, i and j ascending, in ONE fma chain (the chunking of X does not
// change it: KC % 1024 == 0), then the 64 lanes in wave_sum's tree, then the scale.  Nothing of it depends on NB or R.
// MODE 1: the wave's R rows are R / 2 gate rows n and their up rows N + n; the epilogue writes silu(a) * b.
template <int NB, int R, int MODE>
__global__ __launch_bounds__(256) void decode_linear_w8_kernel(const bf16_t* __restrict__ X, long long ldx, const uint8_t* __restrict__ W, long long ldw,
                                                               const float* __restrict__ wscale, const bf16_t* __restrict__ bias, const bf16_t* res,
                                                               long long ldr, bf16_t* Y, long long ldy, int N, int K, int KC) {
  extern __shared__ __attribute__((aligned(16))) uint4 xs[];   // [NB][KC / 8]
  constexpr int RO = MODE ? R / 2 : R;                          // outputs per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * RO;                  // (a wave past N computes clamped rows and stores nothing: it still takes the barriers)
  const uint8_t* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int n = n0 + (r < RO ? r : r - RO);                   // clamp: outputs past N are computed and discarded
    wrow[r] = W + ((long long)(n < N ? n : N - 1) + (r < RO ? 0 : N)) * ldw;
  }
  constexpr int U = 8 / R;                                      // k-steps whose loads are issued together: eight 16-byte loads per lane in flight
  constexpr int NP = NB / 2;                                    // sample pairs: one packed fma (v_pk_fma_f32) carries two samples' chains
  f32x2 acc2[R][NP > 0 ? NP : 1];
  float acc1[R];                                                // the odd last sample
#pragma unroll
  for (int r = 0; r < R; ++r) {
    acc1[r] = 0.f;
#pragma unroll
    for (int q = 0; q < NP; ++q) acc2[r][q] = f32x2{0.f, 0.f};
  }
  const int kc8 = KC >> 3;
  for (int c0 = 0; c0 < K; c0 += KC) {
    const int kc = (K - c0) < KC ? (K - c0) : KC;
    const int n8 = kc >> 3;
    if (c0) __syncthreads();                                    // every wave is done with the chunk before
    for (int i = threadIdx.x; i < NB * n8; i += 256) {
      const int b = i / n8, j = i - b * n8;
      xs[b * kc8 + j] = *(const uint4*)(X + (long long)b * ldx + c0 + j * 8);
    }
    __syncthreads();
    for (int k = lane * 16; k < kc; k += 1024 * U) {
      uint4 wv[U][R];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + 1024 * u < kc) {
#pragma unroll
          for (int r = 0; r < R; ++r) wv[u][r] = load_stream16(wrow[r] + c0 + k + 1024 * u);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k + 1024 * u;
        if (kk < kc) {
          float wf[R][16];
#pragma unroll
          for (int r = 0; r < R; ++r) decode16(wv[u][r], wf[r]);
          // explicit fma chains, k ascending: the arithmetic of one sample must not depend on how many samples share the launch (a packed
          // fma is two independent fmas)
#pragma unroll
          for (int h = 0; h < 2; ++h) {                          // the two 16-byte halves of the lane's 16 columns of X
#pragma unroll
            for (int q = 0; q < NP; ++q) {
              float xa[8], xb[8];
              unpack8(xs[(2 * q) * kc8 + (kk >> 3) + h], xa);
              unpack8(xs[(2 * q + 1) * kc8 + (kk >> 3) + h], xb);
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const f32x2 x2 = {xa[j], xb[j]};
#pragma unroll
                for (int r = 0; r < R; ++r) acc2[r][q] = __builtin_elementwise_fma(f32x2{wf[r][8 * h + j], wf[r][8 * h + j]}, x2, acc2[r][q]);
              }
            }
            if constexpr (NB & 1) {
              float xf[8];
              unpack8(xs[(NB - 1) * kc8 + (kk >> 3) + h], xf);
#pragma unroll
              for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc1[r] = __builtin_fmaf(wf[r][8 * h + j], xf[j], acc1[r]);
            }
          }
        }
      }
    }
  }
  float acc[R][NB];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int q = 0; q < NP; ++q) { acc[r][2 * q] = acc2[r][q][0]; acc[r][2 * q + 1] = acc2[r][q][1]; }
    if constexpr (NB & 1) acc[r][NB - 1] = acc1[r];
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = wave_sum(acc[r][b]);
  if (lane != 0) return;
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    const int n = n0 + r;
    if (n >= N) break;
    if constexpr (MODE) {
      const float sa = wscale[n], sb = wscale[N + n];
      const float ba = bias ? bf16_to_f32(bias[n]) : 0.f, bb = bias ? bf16_to_f32(bias[N + n]) : 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b)
        Y[(long long)b * ldy + n] =
            f32_to_bf16(__fmul_rn(silu_f(__fadd_rn(__fmul_rn(sa, acc[r][b]), ba)), __fadd_rn(__fmul_rn(sb, acc[r + RO][b]), bb)));
    } else {
      const float s = wscale[n];
      const float bv = bias ? bf16_to_f32(bias[n]) : 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float v = __fadd_rn(__fmul_rn(s, acc[r][b]), bv);
        if (res) v = __fadd_rn(v, bf16_to_f32(res[(long long)b * ldr + n]));
        Y[(long long)b * ldy + n] = f32_to_bf16(v);
      }
    }
  }
}

template <int NB, int R, int MODE>
void launch_w8(const void* X, long long ldx, const void* W, long long ldw, const float* ws, const void* bias, const void* res, long long ldr, void* Y,
               long long ldy, int N, int K, int KC, hipStream_t stream) {
  constexpr int RO = MODE ? R / 2 : R;
  const unsigned blocks = (unsigned)((N + 4 * RO - 1) / (4 * RO));
  hipLaunchKernelGGL((decode_linear_w8_kernel<NB, R, MODE>), dim3(blocks), dim3(256), (size_t)NB * KC * 2, stream, (const bf16_t*)X, ldx,
                     (const uint8_t*)W, ldw, ws, (const bf16_t*)bias, (const bf16_t*)res, ldr, (bf16_t*)Y, ldy, N, K, KC);
}

template <int NB>
void launch_w8_nb(bool wide, int mode, const void* X, long long ldx, const void* W, long long ldw, const float* ws, const void* bias, const void* res,
                  long long ldr, void* Y, long long ldy, int N, int K, int KC, hipStream_t stream) {
  if (mode) {
    if (wide) launch_w8<NB, 4, 1>(X, ldx, W, ldw, ws, bias, res, ldr, Y, ldy, N, K, KC, stream);
    else launch_w8<NB, 2, 1>(X, ldx, W, ldw, ws, bias, res, ldr, Y, ldy, N, K, KC, stream);
  } else {
    if (wide) launch_w8<NB, 4, 0>(X, ldx, W, ldw, ws, bias, res, ldr, Y, ldy, N, K, KC, stream);
    else launch_w8<NB, 2, 0>(X, ldx, W, ldw, ws, bias, res, ldr, Y, ldy, N, K, KC, stream);
  }
}

}  // namespace

extern "C" {

int x2i_qwen_decode_linear_w8_bf16(const void* X, int64_t ldx, const void* W8, int64_t ldw, const float* w_scale, const void* bias,
                                   const void* res, int64_t ldr, void* Y, int64_t ldy, int32_t B, int32_t N, int32_t K, int32_t mode,
                                   x2i_stream_t stream) {
  if (!X || !W8 || !Y) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear_w8: null pointer");
  if (!w_scale) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear_w8: the row scales w_scale are required (null pointer)");
  if (B < 1 || B > 8) return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_linear_w8: B=%d is not in 1..8", B);
  if (mode != 0 && mode != 1) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear_w8: mode=%d is not 0 or 1", mode);
  if (mode == 1 && res) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear_w8: the gate (mode 1) takes no residual");
  if (N <= 0 || K <= 0 || K % 16 || N > (1 << 29))
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_linear_w8: K=%d must be a positive multiple of 16 (N=%d)", K, N);
  if (ldx < K || ldw < K || ldx % 8 || ldw % 16 || ldy < N || (res && ldr < N) || !al16(X) || !al16(W8) || (((uintptr_t)w_scale) & 3) ||
      (((uintptr_t)Y) & 1) || (((uintptr_t)res) & 1) || (((uintptr_t)bias) & 1))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "qwen_decode_linear_w8: ldx must be a multiple of 8 and ldw (bytes) of 16, both >= K, ldy (ldr) >= N, X and W8 16-byte "
                         "aligned, w_scale 4-byte aligned");
  // X in LDS: all of K when B * K bf16 fit 64 KiB, else chunks of a multiple of 1024 columns (the lanes' k sequences do not change)
  int KC = K;
  if ((long long)B * K * 2 > 65536) KC = (32768 / B) & ~1023;
  // rows per wave: four where that still gives every CU two workgroups, else two
  const long long rows = mode ? 2LL * N : N;
  const bool wide = rows >= 32LL * x2i_num_cus();
  const hipStream_t st = (hipStream_t)stream;
#define DL_CASE(NB) \
  case NB: launch_w8_nb<NB>(wide, mode, X, ldx, W8, ldw, w_scale, bias, res, ldr, Y, ldy, N, K, KC, st); break;
  switch (B) { DL_CASE(1) DL_CASE(2) DL_CASE(3) DL_CASE(4) DL_CASE(5) DL_CASE(6) DL_CASE(7) DL_CASE(8) }
#undef DL_CASE
  return x2i_check_launch("qwen_decode_linear_w8");
}

}  // extern "C"
