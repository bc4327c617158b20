// The streaming dot products of an nn.Linear at 1..8 rows: the body of decode_linear_kernel (qwen_decode.hip) as a device function, which
// the vocabulary head (qwen_head.hip) calls.  Both promise that the bits of sum_k W[n][k] X[b][k] depend on row n of W and row b of X alone,
// and a logit of the head is bit for bit decode_linear's mode-0 sum (tests/test_qwen_head_gpu.py compares them).  qwen_decode.hip still
// carries its own copy of this body; it is to call this one ("Token selection").
#pragma once
#include "encoder_common.h"
#include "x2i_kernels.h"

// 16 bytes that are read once: do not keep them in the caches
__device__ __forceinline__ uint4 load_stream16(const bf16_t* p) {
  return __builtin_bit_cast(uint4, __builtin_nontemporal_load((const bf16x8_t*)p));
}

// X in LDS: all of K when B * K bf16 fit 64 KiB less `reserve` bytes of the kernel's own static LDS, else chunks of a multiple of 512 columns
// (the lanes' k sequences do not change)
inline int decode_linear_kc(int B, int K, int reserve = 0) {
  return ((long long)B * K * 2 > 65536 - reserve) ? (((32768 - reserve / 2) / B) & ~511) : K;
}

// acc[r][b] = sum_k wrow[r][k] X[b][k] for NB rows b, the same value in every lane.  Called by all 256 threads of a workgroup (it takes
// barriers).  A wave owns R weight rows and streams them once, 16 bytes per lane and row, straight to registers (the weight is read once and
// shared with nobody: an LDS round trip would be overhead); the loads of 8 / R k-steps are issued together before their arithmetic, so eight
// loads (128 bytes) per lane are in flight.  X is staged once per workgroup in LDS as bf16 [NB][KC] (KC = decode_linear_kc(NB, K)) and read
// back 16 bytes per lane, conflict-free.
// The arithmetic of one (row, sample): lane l sums k = 8 l + 512 i + j, i and j ascending, in ONE fma chain (the chunking of X does not
// change it: KC % 512 == 0), then the 64 lanes in wave_sum's tree.  Nothing of it depends on NB or R.
template <int NB, int R>
__device__ __forceinline__ void decode_linear_dot(const bf16_t* __restrict__ X, long long ldx, const bf16_t* (&wrow)[R], int K, int KC,
                                                  uint4* xs, float (&acc)[R][NB]) {
  const int lane = threadIdx.x & 63;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
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
    for (int k = lane * 8; k < kc; k += 512 * U) {
      uint4 wv[U][R];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + 512 * u < kc) {
#pragma unroll
          for (int r = 0; r < R; ++r) wv[u][r] = load_stream16(wrow[r] + c0 + k + 512 * u);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k + 512 * u;
        if (kk < kc) {
          float wf[R][8];
#pragma unroll
          for (int r = 0; r < R; ++r) unpack8(wv[u][r], wf[r]);
          // explicit fma chains, k ascending: the arithmetic of one sample must not depend on how many samples share the launch (a packed
          // fma is two independent fmas)
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            float xa[8], xb[8];
            unpack8(xs[(2 * q) * kc8 + (kk >> 3)], xa);
            unpack8(xs[(2 * q + 1) * kc8 + (kk >> 3)], xb);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const f32x2 x2 = {xa[j], xb[j]};
#pragma unroll
              for (int r = 0; r < R; ++r) acc2[r][q] = __builtin_elementwise_fma(f32x2{wf[r][j], wf[r][j]}, x2, acc2[r][q]);
            }
          }
          if constexpr (NB & 1) {
            float xf[8];
            unpack8(xs[(NB - 1) * kc8 + (kk >> 3)], xf);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
              for (int j = 0; j < 8; ++j) acc1[r] = __builtin_fmaf(wf[r][j], xf[j], acc1[r]);
          }
        }
      }
    }
  }
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
}
