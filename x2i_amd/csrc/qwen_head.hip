// Token selection of greedy Qwen2 decoding (include/x2i_qwen_head.h): the last hidden state of 1..8 samples to their next tokens.
//   logits_argmax   the vocabulary projection (decode_linear's streaming dot products), the repetition penalty, optional f32 scores,
//                   and per workgroup the largest penalised logit with its lowest row index
//   select          one workgroup per sample: the partials in ascending order, then the end-token bookkeeping of a generation loop
// They stand behind `lm_head`, RepetitionPenaltyLogitsProcessor, argmax and the torch ops of handoff.HipGenerate's step loop.  Two
// launches and no grid-wide wait: a partial slot is written by one workgroup of the first launch and read by the second.  Every word of
// state comes from device memory: a captured step replays.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "decode_linear_core.h"
#include "qwen_head_book.h"
#include "../../include/x2i_qwen_head.h"

#include <cmath>

namespace {

constexpr int ROWS = X2I_QWEN_HEAD_ROWS;
using head_book::HDR;
using head_book::NO_STEP;
static_assert(ROWS == 16, "four waves of four rows");

// Workgroup g owns the rows [16 g, 16 g + 16), wave w four of them.  Lane 0 of a wave holds the wave's R * NB sums and does its epilogue; the
// four waves' bests meet in LDS and threads < NB write the workgroup's partials.
template <int NB>
__global__ __launch_bounds__(256) void head_logits_kernel(const bf16_t* __restrict__ X, long long ldx, const bf16_t* __restrict__ W, long long ldw,
                                                          const uint8_t* __restrict__ seen, long long ld_seen, float penalty, float* logits,
                                                          long long ldl, const int32_t* __restrict__ step, float* ws, int V, int K, int KC) {
  extern __shared__ __attribute__((aligned(16))) uint4 xs[];   // [NB][KC / 8]
  __shared__ float best_v[4][NB];
  __shared__ int best_i[4][NB];
  constexpr int R = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * R;                   // (a wave past V computes clamped rows and offers nothing: it still takes the barriers)
  const bf16_t* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wrow[r] = W + (long long)(n0 + r < V ? n0 + r : V - 1) * ldw;
  float acc[R][NB];
  decode_linear_dot<NB, R>(X, ldx, wrow, K, KC, xs, acc);
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float bv = -INFINITY;
      int bi = n0 < V ? n0 : V - 1;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = n0 + r;
        if (n < V) {
          float v = acc[r][b];
          if (seen && seen[(long long)b * ld_seen + n]) v = v < 0.f ? __fmul_rn(v, penalty) : __fdiv_rn(v, penalty);
          if (logits) logits[(long long)b * ldl + n] = v;
          if (v > bv) { bv = v; bi = n; }                       // strictly greater: the lowest row wins among equals, a NaN never
        }
      }
      best_v[wave][b] = bv;
      best_i[wave][b] = bi;
    }
  }
  __syncthreads();
  if (threadIdx.x < NB) {
    const int b = threadIdx.x;
    float bv = best_v[0][b];
    int bi = best_i[0][b];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (best_v[w][b] > bv) { bv = best_v[w][b]; bi = best_i[w][b]; }
    float2* part = (float2*)(ws + HDR) + (long long)b * gridDim.x + blockIdx.x;
    *part = float2{bv, __int_as_float(bi)};
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ws[0] = __int_as_float(step ? *step : NO_STEP);
}

// grid B, 256 threads.  Thread t reduces the contiguous partials [t * per, (t + 1) * per) in ascending order; the tree joins NEIGHBOURING runs of threads and
// lets the upper run win only when strictly greater, so the whole reduction is the ascending one.  Thread 0 does the bookkeeping.
__global__ __launch_bounds__(256) void head_select_kernel(const float* __restrict__ ws, int nwg, int V, int32_t* step, long long* token,
                                                          long long* sequences, long long ld_seq, int ncols, long long* lengths, uint8_t* done,
                                                          const long long* __restrict__ eos, int n_eos, long long pad, uint8_t* seen,
                                                          long long ld_seen) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float2* part = (const float2*)(ws + HDR) + (long long)b * nwg;
  const int per = (nwg + 255) / 256;
  const int g0 = tid * per, g1 = g0 + per < nwg ? g0 + per : nwg;
  float bv = -INFINITY;
  int bi = 0;
  for (int g = g0; g < g1; ++g) {
    const float2 p = part[g];
    if (p.x > bv) { bv = p.x; bi = __float_as_int(p.y); }
  }
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {                           // slot tid holds the threads [tid, tid + s), its neighbour the s after them
    if ((tid & (2 * s - 1)) == 0 && sv[tid + s] > sv[tid]) { sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; }
    __syncthreads();
  }
  if (tid != 0) return;
  head_book::generated_token(b, si[0], __float_as_int(ws[0]), V, step, token, sequences, ld_seq, ncols, lengths, done, eos, n_eos, pad, seen, ld_seen);
}

template <int NB>
void launch_head_logits(const void* X, long long ldx, const void* W, long long ldw, const uint8_t* seen, long long ld_seen, float penalty,
                        float* logits, long long ldl, const int32_t* step, float* ws, int V, int K, int KC, hipStream_t stream) {
  const unsigned blocks = (unsigned)((V + ROWS - 1) / ROWS);
  hipLaunchKernelGGL((head_logits_kernel<NB>), dim3(blocks), dim3(256), (size_t)NB * KC * 2, stream, (const bf16_t*)X, ldx, (const bf16_t*)W, ldw, seen,
                     ld_seen, penalty, logits, ldl, step, ws, V, K, KC);
}

}  // namespace

extern "C" {

int x2i_qwen_head_logits_argmax_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const uint8_t* seen, int64_t ld_seen, float penalty,
                                     float* logits, int64_t ldl, const int32_t* step, float* ws, int64_t ws_floats, int32_t B, int32_t V, int32_t K,
                                     x2i_stream_t stream) {
  if (!X || !W || !ws) return x2i_set_error(X2I_ERR_ARG, "qwen_head_logits_argmax: null pointer");
  if (B < 1 || B > 8) return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_logits_argmax: B=%d is not in 1..8", B);
  if (V <= 0 || K <= 0 || K % 8 || V > (1 << 29))
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_logits_argmax: K=%d must be a positive multiple of 8 (V=%d)", K, V);
  if (!(penalty > 0.f) || !std::isfinite(penalty))
    return x2i_set_error(X2I_ERR_ARG, "qwen_head_logits_argmax: the penalty must be positive and finite");
  if (ldx < K || ldw < K || ldx % 8 || ldw % 8 || (seen && ld_seen < V) || (logits && ldl < V) || !al16(X) || !al16(W) || !al16(ws) ||
      (((uintptr_t)logits) & 3) || (((uintptr_t)step) & 3))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "qwen_head_logits_argmax: ldx and ldw must be multiples of 8 and >= K, ld_seen and ldl >= V, X, W and ws 16-byte aligned, "
                         "logits and step 4-byte aligned");
  const int64_t need = X2I_QWEN_HEAD_WS_FLOATS(B, V);
  if (ws_floats < need)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_logits_argmax: workspace too small (%lld f32 given, %lld needed)", (long long)ws_floats,
                         (long long)need);
  const int KC = decode_linear_kc(B, K, 512);   // (best_v, best_i: 256 bytes of static LDS beside X)
  const hipStream_t st = (hipStream_t)stream;
#define HL_CASE(NB) \
  case NB: launch_head_logits<NB>(X, ldx, W, ldw, seen, ld_seen, penalty, logits, ldl, step, ws, V, K, KC, st); break;
  switch (B) { HL_CASE(1) HL_CASE(2) HL_CASE(3) HL_CASE(4) HL_CASE(5) HL_CASE(6) HL_CASE(7) HL_CASE(8) }
#undef HL_CASE
  return x2i_check_launch("qwen_head_logits_argmax");
}

int x2i_qwen_head_select(const float* ws, int64_t ws_floats, int32_t* step, int64_t* token, int64_t* sequences, int64_t ld_seq, int32_t ncols,
                         int64_t* lengths, uint8_t* done, const int64_t* eos, int32_t n_eos, int64_t pad, uint8_t* seen, int64_t ld_seen, int32_t B,
                         int32_t V, x2i_stream_t stream) {
  if (!ws || !step || !token || !sequences || !lengths || !done) return x2i_set_error(X2I_ERR_ARG, "qwen_head_select: null pointer");
  if (B < 1 || B > 8) return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_select: B=%d is not in 1..8", B);
  if (V <= 0 || V > (1 << 29)) return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_select: V=%d is not positive", V);
  if (n_eos < 0 || n_eos > 8) return x2i_set_error(X2I_ERR_ARG, "qwen_head_select: n_eos=%d is not in 0..8", n_eos);
  if (n_eos > 0 && !eos) return x2i_set_error(X2I_ERR_ARG, "qwen_head_select: null pointer (eos with n_eos=%d)", n_eos);
  if (pad < 0 || pad >= V) return x2i_set_error(X2I_ERR_ARG, "qwen_head_select: pad=%lld is not a token of the vocabulary [0, %d)", (long long)pad, V);
  if (ncols < 0 || ld_seq < ncols || (seen && ld_seen < V))
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_select: need ncols >= 0, ld_seq >= ncols and ld_seen >= V (ncols=%d)", ncols);
  if (!al16(ws) || (((uintptr_t)step) & 3) || (((uintptr_t)token) & 7) || (((uintptr_t)sequences) & 7) || (((uintptr_t)lengths) & 7) ||
      (((uintptr_t)eos) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_head_select: ws must be 16-byte, token, sequences, lengths and eos 8-byte, step 4-byte aligned");
  const int64_t need = X2I_QWEN_HEAD_WS_FLOATS(B, V);
  if (ws_floats < need)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_head_select: workspace too small (%lld f32 given, %lld needed)", (long long)ws_floats, (long long)need);
  const int nwg = (V + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(head_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ws, nwg, V, step, (long long*)token, (long long*)sequences,
                     (long long)ld_seq, ncols, (long long*)lengths, done, (const long long*)eos, n_eos, (long long)pad, seen, (long long)ld_seen);
  return x2i_check_launch("qwen_head_select");
}

}  // extern "C"
