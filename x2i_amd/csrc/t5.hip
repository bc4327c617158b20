// The T5 encoder's kernels (include/x2i_t5.h): the head split in front of the relative-position-bias attention, T5LayerNorm (an RMS norm
// over the model width) and the gate of the gated-GELU feed-forward; the attention itself is encoder_attention.hip's RELBIAS mode.  They
// stand behind `transformers`' T5Attention / T5LayerNorm / T5DenseGatedActDense as the reference uses them (model_internvl/proj.py:153-159,167
// and train/train_qwenvl.py:666,778).  bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_t5.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- head split
// head_split_body (encoder_common.h) with the heads stored at their own width
__global__ __launch_bounds__(256) void t5_head_split_kernel(const bf16_t* __restrict__ qkv, long long ld, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                            bf16_t* __restrict__ VT, int S, int Spad, int H, int dk) {
  head_split_body(qkv, ld, Q, K, VT, S, Spad, H, dk, dk);
}

// ------------------------------------------------------------------------------------------------------------------- T5LayerNorm
// A wave per row, four rows per workgroup; a lane keeps up to RMS_REG 16-byte chunks of its row in registers (D <= 4096) and re-reads the rest.
constexpr int RMS_REG = 8;
__global__ __launch_bounds__(256) void t5_rms_rows_kernel(const bf16_t* __restrict__ X, long long ldx, bf16_t* __restrict__ Y, long long ldy,
                                                          const bf16_t* __restrict__ W, long long rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* x = X + row * ldx;
  bf16_t* y = Y + row * ldy;
  const int nc = D >> 3;
  uint4 buf[RMS_REG];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < RMS_REG; ++k) {
    const int c = lane + k * 64;
    buf[k] = make_uint4(0u, 0u, 0u, 0u);
    if (c < nc) buf[k] = *(const uint4*)(x + c * 8);
    float v[8];
    unpack8(buf[k], v);
    ss += sumsq8(v);
  }
  for (int c = lane + RMS_REG * 64; c < nc; c += 64) {
    float v[8];
    unpack8(*(const uint4*)(x + c * 8), v);
    ss += sumsq8(v);
  }
  const float r = rsqrtf(__fadd_rn(wave_sum(ss) / (float)D, eps));
  auto emit = [&](int c, const uint4& px) {
    float v[8], w[8];
    unpack8(px, v);
    unpack8(*(const uint4*)(W + c * 8), w);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // one rounding: the normalised value stays f32 until the weight has multiplied it (the library rounds it to bf16 in between)
      o[j >> 1] = pack_bf16x2(__fmul_rn(w[j], __fmul_rn(v[j], r)), __fmul_rn(w[j + 1], __fmul_rn(v[j + 1], r)));
    }
    *(uint4*)(y + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  };
#pragma unroll
  for (int k = 0; k < RMS_REG; ++k) {
    const int c = lane + k * 64;
    if (c < nc) emit(c, buf[k]);
  }
  for (int c = lane + RMS_REG * 64; c < nc; c += 64) emit(c, *(const uint4*)(x + c * 8));
}

}  // namespace

extern "C" {

int x2i_t5_attention_bf16(const void* Q, const void* K, const void* VT, const float* bias_tab, void* O, int32_t B, int32_t H, int32_t S,
                          int32_t Spad, int32_t dk, int32_t R, int32_t ldo, int64_t o_batch_stride, x2i_stream_t stream) {
  if (!Q || !K || !VT || !bias_tab || !O) return x2i_set_error(X2I_ERR_ARG, "t5_attention: null pointer");
  if (dk != 32 && dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "t5_attention: head width dk=%d is not one of 32, 64, 128", dk);
  if (const int rc = x2i_encoder_attention_refuse_shape("t5_attention", B, H, S, Spad)) return rc;
  if (R < 0 || R > RELBIAS_RMAX) return x2i_set_error(X2I_ERR_SHAPE, "t5_attention: clamp distance R=%d outside 0..%d", R, RELBIAS_RMAX);
  if (const int rc = x2i_encoder_attention_refuse_launch("t5_attention", "H", "", Q, K, VT, nullptr, nullptr, O, B, H, S, dk, ldo, o_batch_stride)) return rc;
  return x2i_launch_encoder_attention_relbias(Q, K, VT, bias_tab, O, B, H, S, Spad, dk, R, ldo, o_batch_stride, (hipStream_t)stream);
}

int x2i_t5_head_split_bf16(const void* qkv, int64_t ld, void* Q, void* K, void* VT, int32_t B, int32_t S, int32_t Spad, int32_t H, int32_t dk,
                           x2i_stream_t stream) {
  if (!qkv || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "t5_head_split: null pointer");
  if (dk != 32 && dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "t5_head_split: head width dk=%d is not one of 32, 64, 128", dk);
  if (B <= 0 || S <= 0 || H <= 0 || Spad < S || Spad % 8 || H > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "t5_head_split: bad shape (B=%d S=%d Spad=%d H=%d)", B, S, Spad, H);
  if (ld < 3LL * H * dk || ld % 8 || !al16(qkv) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_head_split: ld must be a multiple of 8 and >= 3*H*dk, pointers 16-byte aligned");
  hipLaunchKernelGGL(t5_head_split_kernel, dim3((S + 63) / 64, H, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld,
                     (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, S, Spad, H, dk);
  return x2i_check_launch("t5_head_split");
}

int x2i_t5_rms_rows_bf16(const void* X, int64_t ldx, void* Y, int64_t ldy, const void* weight, int64_t rows, int32_t D, float eps,
                         x2i_stream_t stream) {
  if (!X || !Y || !weight) return x2i_set_error(X2I_ERR_ARG, "t5_rms_rows: null pointer");
  if (rows <= 0 || D <= 0 || D % 8 || (rows + 3) / 4 > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "t5_rms_rows: D=%d must be a positive multiple of 8", D);
  if (ldx < D || ldy < D || ldx % 8 || ldy % 8 || !al16(X) || !al16(Y) || !al16(weight))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_rms_rows: row strides must be multiples of 8 and >= D, pointers 16-byte aligned");
  hipLaunchKernelGGL(t5_rms_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, (long long)ldx,
                     (bf16_t*)Y, (long long)ldy, (const bf16_t*)weight, (long long)rows, D, eps);
  return x2i_check_launch("t5_rms_rows");
}

int x2i_t5_gated_gelu_bf16(const void* AB, int64_t ld_in, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream) {
  if (!AB || !Y) return x2i_set_error(X2I_ERR_ARG, "t5_gated_gelu: null pointer");
  if (rows <= 0 || F <= 0 || F % 8) return x2i_set_error(X2I_ERR_SHAPE, "t5_gated_gelu: F=%d must be a positive multiple of 8", F);
  if (ld_in < 2LL * F || ldy < F || ld_in % 8 || ldy % 8 || !al16(AB) || !al16(Y))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_gated_gelu: row strides must be multiples of 8 (ld_in >= 2F, ldy >= F), pointers 16-byte aligned");
  return launch_row_act<GeluTanhAct, true>("t5_gated_gelu", AB, ld_in, Y, ldy, rows, F, (hipStream_t)stream);
}

}  // extern "C"
