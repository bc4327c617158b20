// The Qwen2 decoder prefill's kernels (include/x2i_qwen.h): rotate-half RoPE with the head split in front of the attention, and the SwiGLU
// gate; the causal attention with grouped key/value heads and a per-sample key range for 64- and 128-wide heads is
// encoder_attention.hip's CAUSAL mode.  They stand behind `transformers`' Qwen2Attention / apply_rotary_pos_emb
// (apply_multimodal_rotary_pos_emb) / Qwen2MLP as the MLLMs of the reference's sampling scripts run them over a prompt
// (infer/inference_*.py).  bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_qwen.h"

namespace {

// RoPE + head split: rope_split_body of encoder_common.h, which the vision tower's kernel shares; heads are stored at their own width here
__global__ __launch_bounds__(256) void qwen_rope_split_kernel(const bf16_t* __restrict__ qkv, long long ld, const float* __restrict__ cs,
                                                              const float* __restrict__ sn, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                              bf16_t* __restrict__ VT, int S, int Spad, int Hq, int Hkv, int dk) {
  rope_split_body(qkv, ld, cs, sn, Q, K, VT, S, Spad, Hq, Hkv, dk, dk);
}

}  // namespace

extern "C" {

int x2i_qwen_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* k_lo, const int32_t* k_hi, void* O, int32_t B,
                            int32_t Hq, int32_t Hkv, int32_t S, int32_t Spad, int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride,
                            x2i_stream_t stream) {
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "qwen_attention: null pointer");
  if ((k_lo == nullptr) != (k_hi == nullptr))
    return x2i_set_error(X2I_ERR_ARG, "qwen_attention: k_lo and k_hi must both be null or both be given");
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "qwen_attention: head width dk=%d is not one of 64, 128", dk);
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_attention: need Hq %% Hkv == 0 (B=%d Hq=%d Hkv=%d)", B, Hq, Hkv);
  if (const int rc = x2i_encoder_attention_refuse_shape("qwen_attention", B, Hq, S, Spad)) return rc;
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "qwen_attention: scale must be positive and finite");
  if (const int rc = x2i_encoder_attention_refuse_launch("qwen_attention", "Hq", ", k_lo and k_hi 4-byte aligned", Q, K, VT, k_lo, k_hi, O, B, Hq, S, dk,
                                                         ldo, o_batch_stride))
    return rc;
  return x2i_launch_encoder_attention_causal(Q, K, VT, k_lo, k_hi, O, B, Hq, Hkv, S, Spad, dk, scale, ldo, o_batch_stride,
                                             (hipStream_t)stream);
}

int x2i_qwen_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                             int32_t S, int32_t Spad, int32_t Hq, int32_t Hkv, int32_t dk, x2i_stream_t stream) {
  if (!qkv || !cos || !sin || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "qwen_rope_split: null pointer");
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "qwen_rope_split: head width dk=%d is not one of 64, 128", dk);
  if (B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || Spad < S || Spad % 8 || Hq + Hkv > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_rope_split: bad shape (B=%d S=%d Spad=%d Hq=%d Hkv=%d)", B, S, Spad, Hq, Hkv);
  if (ld < ((long long)Hq + 2LL * Hkv) * dk || ld % 8 || !al16(qkv) || !al16(cos) || !al16(sin) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_rope_split: ld must be a multiple of 8 and >= (Hq+2*Hkv)*dk, pointers 16-byte aligned");
  hipLaunchKernelGGL(qwen_rope_split_kernel, dim3((S + 63) / 64, Hq + Hkv, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld,
                     cos, sin, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, S, Spad, Hq, Hkv, dk);
  return x2i_check_launch("qwen_rope_split");
}

int x2i_qwen_swiglu_bf16(const void* AB, int64_t ld_in, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream) {
  if (!AB || !Y) return x2i_set_error(X2I_ERR_ARG, "qwen_swiglu: null pointer");
  if (rows <= 0 || F <= 0 || F % 8) return x2i_set_error(X2I_ERR_SHAPE, "qwen_swiglu: F=%d must be a positive multiple of 8", F);
  if (ld_in < 2LL * F || ldy < F || ld_in % 8 || ldy % 8 || !al16(AB) || !al16(Y))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_swiglu: row strides must be multiples of 8 (ld_in >= 2F, ldy >= F), pointers 16-byte aligned");
  return launch_row_act<SiluAct, true>("qwen_swiglu", AB, ld_in, Y, ldy, rows, F, (hipStream_t)stream);
}

}  // extern "C"
