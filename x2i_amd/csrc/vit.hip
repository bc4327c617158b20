// The Qwen2.5-VL vision tower's kernels (include/x2i_vit.h): rotate-half RoPE with the head split in front of the attention; the
// bidirectional attention with a key range per query row for heads of 64, 80 and 128 is encoder_attention.hip's SEGMENT mode.  They stand
// behind `transformers`' Qwen2_5_VLVisionAttention / apply_rotary_pos_emb_vision.  bf16 in and out, f32 arithmetic; every launcher enqueues
// on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_vit.h"

namespace {

// RoPE + head split: rope_split_body of encoder_common.h (qwen.hip's kernel) with as many key/value heads as query heads -- [q | k | v] of
// nn.Linear(dim, 3 dim) is its column layout at Hq = Hkv = H -- and heads stored dkp wide.  dk / 2 = 40 is five groups of eight pairs.
__global__ __launch_bounds__(256) void vit_rope_split_kernel(const bf16_t* __restrict__ qkv, long long ld, const float* __restrict__ cs,
                                                             const float* __restrict__ sn, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                             bf16_t* __restrict__ VT, int S, int Spad, int H, int dk, int dkp) {
  rope_split_body(qkv, ld, cs, sn, Q, K, VT, S, Spad, H, H, dk, dkp);
}

}  // namespace

extern "C" {

int x2i_vit_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* row_lo, const int32_t* row_hi, void* O, int32_t B,
                           int32_t H, int32_t S, int32_t Spad, int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride,
                           x2i_stream_t stream) {
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "vit_attention: null pointer");
  if ((row_lo == nullptr) != (row_hi == nullptr))
    return x2i_set_error(X2I_ERR_ARG, "vit_attention: row_lo and row_hi must both be null or both be given");
  if (dk != 64 && dk != 80 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "vit_attention: head width dk=%d is not one of 64, 80, 128", dk);
  if (const int rc = x2i_encoder_attention_refuse_shape("vit_attention", B, H, S, Spad)) return rc;
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "vit_attention: scale must be positive and finite");
  if (const int rc = x2i_encoder_attention_refuse_launch("vit_attention", "H", ", row_lo and row_hi 4-byte aligned", Q, K, VT, row_lo, row_hi, O, B, H, S,
                                                         dk, ldo, o_batch_stride))
    return rc;
  return x2i_launch_encoder_attention_segment(Q, K, VT, row_lo, row_hi, O, B, H, S, Spad, dk, scale, ldo, o_batch_stride, (hipStream_t)stream);
}

int x2i_vit_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                            int32_t S, int32_t Spad, int32_t H, int32_t dk, x2i_stream_t stream) {
  if (!qkv || !cos || !sin || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "vit_rope_split: null pointer");
  if (dk != 64 && dk != 80 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "vit_rope_split: head width dk=%d is not one of 64, 80, 128", dk);
  if (B <= 0 || S <= 0 || H <= 0 || Spad < S || Spad % 8 || 2 * (long long)H > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "vit_rope_split: bad shape (B=%d S=%d Spad=%d H=%d)", B, S, Spad, H);
  if (ld < 3LL * H * dk || ld % 8 || !al16(qkv) || !al16(cos) || !al16(sin) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "vit_rope_split: ld must be a multiple of 8 and >= 3*H*dk, pointers 16-byte aligned");
  hipLaunchKernelGGL(vit_rope_split_kernel, dim3((S + 63) / 64, 2 * H, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld, cos,
                     sin, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, S, Spad, H, dk, stored_width(dk));
  return x2i_check_launch("vit_rope_split");
}

}  // extern "C"
