/* x2i_t5.h -- extension header of libx2i_hip.so: the T5 encoder's kernels (csrc/t5.hip, csrc/encoder_attention.hip).
 *
 * The conventions are those of x2i.h (device pointers owned by the caller, raw bf16 storage, `stream` a hipStream_t passed as
 * void*, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_* code with the message in
 * x2i_last_error()).  The entry points live in an extension header because x2i.h's table of exports is closed under ABI
 * version 5; the binding is x2i_amd/t5_ops.py, the host modules x2i_amd/t5.py (T5Stack, T5EncoderModel).
 *
 * All four stand behind the encoder of `transformers`' T5 (models/t5/modeling_t5.py), which the reference uses in two places:
 * the T5Stack of the legacy projector heads (model_internvl/proj.py:153-159,167) and the distillation teacher's prompt encoder
 * T5EncoderModel `text_encoder_2` (train/train_qwenvl.py:666,778).
 */
#ifndef X2I_T5_H
#define X2I_T5_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* T5Attention (encoder self-attention, no mask): flash attention with a learned additive relative-position bias and NO
 * softmax scale.
 *   score[i][j] = sum_d q[i][d] k[j][d] + bias_tab[h][clamp(j - i, -R, R) + R]        for keys j < S
 *   O[b][i][h*dk + d] = sum_j softmax_j(score[i][j]) v[j][d]
 * Q, K: bf16 [B][H][Spad][dk]; VT: bf16 [B][H][dk][Spad] (V transposed; its columns >= S must be zero -- the caller's
 * contract, x2i_t5_head_split_bf16 into a zeroed buffer keeps it); bias_tab: f32 [H][2R+1], the bias of key offset r = j - i
 * at index r + R.  T5's bucket function saturates at relative_attention_max_distance, so with R >= that distance the table
 * read by the clamped offset IS T5Attention.compute_bias, for any S.  Keys j >= S are masked by index (a zero K row would
 * still score 0 + bias).  O: bf16 token-major, row i of sample b at O + b * o_batch_stride + i * ldo (elements), as
 * x2i_attention_bf16 addresses it; only rows < S and columns < H*dk are written.
 * Arithmetic: scores, the bias add and the softmax (running maximum, exp2 domain) in f32; P rounded to bf16 for the P V
 * product; O accumulated in f32, normalised and rounded once.
 * Needs dk in {32, 64, 128}, Spad % 64 == 0, Spad >= S, 0 <= R <= 2047, 8-byte aligned output rows (ldo, o_batch_stride % 4);
 * anything else returns an error code. */
int x2i_t5_attention_bf16(const void* Q, const void* K, const void* VT, const float* bias_tab, void* O, int32_t B, int32_t H,
                          int32_t S, int32_t Spad, int32_t dk, int32_t R, int32_t ldo, int64_t o_batch_stride,
                          x2i_stream_t stream);

/* The head split in front of T5Attention's score product (its q / k / v `.view(B, S, H, dk).transpose(1, 2)`), from the rows
 * of ONE GEMM over the stacked q|k|v weight:
 *   qkv: bf16 [B*S][3*H*dk] (row stride ld elements), columns [q (H*dk) | k (H*dk) | v (H*dk)]
 *   Q[b][h][s][d] = q, K[b][h][s][d] = k   (bf16 [B][H][Spad][dk]),   VT[b][h][d][s] = v   (bf16 [B][H][dk][Spad])
 * A plain permutation: no norm, no rotary embedding, bit-exact.  Only rows (Q, K) and columns (VT) s < S are written.
 * Needs dk in {32, 64, 128}, Spad >= S, ld % 8 == 0, Spad % 8 == 0 and 16-byte aligned pointers. */
int x2i_t5_head_split_bf16(const void* qkv, int64_t ld, void* Q, void* K, void* VT, int32_t B, int32_t S, int32_t Spad,
                           int32_t H, int32_t dk, x2i_stream_t stream);

/* T5LayerNorm (an RMS norm over the model width: no mean subtraction, no bias) on bf16 weights:
 *   y[r][c] = bf16( w[c] * ( x[r][c] * rsqrt( mean_c(x[r][c]^2) + eps ) ) )
 * with the mean, the reciprocal square root and both products in f32 and ONE rounding, of the result.  (The library casts the
 * normalised row to the weight's dtype before the weight multiplies it: two roundings, up to 2^-7 relative; this is within
 * 2^-8 of the exact value, tests/t5_ref.py.)  X, Y: bf16 rows of D elements, row strides
 * ldx / ldy elements; weight: bf16 [D].  Needs D % 8 == 0, ldx % 8 == 0, ldy % 8 == 0 and 16-byte aligned pointers. */
int x2i_t5_rms_rows_bf16(const void* X, int64_t ldx, void* Y, int64_t ldy, const void* weight, int64_t rows, int32_t D,
                         float eps, x2i_stream_t stream);

/* The gate of T5DenseGatedActDense (feed_forward_proj = "gated-gelu", dense_act_fn = "gelu_new") on the rows of ONE GEMM over
 * the stacked [wi_0; wi_1] weight:
 *   AB: bf16 [rows][a (F) | b (F)] (row stride ld_in elements),   y[r][c] = bf16( gelu_tanh(a[r][c]) * b[r][c] )
 * in f32 with ONE rounding, of the product (the library rounds the activation to bf16 before the gate multiplies it).
 * gelu_tanh is the tanh form 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) as the GEMM epilogues evaluate it (X2I_ACT_GELU_TANH_).
 * Y: bf16 [rows][F], row stride ldy.  Needs F % 8 == 0, ld_in % 8 == 0, ldy % 8 == 0 and 16-byte aligned pointers. */
int x2i_t5_gated_gelu_bf16(const void* AB, int64_t ld_in, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
