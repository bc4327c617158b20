/* x2i_vit.h -- extension header of libx2i_hip.so: the Qwen2.5-VL vision tower's kernels (csrc/vit.hip, csrc/encoder_attention.hip).
 *
 * The conventions are those of x2i.h, x2i_t5.h, x2i_clip.h and x2i_qwen.h (device pointers owned by the caller, raw bf16 storage,
 * `stream` a hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative
 * X2I_ERR_* code with the message in x2i_last_error(); every argument is validated before any launch).  The entry points live in an
 * extension header because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/vit_ops.py, the host module
 * x2i_amd/qwen_vision.py (Qwen2_5VisionTower).
 *
 * Both stand behind `transformers`' Qwen2_5_VLVisionAttention (models/qwen2_5_vl/modeling_qwen2_5_vl.py) inside
 * Qwen2_5_VisionTransformerPretrainedModel, the module behind `model.visual` of Qwen2.5-VL 3B / 7B.  The rest of a block runs on entry
 * points that exist: x2i_t5_rms_rows_bf16 (Qwen2_5_VLRMSNorm), x2i_gemm_bf16 (the biased projections, the residuals, the merger's GELU)
 * and x2i_qwen_swiglu_bf16.
 *
 * Heads of 80 (1280 / 16) are STORED 128 wide: with dkp = 128 for dk = 80 and dkp = dk otherwise, Q and K are rows of dkp elements and V^T
 * has dkp rows per head.  Neither entry point reads or writes the padding (columns dk..dkp-1 of Q / K, rows dk..dkp-1 of V^T) in a way
 * that reaches a result: x2i_vit_rope_split_bf16 leaves it untouched, and x2i_vit_attention_bf16's output does not depend on what it
 * holds, NaN included.
 */
#ifndef X2I_VIT_H
#define X2I_VIT_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Bidirectional flash attention with a key range per QUERY ROW: the windows and the frames of one packed sequence of patches.
 *   score[i][j] = scale * sum_{d < dk} q[i][d] k[j][d]
 *   O[b][i][h*dk + d] = sum_j softmax_j(score[i][j]) v[j][d]     over the keys j that COUNT for row i of sample b:
 *                                                                  row_lo[b][i] <= j < row_hi[b][i]
 * Q, K: bf16 [B][H][Spad][dkp]; VT: bf16 [B][H][dkp][Spad] (V transposed), the layouts of x2i_vit_rope_split_bf16's outputs.
 * row_lo, row_hi: device int32 [B][S]; both NULL means [0, S) for every row; values outside [0, S] are clamped into it.  The arrays need
 * not be monotonic in i, and a row's range need not hold the row itself: the walk over the key tiles is derived in the kernel, from
 * min(row_lo) / 64 to (max(row_hi) - 1) / 64 over each block of 128 query rows, and with the clamp no tile outside [0, Spad) is read
 * whatever the arrays hold.
 * O: bf16 token-major, row i of sample b at O + b * o_batch_stride + i * ldo (elements), head h at columns h*dk .. h*dk + dk - 1 (NOT
 * dkp); only rows < S and columns < H*dk are written, and every one of them is written.
 * The mask is by index, never by data: a key that does not count never enters the running maximum or the sum, whatever K and V^T hold
 * there; rows / columns < dk of K and V^T only need to be finite everywhere in [0, Spad), since a probability of exactly 0 multiplies V^T.
 * A row whose clamped range is empty gets O exactly 0, and it is written.
 * Arithmetic: that of x2i_qwen_attention_bf16 -- scores and the softmax (running maximum, exp2 domain, scale * log2 e folded into one
 * multiply) in f32; P rounded to bf16 for the P V product; O accumulated in f32, normalised and rounded once.
 * Needs dk in {64, 80, 128}, Spad % 64 == 0, Spad >= S, a positive finite scale, row_lo and row_hi both NULL or both given (4-byte
 * aligned), 8-byte aligned output rows (ldo, o_batch_stride % 4) with ldo >= H*dk and 16-byte aligned Q, K, VT; anything else returns an
 * error code.  Output rows that are 16-byte aligned (ldo, o_batch_stride % 8) take 16-byte stores. */
int x2i_vit_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* row_lo, const int32_t* row_hi, void* O, int32_t B,
                           int32_t H, int32_t S, int32_t Spad, int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride,
                           x2i_stream_t stream);

/* Rotate-half RoPE on q and k, and the head split, of one [q | k | v] projection: nn.Linear(dim, 3 dim) reshaped to [S, 3, H, dk] (biases
 * already added by the GEMM's epilogue).
 * qkv: bf16 rows [B*S] of 3 * H * dk elements, row stride ld.  cos, sin: f32 [B][S][dk/2], the HALF tables (the library's are the two
 * halves concatenated).  For d < dk/2, on q and on k:
 *   y[d]        = bf16( x[d] c[d] - x[d + dk/2] s[d] )
 *   y[d + dk/2] = bf16( x[d + dk/2] c[d] + x[d] s[d] )          in f32 with ONE rounding: x2i_qwen_rope_split_bf16's arithmetic, and the
 * library's (apply_rotary_pos_emb_vision computes in f32 from f32 tables and rounds once)
 * -> Q, K bf16 [B][H][Spad][dkp]; v is a plain transposition -> VT bf16 [B][H][dkp][Spad].  Only rows / columns s < S and d < dk are
 * written.
 * Needs dk in {64, 80, 128}, Spad >= S, Spad % 8 == 0, 2 H, B <= 65535, ld % 8 == 0, ld >= 3 * H * dk and 16-byte aligned pointers. */
int x2i_vit_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                            int32_t S, int32_t Spad, int32_t H, int32_t dk, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
