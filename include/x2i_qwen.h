/* x2i_qwen.h -- extension header of libx2i_hip.so: the Qwen2 decoder prefill's kernels (csrc/qwen.hip, csrc/encoder_attention.hip).
 *
 * The conventions are those of x2i.h, x2i_t5.h and x2i_clip.h (device pointers owned by the caller, raw bf16 storage, `stream` a
 * hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The entry points live in an extension
 * header because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/qwen_ops.py, the host module
 * x2i_amd/qwen.py (Qwen2DecoderStack).
 *
 * All three stand behind `transformers`' Qwen2Model / Qwen2_5_VLTextModel (models/qwen2/modeling_qwen2.py,
 * models/qwen2_5_vl/modeling_qwen2_5_vl.py), the decoder stack inside every MLLM the reference conditions on (Qwen2.5-VL 3B / 7B,
 * MiniCPM-o, InternVL2.5), run once over the prompt.  The rest of a layer runs on entry points that exist: x2i_t5_rms_rows_bf16 (which
 * is Qwen2RMSNorm) and x2i_gemm_bf16 (the projections with their biases and residuals).
 */
#ifndef X2I_QWEN_H
#define X2I_QWEN_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Qwen2Attention over a prompt: causal flash attention with grouped key/value heads and a per-sample key range.
 *   score[i][j] = scale * sum_d q[i][d] k[j][d]
 *   O[b][i][h*dk + d] = sum_j softmax_j(score[i][j]) v[j][d]     over the keys j that COUNT for row i of sample b:
 *                                                                  k_lo[b] <= j < k_hi[b]  and  j <= i
 * Q: bf16 [B][Hq][Spad][dk]; K: bf16 [B][Hkv][Spad][dk]; VT: bf16 [B][Hkv][dk][Spad] (V transposed), the layouts of
 * x2i_qwen_rope_split_bf16's outputs.  Query head h reads key/value head h / (Hq / Hkv): the library's repeat_kv.
 * k_lo, k_hi: device int32 [B], the valid keys of each sample (a left- or right-padded prompt); both NULL means [0, S) for every
 * sample; values outside [0, S] are clamped into it.  O: bf16 token-major, row i of sample b at O + b * o_batch_stride + i * ldo
 * (elements); only rows < S and columns < Hq*dk are written, and every one of them is written.
 * The mask is by index, never by data: a key that does not count never enters the running maximum or the sum, whatever K and V^T hold
 * there (real tokens or padding); they only need to be finite, since a probability of exactly 0 multiplies V^T.  A query block walks
 * only the key tiles from k_lo / 64 to min(its diagonal, (k_hi - 1) / 64).
 * Rows with no counted key -- i < k_lo[b] (the rows of left padding), or an empty range -- get O exactly 0, and it is written.  That is
 * this library's contract because the library it stands behind has none: `transformers` 5.15 returns NaN there under its eager
 * attention and an implementation-dependent finite value under sdpa.  Every other row agrees with the library under both paddings.
 * Arithmetic: scores and the softmax (running maximum, exp2 domain, scale * log2 e folded into one multiply) in f32; P rounded to
 * bf16 for the P V product; O accumulated in f32, normalised and rounded once.
 * Needs dk in {64, 128}, Hq % Hkv == 0, Spad % 64 == 0, Spad >= S, a positive finite scale, k_lo and k_hi both NULL or both given
 * (4-byte aligned), 8-byte aligned output rows (ldo, o_batch_stride % 4) with ldo >= Hq*dk and 16-byte aligned Q, K, VT; anything else
 * returns an error code. */
int x2i_qwen_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* k_lo, const int32_t* k_hi, void* O, int32_t B,
                            int32_t Hq, int32_t Hkv, int32_t S, int32_t Spad, int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride,
                            x2i_stream_t stream);

/* Rotate-half RoPE on q and k, and the head split, of one fused q|k|v projection (biases already added by the GEMM's epilogue).
 * qkv: bf16 rows [B*S] of (Hq + 2 Hkv) * dk elements, columns [q (Hq*dk) | k (Hkv*dk) | v (Hkv*dk)], row stride ld.
 * cos, sin: f32 [B][S][dk/2], the HALF tables (the library's are the two halves concatenated).  For d < dk/2, on q and on k:
 *   y[d]        = bf16( x[d] c[d] - x[d + dk/2] s[d] )
 *   y[d + dk/2] = bf16( x[d + dk/2] c[d] + x[d] s[d] )          in f32 with ONE rounding
 * -> Q bf16 [B][Hq][Spad][dk], K bf16 [B][Hkv][Spad][dk]; v is a plain transposition -> VT bf16 [B][Hkv][dk][Spad].  Only rows /
 * columns s < S are written.  The kernel knows nothing of position ids: 1-D RoPE and Qwen2.5-VL's M-RoPE differ only in the tables.
 * Needs dk in {64, 128}, Spad >= S, Spad % 8 == 0, Hq, Hkv, B <= 65535, ld % 8 == 0, ld >= (Hq + 2 Hkv) * dk and 16-byte aligned
 * pointers. */
int x2i_qwen_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                             int32_t S, int32_t Spad, int32_t Hq, int32_t Hkv, int32_t dk, x2i_stream_t stream);

/* Qwen2MLP's gate on one stacked [gate_proj; up_proj] projection:   y[r][c] = bf16( silu(a[r][c]) * b[r][c] )   in f32 with ONE
 * rounding (the library rounds silu(a) to bf16 in between).  AB: bf16 rows [a (F) | b (F)], row stride ld_in; Y: bf16 rows of F
 * elements, row stride ldy.  Needs F % 8 == 0, ld_in % 8 == 0 and >= 2F, ldy % 8 == 0 and >= F, 16-byte aligned pointers. */
int x2i_qwen_swiglu_bf16(const void* AB, int64_t ld_in, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
