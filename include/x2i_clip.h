/* x2i_clip.h -- extension header of libx2i_hip.so: the CLIP text encoder's kernels (csrc/clip.hip, csrc/encoder_attention.hip).
 *
 * The conventions are those of x2i.h and x2i_t5.h (device pointers owned by the caller, raw bf16 storage, `stream` a hipStream_t
 * passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_* code with
 * the message in x2i_last_error(); every argument is validated before any launch).  The entry points live in an extension header
 * because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/clip_ops.py, the host module
 * x2i_amd/clip.py (CLIPTextModel).
 *
 * All four stand behind `transformers`' CLIPTextModel (models/clip/modeling_clip.py), the first of the two prompt encoders of the
 * reference's sampling scripts and of its distillation teacher (infer/inference_*.py get_t5_input_embeds:
 * `clip_model(ids, output_hidden_states=False).pooler_output`; train/train_qwenvl.py:665,778).  The rest of a layer runs on
 * entry points that exist: x2i_ln_affine_bf16 (the three LayerNorms), x2i_gemm_bf16 (the projections with their biases and
 * residuals) and x2i_t5_head_split_bf16 (a plain permutation: the q|k|v biases go on in the GEMM), so no fifth kernel is needed.
 */
#ifndef X2I_CLIP_H
#define X2I_CLIP_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* CLIPAttention under the text model's causal mask: flash attention over the keys j <= i.
 *   score[i][j] = scale * sum_d q[i][d] k[j][d]                                  for keys j <= i
 *   O[b][i][h*dk + d] = sum_{j <= i} softmax_j(score[i][j]) v[j][d]
 * Q, K: bf16 [B][H][Spad][dk]; VT: bf16 [B][H][dk][Spad] (V transposed), the layouts of x2i_t5_attention_bf16 and of
 * x2i_t5_head_split_bf16's outputs.  O: bf16 token-major, row i of sample b at O + b * o_batch_stride + i * ldo (elements); only
 * rows < S and columns < H*dk are written.
 * The mask is by index, not by data: a key j > i never enters the running maximum or the sum, inside the diagonal tile too, where
 * K and V^T hold real future tokens; the padding keys j >= S fall under the same rule.  (V^T beyond S must still be finite, since
 * a probability of exactly 0 multiplies it: x2i_t5_head_split_bf16 into a zeroed buffer keeps it zero.)  A query block visits only
 * the key tiles up to its diagonal.
 * Arithmetic: scores and the softmax (running maximum, exp2 domain, scale * log2 e folded into one multiply) in f32; P rounded to
 * bf16 for the P V product; O accumulated in f32, normalised and rounded once.
 * Needs dk == 64 (every CLIP text tower has 64-wide heads), Spad % 64 == 0, Spad >= S, a positive finite scale, 8-byte aligned
 * output rows (ldo, o_batch_stride % 4) with ldo >= H*dk and 16-byte aligned Q, K, VT; anything else returns an error code. */
int x2i_clip_attention_bf16(const void* Q, const void* K, const void* VT, void* O, int32_t B, int32_t H, int32_t S, int32_t Spad,
                            int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride, x2i_stream_t stream);

/* CLIPTextEmbeddings: token embedding + learned position embedding,
 *   X[b*S + s][:] = bf16( float(tok[ids[b][s]][:]) + float(pos[s][:]) )
 * ids: int64 [B][S] on the device; tok: bf16 [vocab][D]; pos: bf16 [>= S][D]; X: bf16 [B*S][D], contiguous.  An id outside
 * [0, vocab) is a contract violation that the host cannot see: the kernel clamps it into the table, so that no launch reads out
 * of bounds (what such a row then holds is unspecified).  Needs D % 8 == 0 and 16-byte aligned tok, pos, X. */
int x2i_clip_embed_bf16(const int64_t* ids, const void* tok, const void* pos, void* X, int32_t B, int32_t S, int32_t D, int32_t vocab,
                        x2i_stream_t stream);

/* hidden_act = "quick_gelu" of CLIPMLP:   y[r][c] = bf16( x[r][c] * sigmoid(1.702 x[r][c]) )   in f32 with ONE rounding.
 * X2I_ACT_* has no quick-GELU and that table is closed, so fc1 runs as x2i_gemm_bf16 with its bias and no activation, followed
 * by this launch.  X, Y: bf16 rows of F elements, row strides ldx / ldy elements (Y may be X).  Needs F % 8 == 0, ldx % 8 == 0,
 * ldy % 8 == 0 and 16-byte aligned pointers. */
int x2i_clip_quick_gelu_bf16(const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream);

/* CLIPTextModel's pooled output: the hidden state at each sample's end-of-text token,
 *   pooled[b][:] = Hs[b*S + idx_b][:]
 * with eos_token_id == 2 (the library's legacy rule, and the value in FLUX's text_encoder/config.json): idx_b = argmax_s ids[b][s],
 * ties to the first position; otherwise idx_b = the first s with ids[b][s] == eos_token_id, 0 when there is none (as
 * (ids == eos).int().argmax() gives).  One workgroup per sample; the index never reaches the host, so the forward stays capturable.
 * ids: int64 [B][S]; Hs: bf16 [B*S] rows of D elements, row stride ldh; pooled: bf16 [B] rows, row stride ldp.
 * Needs D % 8 == 0, ldh % 8 == 0, ldp % 8 == 0 and 16-byte aligned Hs, pooled. */
int x2i_clip_pool_bf16(const int64_t* ids, const void* Hs, int64_t ldh, void* pooled, int64_t ldp, int32_t B, int32_t S, int32_t D,
                       int32_t eos_token_id, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
