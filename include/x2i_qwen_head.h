/* x2i_qwen_head.h -- extension header of libx2i_hip.so: token selection of greedy Qwen2 decoding (csrc/qwen_head.hip).
 *
 * The conventions are those of x2i.h and the other extension headers (device pointers owned by the caller, raw bf16 storage, `stream` a
 * hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The binding is
 * x2i_amd/qwen_head_ops.py, the host module x2i_amd/handoff.py (HipGenerate with hip_head=True).
 *
 * The two entry points turn the last hidden state of 1..8 samples into their next tokens: the vocabulary projection (`lm_head`) with
 * `transformers`' RepetitionPenaltyLogitsProcessor and a per-workgroup argmax in one launch, the reduction of those partials with the
 * end-token bookkeeping of a generation loop in a second.  No [B, V] array is written unless the caller asks for the scores.  Every
 * word of state that changes from token to token lives in DEVICE memory, so the pair can be captured in a graph once and replayed.
 * No workgroup waits on another: there is no spin, no arrival counter and no atomic; each partial slot is written by exactly one
 * workgroup of the first launch and read by the second.
 */
#ifndef X2I_QWEN_HEAD_H
#define X2I_QWEN_HEAD_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Vocabulary rows per workgroup of the first launch (four waves of four rows), whatever B, V, K or the device. */
#define X2I_QWEN_HEAD_ROWS 16

/* f32 elements of the workspace both entry points share: a header of four words (the snapshot of the step counter), then per
 * (sample, workgroup) the largest penalised logit of the workgroup's rows and its row index. */
#define X2I_QWEN_HEAD_WS_FLOATS(B, V) (4 + 2 * (int64_t)(B) * (((int64_t)(V) + X2I_QWEN_HEAD_ROWS - 1) / X2I_QWEN_HEAD_ROWS))

/* Vocabulary projection, repetition penalty, optional scores and the argmax partials:
 *   l[b][n] = sum_k W[n][k] X[b][k]                                          f32, the sum of x2i_qwen_decode_linear_bf16 (mode 0, no bias)
 *   p[b][n] = seen[b][n] ? (l < 0 ? l * penalty : l / penalty) : l           f32, one rounding; the division is a true division
 *   part[b][g] = (max_n p[b][n], the LOWEST such n) over the rows n of workgroup g: [g * X2I_QWEN_HEAD_ROWS, (g + 1) * X2I_QWEN_HEAD_ROWS)
 * X: bf16 [B] rows of K elements (row stride ldx); W: bf16 [V][K] (row stride ldw), streamed once, no bias; seen: uint8 [B] rows of V
 * bytes (row stride ld_seen), non-zero = the token is in the sample's sequence, or NULL (nothing is penalised); logits: f32 [B] rows
 * of V elements (row stride ldl) or NULL; it receives p, columns < V only.  step: device int32, the column counter of
 * x2i_qwen_head_select, or NULL; its value is copied into the workspace's header for the select call that follows (NULL: no
 * column and no advance), so that no workgroup of that launch reads a word another one writes.
 * The bits of l[b][n] depend on row n of W and row b of X alone: not on B, on V, or on where row n falls in a wave or a workgroup
 * (x2i_qwen_decode_linear_bf16's promise).  Equal rows of W give equal logits, and the lowest index wins among them.
 * Inputs are taken to be finite.  A NaN never wins a comparison; every index written is in [0, V).
 * ws: f32, ws_floats >= X2I_QWEN_HEAD_WS_FLOATS(B, V) elements, contents irrelevant before.
 * Needs B in 1..8, V > 0, K > 0, K % 8 == 0, ldx, ldw % 8 == 0 and >= K, ld_seen >= V, ldl >= V, a positive finite penalty, 16-byte
 * aligned X, W and ws, a 4-byte aligned logits and step. */
int x2i_qwen_head_logits_argmax_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const uint8_t* seen, int64_t ld_seen, float penalty,
                                     float* logits, int64_t ldl, const int32_t* step, float* ws, int64_t ws_floats, int32_t B, int32_t V, int32_t K,
                                     x2i_stream_t stream);

/* One workgroup per sample: the argmax over the sample's partials and the bookkeeping of one generated token.
 * The partials are reduced in ascending workgroup order and a value wins only when strictly greater, so among equal f32 values the lowest
 * index wins (torch.argmax's rule).  The result is clamped into [0, V).  Then, with col the counter's value as the logits call left it
 * in the workspace:
 *   tok = done[b] ? pad : argmax
 *   token[b] = tok                                     int64 [B]: what the embedding gather of the next step reads
 *   sequences[b * ld_seq + col] = tok                  int64; skipped when col is outside [0, ncols): the call does not fault
 *   lengths[b] += !done[b]                             int64 [B]
 *   done[b] |= tok in eos[0 .. n_eos)                  done uint8 [B] (0 / 1); eos device int64 [n_eos], n_eos in 0..8 (0: eos may be NULL)
 *   seen[b * ld_seen + tok] = 1                        when seen is not NULL
 *   *step = col + 1                                    by sample 0's workgroup
 * ws: the workspace of the x2i_qwen_head_logits_argmax_bf16 call before it on the same stream, with the same B and V.
 * Needs B in 1..8, V > 0, ws_floats >= X2I_QWEN_HEAD_WS_FLOATS(B, V), 0 <= pad < V, ncols >= 0, ld_seq >= ncols, ld_seen >= V, n_eos in
 * 0..8, a 16-byte aligned ws, 8-byte aligned token, sequences, lengths, eos and a 4-byte aligned step. */
int x2i_qwen_head_select(const float* ws, int64_t ws_floats, int32_t* step, int64_t* token, int64_t* sequences, int64_t ld_seq, int32_t ncols,
                         int64_t* lengths, uint8_t* done, const int64_t* eos, int32_t n_eos, int64_t pad, uint8_t* seen, int64_t ld_seen, int32_t B,
                         int32_t V, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
