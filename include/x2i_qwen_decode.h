/* x2i_qwen_decode.h -- extension header of libx2i_hip.so: the kernels of Qwen2 decoding with a key/value cache (csrc/qwen_decode.hip).
 *
 * The conventions are those of x2i.h and the other extension headers (device pointers owned by the caller, raw bf16 storage, `stream` a
 * hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The binding is
 * x2i_amd/qwen_decode_ops.py, the host module x2i_amd/qwen.py (Qwen2DecoderStack.new_cache / prefill / decode_step).
 *
 * A decode step runs ONE token per sample through every layer against the keys and values of the tokens before it.  The three entry
 * points stand behind `transformers`' Qwen2Attention with a DynamicCache (apply_rotary_pos_emb, cache.update, the attention over the
 * cached keys) and the nn.Linear projections of a layer at 1..8 rows, where the library's own GEMMs have no form that streams a weight
 * at the memory rate.  Every per-step scalar that changes from token to token (the append slot, the key range) is read from DEVICE
 * memory, so a step can be captured in a graph once and replayed.  The two RMS norms of a step run on x2i_t5_rms_rows_bf16.
 *
 * The cache of one layer is K bf16 [B][Hkv][cap][dk] and VT bf16 [B][Hkv][dk][cap] (V transposed): the layouts of
 * x2i_qwen_rope_split_bf16's outputs with Spad = cap, so a prefill writes the prompt straight into it.
 */
#ifndef X2I_QWEN_DECODE_H
#define X2I_QWEN_DECODE_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Keys per split of the decode attention's key axis.  Chunk c holds the keys [c * CHUNK, (c + 1) * CHUNK) of the cache whatever the
 * launch's batch, head counts or the device, so the cut of a sample depends only on its own range and on this constant. */
#define X2I_QWEN_DECODE_CHUNK 256

/* f32 elements of x2i_qwen_decode_attention_bf16's workspace: per (sample, query head, chunk) the running maximum, the sum and dk
 * unnormalised outputs. */
#define X2I_QWEN_DECODE_WS_FLOATS(B, Hq, cap, dk) \
  ((int64_t)(B) * (Hq) * (((cap) + X2I_QWEN_DECODE_CHUNK - 1) / X2I_QWEN_DECODE_CHUNK) * ((dk) + 2))

/* Rotate-half RoPE on the q and k of ONE new token per sample, and the append of its k and v to the cache.
 * qkv: bf16 rows [B] of (Hq + 2 Hkv) * dk elements, columns [q (Hq*dk) | k (Hkv*dk) | v (Hkv*dk)] (biases added), row stride ld.
 * cos, sin: f32 [B][dk/2], the half tables of the token's position; the arithmetic is x2i_qwen_rope_split_bf16's:
 *   y[d]        = bf16( x[d] c[d] - x[d + dk/2] s[d] )
 *   y[d + dk/2] = bf16( x[d + dk/2] c[d] + x[d] s[d] )          in f32 with ONE rounding
 * slot: device int32 [B].  q -> Qd bf16 [B][Hq][dk]; k -> row slot[b] of K bf16 [B][Hkv][cap][dk]; v -> column slot[b] of VT bf16
 * [B][Hkv][dk][cap].  Nothing else of K or VT is written.  A sample whose slot lies outside [0, cap) gets nothing written (Qd
 * neither), and the call does not fault.  Position comes from the tables, not from the slot.
 * Needs dk in {64, 128}, cap % 64 == 0, B, Hq, Hkv in 1..65535, ld % 8 == 0, ld >= (Hq + 2 Hkv) * dk, 16-byte aligned qkv, cos, sin,
 * Qd, K, VT and a 4-byte aligned slot. */
int x2i_qwen_decode_rope_append_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, const int32_t* slot, void* Qd, void* K,
                                     void* VT, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t dk, x2i_stream_t stream);

/* Qwen2Attention of one query token per sample over the cached keys:
 *   O[b][h*dk + d] = sum_j softmax_j(scale q_h . k_j) v_j[d]     over the keys k_lo[b] <= j < k_hi[b]
 * Qd: bf16 [B][Hq][dk]; K: bf16 [B][Hkv][cap][dk]; VT: bf16 [B][Hkv][dk][cap]; query head h reads key/value head h / (Hq / Hkv).
 * k_lo, k_hi: device int32 [B], REQUIRED, clamped into [0, cap].  O: bf16, row b at O + b * ldo (elements); columns < Hq*dk are
 * written, every one of them, and nothing else.
 * The mask is by index, never by data: a key outside the range never enters a maximum or a sum, whatever K and VT hold there; they
 * only need to be finite.  An empty range (k_hi <= k_lo after the clamp) gives O exactly 0, and it is written.
 * Arithmetic (the contract of x2i_qwen_attention_bf16): scores and the softmax in f32 in the exp2 domain (scale * log2 e folded into
 * one multiply); P rounded to bf16 for the P V product; O accumulated in f32, normalised and rounded once.
 * The key axis is cut into the fixed chunks of X2I_QWEN_DECODE_CHUNK keys: one launch writes each non-empty chunk's partial (maximum,
 * sum, f32 O) to ws, a second launch in the same call combines a sample's partials in ascending chunk order.  The cut depends only
 * on the sample's own range and the constant -- never on B, the head counts or the device -- so a sample's result is bit-identical
 * whatever batch it is launched in, and a relaunch is bit-identical.
 * ws: f32, ws_floats >= X2I_QWEN_DECODE_WS_FLOATS(B, Hq, cap, dk) elements, contents irrelevant before and undefined after.
 * Needs dk in {64, 128}, Hq % Hkv == 0, Hq / Hkv <= 16, cap % 64 == 0, B, Hq in 1..65535, a positive finite scale, ldo >= Hq*dk,
 * ldo % 4 == 0 and an 8-byte aligned O, 16-byte aligned Qd, K, VT, ws, and 4-byte aligned k_lo, k_hi. */
int x2i_qwen_decode_attention_bf16(const void* Qd, const void* K, const void* VT, const int32_t* k_lo, const int32_t* k_hi, void* O, float* ws,
                                   int64_t ws_floats, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t dk, float scale, int32_t ldo,
                                   x2i_stream_t stream);

/* nn.Linear at 1..8 rows, streaming the weight once at the memory rate:
 *   mode 0:   Y[b][n] = bf16( bias[n] + sum_k W[n][k] X[b][k]  (+ res[b][n]) )
 *   mode 1:   Y[b][n] = bf16( silu(a_n) * b_n ),  a_n = bias[n] + sum_k W[n][k] X[b][k],  b_n = bias[N + n] + sum_k W[N + n][k] X[b][k]
 * X: bf16 [B] rows of K elements (row stride ldx); W: bf16 [N][K] in mode 0, the stacked [gate_proj; up_proj] weight [2N][K] in mode 1
 * (row stride ldw); bias: bf16 [N] ([2N] in mode 1) or NULL; res: bf16 [B] rows of N elements (row stride ldr) or NULL, mode 0 only;
 * Y: bf16 [B] rows of N elements (row stride ldy); only columns < N are written.  Y may be res (each element is read before it is
 * written, by the same lane).
 * The sum is in f32 (fma chains in ascending k per lane, then a fixed cross-lane tree), the bias one f32 add, the residual one more f32
 * add, and there is ONE rounding: the epilogue contract of x2i_gemm_bf16.  In mode 1 a and b stay in f32 (MLP gate of Qwen2MLP, which
 * the library rounds to bf16 twice in between).  The arithmetic of a row does not depend on how many rows share the call: row 0 is
 * bit-identical at B = 1 and B = 8.
 * Needs B in 1..8, N > 0, K > 0, K % 8 == 0, ldx, ldw % 8 == 0 and >= K, ldy (ldr) >= N, mode in {0, 1}, no res in mode 1, and
 * 16-byte aligned X and W. */
int x2i_qwen_decode_linear_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const void* res, int64_t ldr, void* Y,
                                int64_t ldy, int32_t B, int32_t N, int32_t K, int32_t mode, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
