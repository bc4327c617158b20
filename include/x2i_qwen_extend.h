/* x2i_qwen_extend.h -- extension header of libx2i_hip.so: the Qwen2 prompt extension's kernels (csrc/qwen_extend.hip,
 * csrc/encoder_attention.hip): a chunk of n new rows run against a key/value cache that already holds the keys before them.
 *
 * The conventions are those of x2i.h and the other extension headers (device pointers owned by the caller, raw bf16 storage, `stream` a
 * hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The binding is
 * x2i_amd/qwen_extend_ops.py, the host module x2i_amd/qwen.py (Qwen2DecoderStack.extend).
 *
 * All coordinates are PHYSICAL CACHE SLOTS ("absolute rows"): the chunk's row s lives at slot row0 + s of buffers that hold cap slots per
 * head; row0 and n are host integers, the same for every sample.  Both entry points refuse row0 < 0, n < 1, row0 + n > cap and
 * cap % 64 != 0 (X2I_ERR_SHAPE); row0 is otherwise arbitrary -- no multiple of 8, 64 or 128.
 */
#ifndef X2I_QWEN_EXTEND_H
#define X2I_QWEN_EXTEND_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Rotate-half RoPE and head split of n new rows per sample: x2i_qwen_rope_split_bf16's arithmetic element for element (f32, one rounding),
 * written at slot row0 + s instead of s.
 * qkv: bf16 [B * n] rows [q (Hq*dk) | k (Hkv*dk) | v (Hkv*dk)], row stride ld (elements); cos, sin: f32 [B][n][dk/2], the half tables of
 * the CHUNK's positions (the position is not the slot).  Writes q to rows row0 + s of Q [B][Hq][cap][dk], k to rows row0 + s of
 * K [B][Hkv][cap][dk] and v to COLUMNS row0 + s of VT [B][Hkv][dk][cap], s = 0 .. n-1, and nothing else of Q, K or VT: a run of V^T
 * columns starts and ends anywhere inside a 16-byte group; its ragged head and tail are 2-, 4- and 8-byte stores, its middle 16-byte
 * stores.
 * Needs dk in {64, 128}, B in 1..65535, Hq + Hkv <= 65535, ld % 8 == 0 and >= (Hq + 2 Hkv) dk, 16-byte aligned pointers. */
int x2i_qwen_extend_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                                    int32_t row0, int32_t n, int32_t cap, int32_t Hq, int32_t Hkv, int32_t dk, x2i_stream_t stream);

/* Causal attention with grouped key/value heads of the query rows row0 .. row0 + n - 1 of Q [B][Hq][cap][dk] over K [B][Hkv][cap][dk] and
 * VT [B][Hkv][dk][cap]: key j counts for absolute row i iff k_lo[b] <= j <= i.  k_lo: device int32 [B], clamped into [0, row0 + n]; NULL
 * means 0.  Output row s = i - row0 goes to O + b * o_batch_stride + s * ldo (elements), Hq*dk columns; every one of the n rows is
 * written and nothing else; a row with no counted key (i < k_lo[b]) is exactly 0.
 * Two promises (tests/test_qwen_extend_gpu.py asserts both):
 *   - a live row's result is a function of live data only: the chunk's Q rows and the K / V^T slots [k_lo, row0 + n).  Everything else
 *     in Q, K and VT need only be finite; no other row of Q is read at all, and the mask is by index;
 *   - a live row whose 32-row group (absolute rows 32g .. 32g + 31) holds no row below row0 equals, bit for bit, the same row of
 *     x2i_qwen_attention_bf16 on the same buffers with S = row0 + n, Spad = cap, k_hi = row0 + n: the same tile walk, the same step.
 *     (That launch also READS the rows S .. of Q, which this one never does; the identity holds where those rows do not move a rescale
 *     of their wave: equal to row S - 1, or zero.)  With row0 % 32 == 0 that is every row.  A relaunch is bit-identical.
 * Needs dk in {64, 128}, Hq % Hkv == 0, a positive finite scale, ldo >= Hq dk, ldo % 4 == 0, o_batch_stride % 4 == 0, 16-byte aligned
 * Q, K, VT, an 8-byte aligned O and a 4-byte aligned k_lo. */
int x2i_qwen_extend_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* k_lo, void* O, int32_t B, int32_t Hq,
                                   int32_t Hkv, int32_t row0, int32_t n, int32_t cap, int32_t dk, float scale, int32_t ldo,
                                   int64_t o_batch_stride, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
