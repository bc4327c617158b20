/* x2i_sample.h -- extension header of libx2i_hip.so: sampled token selection of Qwen2 decoding (csrc/qwen_sample.hip): temperature, top-k,
 * top-p and an inverse-CDF draw, in the place of x2i_qwen_head_select's argmax.
 *
 * The conventions are those of x2i.h and of the other extension headers (device pointers owned by the caller, `stream` a hipStream_t passed
 * as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_* code with the message in
 * x2i_last_error(); every argument is validated before any launch).  The header stands under include/ext/sample/ because the sets of
 * include/x2i_*.h and include/ext/*.h headers are closed; the binding is x2i_amd/sample_binding.py, the host module x2i_amd/handoff.py
 * (HipGenerate with hip_head=True, sample=True).
 *
 * The one entry point runs behind an x2i_qwen_head_logits_argmax_bf16 call (x2i_qwen_head.h) on the same stream that was given a `logits`
 * buffer: that call leaves the penalised f32 scores p[b][n], per workgroup the largest of them (the softmax's maximum) and the snapshot
 * of the step counter.  One workgroup per sample.  The scores are the only [B, V] array: every pass reads them and none rewrites them;
 * no probability and no sorted index is written, nothing is sorted.  No workgroup waits on another, there is no spin, no arrival counter
 * and no floating-point atomic: counts and masses are integers (LDS integer atomics, integer scans), so no sum depends on an order.
 */
#ifndef X2I_SAMPLE_H
#define X2I_SAMPLE_H
#include "../../x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The entry point needs no workspace of its own beyond the head's: this is the size of that one, X2I_QWEN_HEAD_WS_FLOATS(B, V) of
 * x2i_qwen_head.h, restated so that a caller of this header alone can size it (16 vocabulary rows per workgroup of the head launch). */
#define X2I_SAMPLE_HEAD_WS_FLOATS(B, V) (4 + 2 * (int64_t)(B) * (((int64_t)(V) + 15) / 16))
/* f32 elements per sample of the optional diagnostics */
#define X2I_SAMPLE_DIAG_FLOATS 4
/* One unit of probability mass: a weight w in [0, 1] is the integer round(w * 2^34), so that 2^29 of them fit 64 bits. */
#define X2I_SAMPLE_MASS_BITS 34

/* `transformers`' warpers in the order _get_logits_processor applies them, then one draw.  Per sample b, with p its row of `logits`:
 *   s[n] = p[n] / temperature                                f32, a true division (a -0 counts as +0)
 *   top-k (top_k = 0: off; k = min(top_k, V)):  keep n when s[n] >= the k-th largest value of s; equal values at the threshold are all kept
 *   w[n] = exp(min(s[n] - s_max, 0))                         f32 (s_max = max_n s[n], from the workspace's partials), then the integer
 *   m[n] = round(w[n] * 2^34)                                the mass of token n: every sum below is a sum of these integers
 *   top-p (top_p = 1: off), over the top-k survivors with Zk their mass:  keep n when the mass of survivors with a value STRICTLY greater
 *     than s[n] is < top_p * Zk (compared exactly, as integers).  Without ties this is TopPLogitsWarper (ascending cumulative sum, remove
 *     <= 1 - top_p, keep at least one).  THE ONE DEVIATION: tokens of equal value are kept or dropped together, where the library splits
 *     such a run by its sort position.
 *   draw: Z = sum of m over the kept set; the token is the smallest kept n, in ascending token index, with sum_{kept i <= n} m[i] >
 *     u * Z (compared exactly); if there is none, the largest kept index.
 *   u = u_in[b] where u_in is not NULL (device f32 [B], values in [0, 1); anything else is clamped into that range), otherwise
 *     u = (x0 >> 8) * 2^-24 with x0 word 0 of Philox4x32-10 under the key (lo32(rng[0]), hi32(rng[0])) and the counter
 *     (lo32(c), hi32(c), b, 0), c = rng[1] + col (mod 2^64; col sign-extended, 0 where the logits call had no counter).  rng: device
 *     uint64 [2] = {seed, offset}; it is read and never written, so a generated token consumes one draw and a replayed graph walks
 *     the stream through col.
 * Then, with col the counter's value as the logits call left it in the workspace, the bookkeeping of x2i_qwen_head_select in its order
 * (the same device function): the token is clamped into [0, V); tok = done[b] ? pad : token; token[b]; sequences[b * ld_seq + col]
 * unless col is outside [0, ncols); lengths[b] += !done[b]; done[b] |= tok in eos; seen[b * ld_seen + tok] = 1; *step = col + 1.
 * diag: f32 [B][4] or NULL: the kept count, the smallest kept value of s, Z * 2^-34 and u.
 * A sample's token depends on its scores, its u and the parameters alone: not on B, on its row, or on the run.  Scores are taken to be
 * finite; every token written is in [0, V) whatever the buffers held.
 * logits: f32 [B] rows of V (row stride ldl); ws: the workspace of the logits call, with the same B and V.
 * Needs B in 1..8, 0 < V <= 2^29, ldl >= V, ws_floats >= X2I_SAMPLE_HEAD_WS_FLOATS(B, V), a finite temperature > 0, top_k >= 0,
 * 0 < top_p <= 1, rng or u_in not NULL, 0 <= pad < V, ncols >= 0, ld_seq >= ncols, ld_seen >= V, n_eos in 0..8, a 16-byte aligned ws,
 * 8-byte aligned rng, token, sequences, lengths and eos, 4-byte aligned logits, u_in, diag and step. */
int x2i_sample_select_f32(const float* logits, int64_t ldl, const float* ws, int64_t ws_floats, float temperature, int32_t top_k, float top_p,
                          const void* rng, const float* u_in, float* diag, int32_t* step, int64_t* token, int64_t* sequences, int64_t ld_seq,
                          int32_t ncols, int64_t* lengths, uint8_t* done, const int64_t* eos, int32_t n_eos, int64_t pad, uint8_t* seen,
                          int64_t ld_seen, int32_t B, int32_t V, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
