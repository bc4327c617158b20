/* x2i_qwen_decode_w8.h -- extension header of libx2i_hip.so: the decode-step linear of x2i_qwen_decode.h with an e4m3 weight
 * (csrc/qwen_decode_w8.hip).
 *
 * The conventions are those of x2i.h and the other extension headers (device pointers owned by the caller, raw bf16 storage, `stream` a
 * hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The binding is
 * x2i_amd/qwen_decode_w8_ops.py, the host module x2i_amd/qwen.py (Qwen2DecoderStack.pack_w8 / decode_step(w8=True)).
 *
 * A decode step is bound by the weight bytes it streams once per token.  This entry point reads them as OCP e4m3fn codes with one f32
 * scale per output row (x2i_quantize_rows_fp8's output: scale = amax / 448, an all-zero row has scale 1 and codes 0): half the bytes
 * of x2i_qwen_decode_linear_bf16.  Activations stay bf16, accumulation stays f32.
 */
#ifndef X2I_QWEN_DECODE_W8_H
#define X2I_QWEN_DECODE_W8_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* x2i_qwen_decode_linear_bf16 with the weight W[n][k] = w_scale[n] * e4m3(W8[n][k]):
 *   mode 0:   Y[b][n] = bf16( w_scale[n] * sum_k e4m3(W8[n][k]) X[b][k] + bias[n]  (+ res[b][n]) )
 *   mode 1:   Y[b][n] = bf16( silu(a_n) * b_n ),  a_n = w_scale[n] * sum_k e4m3(W8[n][k]) X[b][k] + bias[n],
 *                                                 b_n = w_scale[N + n] * sum_k e4m3(W8[N + n][k]) X[b][k] + bias[N + n]
 * X: bf16 [B] rows of K elements (row stride ldx, elements); W8: OCP e4m3fn codes, one byte each, [N][K] in mode 0, the stacked
 * [gate_proj; up_proj] weight [2N][K] in mode 1, row stride ldw in BYTES; w_scale: f32 [N] ([2N] in mode 1); bias: bf16 [N] ([2N] in
 * mode 1) or NULL; res: bf16 [B] rows of N elements (row stride ldr) or NULL, mode 0 only; Y: bf16 [B] rows of N elements (row stride
 * ldy); only columns < N are written.  Y may be res (each element is read before it is written, by the same lane).
 * Arithmetic: the sum is in f32, and every product of an e4m3 and a bf16 value is exact in f32 (4 + 8 significand bits).  Summation
 * order of one (row, sample): lane l of the 64 lanes of a wave sums the columns k = 16 l + 1024 i + j, i = 0, 1, .. and j = 0 .. 15
 * ascending, in ONE fma chain that starts at +0; the 64 lane sums are then added in a fixed butterfly (xor 32, 16, 8, 4, 2, 1).  Then one
 * f32 multiply by the row's scale, one f32 add of the bias, one f32 add of the residual, and ONE rounding to bf16.  In mode 1 a and b stay
 * in f32 (as in the bf16 entry point) and the product silu(a) * b is one f32 multiply before the rounding.
 * Two promises (tests/test_qwen_decode_w8_gpu.py asserts both):
 *   - the arithmetic of one (row, sample) does not depend on how many samples share the launch, nor on whether X is staged in chunks:
 *     row 0 is bit-identical at B = 1 and B = 8;
 *   - a relaunch is bit-identical.
 * The codes 0x7F and 0xFF (NaN) are never produced by x2i_quantize_rows_fp8; the result of a row that holds one is unspecified.
 * Needs B in 1..8, N > 0, K > 0, K % 16 == 0 (a lane's 16-byte load is 16 weights), ldw % 16 == 0 and >= K, ldx % 8 == 0 and >= K,
 * ldy (ldr) >= N, mode in {0, 1}, no res in mode 1, 16-byte aligned X and W8, and a 4-byte aligned, non-NULL w_scale. */
int x2i_qwen_decode_linear_w8_bf16(const void* X, int64_t ldx, const void* W8, int64_t ldw, const float* w_scale, const void* bias,
                                   const void* res, int64_t ldr, void* Y, int64_t ldy, int32_t B, int32_t N, int32_t K, int32_t mode,
                                   x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
