/* x2i_whisper.h -- extension header of libx2i_hip.so: the MiniCPM-o Whisper audio tower's kernels (csrc/whisper.hip).
 *
 * The conventions are those of x2i.h and of the other extension headers, x2i_siglip.h the nearest (device pointers owned by the caller, raw
 * bf16 storage, `stream` a hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a
 * negative X2I_ERR_* code with the message in x2i_last_error(); every argument is validated before any launch).  The entry points live
 * in an extension header because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/whisper_ops.py, the host
 * module x2i_amd/whisper.py (WhisperAudioTower).
 *
 * They stand at the two ends of the audio path behind `model.apm` (MiniCPMWhisperEncoder: Whisper's encoder), `audio_projection_layer`
 * and `audio_avg_pooler` of MiniCPM-o 2.6: the windows of the Conv1d stem's first convolution, and the average pooling of the tail.  Both
 * are memory-bound row kernels with no matrix product; everything of the tower that carries FLOPs runs on entry points that exist:
 * x2i_gemm_bf16 (conv1 over the rows written here; conv2 as a GEMM over OVERLAPPING rows of conv1's zero-padded output, lda = 2 * D and
 * K = 3 * D, no kernel and no copy; the biased projections, GELU-erf, ReLU, the residuals), x2i_siglip_add_positions_bf16 (the position
 * table), x2i_ln_affine_bf16, x2i_siglip_head_split_bf16 at dk = 64 and x2i_vit_attention_bf16 (a key range per row: the padding and
 * the chunk mask of get_audio_embedding).
 */
#ifndef X2I_WHISPER_H
#define X2I_WHISPER_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The windows of Conv1d(Cin, D, 3, padding = 1) over B mel spectrograms as the rows of a GEMM (its A operand; the weight [D, Cin, 3]
 * flattened to [D, 3*Cin] is the W operand, and the bias and the GELU go on in that GEMM).
 * mel: bf16 [B][Cin][T]; element (b, ci, t) at mel + b * mel_batch_stride + ci * mel_ld + t (elements).
 *   Xr[b*T + t][ci*3 + k]    = mel[b][ci][t + k - 1]   for ci < Cin, k < 3, and 0 where t + k - 1 lies outside [0, T)
 *   Xr[b*T + t][3*Cin .. Kp-1] = 0
 * Xr: bf16 rows of ldx elements; every element of columns < Kp of the B*T rows is written, nothing at or beyond column Kp is and nothing
 * beyond row B*T.  A plain permutation, bit-exact.  mel is read element by element (coalesced along t, through an LDS tile), so its start
 * may be only 2-byte aligned; Xr is written in 16-byte pieces.
 * Needs B, Cin, T >= 1, B <= 65535, Kp % 8 == 0, Kp >= 3*Cin, ldx % 8 == 0, ldx >= Kp, mel_ld >= T, mel_batch_stride >= Cin*mel_ld and a
 * 16-byte aligned Xr. */
int x2i_whisper_mel_rows_bf16(const void* mel, int64_t mel_batch_stride, int64_t mel_ld, void* Xr, int64_t ldx, int32_t B, int32_t Cin,
                              int32_t T, int32_t Kp, x2i_stream_t stream);

/* AvgPool1d(k, stride = k) over the time axis of token-major rows:
 *   Y[b][j][c] = bf16( (float(X[b][k*j][c]) + ... + float(X[b][k*j + k-1][c])) / k )   for j < n_out = (S - k) / k + 1, c < D
 * -- the f32 sum in index order, one division, one rounding.  Element (b, s, c) of X at X + b * x_batch_stride + s * ldx + c, (b, j, c)
 * of Y at Y + b * y_batch_stride + j * ldy + c (elements).  Rows of X at or beyond k * n_out are not read; only rows < n_out and
 * columns < D of Y are written.
 * Needs B >= 1, k in 1..8, S >= k, D % 8 == 0, ldx % 8 == 0, ldx >= D, ldy % 8 == 0, ldy >= D, x_batch_stride % 8 == 0,
 * x_batch_stride >= S*ldx, y_batch_stride % 8 == 0, y_batch_stride >= n_out*ldy and 16-byte aligned X and Y. */
int x2i_whisper_pool_rows_bf16(const void* X, int64_t x_batch_stride, int64_t ldx, void* Y, int64_t y_batch_stride, int64_t ldy, int32_t B,
                               int32_t S, int32_t D, int32_t k, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
