/* x2i_logmel.h -- extension header of libx2i_hip.so: the Whisper log-mel front end (csrc/logmel.hip), a 16 kHz waveform to the log-mel
 * features that WhisperFeatureExtractor computes on the host and the audio tower (x2i_whisper.h) reads.
 *
 * The conventions are those of x2i.h and of the other extension headers (device pointers owned by the caller, `stream` a hipStream_t passed
 * as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_* code with the message in
 * x2i_last_error(); every argument is validated before any launch).  The header stands under include/ext/ because the set of
 * include/x2i_*.h headers is closed like x2i.h's table of exports; the binding is x2i_amd/logmel_binding.py, the host module
 * x2i_amd/logmel.py (LogMel).
 *
 * Compile-time constants: n_fft = 400 samples per frame, hop = 160, 201 bins.  Arguments: the chunk length N_max in samples (a multiple of
 * 160, at least 320; Whisper's is 480000) and n_mels in 1..128.  T = N_max / 160 frames per chunk; a workgroup computes 32 frames, so a
 * sample has NB = (T + 31) / 32 workgroups.
 *
 * Sample b is the first n[b] values of its row of `wave`, extended by zeros to N_max; THAT signal is reflect-padded by 200 on both sides:
 * index i < 0 reads x[-i], index i >= N_max reads x[2 (N_max - 1) - i], and every read at or beyond n[b] gives 0.  Frame t < T covers
 * the indices 160 t - 200 .. 160 t + 199 (the extractor's extra last frame does not exist here).  With w the periodic Hann window,
 *   X_t[k]      = sum_j w[j] x[160 t - 200 + j] exp(-2 pi i j k / 400),  k < 201
 *   lg[b][m][t] = log10(max(sum_k |X_t[k]|^2 F[k][m], 1e-10))           (exactly -10 where the sum is at most 1e-10)
 *   out[b][m][t] = (max(lg[b][m][t], mx_b - 8) + 4) / 4 for t < L_b, 0 for L_b <= t < T_out,   mx_b = max over ALL m, t < T of lg[b]
 * L_b = min(ceil(n[b] / 160), T) frames are kept; A_b = min(T, (n[b] + 199) / 160 + 1) >= L_b frames can see a non-zero sample, and all
 * of them take part in mx_b.  Frames at or beyond A_b are exactly -10 and are neither computed nor stored.
 * Everything is float32: f32-input matrix instructions, each sum a chain of f32 fused multiply-adds.  A sample's bits depend on its own
 * n[b] values, N_max and n_mels alone: not on B, the other samples, or T_out.
 *
 * Tables, computed by the host in float64 and rounded to float32 (x2i_amd/logmel.py):
 *   dft    f32 [400][448]: row j, column 64 q + c holds  w[j] cos(2 pi j k / 400) for c < 32, k = 32 q + c, and
 *                          -w[j] sin(2 pi j k / 400) for 32 <= c < 64, k = 32 q + c - 32; zero where k >= 201.  16-byte aligned.
 *   fbank  f32 [224][128]: row k < 201, column m < n_mels holds F[k][m] (the extractor's mel_filters); every other element is zero.
 *                          16-byte aligned.
 */
#ifndef X2I_LOGMEL_H
#define X2I_LOGMEL_H
#include "../x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* wave: f32 [B][ldw], sample b at wave + b * ldw; only indices < min(n[b], N_max, ldw) are read, so ldw may be shorter than N_max.
 * n: int32 [B] in device memory (a negative count is read as 0).
 * lg: f32 workspace of lg_floats >= B * n_mels * T elements, (b, m, t) at (b * n_mels + m) * T + t; only the frames of workgroups g
 * with 32 g < A_b are written.
 * part: f32 workspace of part_floats >= B * NB elements: the maximum of lg over workgroup g of sample b at b * NB + g, written for
 * 32 g < A_b only (plain stores).
 * Needs B in 1..65535, N_max % 160 == 0, 320 <= N_max <= 2^30, n_mels in 1..128, ldw >= 1, wave / n / lg / part 4-byte aligned. */
int x2i_logmel_spectrum_f32(const void* wave, int64_t ldw, const void* n, const void* dft, const void* fbank, void* lg, int64_t lg_floats,
                            void* part, int64_t part_floats, int32_t B, int32_t N_max, int32_t n_mels, x2i_stream_t stream);

/* lg, part: as x2i_logmel_spectrum_f32 left them for the same B, N_max and n_mels.
 * out: [B][n_mels][T_out], element (b, m, t) at out + b * out_batch_stride + m * out_ld + t (elements); float32, or bf16 (one rounding of
 * the float32 value, to nearest even) where out_bf16 != 0.  Every column < T_out of the B * n_mels rows is written, nothing else is.
 * T_out may be smaller or larger than T.
 * Needs B in 1..65535, N_max as above, n_mels in 1..128, T_out >= 1, out_ld >= T_out, out_batch_stride >= n_mels * out_ld, out aligned
 * to its element size. */
int x2i_logmel_finish(const void* lg, int64_t lg_floats, const void* part, int64_t part_floats, const void* n, void* out,
                      int64_t out_batch_stride, int64_t out_ld, int32_t B, int32_t N_max, int32_t n_mels, int32_t T_out, int32_t out_bf16,
                      x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
