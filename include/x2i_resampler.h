/* x2i_resampler.h -- extension header of libx2i_hip.so: the MiniCPM-o Resampler's kernels (csrc/resampler.hip).
 *
 * The conventions are those of x2i.h and of the six extension headers before this one (device pointers owned by the caller, raw bf16
 * storage, `stream` a hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a
 * negative X2I_ERR_* code with the message in x2i_last_error(); every argument is validated before any launch).  The entry points live
 * in an extension header because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/resampler_ops.py, the
 * host module x2i_amd/resampler.py (Resampler).
 *
 * The Resampler behind `model.resampler` of MiniCPM-o 2.6 is a perceiver: NQ learned queries cross-attend over the patches of each
 * frame that the SigLIP tower (x2i_siglip.h) hands it.  Its matrix products run on x2i_gemm_bf16 and its plain LayerNorms on
 * x2i_ln_affine_bf16; what is here is the attention, whose queries are a parameter and not a sequence, and the two row kernels around
 * the key / value projections.
 */
#ifndef X2I_RESAMPLER_H
#define X2I_RESAMPLER_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Learned-query attention: O[b][i][128h ..] = softmax_j( scale * Q[h][i] . K[b][h][j] ) V[b][h][j] over the keys j < n_keys[b].
 *   Q:  bf16 [H][NQpad][128], the SAME queries for all B samples (never replicated); NQpad = NQ rounded up to 32, 1 <= NQ <= 64.  Rows
 *       NQ .. NQpad-1 may hold anything, NaN included.
 *   K:  bf16 [B][H][Lpad][128];   VT: bf16 [B][H][128][Lpad] (the layouts of x2i_vit.h).  Both need only be finite in [0, Lpad).
 *   n_keys: device int32 [B], clamped into [0, L] in the kernel; NULL means L for every sample.  Key j of sample b counts iff
 *       j < n_keys[b]: the mask is by index, never by data.
 *   O:  bf16, token-major: row i of sample b at O + b * o_batch_stride + i * ldo (elements), head h at columns 128h .. 128h+127.  Only rows
 *       < NQ and columns < 128 H are written, and every one of them is.  A sample with n_keys == 0 gets exactly 0 there.
 * The arithmetic is x2i_vit_attention_bf16's: f32 scores, scale * log2 e folded into one multiply, a running maximum in the exp2 domain
 * that starts at a floor far below any score, P rounded to bf16 for the P V product, O accumulated in f32, normalised and rounded once.
 * One workgroup of four waves per (sample, head).  The waves split the key walk between them (halves at NQ > 32, where two waves hold
 * the two 32-row groups of queries; quarters below that) and merge their partial (maximum, sum, O) states in f32 in a fixed order, so a
 * sample's result is a function of its own K, VT and n_keys alone, bit for bit, whatever B is and whatever the other samples hold.
 * Needs B, H >= 1, 1 <= NQ <= 64, Lpad % 64 == 0, Lpad >= L >= 1, a positive finite scale, 16-byte aligned Q, K, VT and O, a 4-byte
 * aligned n_keys, ldo >= 128 H, ldo % 8 == 0 and o_batch_stride % 8 == 0. */
int x2i_resampler_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* n_keys, void* O, int32_t B, int32_t H,
                                 int32_t NQ, int32_t L, int32_t Lpad, float scale, int64_t ldo, int64_t o_batch_stride, x2i_stream_t stream);

/* ln_kv and the position add in one pass over X (the Resampler's `ln_kv(x)` and the bf16 `x + pos_embed` behind it):
 *   XV[r][c] = x2i_ln_affine_bf16 of X[r] (weight, bias, eps), bit for bit                                  r < rows, c < D
 *   XK[r][c] = bf16( float(XV[r][c]) + float(pos[ids[r]][c]) ): x2i_siglip_add_positions_bf16's arithmetic on the ROUNDED XV
 * X, XV, XK: bf16 rows of ldx, ldv, ldk elements; weight, bias: bf16 [D]; ids: device int32 [rows]; pos: bf16 [n_pos][D], contiguous.
 * ids[r] < 0 marks a padding row: XK[r] = XV[r] (the reference pads its position rows with 0.0).  ids[r] >= n_pos is clamped into the
 * table.  X may overlap neither output (XV and XK are distinct too).  Columns >= D are neither read nor written.
 * Needs rows, n_pos >= 1, D % 8 == 0, D <= 4096, every row stride a multiple of 8 and >= D, 16-byte aligned X, XV, XK, weight, bias and
 * pos, a 4-byte aligned ids and a finite eps >= 0. */
int x2i_resampler_ln_pos_bf16(const void* X, int64_t ldx, const void* weight, const void* bias, float eps, const int32_t* ids,
                              const void* pos, int32_t n_pos, void* XV, int64_t ldv, void* XK, int64_t ldk, int64_t rows, int32_t D,
                              x2i_stream_t stream);

/* The head split in front of x2i_resampler_attention_bf16, from the rows of the k and the v projection (two GEMMs with different A
 * operands, XK and XV; they may write side by side into one buffer: Kr and Vr are then two column offsets into it and ldk == ldv):
 *   Kr, Vr: bf16 [B*L][H*128] (row strides ldk, ldv)
 *   K[b][h][s][d] = Kr[b*L + s][128h + d]   (bf16 [B][H][Lpad][128]),   VT[b][h][d][s] = Vr[b*L + s][128h + d]   (bf16 [B][H][128][Lpad])
 * A plain permutation, bit-exact.  Only rows (K) / columns (VT) s < L are written.
 * Needs B, L, H >= 1, B, H <= 65535, Lpad >= L, Lpad % 8 == 0, ldk and ldv multiples of 8 and >= 128 H, 16-byte aligned pointers. */
int x2i_resampler_kv_split_bf16(const void* Kr, int64_t ldk, const void* Vr, int64_t ldv, void* K, void* VT, int32_t B, int32_t L,
                                int32_t Lpad, int32_t H, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
