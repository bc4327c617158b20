/* x2i_siglip.h -- extension header of libx2i_hip.so: the MiniCPM-o SigLIP (NaViT) vision tower's kernels (csrc/siglip.hip).
 *
 * The conventions are those of x2i.h, x2i_t5.h, x2i_clip.h, x2i_qwen.h and x2i_vit.h (device pointers owned by the caller, raw bf16
 * storage, `stream` a hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a
 * negative X2I_ERR_* code with the message in x2i_last_error(); every argument is validated before any launch).  The entry points live
 * in an extension header because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/siglip_ops.py, the host
 * module x2i_amd/siglip.py (SiglipVisionTower).
 *
 * They stand behind SiglipVisionEmbeddings and the head reshape of SiglipAttention in the NaViT SigLIP tower behind `model.vpm` of
 * MiniCPM-o 2.6 (the same module as `transformers`' Idefics2VisionTransformer).  All three are memory-bound row kernels with no matrix
 * product; everything of the tower that carries FLOPs runs on entry points that exist: x2i_gemm_bf16 (the patch embedding, the biased
 * projections, GELU-tanh, the residuals), x2i_ln_affine_bf16 and x2i_vit_attention_bf16 (bidirectional, a key range per row).
 *
 * The tower's heads are 72 wide (1152 / 16).  The host module pads every head of the packed q|k|v weight to 80 with zero rows, so the
 * kernels here and the attention see heads of 80, which x2i_vit.h STORES 128 wide: x2i_siglip_head_split_bf16 writes that layout.
 */
#ifndef X2I_SIGLIP_H
#define X2I_SIGLIP_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The patches of B pixel strips as the rows of the patch embedding's GEMM (its A operand; the Conv2d bias goes on in that GEMM).
 * strips: bf16 [B][3][P][P*L] -- one strip of L patches per image, P pixel rows high, patch p at columns P*p .. P*p + P-1; element
 * (b, ci, r, x) at strips + b * strip_batch_stride + (ci * P + r) * strip_ld + x (elements).
 *   Xp[b*L + p][ci*P*P + r*P + c] = strips[b][ci][r][P*p + c]        for ci < 3 and r, c < P: the column order of the Conv2d weight
 *   Xp[b*L + p][3*P*P .. Kp-1]    = 0
 * Xp: bf16 rows of ldx elements; every element of columns < Kp of the B*L rows is written, nothing at or beyond column Kp is.  A plain
 * permutation, bit-exact.  A patch starts at an element offset that is a multiple of P only (28 bytes for P = 14), so the strip is read
 * element by element; Xp is written in 16-byte pieces.
 * Needs B, L >= 1, P in 1..32, Kp % 8 == 0, Kp >= 3*P*P, ldx % 8 == 0, ldx >= Kp, strip_ld >= P*L, strip_batch_stride >= 3*P*strip_ld
 * and a 16-byte aligned Xp. */
int x2i_siglip_patch_rows_bf16(const void* strips, int64_t strip_batch_stride, int64_t strip_ld, void* Xp, int64_t ldx, int32_t B,
                               int32_t L, int32_t P, int32_t Kp, x2i_stream_t stream);

/* The position embedding of SiglipVisionEmbeddings, added in place:
 *   X[r][c] = bf16( float(X[r][c]) + float(pos[ids[r]][c]) )        for r < rows, c < D: one f32 add and one rounding, which is bit for
 * bit the library's bf16 `embeddings + position_embedding(position_ids)`.
 * X: bf16 rows of ldx elements; ids: device int32 [rows]; pos: bf16 [n_pos][D], contiguous.  An id outside [0, n_pos) is clamped into
 * the table (the host cannot see it, and no launch reads out of bounds): the contract of x2i_clip_embed_bf16.  Columns >= D of X are
 * neither read nor written.
 * Needs rows, n_pos >= 1, D % 8 == 0, ldx % 8 == 0, ldx >= D, 16-byte aligned X and pos and a 4-byte aligned ids. */
int x2i_siglip_add_positions_bf16(void* X, int64_t ldx, const int32_t* ids, const void* pos, int32_t n_pos, int64_t rows, int32_t D,
                                  x2i_stream_t stream);

/* The head split in front of x2i_vit_attention_bf16 (SiglipAttention's q / k / v `.view(B, L, H, dk).transpose(1, 2)`), from the rows of
 * ONE GEMM over the stacked q|k|v weight: x2i_t5_head_split_bf16 for the head widths and the storage of x2i_vit.h.
 *   qkv: bf16 [B*S][3*H*dk] (row stride ld elements), columns [q (H*dk) | k (H*dk) | v (H*dk)]
 *   Q[b][h][s][d] = q, K[b][h][s][d] = k   (bf16 [B][H][Spad][dkp]),   VT[b][h][d][s] = v   (bf16 [B][H][dkp][Spad])
 * with dkp = 128 for dk = 80 and dkp = dk otherwise.  A plain permutation, bit-exact.  Only rows (Q, K) / columns (VT) s < S and columns
 * (Q, K) / rows (VT) d < dk are written.
 * Needs dk in {64, 80, 128}, Spad >= S, Spad % 8 == 0, H, B <= 65535, ld % 8 == 0, ld >= 3*H*dk and 16-byte aligned pointers. */
int x2i_siglip_head_split_bf16(const void* qkv, int64_t ld, void* Q, void* K, void* VT, int32_t B, int32_t S, int32_t Spad, int32_t H,
                               int32_t dk, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
