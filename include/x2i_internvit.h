/* x2i_internvit.h -- extension header of libx2i_hip.so: the InternVL2.5 InternViT vision tower's kernels (csrc/internvit.hip).
 *
 * The conventions are those of x2i.h and of the other extension headers (device pointers owned by the caller, raw bf16 storage, `stream`
 * a hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The entry points live in an extension
 * header because x2i.h's table of exports is closed under ABI version 5; the binding is x2i_amd/internvit_ops.py, the host modules
 * x2i_amd/internvit.py (InternVisionTower, InternVLVision).
 *
 * They stand behind InternVisionEmbeddings (the Conv2d's im2col and the class token / position add) and behind the tail of the chat
 * model's extract_feature (dropping the class token, pixel_shuffle(0.5) and mlp1[0], a LayerNorm over four tokens' channels).  All three
 * are memory-bound row kernels with no matrix product; everything of the tower that carries FLOPs runs on entry points that exist:
 * x2i_gemm_bf16 (the patch embedding, the biased projections, GELU-erf, LayerScale and the residual in the gate epilogue),
 * x2i_ln_affine_bf16 / x2i_t5_rms_rows_bf16, x2i_siglip_head_split_bf16 and x2i_vit_attention_bf16 (bidirectional, no key ranges).
 */
#ifndef X2I_INTERNVIT_H
#define X2I_INTERNVIT_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The patches of B NCHW tiles as the rows of the patch embedding's GEMM (its A operand; the Conv2d bias goes on in that GEMM).
 * img: bf16 [B][3][gh*P][gw*P]; element (b, ci, y, x) at img + b * img_batch_stride + ci * img_chan_stride + y * img_ld + x (elements).
 * With L = gh * gw:
 *   Xp[b*L + r*gw + q][ci*P*P + y*P + x] = img[b][ci][r*P + y][q*P + x]    for ci < 3 and y, x < P: the column order of the Conv2d weight
 *   Xp[b*L + r*gw + q][3*P*P .. Kp-1]    = 0
 * Xp: bf16 rows of ldx elements; every element of columns < Kp of the B*L rows is written, nothing at or beyond column Kp is.  A plain
 * permutation, bit-exact.  A patch row starts at an element offset that is a multiple of P only (28 bytes for P = 14), so the image is
 * read element by element; Xp is written in 16-byte pieces.
 * Needs B, gh, gw >= 1, B*gh*gw < 2^31, P in 1..32, Kp % 8 == 0, Kp >= 3*P*P, ldx % 8 == 0, ldx >= Kp, img_ld >= gw*P,
 * img_chan_stride >= gh*P*img_ld, img_batch_stride >= 3*img_chan_stride, a 2-byte aligned img and a 16-byte aligned Xp. */
int x2i_internvit_patch_rows_bf16(const void* img, int64_t img_batch_stride, int64_t img_chan_stride, int64_t img_ld, void* Xp, int64_t ldx,
                                  int32_t B, int32_t gh, int32_t gw, int32_t P, int32_t Kp, x2i_stream_t stream);

/* InternVisionEmbeddings.forward behind the patch embedding's GEMM, IN PLACE: the GEMM writes its bf16 output (the Conv2d bias added in
 * the GEMM and rounded once: the library's bf16 conv output) straight into rows 1 .. L of every sample of X (x2i_gemm_args: c_offset = D
 * elements, c_batch_stride = (1+L)*D, batch = B), and this kernel writes the class row and adds the position table:
 *   X[b][0][c]   = bf16( float(cls[c]) + float(pos[0][c]) )
 *   X[b][1+p][c] = bf16( float(X[b][1+p][c]) + float(pos[1+p][c]) )        for p < L, c < D
 * one f32 add and one rounding per element, which is bit for bit the library's bf16 `cat([class, patches]) + position_embedding`.
 * X: bf16 [B][1+L][D], contiguous; cls: bf16 [D]; pos: bf16 [1+L][D], contiguous.  Row 0 of a sample is written without being read; all
 * B*(1+L)*D elements of X are written and nothing else.
 * Needs B, L >= 1, D % 8 == 0 and 16-byte aligned X, cls and pos. */
int x2i_internvit_embed_bf16(void* X, const void* cls, const void* pos, int32_t B, int32_t L, int32_t D, x2i_stream_t stream);

/* The head of extract_feature in one pass: drop the class token, pixel_shuffle(scale 0.5) and mlp1[0] = LayerNorm(4*D).
 * X: bf16 [B][1 + g*g][D] (row stride ldx, sample stride x_batch_stride, elements), the tower's output on a g x g grid, g even.
 * Output row b*(g/2)^2 + t, gathered column c4 in [0, 4*D):
 *   x[c4] = X[b][1 + (2*r' + c4 / (2*D)) * g + 2*q' + (c4 % (2*D)) / D][c4 % D]
 * with t = r'*(g/2) + q' for ps_version 'v2' (v1 == 0) and t = q'*(g/2) + r' for 'v1' (v1 != 0): the four D-wide chunks of a row come
 * from the tokens (2r' + dr, 2q' + dq), (dr, dq) = (0,0), (0,1), (1,0), (1,1).  Then, over the 4*D gathered values, in f32 with the
 * row in registers: mean, variance about the mean (two passes), rstd = rsqrtf(var + eps), and
 *   Y[row][c4] = bf16( (x - mean) * rstd * weight[c4] + bias[c4] )        one rounding
 * -- x2i_ln_affine_bf16 over the gathered row, bit for bit (the same lane-to-column map and summation order).
 * Y: bf16 rows of ldy elements; columns < 4*D of the B*(g/2)^2 rows are written, nothing else.  Every input element of rows >= 1 is read
 * once; the class row (row 0 of a sample) is never read.  weight, bias: bf16 [4*D].
 * Needs B >= 1, g >= 2 and even, D % 8 == 0, 4*D <= 4096 (x2i_ln_affine_bf16's limit), ldx % 8 == 0, ldx >= D, x_batch_stride % 8 == 0,
 * x_batch_stride >= (1 + g*g)*ldx, ldy % 8 == 0, ldy >= 4*D and 16-byte aligned X, Y, weight and bias. */
int x2i_internvit_shuffle_ln_bf16(const void* X, int64_t x_batch_stride, int64_t ldx, void* Y, int64_t ldy, const void* weight,
                                  const void* bias, int32_t B, int32_t g, int32_t D, float eps, int32_t v1, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
