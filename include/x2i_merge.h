/* x2i_merge.h -- extension header of libx2i_hip.so: the prompt merge in front of the Qwen2 decoder stack (csrc/merge.hip).
 *
 * The conventions are those of x2i.h and the other extension headers (device pointers owned by the caller, raw bf16 storage, `stream` a
 * hipStream_t passed as void* and the last argument, work enqueued and never synchronised, no allocation, 0 or a negative X2I_ERR_*
 * code with the message in x2i_last_error(); every argument is validated before any launch).  The binding is
 * x2i_amd/merge_ops.py, the host modules x2i_amd/merge.py (MergePlan) and x2i_amd/qwen.py (Qwen2DecoderStack's `merge=`).
 *
 * Two entry points build layer 0's input of a multimodal prompt where it is consumed: the rows of the token table, with the rows of up
 * to two feature arrays (vision, audio) in the places the prompt reserves for them, written straight into entry 0 of the decoder's
 * [B, C, S, H] slab.  Which row goes where is a device vector `src` of one int32 per prompt row; x2i_merge_rank_i32 builds it from the
 * ids for models that mark the places by a placeholder token (InternVL), the host builds it from bound lists otherwise (MiniCPM-o).
 * No workgroup waits on another: there is no spin, no arrival counter and no atomic.  The rank is two launches, the per-chunk counts
 * of the first read by the second; the error flag of the merge is only ever stored to, with the one value 1.
 */
#ifndef X2I_MERGE_H
#define X2I_MERGE_H
#include "x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Rows per workgroup of both rank launches (four waves of eight 64-row steps), whatever n or the device. */
#define X2I_MERGE_RANK_CHUNK 2048

/* int32 elements of the rank's workspace: one count per chunk. */
#define X2I_MERGE_RANK_WS_INTS(n) (((int64_t)(n) + X2I_MERGE_RANK_CHUNK - 1) / X2I_MERGE_RANK_CHUNK)

/* What an element of `src` says.  Negative: the row comes from the token table.  Otherwise bit 30 (X2I_MERGE_SRC_ARRAY_BIT) picks the
 * feature array -- 0: feat0, 1: feat1 -- and bits 0..29 (X2I_MERGE_SRC_ROW_MASK) are the row inside it. */
#define X2I_MERGE_SRC_ARRAY_BIT 30
#define X2I_MERGE_SRC_ROW_MASK 0x3fffffff

/* The exclusive rank of every placeholder row:
 *   src[r] = #{r' < r : ids[r'] == placeholder}   when ids[r] == placeholder
 *   src[r] = -1                                    otherwise
 *   *total = #{r : ids[r] == placeholder}
 * ids: int64 [n], the flattened [B, S] rows of a prompt batch -- the row order of `input_embeds[selected] = vit_embeds.reshape(-1, C)`;
 * src: int32 [n]; total: device int32.  The ranks count into feature array 0 (bit 30 clear).
 * Two launches of ceil(n / X2I_MERGE_RANK_CHUNK) workgroups: the first leaves every chunk's count in ws, the second adds the counts of
 * the chunks before its own and ranks its rows by ballot and popcount inside each wave; the last chunk's workgroup writes *total.
 * ws: int32, ws_ints >= X2I_MERGE_RANK_WS_INTS(n) elements, contents irrelevant before.
 * Needs 1 <= n <= 2^24 (a prompt batch is at most 8 x 32768 rows; every rank then has bit 30 clear), 8-byte aligned ids, 4-byte aligned src, total and ws. */
int x2i_merge_rank_i32(const int64_t* ids, int64_t n, int64_t placeholder, int32_t* src, int32_t* total, int32_t* ws, int64_t ws_ints,
                       x2i_stream_t stream);

/* The merged rows of a [B, S] prompt, row r = b * S + s, H bf16 elements each:
 *   out[b][s] = feat_a[k]                    when src[r] >= 0, a = bit 30 of src[r], k = its bits 0..29: copied bit for bit
 *   out[b][s] = bf16(scale * table[ids[r]])  when src[r] < 0: one f32 multiply, one rounding (torch's bf16 tensor * Python float);
 *                                            with scale == 1 the row is copied bit for bit
 * out[b][s] starts b * out_batch_stride + s * ldo elements into `out`, so that out can be entry 0 of a [B, C, S, H] slab (ldo = H,
 * out_batch_stride = C * S * H); table: bf16 [V] rows (row stride ldt); feat0 / feat1: bf16 [n0] / [n1] rows (row strides ldf0, ldf1),
 * NULL with a count of 0 when there is no such array; ids: int64 [B * S]; src: int32 [B * S], or NULL: every row is a table row.
 * Overwrite mode: with table == NULL (ids may be NULL too) rows with src[r] < 0 are not touched at all; src is then required.
 * ids and src are device data and checked by the kernel: a table row with ids[r] outside [0, V), and a feature row with k >= the
 * array's count, are written as H zeros, and 1 is stored to *err (device int32; the call never clears it: zero it before, read it
 * whenever convenient).  Nothing outside the table and the feature arrays is read, nothing outside columns < H of the B * S rows is written.
 * One thread per 16-byte piece of a row, 16-byte loads and stores, ceil(B * S * H / 8 / 256) workgroups.
 * Needs B, S > 0, B * S <= 2^30, H > 0, H % 8 == 0, V > 0 with a table, n0, n1 in [0, 2^30], every row stride a multiple of 8 and >= H,
 * out_batch_stride a multiple of 8 and (B > 1) >= (S - 1) * ldo + H, a finite scale, 16-byte aligned table, feat0, feat1 and out, 8-byte
 * aligned ids, 4-byte aligned src and err. */
int x2i_embed_merge_bf16(const int64_t* ids, const int32_t* src, const void* table, int64_t ldt, int32_t V, float scale, const void* feat0,
                         int64_t ldf0, int32_t n0, const void* feat1, int64_t ldf1, int32_t n1, void* out, int64_t ldo, int64_t out_batch_stride,
                         int32_t* err, int32_t B, int32_t S, int32_t H, x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
