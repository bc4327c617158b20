// The MiniCPM-o SigLIP (NaViT) vision tower's kernels (include/x2i_siglip.h): the pixel strips as rows of the patch embedding's GEMM, the
// bucketised position embedding added in place, and the head split for heads stored as x2i_vit_attention_bf16 reads them.  They stand
// behind SiglipVisionEmbeddings and SiglipAttention's head reshape of the tower behind `model.vpm` (`transformers`'
// Idefics2VisionTransformer is the same module).  Memory-bound row kernels, bf16 in and out, f32 arithmetic; every launcher enqueues on
// the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_siglip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- patch rows
// patch_rows_body (encoder_common.h) on a grid of one row of L patches: column ci*P*P + r*P + c of row b*L + p is strips[b][ci][r][P*p + c]
__global__ __launch_bounds__(256) void siglip_patch_rows_kernel(const bf16_t* __restrict__ strips, long long sbs, long long sld,
                                                                bf16_t* __restrict__ Xp, long long ldx, long long rows, int L, int P, int Kp) {
  patch_rows_body(strips, sbs, P * sld, sld, Xp, ldx, rows, L, L, P, Kp);
}

// ------------------------------------------------------------------------------------------------------------------- position embedding
// One thread per 16-byte chunk of X.  An id outside [0, n_pos) is clamped: the host cannot see it, and no launch reads out of bounds.
__global__ __launch_bounds__(256) void siglip_add_positions_kernel(bf16_t* __restrict__ X, long long ldx, const int* __restrict__ ids,
                                                                   const bf16_t* __restrict__ pos, int n_pos, long long rows, int D) {
  const int nc = D >> 3;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= n_pos ? n_pos - 1 : id);
    bf16_t* x = X + row * ldx + c * 8;
    float a[8], p[8];
    unpack8(*(const uint4*)x, a);
    unpack8(*(const uint4*)(pos + (long long)id * D + c * 8), p);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) o[j >> 1] = pack_bf16x2(__fadd_rn(a[j], p[j]), __fadd_rn(a[j + 1], p[j + 1]));
    *(uint4*)x = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------- head split
// head_split_body (encoder_common.h) with heads stored dkp >= dk wide, as x2i_vit_attention_bf16 reads them
__global__ __launch_bounds__(256) void siglip_head_split_kernel(const bf16_t* __restrict__ qkv, long long ld, bf16_t* __restrict__ Q,
                                                                bf16_t* __restrict__ K, bf16_t* __restrict__ VT, int S, int Spad, int H, int dk,
                                                                int dkp) {
  head_split_body(qkv, ld, Q, K, VT, S, Spad, H, dk, dkp);
}

}  // namespace

extern "C" {

int x2i_siglip_patch_rows_bf16(const void* strips, int64_t strip_batch_stride, int64_t strip_ld, void* Xp, int64_t ldx, int32_t B, int32_t L,
                               int32_t P, int32_t Kp, x2i_stream_t stream) {
  if (!strips || !Xp) return x2i_set_error(X2I_ERR_ARG, "siglip_patch_rows: null pointer");
  if (B <= 0 || L <= 0 || P < 1 || P > 32) return x2i_set_error(X2I_ERR_SHAPE, "siglip_patch_rows: bad shape (B=%d L=%d P=%d; P in 1..32)", B, L, P);
  if (Kp <= 0 || Kp % 8 || Kp < 3 * P * P)
    return x2i_set_error(X2I_ERR_SHAPE, "siglip_patch_rows: Kp=%d must be a multiple of 8 and >= 3*P*P = %d", Kp, 3 * P * P);
  if (strip_ld < (long long)P * L || strip_batch_stride < 3LL * P * strip_ld)
    return x2i_set_error(X2I_ERR_SHAPE, "siglip_patch_rows: strip_ld must be >= P*L = %lld and strip_batch_stride >= 3*P*strip_ld", (long long)P * L);
  if (ldx < Kp || ldx % 8 || !al16(Xp) || (((uintptr_t)strips) & 1))
    return x2i_set_error(X2I_ERR_ALIGN, "siglip_patch_rows: ldx must be a multiple of 8 and >= Kp, Xp 16-byte aligned, strips 2-byte aligned");
  const long long rows = (long long)B * L;
  hipLaunchKernelGGL(siglip_patch_rows_kernel, dim3(chunk_blocks(rows * (Kp / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)strips,
                     (long long)strip_batch_stride, (long long)strip_ld, (bf16_t*)Xp, (long long)ldx, rows, L, P, Kp);
  return x2i_check_launch("siglip_patch_rows");
}

int x2i_siglip_add_positions_bf16(void* X, int64_t ldx, const int32_t* ids, const void* pos, int32_t n_pos, int64_t rows, int32_t D,
                                  x2i_stream_t stream) {
  if (!X || !ids || !pos) return x2i_set_error(X2I_ERR_ARG, "siglip_add_positions: null pointer");
  if (rows <= 0 || n_pos <= 0 || D <= 0 || D % 8)
    return x2i_set_error(X2I_ERR_SHAPE, "siglip_add_positions: D=%d must be a positive multiple of 8 (rows=%lld n_pos=%d)", D, (long long)rows, n_pos);
  if (ldx < D || ldx % 8 || !al16(X) || !al16(pos) || (((uintptr_t)ids) & 3))
    return x2i_set_error(X2I_ERR_ALIGN, "siglip_add_positions: ldx must be a multiple of 8 and >= D, X and pos 16-byte aligned, ids 4-byte aligned");
  hipLaunchKernelGGL(siglip_add_positions_kernel, dim3(chunk_blocks((long long)rows * (D / 8))), dim3(256), 0, (hipStream_t)stream, (bf16_t*)X,
                     (long long)ldx, (const int*)ids, (const bf16_t*)pos, n_pos, (long long)rows, D);
  return x2i_check_launch("siglip_add_positions");
}

int x2i_siglip_head_split_bf16(const void* qkv, int64_t ld, void* Q, void* K, void* VT, int32_t B, int32_t S, int32_t Spad, int32_t H, int32_t dk,
                               x2i_stream_t stream) {
  if (!qkv || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "siglip_head_split: null pointer");
  if (dk != 64 && dk != 80 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "siglip_head_split: head width dk=%d is not one of 64, 80, 128", dk);
  if (B <= 0 || S <= 0 || H <= 0 || Spad < S || Spad % 8 || H > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "siglip_head_split: bad shape (B=%d S=%d Spad=%d H=%d)", B, S, Spad, H);
  if (ld < 3LL * H * dk || ld % 8 || !al16(qkv) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "siglip_head_split: ld must be a multiple of 8 and >= 3*H*dk, pointers 16-byte aligned");
  hipLaunchKernelGGL(siglip_head_split_kernel, dim3((S + 63) / 64, H, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld,
                     (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, S, Spad, H, dk, stored_width(dk));
  return x2i_check_launch("siglip_head_split");
}

}  // extern "C"
