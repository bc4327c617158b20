// The InternVL2.5 InternViT vision tower's kernels (include/x2i_internvit.h): the NCHW tiles as rows of the patch embedding's GEMM, the class
// token and the position table added in place behind that GEMM, and the head of extract_feature -- class token dropped, pixel_shuffle(0.5),
// LayerNorm over the four tokens' channels -- in one pass.  They stand behind InternVisionEmbeddings and the chat model's pixel_shuffle /
// mlp1[0].  Memory-bound row kernels, bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_internvit.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- patch rows
// patch_rows_body (encoder_common.h) on the gh x gw grid of a tile
__global__ __launch_bounds__(256) void internvit_patch_rows_kernel(const bf16_t* __restrict__ img, long long ibs, long long ics, long long ild,
                                                                   bf16_t* __restrict__ Xp, long long ldx, long long rows, int L, int gw, int P,
                                                                   int Kp) {
  patch_rows_body(img, ibs, ics, ild, Xp, ldx, rows, L, gw, P, Kp);
}

// ------------------------------------------------------------------------------------------------------------------- embeddings
// One thread per 16-byte chunk of X [B][1+L][D].  Row 0 of a sample is class + pos[0] (X is not read there); row 1+p adds pos[1+p] to
// what the patch embedding's GEMM left: one f32 add and one rounding either way.
__global__ __launch_bounds__(256) void internvit_embed_kernel(bf16_t* __restrict__ X, const bf16_t* __restrict__ cls, const bf16_t* __restrict__ pos,
                                                              long long rows, int S, int D) {
  const int nc = D >> 3;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    const int s = (int)(row % S);
    bf16_t* x = X + row * D + c * 8;
    float a[8], p[8];
    unpack8(*(const uint4*)(s ? x : cls + c * 8), a);
    unpack8(*(const uint4*)(pos + (long long)s * D + c * 8), p);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) o[j >> 1] = pack_bf16x2(__fadd_rn(a[j], p[j]), __fadd_rn(a[j + 1], p[j + 1]));
    *(uint4*)x = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------- shuffle + LayerNorm
// A wave per OUTPUT row of 4*D values, four rows per workgroup, the row in registers: ln_kernel<true> of elementwise.hip (what stands behind
// x2i_ln_affine_bf16) with the loads redirected.  Chunk c = lane + 64 i of the row lies inside one of the four D-wide pieces (D % 8 == 0);
// piece k = 2 dr + dq comes from token (2r' + dr, 2q' + dq) of the g x g grid, behind the class row.  The lane-to-column map, the order of
// the sums and the expression of the output are ln_kernel's, so the two agree bit for bit.
constexpr int SLN_MAXV = 8;  // up to 4*D = 4096

__global__ __launch_bounds__(256) void internvit_shuffle_ln_kernel(const bf16_t* __restrict__ X, long long xbs, long long ldx, bf16_t* __restrict__ Y,
                                                                   long long ldy, const bf16_t* __restrict__ aw, const bf16_t* __restrict__ ab,
                                                                   long long rows, int g, int D, float eps, int v1) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int g2 = g >> 1, T = g2 * g2;
  const long long b = row / T;
  const int t = (int)(row - b * T);
  const int hi = t / g2, lo = t - hi * g2;
  const int rr = v1 ? lo : hi, qq = v1 ? hi : lo;     // t = r' g/2 + q' (v2), t = q' g/2 + r' (v1)
  const bf16_t* x = X + b * xbs + (1 + (long long)(2 * rr) * g + 2 * qq) * ldx;   // token (2r', 2q'), behind the class row
  bf16_t* y = Y + row * ldy;
  const int D4 = 4 * D;
  const int nv = D4 >> 3;  // 16-byte chunks per output row
  float v[SLN_MAXV][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < SLN_MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      const int col = c * 8;
      const int k = col / D;
      const bf16_t* src = x + ((long long)(k >> 1) * g + (k & 1)) * ldx + (col - k * D);
      unpack8(*(const uint4*)src, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  const float mean = wave_sum(sum) / (float)D4;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < SLN_MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = __fsub_rn(v[i][j], mean);
        sq = __builtin_fmaf(d, d, sq);
      }
    }
  }
  const float rstd = rsqrtf(__fadd_rn(wave_sum(sq) / (float)D4, eps));
#pragma unroll
  for (int i = 0; i < SLN_MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      float w[8], bb[8], o[8];
      unpack8(*(const uint4*)(aw + c * 8), w);
      unpack8(*(const uint4*)(ab + c * 8), bb);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * w[j] + bb[j];
      *(uint4*)(y + c * 8) = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
    }
  }
}

}  // namespace

extern "C" {

int x2i_internvit_patch_rows_bf16(const void* img, int64_t img_batch_stride, int64_t img_chan_stride, int64_t img_ld, void* Xp, int64_t ldx,
                                  int32_t B, int32_t gh, int32_t gw, int32_t P, int32_t Kp, x2i_stream_t stream) {
  if (!img || !Xp) return x2i_set_error(X2I_ERR_ARG, "internvit_patch_rows: null pointer");
  if (B <= 0 || gh <= 0 || gw <= 0 || P < 1 || P > 32 || (long long)B * gh * gw > 0x7fffffffLL)
    return x2i_set_error(X2I_ERR_SHAPE, "internvit_patch_rows: bad shape (B=%d gh=%d gw=%d P=%d; P in 1..32, B*gh*gw < 2^31)", B, gh, gw, P);
  if (Kp <= 0 || Kp % 8 || Kp < 3 * P * P)
    return x2i_set_error(X2I_ERR_SHAPE, "internvit_patch_rows: Kp=%d must be a multiple of 8 and >= 3*P*P = %d", Kp, 3 * P * P);
  if (img_ld < (long long)gw * P || img_chan_stride < (long long)gh * P * img_ld || img_batch_stride < 3 * img_chan_stride)
    return x2i_set_error(X2I_ERR_SHAPE,
                         "internvit_patch_rows: img_ld must be >= gw*P = %lld, img_chan_stride >= gh*P*img_ld and img_batch_stride >= 3*img_chan_stride",
                         (long long)gw * P);
  if (ldx < Kp || ldx % 8 || !al16(Xp) || (((uintptr_t)img) & 1))
    return x2i_set_error(X2I_ERR_ALIGN, "internvit_patch_rows: ldx must be a multiple of 8 and >= Kp, Xp 16-byte aligned, img 2-byte aligned");
  const int L = gh * gw;
  const long long rows = (long long)B * L;
  hipLaunchKernelGGL(internvit_patch_rows_kernel, dim3(chunk_blocks(rows * (Kp / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)img,
                     (long long)img_batch_stride, (long long)img_chan_stride, (long long)img_ld, (bf16_t*)Xp, (long long)ldx, rows, L, gw, P, Kp);
  return x2i_check_launch("internvit_patch_rows");
}

int x2i_internvit_embed_bf16(void* X, const void* cls, const void* pos, int32_t B, int32_t L, int32_t D, x2i_stream_t stream) {
  if (!X || !cls || !pos) return x2i_set_error(X2I_ERR_ARG, "internvit_embed: null pointer");
  if (B <= 0 || L <= 0 || D <= 0 || D % 8 || L == 0x7fffffff)
    return x2i_set_error(X2I_ERR_SHAPE, "internvit_embed: D=%d must be a positive multiple of 8 (B=%d L=%d)", D, B, L);
  if (!al16(X) || !al16(cls) || !al16(pos)) return x2i_set_error(X2I_ERR_ALIGN, "internvit_embed: X, cls and pos must be 16-byte aligned");
  const long long rows = (long long)B * (L + 1);
  hipLaunchKernelGGL(internvit_embed_kernel, dim3(chunk_blocks(rows * (D / 8))), dim3(256), 0, (hipStream_t)stream, (bf16_t*)X, (const bf16_t*)cls,
                     (const bf16_t*)pos, rows, L + 1, D);
  return x2i_check_launch("internvit_embed");
}

int x2i_internvit_shuffle_ln_bf16(const void* X, int64_t x_batch_stride, int64_t ldx, void* Y, int64_t ldy, const void* weight,
                                  const void* bias, int32_t B, int32_t g, int32_t D, float eps, int32_t v1, x2i_stream_t stream) {
  if (!X || !Y || !weight || !bias) return x2i_set_error(X2I_ERR_ARG, "internvit_shuffle_ln: null pointer");
  if (B <= 0 || g < 2 || g % 2 || g > 32766) return x2i_set_error(X2I_ERR_SHAPE, "internvit_shuffle_ln: the grid g=%d must be even and >= 2 (B=%d)", g, B);
  if (D <= 0 || D % 8 || 4 * (long long)D > 64 * 8 * SLN_MAXV)
    return x2i_set_error(X2I_ERR_SHAPE, "internvit_shuffle_ln: D=%d must be a positive multiple of 8 with 4*D <= %d", D, 64 * 8 * SLN_MAXV);
  if (ldx < D || ldx % 8 || x_batch_stride % 8 || x_batch_stride < (1 + (long long)g * g) * ldx || ldy < 4 * D || ldy % 8)
    return x2i_set_error(X2I_ERR_SHAPE,
                         "internvit_shuffle_ln: ldx must be a multiple of 8 and >= D, x_batch_stride a multiple of 8 and >= (1+g*g)*ldx, ldy a "
                         "multiple of 8 and >= 4*D");
  if (!al16(X) || !al16(Y) || !al16(weight) || !al16(bias))
    return x2i_set_error(X2I_ERR_ALIGN, "internvit_shuffle_ln: X, Y, weight and bias must be 16-byte aligned");
  const long long rows = (long long)B * (g / 2) * (g / 2);
  if ((rows + 3) / 4 > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "internvit_shuffle_ln: too many rows (B=%d g=%d)", B, g);
  hipLaunchKernelGGL(internvit_shuffle_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X,
                     (long long)x_batch_stride, (long long)ldx, (bf16_t*)Y, (long long)ldy, (const bf16_t*)weight, (const bf16_t*)bias, rows, g, D, eps,
                     v1);
  return x2i_check_launch("internvit_shuffle_ln");
}

}  // extern "C"
