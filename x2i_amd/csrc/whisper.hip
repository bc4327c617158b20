// The MiniCPM-o Whisper audio tower's kernels (include/x2i_whisper.h): the windows of the Conv1d stem's first convolution as the rows of a
// GEMM, and the average pooling over time of the projector's tail.  They stand at the two ends of the audio path behind `model.apm`,
// `audio_projection_layer` and `audio_avg_pooler`; everything between them runs on the GEMM, layer-norm, head-split and attention entry
// points that exist.  Memory-bound row kernels, bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_whisper.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- mel rows
// A transposing gather: mel is contiguous along t, Xr along (ci, k).  One workgroup per (MT time steps, MC channels, sample).  The
// (channel, time) tile, with one time step of halo on either side, goes through LDS: it is read from mel coalesced along t (2-byte
// elements: the start of a mel window is only 2-byte aligned) and leaves as 16-byte pieces of Xr rows.  MC channels are 3 * MC = 96
// columns, twelve whole pieces, so a piece never straddles two workgroups; the workgroup of the last channel tile also writes the
// zero columns 3*Cin .. Kp-1.
// LDS: the tile's pitch is MT + 2 = 66 elements = 33 dwords, odd, and on the way out consecutive lanes take consecutive PIECES of one
// row (192 contiguous bytes of Xr per 12 lanes): a piece's eight elements are [ci][t + k] for 8/3 channels, and neighbouring lanes are
// 8/3 channels = 88 dwords apart, so the lanes of a row spread over the banks; lanes of the next row read the neighbouring element.
constexpr int MT = 64, MC = 32, MPITCH = MT + 2;

__global__ __launch_bounds__(256) void whisper_mel_rows_kernel(const bf16_t* __restrict__ mel, long long mbs, long long mld,
                                                               bf16_t* __restrict__ Xr, long long ldx, int Cin, int T, int Kp) {
  __shared__ bf16_t tile[MC * MPITCH];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * MT, c0 = blockIdx.y * MC, b = blockIdx.z;
  const bf16_t* src = mel + (long long)b * mbs;
  for (int i = tid; i < MC * MPITCH; i += 256) {
    const int ci = i / MPITCH, tl = i - ci * MPITCH;
    const int t = t0 + tl - 1;
    tile[i] = (c0 + ci < Cin && t >= 0 && t < T) ? src[(long long)(c0 + ci) * mld + t] : (bf16_t)0;
  }
  __syncthreads();
  const int K3 = 3 * Cin, col0 = 3 * c0;
  const int col_end = blockIdx.y == gridDim.y - 1 ? Kp : col0 + 3 * MC;
  const int nch = (col_end - col0) >> 3;
  for (int i = tid; i < MT * nch; i += 256) {
    const int tl = i / nch, ch = i - tl * nch;
    const int t = t0 + tl;
    if (t >= T) continue;
    int col = col0 + ch * 8;
    int ci = (ch * 8) / 3;
    int k = ch * 8 - ci * 3;
    bf16_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j, ++col) {
      e[j] = col < K3 ? tile[(ci < MC ? ci : 0) * MPITCH + tl + k] : (bf16_t)0;
      if (++k == 3) { k = 0; ++ci; }
    }
    *(uint4*)(Xr + ((long long)b * T + t) * ldx + col0 + ch * 8) =
        make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16));
  }
}

// ------------------------------------------------------------------------------------------------------------------- pool rows
// One thread per 16-byte chunk of Y: the k rows of X are summed in f32 in index order, divided once and rounded once.
__global__ __launch_bounds__(256) void whisper_pool_rows_kernel(const bf16_t* __restrict__ X, long long xbs, long long ldx, bf16_t* __restrict__ Y,
                                                                long long ybs, long long ldy, long long rows, int n_out, int D, int k) {
  const int nc = D >> 3;
  const long long total = rows * nc;
  const float kf = (float)k;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    const long long b = row / n_out;
    const int j = (int)(row - b * n_out);
    const bf16_t* x = X + b * xbs + (long long)k * j * ldx + c * 8;
    float acc[8], v[8];
    unpack8(*(const uint4*)x, acc);
    for (int r = 1; r < k; ++r) {
      unpack8(*(const uint4*)(x + r * ldx), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = __fadd_rn(acc[e], v[e]);
    }
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 8; e += 2) o[e >> 1] = pack_bf16x2(__fdiv_rn(acc[e], kf), __fdiv_rn(acc[e + 1], kf));
    *(uint4*)(Y + b * ybs + j * ldy + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace

extern "C" {

int x2i_whisper_mel_rows_bf16(const void* mel, int64_t mel_batch_stride, int64_t mel_ld, void* Xr, int64_t ldx, int32_t B, int32_t Cin, int32_t T,
                              int32_t Kp, x2i_stream_t stream) {
  if (!mel || !Xr) return x2i_set_error(X2I_ERR_ARG, "whisper_mel_rows: null pointer");
  if (B <= 0 || Cin <= 0 || T <= 0 || B > 65535 || Cin > 32 * 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "whisper_mel_rows: bad shape (B=%d Cin=%d T=%d; B <= 65535)", B, Cin, T);
  if (Kp <= 0 || Kp % 8 || Kp < 3LL * Cin)
    return x2i_set_error(X2I_ERR_SHAPE, "whisper_mel_rows: Kp=%d must be a multiple of 8 and >= 3*Cin = %lld", Kp, 3LL * Cin);
  if (mel_ld < T || mel_batch_stride < (long long)Cin * mel_ld)
    return x2i_set_error(X2I_ERR_SHAPE, "whisper_mel_rows: mel_ld must be >= T = %d and mel_batch_stride >= Cin*mel_ld", T);
  if (ldx < Kp || ldx % 8 || !al16(Xr) || (((uintptr_t)mel) & 1))
    return x2i_set_error(X2I_ERR_ALIGN, "whisper_mel_rows: ldx must be a multiple of 8 and >= Kp, Xr 16-byte aligned, mel 2-byte aligned");
  hipLaunchKernelGGL(whisper_mel_rows_kernel, dim3((T + MT - 1) / MT, (Cin + MC - 1) / MC, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)mel,
                     (long long)mel_batch_stride, (long long)mel_ld, (bf16_t*)Xr, (long long)ldx, Cin, T, Kp);
  return x2i_check_launch("whisper_mel_rows");
}

int x2i_whisper_pool_rows_bf16(const void* X, int64_t x_batch_stride, int64_t ldx, void* Y, int64_t y_batch_stride, int64_t ldy, int32_t B, int32_t S,
                               int32_t D, int32_t k, x2i_stream_t stream) {
  if (!X || !Y) return x2i_set_error(X2I_ERR_ARG, "whisper_pool_rows: null pointer");
  if (B <= 0 || k < 1 || k > 8 || S < k || D <= 0 || D % 8)
    return x2i_set_error(X2I_ERR_SHAPE, "whisper_pool_rows: bad shape (B=%d S=%d D=%d k=%d; k in 1..8, S >= k, D a multiple of 8)", B, S, D, k);
  const int n_out = (S - k) / k + 1;
  if (ldx < D || ldx % 8 || ldy < D || ldy % 8 || x_batch_stride % 8 || y_batch_stride % 8 || x_batch_stride < (long long)S * ldx ||
      y_batch_stride < (long long)n_out * ldy || !al16(X) || !al16(Y))
    return x2i_set_error(X2I_ERR_ALIGN, "whisper_pool_rows: ldx, ldy must be multiples of 8 and >= D, the batch strides multiples of 8 that hold S rows "
                                        "of X and (S - k) / k + 1 = %d rows of Y, X and Y 16-byte aligned", n_out);
  const long long rows = (long long)B * n_out;
  hipLaunchKernelGGL(whisper_pool_rows_kernel, dim3(chunk_blocks(rows * (D / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X,
                     (long long)x_batch_stride, (long long)ldx, (bf16_t*)Y, (long long)y_batch_stride, (long long)ldy, rows, n_out, D, k);
  return x2i_check_launch("whisper_pool_rows");
}

}  // extern "C"
