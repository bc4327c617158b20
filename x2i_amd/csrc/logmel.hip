// The Whisper log-mel front end (include/ext/x2i_logmel.h): a 16 kHz waveform to the features WhisperFeatureExtractor computes on the
// host -- frames of 400 samples every 160, a Hann window, a 201-bin power spectrum, the mel filter bank, log10 with a floor, the clamp at
// the chunk's maximum minus 8.  Two launches: the spectrum (all the FLOPs, and the per-workgroup maxima) and the finish (the maximum,
// the clamp, the padding zeros, the output type).  Everything is f32; every launcher enqueues on the caller's stream and returns.
#include "x2i_common.h"
#include "../../include/ext/x2i_logmel.h"

namespace {

constexpr int NFFT = 400, HOP = 160, FT = 32;             // FT: frames per workgroup, one 32-row tile of the f32 matrix instruction
constexpr int DFT_LD = 448, DFT_TILES = 7;                // 7 tiles of 32 bins, cos | sin side by side: 64 columns per tile
constexpr int FB_ROWS = 224, FB_LD = 128;
constexpr int NS = (FT - 1) * HOP + NFFT;                 // 5360 samples hold a workgroup's 32 overlapping frames
constexpr int S_WORDS = NS + NS / HOP + 1;
constexpr int P_LD = FB_ROWS + 1;
constexpr float LG_FLOOR = -10.f, MEL_FLOOR = 1e-10f;

__device__ __forceinline__ int clamp_count(int n, int N_max) { return n < 0 ? 0 : (n < N_max ? n : N_max); }
// A_b: the frames that can see a non-zero sample (frame t starts at 160 t - 200)
__device__ __forceinline__ int seen_frames(int n, int T) {
  const int a = (n + 199) / HOP + 1;
  return a < T ? a : T;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------------------------------------------------------- spectrum
// One workgroup (four waves) per 32 frames of one sample.  Both products are 32 x 32 x 2 f32-input MFMAs (exact f32, a k-ordered chain of
// fused multiply-adds):
//   DFT   [32 frames x 400 samples] x [400 x 448] (the window-folded table, from L2): wave w takes bin tiles w and w + 4; the cos and
//         the sin accumulator of a bin meet in one lane, so |X|^2 needs no exchange.  The 400 terms of a sum go to four chains of 100
//         (samples j with the same (j >> 1) & 3), added pairwise at the end: eight independent accumulators in flight, and a shorter
//         chain's rounding error.
//   mel   [n_mels x 224 bins] x [224 x 32 frames]: the filter bank is the A operand, so a result register holds 32 consecutive FRAMES
//         of one mel row and the stores to lg are 128 contiguous bytes.
// The frames overlap (400 samples every 160), so the workgroup stages their 5360 samples once, with the reflection and the zeros beyond
// n resolved on the way in.  Sample s sits at LDS word s + s / 160: the A operand reads one sample index of 32 consecutive frames, words
// 161 apart, which is odd -- 32 distinct banks (160 apart would be two).  The power spectrum goes through LDS [32 frames][225]: odd pitch,
// same reason.
__global__ __launch_bounds__(256) void logmel_spectrum_kernel(const float* __restrict__ wave, long long ldw, const int* __restrict__ nsamp,
                                                              const float* __restrict__ dft, const float* __restrict__ fbank,
                                                              float* __restrict__ lg, float* __restrict__ part, int N_max, int n_mels) {
  __shared__ float S[S_WORDS];
  __shared__ float P[FT * P_LD];
  __shared__ float wmax[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, t0 = blockIdx.x * FT, T = N_max / HOP;
  const int n = clamp_count(nsamp[b], N_max);
  if (t0 >= seen_frames(n, T)) return;                    // (uniform) frames of silence: exactly -10, never read by the finish
  const float* x = wave + (long long)b * ldw;
  const long long lim = n < ldw ? n : ldw;
  const int g0 = t0 * HOP - NFFT / 2;
  for (int s = tid; s < NS; s += 256) {
    int g = g0 + s;
    if (g < 0) g = -g;
    if (g >= N_max) g = 2 * (N_max - 1) - g;
    S[s + s / HOP] = (g >= 0 && g < lim) ? x[g] : 0.f;
  }
  __syncthreads();
  for (int q = w; q < DFT_TILES; q += 4) {
    f32x16_t re[4], im[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) re[c][i] = im[c][i] = 0.f;
    const float* tb = dft + 64 * q + r;
    for (int j0 = 0; j0 < NFFT; j0 += 8) {
      // lane (r, h) holds A[frame r][sample j0 + 2c + h] and B[sample j0 + 2c + h][bin 32 q + r]; j0 / 160 is the skew of all eight samples
      const float* sp = S + r * (HOP + 1) + j0 + j0 / HOP + h;
      const float* tp = tb + (j0 + h) * DFT_LD;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a = sp[2 * c];
        re[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tp[2 * c * DFT_LD], re[c], 0, 0, 0);
        im[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tp[2 * c * DFT_LD + 32], im[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h;     // the frame; the lane's column is bin 32 q + r
      const float xr = __fadd_rn(__fadd_rn(re[0][i], re[1][i]), __fadd_rn(re[2][i], re[3][i]));
      const float xi = __fadd_rn(__fadd_rn(im[0][i], im[1][i]), __fadd_rn(im[2][i], im[3][i]));
      P[row * P_LD + 32 * q + r] = __builtin_fmaf(xr, xr, __fmul_rn(xi, xi));
    }
  }
  __syncthreads();
  float mx = LG_FLOOR;
  if (32 * w < n_mels) {                                   // (uniform per wave) mel tile w
    f32x16_t acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][i] = acc[1][i] = 0.f;
    const float* fp = fbank + h * FB_LD + 32 * w + r;      // A[mel 32 w + r][bin k0 + h]
    const float* pp = P + r * P_LD + h;                    // B[bin k0 + h][frame r]
    for (int k0 = 0; k0 < FB_ROWS; k0 += 4) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fp[k0 * FB_LD], pp[k0], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fp[(k0 + 2) * FB_LD], pp[k0 + 2], acc[1], 0, 0, 0);
    }
    const int t = t0 + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = 32 * w + (i & 3) + 8 * (i >> 2) + 4 * h;
      const float v = __fadd_rn(acc[0][i], acc[1][i]);
      const float l = v > MEL_FLOOR ? fmaxf(log10f(v), LG_FLOOR) : LG_FLOOR;
      if (m < n_mels && t < T) {
        lg[((long long)b * n_mels + m) * T + t] = l;
        mx = fmaxf(mx, l);
      }
    }
  }
  mx = wave_max(mx);
  if (lane == 0) wmax[w] = mx;
  __syncthreads();
  if (tid == 0) part[(long long)b * gridDim.x + blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// ------------------------------------------------------------------------------------------------------------------- finish
// One workgroup per 256 output columns of one (sample, mel) row.  Each reduces the sample's partial maxima itself (at most 94 values, L2
// hits): max does not depend on the order, so every workgroup gets the same mx.
template <bool BF16>
__global__ __launch_bounds__(256) void logmel_finish_kernel(const float* __restrict__ lg, const float* __restrict__ part,
                                                            const int* __restrict__ nsamp, void* __restrict__ out, long long obs, long long old,
                                                            int N_max, int n_mels, int T_out) {
  __shared__ float wmax[4];
  const int tid = threadIdx.x, b = blockIdx.z, m = blockIdx.y, T = N_max / HOP, NB = (T + FT - 1) / FT;
  const int n = clamp_count(nsamp[b], N_max);
  const int nb = (seen_frames(n, T) + FT - 1) / FT;
  int L = (n + HOP - 1) / HOP;
  L = L < T ? L : T;
  float mx = LG_FLOOR;
  for (int i = tid; i < nb; i += 256) mx = fmaxf(mx, part[(long long)b * NB + i]);
  mx = wave_max(mx);
  if ((tid & 63) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  const float lo = __fsub_rn(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])), 8.f);
  const int t = blockIdx.x * 256 + tid;
  if (t >= T_out) return;
  float v = 0.f;                                           // the processor's pad_sequence value
  if (t < L) v = __fmul_rn(__fadd_rn(fmaxf(lg[((long long)b * n_mels + m) * T + t], lo), 4.f), 0.25f);
  const long long o = (long long)b * obs + (long long)m * old + t;
  if (BF16)
    ((bf16_t*)out)[o] = f32_to_bf16(v);
  else
    ((float*)out)[o] = v;
}

inline bool al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// The checks the two entry points share; T and NB on success
int check_shape(const char* what, int B, int N_max, int n_mels, long long lg_floats, long long part_floats, int* T, int* NB) {
  if (B <= 0 || B > 65535) return x2i_set_error(X2I_ERR_SHAPE, "%s: B=%d must be in 1..65535", what, B);
  if (N_max < 2 * HOP || N_max % HOP || N_max > (1 << 30))
    return x2i_set_error(X2I_ERR_SHAPE, "%s: N_max=%d must be a multiple of 160 in 320..2^30", what, N_max);
  if (n_mels < 1 || n_mels > FB_LD) return x2i_set_error(X2I_ERR_SHAPE, "%s: n_mels=%d must be in 1..128", what, n_mels);
  *T = N_max / HOP;
  *NB = (*T + FT - 1) / FT;
  if (lg_floats < (long long)B * n_mels * *T)
    return x2i_set_error(X2I_ERR_ARG, "%s: lg_floats=%lld, B * n_mels * (N_max / 160) = %lld are needed", what, lg_floats, (long long)B * n_mels * *T);
  if (part_floats < (long long)B * *NB)
    return x2i_set_error(X2I_ERR_ARG, "%s: part_floats=%lld, B * ((N_max / 160 + 31) / 32) = %lld are needed", what, part_floats, (long long)B * *NB);
  return 0;
}

}  // namespace

extern "C" {

int x2i_logmel_spectrum_f32(const void* wave, int64_t ldw, const void* n, const void* dft, const void* fbank, void* lg, int64_t lg_floats,
                            void* part, int64_t part_floats, int32_t B, int32_t N_max, int32_t n_mels, x2i_stream_t stream) {
  const char* what = "logmel_spectrum";
  if (!wave || !n || !dft || !fbank || !lg || !part) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", what);
  int T, NB;
  if (int rc = check_shape(what, B, N_max, n_mels, lg_floats, part_floats, &T, &NB)) return rc;
  if (ldw < 1) return x2i_set_error(X2I_ERR_SHAPE, "%s: ldw=%lld must be at least 1", what, (long long)ldw);
  if (!al4(wave) || !al4(n) || !al4(lg) || !al4(part) || !al16(dft) || !al16(fbank))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: wave, n, lg and part must be 4-byte aligned, dft and fbank 16-byte aligned", what);
  hipLaunchKernelGGL(logmel_spectrum_kernel, dim3(NB, B), dim3(256), 0, (hipStream_t)stream, (const float*)wave, (long long)ldw, (const int*)n,
                     (const float*)dft, (const float*)fbank, (float*)lg, (float*)part, N_max, n_mels);
  return x2i_check_launch(what);
}

int x2i_logmel_finish(const void* lg, int64_t lg_floats, const void* part, int64_t part_floats, const void* n, void* out,
                      int64_t out_batch_stride, int64_t out_ld, int32_t B, int32_t N_max, int32_t n_mels, int32_t T_out, int32_t out_bf16,
                      x2i_stream_t stream) {
  const char* what = "logmel_finish";
  if (!lg || !part || !n || !out) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", what);
  int T, NB;
  if (int rc = check_shape(what, B, N_max, n_mels, lg_floats, part_floats, &T, &NB)) return rc;
  if (T_out < 1 || out_ld < T_out || out_batch_stride < (long long)n_mels * out_ld)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: T_out=%d must be at least 1, out_ld=%lld >= T_out and out_batch_stride=%lld >= n_mels * out_ld", what,
                         T_out, (long long)out_ld, (long long)out_batch_stride);
  if (!al4(lg) || !al4(part) || !al4(n) || (((uintptr_t)out) & (out_bf16 ? 1 : 3)))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: lg, part and n must be 4-byte aligned, out aligned to its element size", what);
  const dim3 grid((T_out + 255) / 256, n_mels, B);
  if (out_bf16)
    hipLaunchKernelGGL(logmel_finish_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)lg, (const float*)part, (const int*)n, out,
                       (long long)out_batch_stride, (long long)out_ld, N_max, n_mels, T_out);
  else
    hipLaunchKernelGGL(logmel_finish_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)lg, (const float*)part, (const int*)n, out,
                       (long long)out_batch_stride, (long long)out_ld, N_max, n_mels, T_out);
  return x2i_check_launch(what);
}

}  // extern "C"
