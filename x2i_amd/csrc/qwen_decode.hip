// Qwen2 decoding with a key/value cache (include/x2i_qwen_decode.h): one token per sample through a layer against the cached keys and values.
//   decode_linear   the layer's projections at 1..8 rows: an HBM-streaming bf16 GEMV with the bias / residual / SwiGLU epilogues
//   rope_append     rotate-half RoPE on the new token's q and k, and the append of k and v at a slot read from device memory
//   attention       one query per head over the key range [k_lo, k_hi), cut into fixed chunks (partials), then the combine
// They stand behind `transformers`' Qwen2Attention with a DynamicCache and the nn.Linear modules of Qwen2DecoderLayer as
// `generate(use_cache=True)` runs them (the reference's infer/inference_qwenvl.py under --use_answer).  bf16 in and out, f32 arithmetic;
// every launcher enqueues on the caller's stream and returns.  Every per-step scalar comes from device memory: a captured step replays.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_qwen_decode.h"

namespace {

constexpr int CHUNK = X2I_QWEN_DECODE_CHUNK;
constexpr int MAXREP = 16;   // query heads per key/value head
static_assert(CHUNK == 256, "the attention kernel maps one thread to one key of a chunk and is launched with 256 threads");

// ------------------------------------------------------------------------------------------------------------------- linear
// 16 bytes that are read once: do not keep them in the caches
__device__ __forceinline__ uint4 load_stream16(const bf16_t* p) {
  return __builtin_bit_cast(uint4, __builtin_nontemporal_load((const bf16x8_t*)p));
}

// Y[b][n] = sum_k W[n][k] X[b][k] for NB rows b.  A wave owns R weight rows and streams them once, 16 bytes per lane and row, straight to
// registers (the weight is read once and shared with nobody: an LDS round trip would be overhead); the loads of 8 / R k-steps are issued
// together before their arithmetic, so eight loads (128 bytes) per lane are in flight.  X is staged once per workgroup in LDS as bf16 [NB][KC]
// (KC = K when that fits 64 KiB, else a multiple of 512 that does) and read back 16 bytes per lane, conflict-free.
// The arithmetic of one (row, sample): lane l sums k = 8 l + 512 i + j, i and j ascending, in ONE fma chain (the chunking of X does not
// change it: KC % 512 == 0), then the 64 lanes in wave_sum's tree.  Nothing of it depends on NB or R.
// MODE 1: the wave's R rows are R / 2 gate rows n and their up rows N + n; the epilogue writes silu(a) * b.
template <int NB, int R, int MODE>
__global__ __launch_bounds__(256) void decode_linear_kernel(const bf16_t* __restrict__ X, long long ldx, const bf16_t* __restrict__ W, long long ldw,
                                                            const bf16_t* __restrict__ bias, const bf16_t* res, long long ldr, bf16_t* Y,
                                                            long long ldy, int N, int K, int KC) {
  extern __shared__ __attribute__((aligned(16))) uint4 xs[];   // [NB][KC / 8]
  constexpr int RO = MODE ? R / 2 : R;                          // outputs per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * RO;                  // (a wave past N computes clamped rows and stores nothing: it still takes the barriers)
  const bf16_t* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int n = n0 + (r < RO ? r : r - RO);                   // clamp: outputs past N are computed and discarded
    wrow[r] = W + ((long long)(n < N ? n : N - 1) + (r < RO ? 0 : N)) * ldw;
  }
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int U = 8 / R;                                      // k-steps whose loads are issued together: eight 16-byte loads per lane in flight
  constexpr int NP = NB / 2;                                    // sample pairs: one packed fma (v_pk_fma_f32) carries two samples' chains
  f32x2 acc2[R][NP > 0 ? NP : 1];
  float acc1[R];                                                // the odd last sample
#pragma unroll
  for (int r = 0; r < R; ++r) {
    acc1[r] = 0.f;
#pragma unroll
    for (int q = 0; q < NP; ++q) acc2[r][q] = f32x2{0.f, 0.f};
  }
  const int kc8 = KC >> 3;
  for (int c0 = 0; c0 < K; c0 += KC) {
    const int kc = (K - c0) < KC ? (K - c0) : KC;
    const int n8 = kc >> 3;
    if (c0) __syncthreads();                                    // every wave is done with the chunk before
    for (int i = threadIdx.x; i < NB * n8; i += 256) {
      const int b = i / n8, j = i - b * n8;
      xs[b * kc8 + j] = *(const uint4*)(X + (long long)b * ldx + c0 + j * 8);
    }
    __syncthreads();
    for (int k = lane * 8; k < kc; k += 512 * U) {
      uint4 wv[U][R];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + 512 * u < kc) {
#pragma unroll
          for (int r = 0; r < R; ++r) wv[u][r] = load_stream16(wrow[r] + c0 + k + 512 * u);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k + 512 * u;
        if (kk < kc) {
          float wf[R][8];
#pragma unroll
          for (int r = 0; r < R; ++r) unpack8(wv[u][r], wf[r]);
          // explicit fma chains, k ascending: the arithmetic of one sample must not depend on how many samples share the launch (a packed
          // fma is two independent fmas)
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            float xa[8], xb[8];
            unpack8(xs[(2 * q) * kc8 + (kk >> 3)], xa);
            unpack8(xs[(2 * q + 1) * kc8 + (kk >> 3)], xb);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const f32x2 x2 = {xa[j], xb[j]};
#pragma unroll
              for (int r = 0; r < R; ++r) acc2[r][q] = __builtin_elementwise_fma(f32x2{wf[r][j], wf[r][j]}, x2, acc2[r][q]);
            }
          }
          if constexpr (NB & 1) {
            float xf[8];
            unpack8(xs[(NB - 1) * kc8 + (kk >> 3)], xf);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
              for (int j = 0; j < 8; ++j) acc1[r] = __builtin_fmaf(wf[r][j], xf[j], acc1[r]);
          }
        }
      }
    }
  }
  float acc[R][NB];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int q = 0; q < NP; ++q) { acc[r][2 * q] = acc2[r][q][0]; acc[r][2 * q + 1] = acc2[r][q][1]; }
    if constexpr (NB & 1) acc[r][NB - 1] = acc1[r];
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = wave_sum(acc[r][b]);
  if (lane != 0) return;
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    const int n = n0 + r;
    if (n >= N) break;
    if constexpr (MODE) {
      const float ba = bias ? bf16_to_f32(bias[n]) : 0.f, bb = bias ? bf16_to_f32(bias[N + n]) : 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b)
        Y[(long long)b * ldy + n] = f32_to_bf16(__fmul_rn(silu_f(__fadd_rn(acc[r][b], ba)), __fadd_rn(acc[r + RO][b], bb)));
    } else {
      const float bv = bias ? bf16_to_f32(bias[n]) : 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float v = __fadd_rn(acc[r][b], bv);
        if (res) v = __fadd_rn(v, bf16_to_f32(res[(long long)b * ldr + n]));
        Y[(long long)b * ldy + n] = f32_to_bf16(v);
      }
    }
  }
}

template <int NB, int R, int MODE>
void launch_decode_linear(const void* X, long long ldx, const void* W, long long ldw, const void* bias, const void* res, long long ldr, void* Y,
                          long long ldy, int N, int K, int KC, hipStream_t stream) {
  constexpr int RO = MODE ? R / 2 : R;
  const unsigned blocks = (unsigned)((N + 4 * RO - 1) / (4 * RO));
  hipLaunchKernelGGL((decode_linear_kernel<NB, R, MODE>), dim3(blocks), dim3(256), (size_t)NB * KC * 2, stream, (const bf16_t*)X, ldx,
                     (const bf16_t*)W, ldw, (const bf16_t*)bias, (const bf16_t*)res, ldr, (bf16_t*)Y, ldy, N, K, KC);
}

template <int NB>
void launch_decode_linear_nb(bool wide, int mode, const void* X, long long ldx, const void* W, long long ldw, const void* bias, const void* res,
                             long long ldr, void* Y, long long ldy, int N, int K, int KC, hipStream_t stream) {
  if (mode) {
    if (wide) launch_decode_linear<NB, 4, 1>(X, ldx, W, ldw, bias, res, ldr, Y, ldy, N, K, KC, stream);
    else launch_decode_linear<NB, 2, 1>(X, ldx, W, ldw, bias, res, ldr, Y, ldy, N, K, KC, stream);
  } else {
    if (wide) launch_decode_linear<NB, 4, 0>(X, ldx, W, ldw, bias, res, ldr, Y, ldy, N, K, KC, stream);
    else launch_decode_linear<NB, 2, 0>(X, ldx, W, ldw, bias, res, ldr, Y, ldy, N, K, KC, stream);
  }
}

// ------------------------------------------------------------------------------------------------------------------- RoPE + append
// grid (Hq + Hkv, B), 128 threads.  Threads < dk / 16 rotate eight pairs each (rope_split_body's arithmetic); on a key/value head threads
// < dk move one element of v into column slot[b] of V^T.
__global__ __launch_bounds__(128) void decode_rope_append_kernel(const bf16_t* __restrict__ qkv, long long ld, const float* __restrict__ cs,
                                                                 const float* __restrict__ sn, const int32_t* __restrict__ slot,
                                                                 bf16_t* __restrict__ Qd, bf16_t* __restrict__ K, bf16_t* __restrict__ VT, int Hq,
                                                                 int Hkv, int cap, int dk) {
  const int tid = threadIdx.x, hh = blockIdx.x, b = blockIdx.y;
  const int s = slot[b];
  if (s < 0 || s >= cap) return;   // (uniform across the workgroup)
  const bool is_q = hh < Hq;
  const int g = hh - Hq;
  const int half = dk >> 1;
  const bf16_t* row = qkv + (long long)b * ld;
  if (tid < (dk >> 4)) {
    const bf16_t* src = row + (long long)hh * dk + tid * 8;      // q heads, then k heads: column hh * dk either way
    const float* cp = cs + (long long)b * half + tid * 8;
    const float* sp = sn + (long long)b * half + tid * 8;
    float x1[8], x2[8];
    unpack8(*(const uint4*)src, x1);
    unpack8(*(const uint4*)(src + half), x2);
    const float4 c0 = *(const float4*)cp, c1 = *(const float4*)(cp + 4), t0 = *(const float4*)sp, t1 = *(const float4*)(sp + 4);
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float ss[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    uint32_t lo[4], up[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      lo[j >> 1] = pack_bf16x2(__fsub_rn(__fmul_rn(x1[j], cc[j]), __fmul_rn(x2[j], ss[j])),
                               __fsub_rn(__fmul_rn(x1[j + 1], cc[j + 1]), __fmul_rn(x2[j + 1], ss[j + 1])));
      up[j >> 1] = pack_bf16x2(__fadd_rn(__fmul_rn(x2[j], cc[j]), __fmul_rn(x1[j], ss[j])),
                               __fadd_rn(__fmul_rn(x2[j + 1], cc[j + 1]), __fmul_rn(x1[j + 1], ss[j + 1])));
    }
    bf16_t* dst = is_q ? Qd + ((long long)b * Hq + hh) * dk + tid * 8 : K + (((long long)b * Hkv + g) * cap + s) * dk + tid * 8;
    *(uint4*)dst = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *(uint4*)(dst + half) = make_uint4(up[0], up[1], up[2], up[3]);
  }
  if (!is_q && tid < dk) VT[(((long long)b * Hkv + g) * dk + tid) * cap + s] = row[(long long)(Hq + Hkv + g) * dk + tid];
}

// ------------------------------------------------------------------------------------------------------------------- attention
__device__ __forceinline__ void load_range(const int32_t* k_lo, const int32_t* k_hi, int b, int cap, int& lo, int& hi) {
  lo = k_lo[b];
  hi = k_hi[b];
  lo = lo < 0 ? 0 : (lo > cap ? cap : lo);
  hi = hi < 0 ? 0 : (hi > cap ? cap : hi);
}

// One chunk of one key/value head of one sample: grid (chunks, Hkv, B), 256 threads, thread t <-> key c * CHUNK + t.
//   scores   a thread holds its key's row in registers and walks the group's rep query heads (q as f32 in LDS, broadcast reads): one fma
//            chain in ascending d per (head, key); only keys inside [lo, hi) are read.
//   softmax  wave w takes heads w, w + 4, ..: maximum and sum over the keys that count (by index), p = exp2(s - m) rounded to bf16.
//   P V      thread <-> (d = t % DK, part = t / DK): the part's CHUNK * DK / 256 keys of V^T row d, eight at a time, against p from LDS
//            (broadcast: a wave lies inside one part); the parts are added in ascending order through LDS.
// A chunk with no key of the range writes nothing, and the combine does not read it.
template <int DK>
__global__ __launch_bounds__(256) void decode_attention_kernel(const bf16_t* __restrict__ Qd, const bf16_t* __restrict__ K, const bf16_t* __restrict__ VT,
                                                               const int32_t* __restrict__ k_lo, const int32_t* __restrict__ k_hi,
                                                               float* __restrict__ ws, int Hq, int Hkv, int cap, int nch, float scale_log2e) {
  constexpr int PARTS = 256 / DK, PK = CHUNK / PARTS;   // key parts of the P V step and keys per part
  __shared__ __attribute__((aligned(16))) float qs[MAXREP * DK];
  __shared__ __attribute__((aligned(16))) float ps[MAXREP * CHUNK];
  __shared__ __attribute__((aligned(16))) float red[PARTS * MAXREP * DK];
  __shared__ float ml[MAXREP][2];
  const int tid = threadIdx.x, c = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int rep = Hq / Hkv;
  int lo, hi;
  load_range(k_lo, k_hi, b, cap, lo, hi);
  const int j0 = c * CHUNK;
  if (hi <= lo || j0 >= hi || j0 + CHUNK <= lo) return;   // (uniform)
  const bf16_t* q = Qd + ((long long)b * Hq + (long long)g * rep) * DK;
  for (int i = tid; i < rep * DK; i += 256) qs[i] = bf16_to_f32(q[i]);
  const int j = j0 + tid;
  const bool valid = j >= lo && j < hi;
  uint4 kr[DK / 8];
  if (valid) {
    const uint4* kp = (const uint4*)(K + (((long long)b * Hkv + g) * cap + j) * DK);
#pragma unroll
    for (int i = 0; i < DK / 8; ++i) kr[i] = kp[i];
  }
  __syncthreads();
  if (valid) {
    for (int h = 0; h < rep; ++h) {
      const float4* qh = (const float4*)(qs + h * DK);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < DK / 8; ++i) {
        float kf[8];
        unpack8(kr[i], kf);
        const float4 q0 = qh[2 * i], q1 = qh[2 * i + 1];
        s = __builtin_fmaf(q0.x, kf[0], s); s = __builtin_fmaf(q0.y, kf[1], s); s = __builtin_fmaf(q0.z, kf[2], s); s = __builtin_fmaf(q0.w, kf[3], s);
        s = __builtin_fmaf(q1.x, kf[4], s); s = __builtin_fmaf(q1.y, kf[5], s); s = __builtin_fmaf(q1.z, kf[6], s); s = __builtin_fmaf(q1.w, kf[7], s);
      }
      ps[h * CHUNK + tid] = s * scale_log2e;
    }
  }
  __syncthreads();
  {
    const int lane = tid & 63, wave = tid >> 6;
    for (int h = wave; h < rep; h += 4) {
      float sv[4];
      bool ok[4];
      float m = NEG_BIG;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = lane + 64 * i;
        ok[i] = j0 + t >= lo && j0 + t < hi;     // by index: what ps holds at a key that does not count is never read
        sv[i] = ok[i] ? ps[h * CHUNK + t] : NEG_BIG;
        m = fmaxf(m, sv[i]);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float l = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = ok[i] ? __builtin_amdgcn_exp2f(sv[i] - m) : 0.f;
        l += p;
        ps[h * CHUNK + lane + 64 * i] = bf16_to_f32(f32_to_bf16(p));
      }
      l = wave_sum(l);
      if (lane == 0) { ml[h][0] = m; ml[h][1] = l; }
    }
  }
  __syncthreads();
  const int d = tid & (DK - 1), part = tid / DK;
  float o[MAXREP];
#pragma unroll
  for (int h = 0; h < MAXREP; ++h) o[h] = 0.f;
  {
    const bf16_t* vrow = VT + (((long long)b * Hkv + g) * DK + d) * cap + j0;
    for (int kk = part * PK; kk < part * PK + PK; kk += 8) {
      if (j0 + kk >= hi || j0 + kk + 8 <= lo) continue;   // no key of the range in these eight (hi <= cap and cap % 8 == 0: the read stays inside the row)
      float vf[8];
      unpack8(*(const uint4*)(vrow + kk), vf);
#pragma unroll
      for (int h = 0; h < MAXREP; ++h) {
        if (h < rep) {
          const float4 p0 = *(const float4*)(ps + h * CHUNK + kk), p1 = *(const float4*)(ps + h * CHUNK + kk + 4);
          float a = o[h];
          a = __builtin_fmaf(p0.x, vf[0], a); a = __builtin_fmaf(p0.y, vf[1], a); a = __builtin_fmaf(p0.z, vf[2], a); a = __builtin_fmaf(p0.w, vf[3], a);
          a = __builtin_fmaf(p1.x, vf[4], a); a = __builtin_fmaf(p1.y, vf[5], a); a = __builtin_fmaf(p1.z, vf[6], a); a = __builtin_fmaf(p1.w, vf[7], a);
          o[h] = a;
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < MAXREP; ++h)
    if (h < rep) red[(part * MAXREP + h) * DK + d] = o[h];
  __syncthreads();
  for (int i = tid; i < rep * DK; i += 256) {
    const int h = i / DK, dd = i - h * DK;
    float v = red[h * DK + dd];
#pragma unroll
    for (int p = 1; p < PARTS; ++p) v += red[(p * MAXREP + h) * DK + dd];
    float* w = ws + (((long long)b * Hq + (long long)g * rep + h) * nch + c) * (DK + 2);
    w[2 + dd] = v;
    if (dd == 0) { w[0] = ml[h][0]; w[1] = ml[h][1]; }
  }
}

// grid (Hq, B), dk threads: the chunks of [lo, hi) in ascending order under their common maximum
__global__ __launch_bounds__(128) void decode_attention_combine_kernel(const float* __restrict__ ws, const int32_t* __restrict__ k_lo,
                                                                       const int32_t* __restrict__ k_hi, bf16_t* __restrict__ O, int Hq, int cap,
                                                                       int nch, int dk, int ldo) {
  const int d = threadIdx.x, h = blockIdx.x, b = blockIdx.y;
  int lo, hi;
  load_range(k_lo, k_hi, b, cap, lo, hi);
  bf16_t* out = O + (long long)b * ldo + (long long)h * dk + d;
  if (hi <= lo) { *out = 0; return; }
  const int c0 = lo / CHUNK, c1 = (hi - 1) / CHUNK;
  const float* w = ws + ((long long)b * Hq + h) * nch * (dk + 2);
  float m = NEG_BIG;
  for (int c = c0; c <= c1; ++c) m = fmaxf(m, w[(long long)c * (dk + 2)]);
  float l = 0.f, acc = 0.f;
  for (int c = c0; c <= c1; ++c) {
    const float* wc = w + (long long)c * (dk + 2);
    const float f = __builtin_amdgcn_exp2f(wc[0] - m);
    l = __builtin_fmaf(wc[1], f, l);
    acc = __builtin_fmaf(wc[2 + d], f, acc);
  }
  *out = f32_to_bf16(acc / l);
}

}  // namespace

extern "C" {

int x2i_qwen_decode_rope_append_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, const int32_t* slot, void* Qd, void* K,
                                     void* VT, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t dk, x2i_stream_t stream) {
  if (!qkv || !cos || !sin || !slot || !Qd || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_rope_append: null pointer");
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_rope_append: head width dk=%d is not one of 64, 128", dk);
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || cap <= 0 || cap % 64 || Hq + Hkv > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_rope_append: bad shape, cap must be a positive multiple of 64 (B=%d Hq=%d Hkv=%d cap=%d)", B, Hq,
                         Hkv, cap);
  if (ld < ((long long)Hq + 2LL * Hkv) * dk || ld % 8 || !al16(qkv) || !al16(cos) || !al16(sin) || !al16(Qd) || !al16(K) || !al16(VT) ||
      (((uintptr_t)slot) & 3))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "qwen_decode_rope_append: ld must be a multiple of 8 and >= (Hq+2*Hkv)*dk, pointers 16-byte aligned (slot 4-byte aligned)");
  hipLaunchKernelGGL(decode_rope_append_kernel, dim3(Hq + Hkv, B), dim3(128), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld, cos, sin, slot,
                     (bf16_t*)Qd, (bf16_t*)K, (bf16_t*)VT, Hq, Hkv, cap, dk);
  return x2i_check_launch("qwen_decode_rope_append");
}

int x2i_qwen_decode_attention_bf16(const void* Qd, const void* K, const void* VT, const int32_t* k_lo, const int32_t* k_hi, void* O, float* ws,
                                   int64_t ws_floats, int32_t B, int32_t Hq, int32_t Hkv, int32_t cap, int32_t dk, float scale, int32_t ldo,
                                   x2i_stream_t stream) {
  if (!Qd || !K || !VT || !O || !ws) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_attention: null pointer");
  if (!k_lo || !k_hi) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_attention: the key range k_lo, k_hi is required (null pointer)");
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_attention: head width dk=%d is not one of 64, 128", dk);
  if (B <= 0 || B > 65535 || Hq <= 0 || Hq > 65535 || Hkv <= 0 || Hq % Hkv)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_attention: need Hq %% Hkv == 0 (B=%d Hq=%d Hkv=%d)", B, Hq, Hkv);
  if (Hq / Hkv > MAXREP)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_attention: a group of %d query heads per key/value head is above %d", Hq / Hkv, MAXREP);
  if (cap <= 0 || cap % 64) return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_attention: cap=%d must be a positive multiple of 64", cap);
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_attention: scale must be positive and finite");
  if (ldo < (long long)Hq * dk || ldo % 4 || (((uintptr_t)O) & 7) || !al16(Qd) || !al16(K) || !al16(VT) || !al16(ws) || (((uintptr_t)k_lo) & 3) ||
      (((uintptr_t)k_hi) & 3))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "qwen_decode_attention: ldo must be a multiple of 4 and >= Hq*dk, O 8-byte, Qd, K, VT, ws 16-byte, k_lo and k_hi 4-byte aligned");
  const int64_t need = X2I_QWEN_DECODE_WS_FLOATS(B, Hq, cap, dk);
  if (ws_floats < need)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_attention: workspace too small (%lld f32 given, %lld needed)", (long long)ws_floats, (long long)need);
  const int nch = (cap + CHUNK - 1) / CHUNK;
  const float sl = scale * LOG2E;
  const dim3 grid(nch, Hkv, B);
  if (dk == 128)
    hipLaunchKernelGGL(decode_attention_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)Qd, (const bf16_t*)K, (const bf16_t*)VT, k_lo,
                       k_hi, ws, Hq, Hkv, cap, nch, sl);
  else
    hipLaunchKernelGGL(decode_attention_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)Qd, (const bf16_t*)K, (const bf16_t*)VT, k_lo,
                       k_hi, ws, Hq, Hkv, cap, nch, sl);
  if (const int rc = x2i_check_launch("qwen_decode_attention")) return rc;
  hipLaunchKernelGGL(decode_attention_combine_kernel, dim3(Hq, B), dim3(dk), 0, (hipStream_t)stream, (const float*)ws, k_lo, k_hi, (bf16_t*)O, Hq, cap, nch,
                     dk, ldo);
  return x2i_check_launch("qwen_decode_attention (combine)");
}

int x2i_qwen_decode_linear_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const void* res, int64_t ldr, void* Y,
                                int64_t ldy, int32_t B, int32_t N, int32_t K, int32_t mode, x2i_stream_t stream) {
  if (!X || !W || !Y) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear: null pointer");
  if (B < 1 || B > 8) return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_linear: B=%d is not in 1..8", B);
  if (mode != 0 && mode != 1) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear: mode=%d is not 0 or 1", mode);
  if (mode == 1 && res) return x2i_set_error(X2I_ERR_ARG, "qwen_decode_linear: the gate (mode 1) takes no residual");
  if (N <= 0 || K <= 0 || K % 8 || N > (1 << 29)) return x2i_set_error(X2I_ERR_SHAPE, "qwen_decode_linear: K=%d must be a positive multiple of 8 (N=%d)", K, N);
  if (ldx < K || ldw < K || ldx % 8 || ldw % 8 || ldy < N || (res && ldr < N) || !al16(X) || !al16(W) || (((uintptr_t)Y) & 1) ||
      (((uintptr_t)res) & 1) || (((uintptr_t)bias) & 1))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "qwen_decode_linear: ldx and ldw must be multiples of 8 and >= K, ldy (ldr) >= N, X and W 16-byte aligned (rows 16-byte aligned)");
  // X in LDS: all of K when B * K bf16 fit 64 KiB, else chunks of a multiple of 512 columns (the lanes' k sequences do not change)
  int KC = K;
  if ((long long)B * K * 2 > 65536) KC = (32768 / B) & ~511;
  // rows per wave: four where that still gives every CU two workgroups, else two
  const long long rows = mode ? 2LL * N : N;
  const bool wide = rows >= 32LL * x2i_num_cus();
  const hipStream_t st = (hipStream_t)stream;
#define DL_CASE(NB) \
  case NB: launch_decode_linear_nb<NB>(wide, mode, X, ldx, W, ldw, bias, res, ldr, Y, ldy, N, K, KC, st); break;
  switch (B) { DL_CASE(1) DL_CASE(2) DL_CASE(3) DL_CASE(4) DL_CASE(5) DL_CASE(6) DL_CASE(7) DL_CASE(8) }
#undef DL_CASE
  return x2i_check_launch("qwen_decode_linear");
}

}  // extern "C"
