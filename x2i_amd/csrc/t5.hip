// The T5 encoder's kernels (include/x2i_t5.h): flash attention with a relative-position bias for head widths 32 / 64 / 128, the head
// split in front of it, T5LayerNorm (an RMS norm over the model width) and the gate of the gated-GELU feed-forward.  They stand behind
// `transformers`' T5Attention / T5LayerNorm / T5DenseGatedActDense as the reference uses them (model_internvl/proj.py:153-159,167 and
// train/train_qwenvl.py:666,778).  bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
//
// Attention: the mapping of attention.hip (its 4-wave plain-HIP kernel) with the head width as a template parameter
//   * one workgroup = 4 waves, each wave owns 32 query rows; K / V^T stream through LDS in 64-key tiles, double-buffered LDS-DMA
//   * swapped QK^T (S^T = K Q^T, v_mfma_f32_32x32x16_bf16): a lane holds 32 scores of ONE query row, neighbouring lanes hold neighbouring
//     rows; the kvmap row permutation makes P^T directly the B operand of the PV MFMA
//   * K tile rows are 2 DK bytes (64 / 128 / 256): 16 / DK*8 rows share one 256-byte bank row, and the XOR swizzle is
//     chunk ^= (row / rows_per_bank_row) & (chunks_per_row - 1) -- a ds_read_b128 group's 16 lanes read rows that are distinct mod 16, hence
//     16 distinct 16-byte slots for every DK.  V^T tile rows are 128 bytes for every DK: chunk ^= (row >> 1) & 7, as attention.hip has it
//   * the head's bias table (2R + 1 floats, pre-multiplied by log2 e) sits in LDS behind the tiles; a score's bias is one ds_read_b32 at
//     clamp(key - query, -R, R) + R -- consecutive addresses across the lanes of a half-wave, one address inside the clamped region -- and a
//     (wave's query rows, key tile) pair wholly beyond +-R takes one uniform value instead
#include "x2i_common.h"
#include "../../include/x2i_t5.h"
#include <type_traits>

namespace {

constexpr int KVB = 64;          // keys per tile
constexpr int T5_RMAX = 2047;    // largest clamp distance: the table region of the LDS image is 16 KiB
constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int DK>
__global__ __launch_bounds__(256, 2) void t5_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                         const bf16_t* __restrict__ VT, const float* __restrict__ tab,
                                                         bf16_t* __restrict__ O, int H, int S, int Spad, int R, int ldo, long long o_bs,
                                                         int nbatch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][K tile | V^T tile] | bias table f32 [2R+1]
  constexpr int NT = 256;
  constexpr int KTILE = KVB * DK * 2;   // [64 keys][DK]
  constexpr int VTILE = DK * KVB * 2;   // [DK][64 keys]
  constexpr int CK = DK / 8;            // 16-byte chunks per K row
  constexpr int RPB = 16 / CK;          // K rows per 256-byte bank row
  constexpr int CH = DK / 32;           // chunks per thread per tile (64 * CK / 256)
  constexpr int NDS = DK / 16;          // d-steps of the score product
  constexpr int NDB = DK / 32;          // 32-wide d-blocks of O^T
  constexpr int THR = 8;                // defer-max threshold (exp2 domain), as attention.hip
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int li = lane & 31;
  // XCD-aware block order: each XCD walks a contiguous range of (batch, head, q-tile) triples
  const int nqt = gridDim.x / (H * nbatch);
  int bid = blockIdx.x;
  {
    const int T = gridDim.x, q = T >> 3, r = T & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int qt = bid % nqt, h = (bid / nqt) % H, b = bid / (nqt * H);
  const int q0 = qt * 128 + wave * 32;
  const long long bh = (long long)b * H + h;
  const bf16_t* Qh = Q + bh * Spad * DK;
  const bf16_t* Kh = K + bh * Spad * DK;
  const bf16_t* Vh = VT + bh * DK * Spad;
  float* tl = (float*)(smem + 2 * (KTILE + VTILE));

  // ---- the head's bias table into LDS, in the exp2 domain
  for (int i = tid; i < 2 * R + 1; i += NT) tl[i] = tab[(long long)h * (2 * R + 1) + i] * LOG2E;

  // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[q0+li][ds*16 + hi*8 .. +8]; rows past Spad (Spad % 128 != 0) read the last row
  bf16x8_t qf[NDS];
  {
    const int qrow = min(q0 + li, Spad - 1);
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) qf[ds] = *(const bf16x8_t*)(Qh + (long long)qrow * DK + ds * 16 + hi * 8);
  }

  // ---- DMA source offsets (elements); the LDS image is linear, the swizzle goes on the source
  int k_src[CH], v_src[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int p = j * NT + tid;
    {
      const int row = p / CK, cphys = p % CK;
      k_src[j] = row * DK + ((cphys ^ ((row / RPB) & (CK - 1))) << 3);
    }
    {
      const int row = p >> 3, cphys = p & 7;
      v_src[j] = row * Spad + ((cphys ^ ((row >> 1) & 7)) << 3);
    }
  }
  auto stage = [&](int buf, int kv0) {
    char* kb = smem + buf * (KTILE + VTILE);
    char* vb = kb + KTILE;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      glds16(Kh + (long long)kv0 * DK + k_src[j], kb + (j * NT + wave * 64) * 16);
      glds16(Vh + kv0 + v_src[j], vb + (j * NT + wave * 64) * 16);
    }
  };

  // ---- per-lane LDS read offsets
  const int kvm = (li & 0x13) | ((li & 4) << 1) | ((li & 8) >> 1);  // swap bits 2 and 3
  const int k_row_off = kvm * (2 * DK);
  const int k_swz = (kvm / RPB) & (CK - 1);
  const int v_row_off = li * 128;
  const int v_swz = (li >> 1) & 7;

  f32x16_t oacc[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
  float m_run = NEG_BIG, l_run = 0.f;

  const int ntiles = (S + KVB - 1) / KVB;
  const int q = q0 + li;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // tile 0 and the bias table are in LDS

  auto kv_tile = [&](int t, auto last_c) {
    constexpr bool LAST = decltype(last_c)::value;
    const int buf = t & 1;
    if (!LAST) stage(buf ^ 1, (t + 1) * KVB);
    const char* kb = smem + buf * (KTILE + VTILE);
    const char* vb = kb + KTILE;

    // ---- S^T = K Q^T: two 32-key sub-tiles, alternating accumulators
    f32x16_t sacc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[u][r] = 0.f;
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8_t kf = *(const bf16x8_t*)(kb + u * 32 * (2 * DK) + k_row_off + (((ds * 2 + hi) ^ k_swz) << 4));
        sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ds], sacc[u], 0, 0, 0);
      }
    // lane (q = li, hi), sub-tile u, reg r  <->  key = kv0 + u*32 + 16*(r>>3) + 8*hi + (r&7)
    const int kv0 = t * KVB;
    // ---- scores into the exp2 domain, plus the bias of key offset key - q
    if (kv0 - (q0 + 31) >= R || kv0 + (KVB - 1) - q0 <= -R) {   // (wave-uniform) the whole 32 x 64 patch lies in one clamped region
      const float bias = tl[kv0 > q0 ? 2 * R : 0];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[u][r] = __builtin_fmaf(sacc[u][r], LOG2E, bias);
    } else {
      const int rel0 = kv0 + 8 * hi - q;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rel = rel0 + u * 32 + 16 * (r >> 3) + (r & 7);
          sacc[u][r] = __builtin_fmaf(sacc[u][r], LOG2E, tl[min(max(rel, -R), R) + R]);
        }
    }
    if (LAST && kv0 + KVB > S) {  // ragged last tile: keys >= S are masked by index
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kv0 + u * 32 + 16 * (r >> 3) + 8 * hi + (r & 7);
          if (key >= S) sacc[u][r] = NEG_BIG;
        }
    }
    // ---- online softmax
    float mx = NEG_BIG;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[u][r]);
    mx = xhalf_max(mx);
    // defer-max: keep the old running max while no row of this wave grew by more than THR, so that the O rescale is skipped on most tiles
    float m_new = fmaxf(m_run, mx);
    if (__all(m_new - m_run <= (float)THR)) m_new = m_run;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(sacc[u][r] - m_new);
        sacc[u][r] = pv;
        psum += pv;
      }
    l_run = l_run * alpha + psum;
    if (!__all(m_new == m_run)) {
#pragma unroll
      for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
    }
    m_run = m_new;

    // ---- P^T fragments (B operand): sub-tile u, k-step kt uses regs 8kt..8kt+7  (keys u*32+16kt+8hi+0..7)
    bf16x8_t pf[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        union { bf16x8_t v; uint32_t w[4]; } cv;
#pragma unroll
        for (int j = 0; j < 4; ++j) cv.w[j] = pack_bf16x2(sacc[u][kt * 8 + 2 * j], sacc[u][kt * 8 + 2 * j + 1]);
        pf[u][kt] = cv.v;
      }
    // ---- O^T += V^T P^T
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const int u = g >> 1, kt = g & 1;
        const bf16x8_t vf = *(const bf16x8_t*)(vb + db * 32 * 128 + v_row_off + (((4 * u + 2 * kt + hi) ^ v_swz) << 4));
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[u][kt], oacc[db], 0, 0, 0);
      }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next tile's DMA (issued by this wave) has landed
    __syncthreads();
  };
  for (int t = 0; t < ntiles - 1; ++t) kv_tile(t, std::false_type{});
  kv_tile(ntiles - 1, std::true_type{});

  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane (q = li, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3)
  l_run = xhalf_sum(l_run);
  const float inv = 1.f / l_run;
  bf16_t* orow = O + (long long)b * o_bs + (long long)q * ldo + h * DK;
  if ((((uintptr_t)O) & 15) == 0 && (ldo & 7) == 0 && (o_bs & 7) == 0) {
    // half-wave exchange: two 8-byte fragments of neighbouring d-groups become one 16-byte store per lane
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; g += 2) {
        const uint32_t a0 = pack_bf16x2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv);
        const uint32_t a1 = pack_bf16x2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
        const uint32_t b0 = pack_bf16x2(oacc[db][4 * g + 4] * inv, oacc[db][4 * g + 5] * inv);
        const uint32_t b1 = pack_bf16x2(oacc[db][4 * g + 6] * inv, oacc[db][4 * g + 7] * inv);
        const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        if (q < S) *(uint4*)(orow + db * 32 + 8 * (g + hi)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
  } else if (q < S) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * hi;
        *(uint2*)(orow + d) = make_uint2(pack_bf16x2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv),
                                         pack_bf16x2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv));
      }
  }
}

template <int DK>
int launch_t5_attention(const void* Q, const void* K, const void* VT, const float* tab, void* O, int B, int H, int S, int Spad, int R, int ldo,
                        long long o_bs, hipStream_t stream) {
  constexpr int TILES = 2 * 2 * KVB * DK * 2;
  const int rc = x2i_ensure_dynamic_smem((const void*)t5_attn_kernel<DK>, TILES + (2 * T5_RMAX + 2) * 4);
  if (rc) return rc;
  const size_t shm = TILES + (size_t)((2 * R + 1 + 3) & ~3) * 4;
  const dim3 grid((unsigned)(((S + 127) / 128) * H * B));
  hipLaunchKernelGGL((t5_attn_kernel<DK>), grid, dim3(256), shm, stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)VT, tab, (bf16_t*)O, H,
                     S, Spad, R, ldo, o_bs, B);
  return x2i_check_launch("t5_attention");
}

// ------------------------------------------------------------------------------------------------------------------- head split
// One workgroup per (64-token tile, head, sample).  Q and K rows are 16-byte copies; V goes through an LDS tile [64 tokens][dk + 2] and
// leaves as 16-byte pieces of VT rows (scalar stores in the one piece that straddles S: columns >= S stay untouched).
__global__ __launch_bounds__(256) void t5_head_split_kernel(const bf16_t* __restrict__ qkv, long long ld, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                            bf16_t* __restrict__ VT, int S, int Spad, int H, int dk) {
  __shared__ uint32_t tile[64 * (128 + 2) / 2];
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int ck = dk >> 3;           // 16-byte chunks per head row
  const int pitch = (dk + 2) >> 1;  // LDS row pitch in dwords
  const long long bh = (long long)b * H + h;
  const int inner = H * dk;
  for (int c = tid; c < 64 * ck; c += 256) {
    const int tok = c / ck, ch = c - tok * ck;
    const int s = s0 + tok;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (s < S) {
      const bf16_t* src = qkv + ((long long)b * S + s) * ld + h * dk + ch * 8;
      const long long dst = (bh * Spad + s) * dk + ch * 8;
      *(uint4*)(Q + dst) = *(const uint4*)src;
      *(uint4*)(K + dst) = *(const uint4*)(src + inner);
      v = *(const uint4*)(src + 2 * inner);
    }
    uint32_t* t = tile + tok * pitch + ch * 4;
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
  }
  __syncthreads();
  const bf16_t* tb = (const bf16_t*)tile;
  for (int i = tid; i < dk * 8; i += 256) {
    const int tc = i & 7, d = i >> 3;
    const int s = s0 + tc * 8;
    if (s >= S) continue;
    bf16_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = tb[(tc * 8 + j) * (2 * pitch) + d];
    bf16_t* dst = VT + (bh * dk + d) * Spad + s;
    if (s + 8 <= S) {
      *(uint4*)dst = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (s + j < S) dst[j] = e[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- T5LayerNorm
__device__ __forceinline__ void unpack8(const uint4& p, float (&v)[8]) {
  v[0] = __uint_as_float(p.x << 16); v[1] = __uint_as_float(p.x & 0xffff0000u);
  v[2] = __uint_as_float(p.y << 16); v[3] = __uint_as_float(p.y & 0xffff0000u);
  v[4] = __uint_as_float(p.z << 16); v[5] = __uint_as_float(p.z & 0xffff0000u);
  v[6] = __uint_as_float(p.w << 16); v[7] = __uint_as_float(p.w & 0xffff0000u);
}

// A wave per row, four rows per workgroup; a lane keeps up to RMS_REG 16-byte chunks of its row in registers (D <= 4096) and re-reads the rest.
constexpr int RMS_REG = 8;
__global__ __launch_bounds__(256) void t5_rms_rows_kernel(const bf16_t* __restrict__ X, long long ldx, bf16_t* __restrict__ Y, long long ldy,
                                                          const bf16_t* __restrict__ W, long long rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* x = X + row * ldx;
  bf16_t* y = Y + row * ldy;
  const int nc = D >> 3;
  uint4 buf[RMS_REG];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < RMS_REG; ++k) {
    const int c = lane + k * 64;
    buf[k] = make_uint4(0u, 0u, 0u, 0u);
    if (c < nc) buf[k] = *(const uint4*)(x + c * 8);
    float v[8];
    unpack8(buf[k], v);
    ss += sumsq8(v);
  }
  for (int c = lane + RMS_REG * 64; c < nc; c += 64) {
    float v[8];
    unpack8(*(const uint4*)(x + c * 8), v);
    ss += sumsq8(v);
  }
  const float r = rsqrtf(__fadd_rn(wave_sum(ss) / (float)D, eps));
  auto emit = [&](int c, const uint4& px) {
    float v[8], w[8];
    unpack8(px, v);
    unpack8(*(const uint4*)(W + c * 8), w);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // one rounding: the normalised value stays f32 until the weight has multiplied it (the library rounds it to bf16 in between)
      o[j >> 1] = pack_bf16x2(__fmul_rn(w[j], __fmul_rn(v[j], r)), __fmul_rn(w[j + 1], __fmul_rn(v[j + 1], r)));
    }
    *(uint4*)(y + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  };
#pragma unroll
  for (int k = 0; k < RMS_REG; ++k) {
    const int c = lane + k * 64;
    if (c < nc) emit(c, buf[k]);
  }
  for (int c = lane + RMS_REG * 64; c < nc; c += 64) emit(c, *(const uint4*)(x + c * 8));
}

// ------------------------------------------------------------------------------------------------------------------- gated GELU
__global__ __launch_bounds__(256) void t5_gated_gelu_kernel(const bf16_t* __restrict__ AB, long long ld_in, bf16_t* __restrict__ Y, long long ldy,
                                                            long long rows, int F) {
  const int nc = F >> 3;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    const bf16_t* src = AB + row * ld_in + c * 8;
    float a[8], g[8];
    unpack8(*(const uint4*)src, a);
    unpack8(*(const uint4*)(src + F), g);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // one rounding: the activation stays f32 until the gate has multiplied it (the library rounds it to bf16 in between)
      o[j >> 1] = pack_bf16x2(__fmul_rn(gelu_tanh_f(a[j]), g[j]), __fmul_rn(gelu_tanh_f(a[j + 1]), g[j + 1]));
    }
    *(uint4*)(Y + row * ldy + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" {

int x2i_t5_attention_bf16(const void* Q, const void* K, const void* VT, const float* bias_tab, void* O, int32_t B, int32_t H, int32_t S,
                          int32_t Spad, int32_t dk, int32_t R, int32_t ldo, int64_t o_batch_stride, x2i_stream_t stream) {
  if (!Q || !K || !VT || !bias_tab || !O) return x2i_set_error(X2I_ERR_ARG, "t5_attention: null pointer");
  if (dk != 32 && dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "t5_attention: head width dk=%d is not one of 32, 64, 128", dk);
  if (B <= 0 || H <= 0 || S <= 0 || Spad < S || Spad % 64)
    return x2i_set_error(X2I_ERR_SHAPE, "t5_attention: need Spad %% 64 == 0 and Spad >= S (S=%d Spad=%d)", S, Spad);
  if (R < 0 || R > T5_RMAX) return x2i_set_error(X2I_ERR_SHAPE, "t5_attention: clamp distance R=%d outside 0..%d", R, T5_RMAX);
  if ((long long)((S + 127) / 128) * H * B > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "t5_attention: too many work items");
  if (ldo < H * dk || ldo % 4 || o_batch_stride % 4 || (((uintptr_t)O) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_attention: output rows must hold H*dk elements and be 8-byte aligned");
  if (!al16(Q) || !al16(K) || !al16(VT)) return x2i_set_error(X2I_ERR_ALIGN, "t5_attention: Q, K, VT must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dk == 32) return launch_t5_attention<32>(Q, K, VT, bias_tab, O, B, H, S, Spad, R, ldo, o_batch_stride, st);
  if (dk == 64) return launch_t5_attention<64>(Q, K, VT, bias_tab, O, B, H, S, Spad, R, ldo, o_batch_stride, st);
  return launch_t5_attention<128>(Q, K, VT, bias_tab, O, B, H, S, Spad, R, ldo, o_batch_stride, st);
}

int x2i_t5_head_split_bf16(const void* qkv, int64_t ld, void* Q, void* K, void* VT, int32_t B, int32_t S, int32_t Spad, int32_t H, int32_t dk,
                           x2i_stream_t stream) {
  if (!qkv || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "t5_head_split: null pointer");
  if (dk != 32 && dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "t5_head_split: head width dk=%d is not one of 32, 64, 128", dk);
  if (B <= 0 || S <= 0 || H <= 0 || Spad < S || Spad % 8 || H > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "t5_head_split: bad shape (B=%d S=%d Spad=%d H=%d)", B, S, Spad, H);
  if (ld < 3LL * H * dk || ld % 8 || !al16(qkv) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_head_split: ld must be a multiple of 8 and >= 3*H*dk, pointers 16-byte aligned");
  hipLaunchKernelGGL(t5_head_split_kernel, dim3((S + 63) / 64, H, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld,
                     (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, S, Spad, H, dk);
  return x2i_check_launch("t5_head_split");
}

int x2i_t5_rms_rows_bf16(const void* X, int64_t ldx, void* Y, int64_t ldy, const void* weight, int64_t rows, int32_t D, float eps,
                         x2i_stream_t stream) {
  if (!X || !Y || !weight) return x2i_set_error(X2I_ERR_ARG, "t5_rms_rows: null pointer");
  if (rows <= 0 || D <= 0 || D % 8 || (rows + 3) / 4 > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "t5_rms_rows: D=%d must be a positive multiple of 8", D);
  if (ldx < D || ldy < D || ldx % 8 || ldy % 8 || !al16(X) || !al16(Y) || !al16(weight))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_rms_rows: row strides must be multiples of 8 and >= D, pointers 16-byte aligned");
  hipLaunchKernelGGL(t5_rms_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, (long long)ldx,
                     (bf16_t*)Y, (long long)ldy, (const bf16_t*)weight, (long long)rows, D, eps);
  return x2i_check_launch("t5_rms_rows");
}

int x2i_t5_gated_gelu_bf16(const void* AB, int64_t ld_in, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream) {
  if (!AB || !Y) return x2i_set_error(X2I_ERR_ARG, "t5_gated_gelu: null pointer");
  if (rows <= 0 || F <= 0 || F % 8) return x2i_set_error(X2I_ERR_SHAPE, "t5_gated_gelu: F=%d must be a positive multiple of 8", F);
  if (ld_in < 2LL * F || ldy < F || ld_in % 8 || ldy % 8 || !al16(AB) || !al16(Y))
    return x2i_set_error(X2I_ERR_ALIGN, "t5_gated_gelu: row strides must be multiples of 8 (ld_in >= 2F, ldy >= F), pointers 16-byte aligned");
  const long long chunks = (long long)rows * (F / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 < 8192 ? (chunks + 255) / 256 : 8192);
  hipLaunchKernelGGL(t5_gated_gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)AB, (long long)ld_in, (bf16_t*)Y,
                     (long long)ldy, (long long)rows, F);
  return x2i_check_launch("t5_gated_gelu");
}

}  // extern "C"
