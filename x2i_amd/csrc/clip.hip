// The CLIP text encoder's kernels (include/x2i_clip.h): causal flash attention for 64-wide heads, the token + position embedding, the
// quick-GELU of the MLP and the pooled output (the hidden state at each sample's end-of-text token).  They stand behind `transformers`'
// CLIPAttention (under the text model's causal mask) / CLIPTextEmbeddings / CLIPMLP / CLIPTextModel's pooling as the reference uses them
// (infer/inference_*.py: `clip_model(ids, output_hidden_states=False).pooler_output`, train/train_qwenvl.py:665,778).  bf16 in and out,
// f32 arithmetic; every launcher enqueues on the caller's stream and returns.
//
// Attention: t5_attn_kernel<64> (t5.hip) without the bias table, with a softmax scale, and causal
//   * one workgroup = 4 waves, each wave owns 32 query rows; K / V^T stream through LDS in 64-key tiles, double-buffered LDS-DMA; swapped
//     QK^T (S^T = K Q^T, v_mfma_f32_32x32x16_bf16): a lane holds 32 scores of ONE query row
//   * a workgroup (query rows r0 .. r0+127) walks the key tiles 0 .. ceil(min(S, r0 + 128) / 64) - 1 only: the trip count, every DMA issue,
//     every s_waitcnt and every barrier are uniform across the workgroup
//   * a wave (rows q0 .. q0+31) computes a tile only when the tile starts at or before q0 (kv0 <= q0; kv0 is a multiple of 64 and q0 of 32,
//     so a tile that starts after q0 starts after q0 + 31 too and is wholly in that wave's future) and when q0 < S; otherwise it walks
//     the loop (stage, wait, barrier) without MFMAs or exponentials.  Hence in every tile a wave computes, every one of its rows has at
//     least one key <= its index: no row ever sees a wholly masked tile, and tile 0, the first tile of every wave, holds key 0 <= i, so a
//     row's running maximum is a real score from its first tile on (the defer-max test m_new - m_run <= THR fails against NEG_BIG there)
//   * the mask is by index: in a tile that reaches past q0 (kv0 + 63 > q0) a score of key j > min(i, S - 1) becomes NEG_BIG before the
//     maximum and the sum see it, whatever K and V^T hold there; exp2(NEG_BIG - m) is exactly 0.  Rows i >= S (never written) behave as
//     row S - 1, so that no lane of a computing wave carries an empty row
#include "x2i_common.h"
#include "../../include/x2i_clip.h"

namespace {

constexpr int KVB = 64;          // keys per tile
constexpr int DK = 64;           // head width
constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__global__ __launch_bounds__(256, 2) void clip_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                           const bf16_t* __restrict__ VT, bf16_t* __restrict__ O, int H, int S, int Spad,
                                                           float scale2, int ldo, long long o_bs, int nbatch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][K tile | V^T tile]
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

  // workgroup-uniform trip count: the key tiles up to this query block's diagonal (and below S)
  const int ntiles = (min(S, qt * 128 + 128) + KVB - 1) / KVB;
  // wave-uniform: the tiles this wave computes, t < nact  <=>  t * 64 <= q0 (and none for a wave wholly past S)
  const int nact = q0 < S ? min(ntiles, q0 / KVB + 1) : 0;
  const int q = q0 + li;
  const int qlim = min(q, S - 1);   // the last key of this lane's row
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();   // tile 0 is in LDS

  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) stage(buf ^ 1, (t + 1) * KVB);   // (workgroup-uniform)
    if (t < nact) {                                     // (wave-uniform)
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
      // ---- scores into the exp2 domain: one multiply by scale * log2 e
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[u][r] *= scale2;
      if (kv0 + (KVB - 1) > q0) {   // (wave-uniform) the tile reaches past this wave's first row: keys after a row's own index are masked by index
        const int lim = qlim - kv0 - 8 * hi;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (u * 32 + 16 * (r >> 3) + (r & 7) > lim) sacc[u][r] = NEG_BIG;
      }
      // ---- online softmax
      float mx = NEG_BIG;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[u][r]);
      mx = xhalf_max(mx);
      // defer-max: keep the old running max while no row of this wave grew by more than THR, so that the O rescale is skipped on most tiles.
      // (In a wave's first tile m_run is NEG_BIG and mx a real score of every row -- key kv0 = 0 <= i -- so the test fails and m_new is real.)
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
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next tile's DMA (issued by this wave) has landed
    __syncthreads();
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane (q = li, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3)
  l_run = xhalf_sum(l_run);
  const float inv = nact > 0 ? 1.f / l_run : 0.f;   // (a wave wholly past S holds nothing and writes nothing)
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

__device__ __forceinline__ void unpack8(const uint4& p, float (&v)[8]) {
  v[0] = __uint_as_float(p.x << 16); v[1] = __uint_as_float(p.x & 0xffff0000u);
  v[2] = __uint_as_float(p.y << 16); v[3] = __uint_as_float(p.y & 0xffff0000u);
  v[4] = __uint_as_float(p.z << 16); v[5] = __uint_as_float(p.z & 0xffff0000u);
  v[6] = __uint_as_float(p.w << 16); v[7] = __uint_as_float(p.w & 0xffff0000u);
}

// ------------------------------------------------------------------------------------------------------------------- embeddings
// One thread per 16-byte chunk of X.  An id outside [0, vocab) is clamped: the host cannot see it, and no launch reads out of bounds.
__global__ __launch_bounds__(256) void clip_embed_kernel(const long long* __restrict__ ids, const bf16_t* __restrict__ tok,
                                                         const bf16_t* __restrict__ pos, bf16_t* __restrict__ X, long long rows, int S, int D,
                                                         int vocab) {
  const int nc = D >> 3;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    const int s = (int)(row % S);
    long long id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    float a[8], p[8];
    unpack8(*(const uint4*)(tok + id * D + c * 8), a);
    unpack8(*(const uint4*)(pos + (long long)s * D + c * 8), p);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) o[j >> 1] = pack_bf16x2(__fadd_rn(a[j], p[j]), __fadd_rn(a[j + 1], p[j + 1]));
    *(uint4*)(X + row * D + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------- quick GELU
// x * sigmoid(1.702 x) = x / (1 + exp2(-1.702 log2(e) x)): the form (and the v_exp_f32 / v_rcp_f32 pair) of silu_f
__device__ __forceinline__ float quick_gelu_f(float x) {
  constexpr float C = (float)(-1.702 * 1.4426950408889634);
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(C * x));
}

__global__ __launch_bounds__(256) void clip_quick_gelu_kernel(const bf16_t* __restrict__ X, long long ldx, bf16_t* __restrict__ Y, long long ldy,
                                                              long long rows, int F) {
  const int nc = F >> 3;
  const long long total = rows * nc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nc;
    const int c = (int)(i - row * nc);
    float a[8];
    unpack8(*(const uint4*)(X + row * ldx + c * 8), a);
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) o[j >> 1] = pack_bf16x2(quick_gelu_f(a[j]), quick_gelu_f(a[j + 1]));   // one rounding
    *(uint4*)(Y + row * ldy + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------- pooled output
// One workgroup per sample.  Every thread scans ids[b][tid], ids[b][tid + 256], ... in ascending position and keeps its best
// (value, first position); an LDS tree picks the workgroup's, preferring the smaller position among equal values; then the row is copied.
//   legacy rule (eos_token_id == 2): value = the id itself           -> the first position of the largest id
//   otherwise:                       value = (id == eos_token_id)    -> the first eos, or position 0 when there is none (all values 0)
__global__ __launch_bounds__(256) void clip_pool_kernel(const long long* __restrict__ ids, const bf16_t* __restrict__ Hs, long long ldh,
                                                        bf16_t* __restrict__ pooled, long long ldp, int S, int D, int eos, int legacy) {
  __shared__ long long sval[256];
  __shared__ int spos[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const long long* row = ids + (long long)b * S;
  long long best = 0;
  int bpos = -1;
  for (int s = tid; s < S; s += 256) {
    const long long id = row[s];
    const long long v = legacy ? id : (long long)(id == (long long)eos);
    if (bpos < 0 || v > best) { best = v; bpos = s; }
  }
  sval[tid] = best;
  spos[tid] = bpos;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const long long v = sval[tid + w];
      const int p = spos[tid + w];
      if (p >= 0 && (spos[tid] < 0 || v > sval[tid] || (v == sval[tid] && p < spos[tid]))) { sval[tid] = v; spos[tid] = p; }
    }
    __syncthreads();
  }
  const int idx = spos[0];   // 0 <= idx < S: S >= 1, so thread 0 holds a position
  const bf16_t* src = Hs + ((long long)b * S + idx) * ldh;
  bf16_t* dst = pooled + (long long)b * ldp;
  for (int c = tid; c < (D >> 3); c += 256) *(uint4*)(dst + c * 8) = *(const uint4*)(src + c * 8);
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" {

int x2i_clip_attention_bf16(const void* Q, const void* K, const void* VT, void* O, int32_t B, int32_t H, int32_t S, int32_t Spad, int32_t dk,
                            float scale, int32_t ldo, int64_t o_batch_stride, x2i_stream_t stream) {
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "clip_attention: null pointer");
  if (dk != DK) return x2i_set_error(X2I_ERR_SHAPE, "clip_attention: head width dk=%d is not 64", dk);
  if (B <= 0 || H <= 0 || S <= 0 || Spad < S || Spad % 64)
    return x2i_set_error(X2I_ERR_SHAPE, "clip_attention: need Spad %% 64 == 0 and Spad >= S (S=%d Spad=%d)", S, Spad);
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "clip_attention: scale must be positive and finite");
  if ((long long)((S + 127) / 128) * H * B > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "clip_attention: too many work items");
  if (ldo < H * dk || ldo % 4 || o_batch_stride % 4 || (((uintptr_t)O) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "clip_attention: output rows must hold H*dk elements and be 8-byte aligned");
  if (!al16(Q) || !al16(K) || !al16(VT)) return x2i_set_error(X2I_ERR_ALIGN, "clip_attention: Q, K, VT must be 16-byte aligned");
  constexpr int TILES = 2 * 2 * KVB * DK * 2;
  const int rc = x2i_ensure_dynamic_smem((const void*)clip_attn_kernel, TILES);
  if (rc) return rc;
  const dim3 grid((unsigned)(((S + 127) / 128) * H * B));
  hipLaunchKernelGGL(clip_attn_kernel, grid, dim3(256), TILES, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)VT,
                     (bf16_t*)O, H, S, Spad, scale * LOG2E, ldo, (long long)o_batch_stride, B);
  return x2i_check_launch("clip_attention");
}

int x2i_clip_embed_bf16(const int64_t* ids, const void* tok, const void* pos, void* X, int32_t B, int32_t S, int32_t D, int32_t vocab,
                        x2i_stream_t stream) {
  if (!ids || !tok || !pos || !X) return x2i_set_error(X2I_ERR_ARG, "clip_embed: null pointer");
  if (B <= 0 || S <= 0 || vocab <= 0 || D <= 0 || D % 8)
    return x2i_set_error(X2I_ERR_SHAPE, "clip_embed: D=%d must be a positive multiple of 8 (B=%d S=%d vocab=%d)", D, B, S, vocab);
  if (!al16(tok) || !al16(pos) || !al16(X) || (((uintptr_t)ids) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "clip_embed: tok, pos, X must be 16-byte aligned, ids 8-byte aligned");
  const long long rows = (long long)B * S, chunks = rows * (D / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 < 8192 ? (chunks + 255) / 256 : 8192);
  hipLaunchKernelGGL(clip_embed_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, (const bf16_t*)tok,
                     (const bf16_t*)pos, (bf16_t*)X, rows, S, D, vocab);
  return x2i_check_launch("clip_embed");
}

int x2i_clip_quick_gelu_bf16(const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream) {
  if (!X || !Y) return x2i_set_error(X2I_ERR_ARG, "clip_quick_gelu: null pointer");
  if (rows <= 0 || F <= 0 || F % 8) return x2i_set_error(X2I_ERR_SHAPE, "clip_quick_gelu: F=%d must be a positive multiple of 8", F);
  if (ldx < F || ldy < F || ldx % 8 || ldy % 8 || !al16(X) || !al16(Y))
    return x2i_set_error(X2I_ERR_ALIGN, "clip_quick_gelu: row strides must be multiples of 8 and >= F, pointers 16-byte aligned");
  const long long chunks = (long long)rows * (F / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 < 8192 ? (chunks + 255) / 256 : 8192);
  hipLaunchKernelGGL(clip_quick_gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, (long long)ldx, (bf16_t*)Y,
                     (long long)ldy, (long long)rows, F);
  return x2i_check_launch("clip_quick_gelu");
}

int x2i_clip_pool_bf16(const int64_t* ids, const void* Hs, int64_t ldh, void* pooled, int64_t ldp, int32_t B, int32_t S, int32_t D,
                       int32_t eos_token_id, x2i_stream_t stream) {
  if (!ids || !Hs || !pooled) return x2i_set_error(X2I_ERR_ARG, "clip_pool: null pointer");
  if (B <= 0 || S <= 0 || D <= 0 || D % 8) return x2i_set_error(X2I_ERR_SHAPE, "clip_pool: D=%d must be a positive multiple of 8 (B=%d S=%d)", D, B, S);
  if (ldh < D || ldp < D || ldh % 8 || ldp % 8 || !al16(Hs) || !al16(pooled) || (((uintptr_t)ids) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "clip_pool: row strides must be multiples of 8 and >= D, pointers 16-byte aligned");
  hipLaunchKernelGGL(clip_pool_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, (const bf16_t*)Hs,
                     (long long)ldh, (bf16_t*)pooled, (long long)ldp, S, D, eos_token_id, eos_token_id == 2 ? 1 : 0);
  return x2i_check_launch("clip_pool");
}

}  // extern "C"
