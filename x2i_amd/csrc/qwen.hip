// The Qwen2 decoder prefill's kernels (include/x2i_qwen.h): causal flash attention with grouped key/value heads and a per-sample key range
// for 64- and 128-wide heads, rotate-half RoPE with the head split in front of it, and the SwiGLU gate.  They stand behind `transformers`'
// Qwen2Attention / apply_rotary_pos_emb (apply_multimodal_rotary_pos_emb) / Qwen2MLP as the MLLMs of the reference's sampling scripts run
// them over a prompt (infer/inference_*.py).  bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
//
// Attention: clip_attn_kernel (clip.hip) with the head width as a template parameter, as t5_attn_kernel<DK> (t5.hip) has it, plus
//   * grouped heads: query head h streams the K / V^T tiles of key/value head h / (Hq / Hkv); the XCD-aware block order keeps the query heads
//     of a group next to each other on one XCD, so that the group's tiles are served from that XCD's L2
//   * a key range [klo, khi) per sample (read from device memory, clamped into [0, S]); key j counts for row i iff klo <= j <= min(i, khi - 1)
//   * a workgroup (query rows r0 .. r0+127) walks the key tiles klo / 64 .. min((min(S, r0 + 128) - 1) / 64, (khi - 1) / 64) only -- none when
//     the range is empty or starts after its last row: the trip count, every DMA issue, every s_waitcnt and every barrier are uniform
//     across the workgroup
//   * a wave (rows q0 .. q0+31) computes a tile only when the tile starts at or before q0, when q0 < S and when one of its rows reaches the
//     range (q0 + 31 >= klo); otherwise it walks the loop (stage, wait, barrier) without MFMAs or exponentials
//   * the mask is by index: in a tile that reaches past min(q0, khi - 1) or starts before klo, a score of a key that does not count becomes
//     NEG_BIG before the maximum and the sum see it, whatever K and V^T hold there
//   * rows with no counted key.  With klo inside a wave's 32 rows, the rows before klo of a computing wave see only masked scores.  clip.hip
//     starts the running maximum AT NEG_BIG and relies on a real score in every row's first tile; here such a row would keep that maximum,
//     exponentiate every masked score to exp2(0) = 1 and come out as the plain average of whatever V^T holds.  So the running maximum starts
//     at M_FLOOR = -1e15, far above NEG_BIG = -1e30 and far below any score: a masked score gives exp2(NEG_BIG - m) = 0 against a real
//     maximum and against the floor alike, such a row's sum stays exactly 0, and the epilogue selects the zero row on that sum (l == 0),
//     which waves that never computed a tile share
#include "x2i_common.h"
#include "../../include/x2i_qwen.h"

namespace {

constexpr int KVB = 64;          // keys per tile
constexpr float NEG_BIG = -1.0e30f;
constexpr float M_FLOOR = -1.0e15f;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int DK>
__global__ __launch_bounds__(256, 2) void qwen_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                           const bf16_t* __restrict__ VT, const int* __restrict__ k_lo,
                                                           const int* __restrict__ k_hi, bf16_t* __restrict__ O, int H, int rep, int S,
                                                           int Spad, float scale2, int ldo, long long o_bs, int nbatch) {
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
  const int Hkv = H / rep;
  const long long bh = (long long)b * H + h;
  const long long bg = (long long)b * Hkv + h / rep;   // repeat_kv: query head h reads key/value head h / rep
  const bf16_t* Qh = Q + bh * Spad * DK;
  const bf16_t* Kh = K + bg * Spad * DK;
  const bf16_t* Vh = VT + bg * DK * Spad;
  // the sample's key range, clamped into [0, S]: the host never sees these values, and no tile outside [0, Spad) may be staged
  const int klo = k_lo ? min(max(__builtin_amdgcn_readfirstlane(k_lo[b]), 0), S) : 0;
  const int khi = k_hi ? min(max(__builtin_amdgcn_readfirstlane(k_hi[b]), 0), S) : S;

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
  float m_run = M_FLOOR, l_run = 0.f;

  // workgroup-uniform: the key tiles t_lo .. t_hi, from the tile that holds klo up to this query block's diagonal and the tile that holds khi - 1
  const int t_lo = klo / KVB;
  const int t_hi = (min(min(S, qt * 128 + 128), khi) - 1) / KVB;
  const int ntiles = khi > klo ? t_hi - t_lo + 1 : 0;   // (<= 0: nothing to walk; every row of the block is a zero row)
  // wave-uniform: the last tile this wave computes (the one its first row lies in), and none for a wave past S or wholly before klo
  const int t_wave = (q0 < S && q0 + 31 >= klo) ? q0 / KVB : -1;
  const int q = q0 + li;
  const int qlim = min(q, khi - 1);   // the last key of this lane's row (khi <= S: rows i >= S, never written, behave as row S - 1 at most)

  if (ntiles > 0) {   // (workgroup-uniform)
    stage(0, t_lo * KVB);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // the first tile is in LDS

    for (int n = 0; n < ntiles; ++n) {
      const int t = t_lo + n;
      const int buf = n & 1;
      if (n + 1 < ntiles) stage(buf ^ 1, (t + 1) * KVB);   // (workgroup-uniform)
      if (t <= t_wave) {                                   // (wave-uniform)
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
        if (kv0 + (KVB - 1) > min(q0, khi - 1) || kv0 < klo) {   // (wave-uniform) the tile holds a key that does not count for one of this wave's rows
          const int up = qlim - kv0 - 8 * hi;
          const int dn = klo - kv0 - 8 * hi;
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = u * 32 + 16 * (r >> 3) + (r & 7);
              if (c > up || c < dn) sacc[u][r] = NEG_BIG;
            }
        }
        // ---- online softmax
        float mx = NEG_BIG;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[u][r]);
        mx = xhalf_max(mx);
        // defer-max: keep the old running max while no row of this wave grew by more than THR, so that the O rescale is skipped on most tiles.
        // (A row's first real score leaves M_FLOOR by far more than THR, so the test fails and m_new is real; a row that has seen no counted
        // key keeps M_FLOOR, against which a masked score still exponentiates to 0.)
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
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane (q = li, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3)
  l_run = xhalf_sum(l_run);
  // the zero row, selected on a row sum that no counted key entered: rows before klo, an empty range, and waves that computed no tile
  // (their accumulators are still 0; 0 * finite V^T is 0 in the rows of a computing wave)
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
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
int launch_qwen_attention(const void* Q, const void* K, const void* VT, const int* k_lo, const int* k_hi, void* O, int B, int Hq, int Hkv, int S,
                          int Spad, float scale, int ldo, long long o_bs, hipStream_t stream) {
  constexpr int TILES = 2 * 2 * KVB * DK * 2;
  const int rc = x2i_ensure_dynamic_smem((const void*)qwen_attn_kernel<DK>, TILES);
  if (rc) return rc;
  const dim3 grid((unsigned)(((S + 127) / 128) * Hq * B));
  hipLaunchKernelGGL((qwen_attn_kernel<DK>), grid, dim3(256), TILES, stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)VT, k_lo, k_hi,
                     (bf16_t*)O, Hq, Hq / Hkv, S, Spad, scale * LOG2E, ldo, o_bs, B);
  return x2i_check_launch("qwen_attention");
}

__device__ __forceinline__ void unpack8(const uint4& p, float (&v)[8]) {
  v[0] = __uint_as_float(p.x << 16); v[1] = __uint_as_float(p.x & 0xffff0000u);
  v[2] = __uint_as_float(p.y << 16); v[3] = __uint_as_float(p.y & 0xffff0000u);
  v[4] = __uint_as_float(p.z << 16); v[5] = __uint_as_float(p.z & 0xffff0000u);
  v[6] = __uint_as_float(p.w << 16); v[7] = __uint_as_float(p.w & 0xffff0000u);
}

// ------------------------------------------------------------------------------------------------------------------- RoPE + head split
// One workgroup per (64-token tile, head, sample); heads 0 .. Hq-1 are query heads, Hq .. Hq+Hkv-1 key/value heads.  A work item rotates
// eight pairs (x[d], x[d + dk/2]), d = 8c .. 8c+7: two 16-byte loads of the row, two 32-byte pieces of each half table, two 16-byte stores.
// A key/value head's V goes through an LDS tile [64 tokens][dk + 2] and leaves as 16-byte pieces of VT rows, as t5_head_split_kernel's
// does (scalar stores in the one piece that straddles S: columns >= S stay untouched).
__global__ __launch_bounds__(256) void qwen_rope_split_kernel(const bf16_t* __restrict__ qkv, long long ld, const float* __restrict__ cs,
                                                              const float* __restrict__ sn, bf16_t* __restrict__ Q, bf16_t* __restrict__ K,
                                                              bf16_t* __restrict__ VT, int S, int Spad, int Hq, int Hkv, int dk) {
  __shared__ uint32_t tile[64 * (128 + 2) / 2];
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, hh = blockIdx.y, b = blockIdx.z;
  const bool is_q = hh < Hq;
  const int g = hh - Hq;            // key/value head (when !is_q)
  const int half = dk >> 1;
  const int cr = dk >> 4;           // work items per token: 16-byte chunks of one half
  const int col = is_q ? hh * dk : (Hq + g) * dk;   // the head's first column in q | k
  bf16_t* dst_base = is_q ? Q + ((long long)b * Hq + hh) * Spad * dk : K + ((long long)b * Hkv + g) * Spad * dk;
  for (int c = tid; c < 64 * cr; c += 256) {
    const int tok = c / cr, ch = c - tok * cr;
    const int s = s0 + tok;
    if (s >= S) continue;
    const bf16_t* src = qkv + ((long long)b * S + s) * ld + col + ch * 8;
    const float* cp = cs + ((long long)b * S + s) * half + ch * 8;
    const float* sp = sn + ((long long)b * S + s) * half + ch * 8;
    float x1[8], x2[8];
    unpack8(*(const uint4*)src, x1);
    unpack8(*(const uint4*)(src + half), x2);
    const float4 c0 = *(const float4*)cp, c1 = *(const float4*)(cp + 4), t0 = *(const float4*)sp, t1 = *(const float4*)(sp + 4);
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float ss[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    uint32_t lo[4], up[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // one rounding: both products and their sum stay f32 (the library rounds each product and the sum to bf16)
      lo[j >> 1] = pack_bf16x2(__fsub_rn(__fmul_rn(x1[j], cc[j]), __fmul_rn(x2[j], ss[j])),
                               __fsub_rn(__fmul_rn(x1[j + 1], cc[j + 1]), __fmul_rn(x2[j + 1], ss[j + 1])));
      up[j >> 1] = pack_bf16x2(__fadd_rn(__fmul_rn(x2[j], cc[j]), __fmul_rn(x1[j], ss[j])),
                               __fadd_rn(__fmul_rn(x2[j + 1], cc[j + 1]), __fmul_rn(x1[j + 1], ss[j + 1])));
    }
    bf16_t* dst = dst_base + (long long)s * dk + ch * 8;
    *(uint4*)dst = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *(uint4*)(dst + half) = make_uint4(up[0], up[1], up[2], up[3]);
  }
  if (is_q) return;   // (uniform across the workgroup)

  // ---- V of key/value head g -> VT
  const int ck = dk >> 3;           // 16-byte chunks per head row
  const int pitch = (dk + 2) >> 1;  // LDS row pitch in dwords
  const int vcol = (Hq + Hkv + g) * dk;
  for (int c = tid; c < 64 * ck; c += 256) {
    const int tok = c / ck, ch = c - tok * ck;
    const int s = s0 + tok;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (s < S) v = *(const uint4*)(qkv + ((long long)b * S + s) * ld + vcol + ch * 8);
    uint32_t* t = tile + tok * pitch + ch * 4;
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
  }
  __syncthreads();
  const bf16_t* tb = (const bf16_t*)tile;
  const long long bg = (long long)b * Hkv + g;
  for (int i = tid; i < dk * 8; i += 256) {
    const int tc = i & 7, d = i >> 3;
    const int s = s0 + tc * 8;
    if (s >= S) continue;
    bf16_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = tb[(tc * 8 + j) * (2 * pitch) + d];
    bf16_t* dst = VT + (bg * dk + d) * Spad + s;
    if (s + 8 <= S) {
      *(uint4*)dst = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (s + j < S) dst[j] = e[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- SwiGLU
__global__ __launch_bounds__(256) void qwen_swiglu_kernel(const bf16_t* __restrict__ AB, long long ld_in, bf16_t* __restrict__ Y, long long ldy,
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
      // one rounding: the activation stays f32 until the up projection has multiplied it (the library rounds it to bf16 in between)
      o[j >> 1] = pack_bf16x2(__fmul_rn(silu_f(a[j]), g[j]), __fmul_rn(silu_f(a[j + 1]), g[j + 1]));
    }
    *(uint4*)(Y + row * ldy + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" {

int x2i_qwen_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* k_lo, const int32_t* k_hi, void* O, int32_t B,
                            int32_t Hq, int32_t Hkv, int32_t S, int32_t Spad, int32_t dk, float scale, int32_t ldo, int64_t o_batch_stride,
                            x2i_stream_t stream) {
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "qwen_attention: null pointer");
  if ((k_lo == nullptr) != (k_hi == nullptr))
    return x2i_set_error(X2I_ERR_ARG, "qwen_attention: k_lo and k_hi must both be null or both be given");
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "qwen_attention: head width dk=%d is not one of 64, 128", dk);
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_attention: need Hq %% Hkv == 0 (B=%d Hq=%d Hkv=%d)", B, Hq, Hkv);
  if (S <= 0 || Spad < S || Spad % 64)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_attention: need Spad %% 64 == 0 and Spad >= S (S=%d Spad=%d)", S, Spad);
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "qwen_attention: scale must be positive and finite");
  if ((long long)((S + 127) / 128) * Hq * B > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "qwen_attention: too many work items");
  if (ldo < (long long)Hq * dk || ldo % 4 || o_batch_stride % 4 || (((uintptr_t)O) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_attention: output rows must hold Hq*dk elements and be 8-byte aligned");
  if (!al16(Q) || !al16(K) || !al16(VT) || (((uintptr_t)k_lo) & 3) || (((uintptr_t)k_hi) & 3))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_attention: Q, K, VT must be 16-byte aligned, k_lo and k_hi 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dk == 64) return launch_qwen_attention<64>(Q, K, VT, k_lo, k_hi, O, B, Hq, Hkv, S, Spad, scale, ldo, o_batch_stride, st);
  return launch_qwen_attention<128>(Q, K, VT, k_lo, k_hi, O, B, Hq, Hkv, S, Spad, scale, ldo, o_batch_stride, st);
}

int x2i_qwen_rope_split_bf16(const void* qkv, int64_t ld, const float* cos, const float* sin, void* Q, void* K, void* VT, int32_t B,
                             int32_t S, int32_t Spad, int32_t Hq, int32_t Hkv, int32_t dk, x2i_stream_t stream) {
  if (!qkv || !cos || !sin || !Q || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "qwen_rope_split: null pointer");
  if (dk != 64 && dk != 128) return x2i_set_error(X2I_ERR_SHAPE, "qwen_rope_split: head width dk=%d is not one of 64, 128", dk);
  if (B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || Spad < S || Spad % 8 || Hq + Hkv > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "qwen_rope_split: bad shape (B=%d S=%d Spad=%d Hq=%d Hkv=%d)", B, S, Spad, Hq, Hkv);
  if (ld < ((long long)Hq + 2LL * Hkv) * dk || ld % 8 || !al16(qkv) || !al16(cos) || !al16(sin) || !al16(Q) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_rope_split: ld must be a multiple of 8 and >= (Hq+2*Hkv)*dk, pointers 16-byte aligned");
  hipLaunchKernelGGL(qwen_rope_split_kernel, dim3((S + 63) / 64, Hq + Hkv, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (long long)ld,
                     cos, sin, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)VT, S, Spad, Hq, Hkv, dk);
  return x2i_check_launch("qwen_rope_split");
}

int x2i_qwen_swiglu_bf16(const void* AB, int64_t ld_in, void* Y, int64_t ldy, int64_t rows, int32_t F, x2i_stream_t stream) {
  if (!AB || !Y) return x2i_set_error(X2I_ERR_ARG, "qwen_swiglu: null pointer");
  if (rows <= 0 || F <= 0 || F % 8) return x2i_set_error(X2I_ERR_SHAPE, "qwen_swiglu: F=%d must be a positive multiple of 8", F);
  if (ld_in < 2LL * F || ldy < F || ld_in % 8 || ldy % 8 || !al16(AB) || !al16(Y))
    return x2i_set_error(X2I_ERR_ALIGN, "qwen_swiglu: row strides must be multiples of 8 (ld_in >= 2F, ldy >= F), pointers 16-byte aligned");
  const long long chunks = (long long)rows * (F / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 < 8192 ? (chunks + 255) / 256 : 8192);
  hipLaunchKernelGGL(qwen_swiglu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)AB, (long long)ld_in, (bf16_t*)Y,
                     (long long)ldy, (long long)rows, F);
  return x2i_check_launch("qwen_swiglu");
}

}  // extern "C"
