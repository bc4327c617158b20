// The MiniCPM-o Resampler's kernels (include/x2i_resampler.h): the learned-query attention, ln_kv fused with the position add, and the
// head split of the k and v projections.  They stand behind `model.resampler` (a perceiver: NQ <= 64 learned queries cross-attend over the
// patches of each frame).  bf16 in and out, f32 arithmetic; every launcher enqueues on the caller's stream and returns.
//
// Learned-query attention.  encoder_attn_kernel (encoder_attention.hip) gives a workgroup 128 query rows of one sequence; here there are at
// most 64 query rows, the same for every sample, and up to a few thousand keys per sample.  So the mapping is turned round:
//   * one workgroup = 4 waves per (sample, head); a wave still owns 32 query rows (swapped QK^T, v_mfma_f32_32x32x16_bf16, the kvmap row
//     permutation, the K / V^T tile images and swizzles of encoder_attn_kernel at DK = 128), and the waves that would have no rows split
//     the KEYS instead.  NP = 2 (NQ > 32): wave w holds row group w & 1 and key part w >> 1.  NP = 4 (NQ <= 32): one row group, key part w
//   * a step of the walk stages 128 consecutive keys -- two 64-key tiles, double-buffered LDS-DMA, 128 KiB of LDS -- and a wave computes
//     its part of them: one whole tile at NP = 2 (the other row group's wave reads the same tile), one 32-key sub-tile at NP = 4.
//     encoder_attention_tile.inc's step owns a whole tile per wave and both of its sub-tiles; the step here is that step's SEGMENT branch
//     with the sub-tile range as a parameter, which is why it is written out and not included
//   * the trip count ceil(n_keys / 128), every DMA issue, every s_waitcnt and every barrier are uniform across the workgroup; a wave whose
//     part of a step starts at or beyond n_keys walks the step without MFMAs or exponentials.  A tile index beyond Lpad / 64 - 1 (the
//     second tile of the last step) is staged from the last tile and never computed
//   * the mask is by index: in a part that reaches past n_keys the scores of keys >= n_keys become NEG_BIG before the maximum and the sum
//     see them.  The running maximum starts at M_FLOOR and the defer-max test is per row, as in SEGMENT
//   * merge: every wave writes (m, l, O^T) to LDS (over the tiles, which nobody reads any more), and the NP waves of a row group each
//     finish 4 / NP of the four 32-wide d-blocks: m = max over the parts, l = sum of l_p exp2(m_p - m) and O likewise, parts in the
//     order 0 .. NP-1, in f32.  A part that computed nothing has m = M_FLOOR, l = 0, O = 0 and weight exp2(M_FLOOR - m) = 0; when no part
//     computed (n_keys == 0) l is 0 and the epilogue selects the zero row on it
// Nothing depends on B, on another sample or on time: a sample's result is a function of its own K, VT and n_keys, bit for bit.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_resampler.h"
#include <math.h>

namespace {

constexpr int RS_DK = 128;
constexpr int RS_TILE = KVB * RS_DK * 2;             // bytes of a K tile [64 keys][128] and of a V^T tile [128][64 keys]
constexpr int RS_SLOT = 2 * RS_TILE;                 // K tile | V^T tile
constexpr int RS_BUF = 2 * RS_SLOT;                  // the two tiles of a step
constexpr int RS_LDS = 2 * RS_BUF;                   // double-buffered: 128 KiB
constexpr int RS_STATE = 16 * 64 * 16 + 2 * 64 * 4;  // a wave's merge record: O^T as 16 float4 per lane, then m and l per lane
static_assert(4 * RS_STATE <= RS_LDS, "the merge records lie over the tiles");

template <int NP>
__global__ __launch_bounds__(256, 1) void resampler_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                const bf16_t* __restrict__ VT, const int* __restrict__ n_keys,
                                                                bf16_t* __restrict__ O, int H, int NQ, int NQpad, int L, int Lpad, float scale2,
                                                                long long ldo, long long o_bs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buffers][2 slots][K tile | V^T tile]; afterwards the merge records
  constexpr int DK = RS_DK, NT = 256, CK = DK / 8, CH = 4, NDS = DK / 16, NDB = DK / 32;
  constexpr int NU = NP == 2 ? 2 : 1;   // 32-key sub-tiles a wave computes per step
  constexpr int NKW = 32 * NU;          // keys a wave computes per step
  constexpr int THR = 8;                // defer-max threshold (exp2 domain), as encoder_attn_kernel
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int li = lane & 31;
  const int rg = NP == 2 ? (wave & 1) : 0;      // row group: query rows rg*32 .. rg*32+31
  const int kp = NP == 2 ? (wave >> 1) : wave;  // key part
  const int slot = NP == 2 ? kp : (kp >> 1);    // the tile of a step this wave reads
  const int u0 = NP == 2 ? 0 : (kp & 1);        // ... and its first sub-tile there
  // XCD-aware block order: each XCD walks a contiguous range of (sample, head) pairs, so the heads of a sample stay together
  int bid = blockIdx.x;
  {
    const int T = gridDim.x, q = T >> 3, r = T & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int h = bid % H, b = bid / H;
  const long long bh = (long long)b * H + h;
  const bf16_t* Qh = Q + (long long)h * NQpad * DK;
  const bf16_t* Kh = K + bh * Lpad * DK;
  const bf16_t* Vh = VT + bh * DK * Lpad;
  // the sample's key count, clamped into [0, L]: the host never sees it, and no tile outside [0, Lpad) may be staged
  const int nk = n_keys ? min(max(__builtin_amdgcn_readfirstlane(n_keys[b]), 0), L) : L;

  // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[rg*32+li][ds*16 + hi*8 .. +8]
  bf16x8_t qf[NDS];
  {
    const int qrow = min(rg * 32 + li, NQpad - 1);
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
      k_src[j] = row * DK + ((cphys ^ (row & (CK - 1))) << 3);
    }
    {
      const int row = p >> 3, cphys = p & 7;
      v_src[j] = row * Lpad + ((cphys ^ ((row >> 1) & 7)) << 3);
    }
  }
  const int last_tile = Lpad / KVB - 1;
  auto stage = [&](int buf, int step) {   // the step's two tiles (workgroup-uniform)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const long long kv0 = (long long)min(2 * step + s, last_tile) * KVB;
      char* kb = smem + buf * RS_BUF + s * RS_SLOT;
      char* vb = kb + RS_TILE;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        glds16(Kh + kv0 * DK + k_src[j], kb + (j * NT + wave * 64) * 16);
        glds16(Vh + kv0 + v_src[j], vb + (j * NT + wave * 64) * 16);
      }
    }
  };

  // ---- per-lane LDS read offsets
  const int kvm = (li & 0x13) | ((li & 4) << 1) | ((li & 8) >> 1);  // swap bits 2 and 3
  const int k_row_off = kvm * (2 * DK);
  const int k_swz = kvm & (CK - 1);
  const int v_row_off = li * 128;
  const int v_swz = (li >> 1) & 7;

  f32x16_t oacc[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
  float m_run = M_FLOOR, l_run = 0.f;

  const int nsteps = (nk + 2 * KVB - 1) / (2 * KVB);   // (workgroup-uniform) 0 for an empty sample
  if (nsteps > 0) {
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int n = 0; n < nsteps; ++n) {
      const int buf = n & 1;
      if (n + 1 < nsteps) stage(buf ^ 1, n + 1);   // (workgroup-uniform)
      const int kw0 = n * 2 * KVB + slot * KVB + u0 * 32;   // this wave's first key of the step
      if (kw0 < nk) {   // (wave-uniform)
        const char* kb = smem + buf * RS_BUF + slot * RS_SLOT;
        const char* vb = kb + RS_TILE;
        // ---- S^T = K Q^T
        f32x16_t sacc[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[u][r] = 0.f;
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            const bf16x8_t kf = *(const bf16x8_t*)(kb + (u0 + u) * 32 * (2 * DK) + k_row_off + (((ds * 2 + hi) ^ k_swz) << 4));
            sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ds], sacc[u], 0, 0, 0);
          }
        // lane (q = li, hi), sub-tile u, reg r  <->  key = kw0 + u*32 + 16*(r>>3) + 8*hi + (r&7)
        // ---- scores into the exp2 domain: one multiply by scale * log2 e
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[u][r] *= scale2;
        if (kw0 + NKW > nk) {   // (wave-uniform) the part reaches past the sample's keys
          const int up = nk - kw0 - 8 * hi;
#pragma unroll
          for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = u * 32 + 16 * (r >> 3) + (r & 7);
              if (c >= up) sacc[u][r] = NEG_BIG;
            }
        }
        // ---- online softmax; the defer-max test is per row (a row's result is a function of its own scores alone)
        float mx = NEG_BIG;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[u][r]);
        mx = xhalf_max(mx);
        float m_new = fmaxf(m_run, mx);
        if (m_new - m_run <= (float)THR) m_new = m_run;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u)
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
        bf16x8_t pf[NU][2];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            union { bf16x8_t v; uint32_t w[4]; } cv;
#pragma unroll
            for (int j = 0; j < 4; ++j) cv.w[j] = pack_bf16x2(sacc[u][kt * 8 + 2 * j], sacc[u][kt * 8 + 2 * j + 1]);
            pf[u][kt] = cv.v;
          }
        // ---- O^T += V^T P^T
#pragma unroll
        for (int g = 0; g < 2 * NU; ++g)
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const int u = g >> 1, kt = g & 1;
            const bf16x8_t vf = *(const bf16x8_t*)(vb + db * 32 * 128 + v_row_off + (((4 * (u0 + u) + 2 * kt + hi) ^ v_swz) << 4));
            oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[u][kt], oacc[db], 0, 0, 0);
          }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next step's DMA (issued by this wave) has landed
      __syncthreads();
    }
  }

  // ---- merge: every wave's (O^T, m, l) through LDS; nobody reads a tile after the walk's last barrier
  l_run = xhalf_sum(l_run);
  {
    char* rec = smem + wave * RS_STATE;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(float4*)(rec + ((db * 4 + g) * 64 + lane) * 16) =
            make_float4(oacc[db][4 * g], oacc[db][4 * g + 1], oacc[db][4 * g + 2], oacc[db][4 * g + 3]);
    float* ml = (float*)(rec + 16 * 64 * 16);
    ml[lane] = m_run;
    ml[64 + lane] = l_run;
  }
  __syncthreads();
  float m_p[NP], w_p[NP];
  float m_all = M_FLOOR;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int w = NP == 2 ? rg + 2 * p : p;   // the wave that holds part p of this row group
    m_p[p] = ((const float*)(smem + w * RS_STATE + 16 * 64 * 16))[lane];
    m_all = fmaxf(m_all, m_p[p]);
  }
  float l_all = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int w = NP == 2 ? rg + 2 * p : p;
    w_p[p] = __builtin_amdgcn_exp2f(m_p[p] - m_all);
    l_all = __builtin_fmaf(((const float*)(smem + w * RS_STATE + 16 * 64 * 16))[64 + lane], w_p[p], l_all);
  }
  // the zero row, selected on a sum that no counted key entered (n_keys == 0: every part is at the floor, its O^T is 0)
  const float inv = l_all > 0.f ? 1.f / l_all : 0.f;
  const int q = rg * 32 + li;
  bf16_t* orow = O + (long long)b * o_bs + (long long)q * ldo + h * DK;
  // this wave finishes the d-blocks kp * NDB / NP .. ; lane (q = li, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3)
#pragma unroll
  for (int i = 0; i < NDB / NP; ++i) {
    const int db = kp * (NDB / NP) + i;
    float o[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int w = NP == 2 ? rg + 2 * p : p;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = *(const float4*)(smem + w * RS_STATE + ((db * 4 + g) * 64 + lane) * 16);
        o[4 * g] = __builtin_fmaf(v.x, w_p[p], o[4 * g]);
        o[4 * g + 1] = __builtin_fmaf(v.y, w_p[p], o[4 * g + 1]);
        o[4 * g + 2] = __builtin_fmaf(v.z, w_p[p], o[4 * g + 2]);
        o[4 * g + 3] = __builtin_fmaf(v.w, w_p[p], o[4 * g + 3]);
      }
    }
    // half-wave exchange: two 8-byte fragments of neighbouring d-groups become one 16-byte store per lane
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const uint32_t a0 = pack_bf16x2(o[4 * g] * inv, o[4 * g + 1] * inv);
      const uint32_t a1 = pack_bf16x2(o[4 * g + 2] * inv, o[4 * g + 3] * inv);
      const uint32_t b0 = pack_bf16x2(o[4 * g + 4] * inv, o[4 * g + 5] * inv);
      const uint32_t b1 = pack_bf16x2(o[4 * g + 6] * inv, o[4 * g + 7] * inv);
      const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      if (q < NQ) *(uint4*)(orow + db * 32 + 8 * (g + hi)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- ln_kv + positions
// One wave per row.  The statistics, the affine and the rounding are ln_kernel<true>'s (elementwise.hip), statement for statement: XV is
// x2i_ln_affine_bf16 bit for bit.  XK adds the position row to the ROUNDED XV in f32 and rounds once (siglip_add_positions_kernel).
constexpr int RS_LN_MAXV = 8;  // up to D = 4096

__device__ __forceinline__ void rs_unpack8(const bf16x8_t& v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = bf16_to_f32((bf16_t)v[i]);
}
__device__ __forceinline__ bf16x8_t rs_pack8(const float (&f)[8]) {
  union { bf16x8_t v; uint32_t u[4]; } r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.u[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
  return r.v;
}

__global__ __launch_bounds__(256) void resampler_ln_pos_kernel(const bf16_t* __restrict__ X, long long ldx, const bf16_t* __restrict__ aw,
                                                               const bf16_t* __restrict__ ab, float eps, const int* __restrict__ ids,
                                                               const bf16_t* __restrict__ pos, int n_pos, bf16_t* __restrict__ XV, long long ldv,
                                                               bf16_t* __restrict__ XK, long long ldk, long long total_rows, int D) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= total_rows) return;
  const bf16_t* x = X + row * ldx;
  const int nv = D >> 3;  // 16-byte chunks per row
  float v[RS_LN_MAXV][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < RS_LN_MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      rs_unpack8(*(const bf16x8_t*)(x + c * 8), v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
  }
  const float mean = wave_sum(sum) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < RS_LN_MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = __fsub_rn(v[i][j], mean);
        sq = __builtin_fmaf(d, d, sq);
      }
    }
  }
  const float rstd = rsqrtf(__fadd_rn(wave_sum(sq) / (float)D, eps));
  int id = ids[row];
  const bool padding = id < 0;   // (wave-uniform)
  id = padding ? 0 : (id >= n_pos ? n_pos - 1 : id);
  const bf16_t* prow = pos + (long long)id * D;
#pragma unroll
  for (int i = 0; i < RS_LN_MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      float o[8], w[8], bb[8];
      rs_unpack8(*(const bf16x8_t*)(aw + c * 8), w);
      rs_unpack8(*(const bf16x8_t*)(ab + c * 8), bb);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * w[j] + bb[j];
      const bf16x8_t xv = rs_pack8(o);
      *(bf16x8_t*)(XV + row * ldv + c * 8) = xv;
      bf16x8_t xk = xv;
      if (!padding) {
        float a[8], p[8];
        rs_unpack8(xv, a);
        rs_unpack8(*(const bf16x8_t*)(prow + c * 8), p);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = __fadd_rn(a[j], p[j]);
        xk = rs_pack8(a);
      }
      *(bf16x8_t*)(XK + row * ldk + c * 8) = xk;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- head split
// siglip_head_split_kernel for two sources and no Q: one workgroup per (64-token tile, head, sample); K rows are 16-byte copies, V goes
// through v_tile_to_vt into the head's 128 V^T rows.  Only s < L is written.
__global__ __launch_bounds__(256) void resampler_kv_split_kernel(const bf16_t* __restrict__ Kr, long long ldk, const bf16_t* __restrict__ Vr,
                                                                 long long ldv, bf16_t* __restrict__ K, bf16_t* __restrict__ VT, int L, int Lpad,
                                                                 int H) {
  constexpr int DK = RS_DK, CK = DK / 8;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const long long bh = (long long)b * H + h;
  for (int c = tid; c < 64 * CK; c += 256) {
    const int tok = c / CK, ch = c - tok * CK;
    const int s = s0 + tok;
    if (s >= L) continue;
    *(uint4*)(K + (bh * Lpad + s) * DK + ch * 8) = *(const uint4*)(Kr + ((long long)b * L + s) * ldk + h * DK + ch * 8);
  }
  v_tile_to_vt(Vr + (long long)b * L * ldv + h * DK, ldv, VT + bh * DK * Lpad, s0, L, Lpad, DK);
}

inline bool overlap(const void* a, long long a_elems, const void* b, long long b_elems) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 2 * (uintptr_t)a_elems, b0 = (uintptr_t)b, b1 = b0 + 2 * (uintptr_t)b_elems;
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int x2i_resampler_attention_bf16(const void* Q, const void* K, const void* VT, const int32_t* n_keys, void* O, int32_t B, int32_t H, int32_t NQ,
                                 int32_t L, int32_t Lpad, float scale, int64_t ldo, int64_t o_batch_stride, x2i_stream_t stream) {
  const char* what = "resampler_attention";
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", what);
  if (B <= 0 || H <= 0 || NQ < 1 || NQ > 64) return x2i_set_error(X2I_ERR_SHAPE, "%s: bad shape (B=%d H=%d NQ=%d; NQ in 1..64)", what, B, H, NQ);
  if (L < 1 || Lpad < L || Lpad % 64) return x2i_set_error(X2I_ERR_SHAPE, "%s: need Lpad %% 64 == 0 and Lpad >= L >= 1 (L=%d Lpad=%d)", what, L, Lpad);
  if ((long long)B * H > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "%s: too many work items", what);
  if (!(scale > 0.f) || !isfinite(scale)) return x2i_set_error(X2I_ERR_ARG, "%s: the scale must be positive and finite", what);
  if (ldo < 128LL * H || ldo % 8 || o_batch_stride % 8 || !al16(O))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: output rows must hold 128*H elements, with ldo and o_batch_stride multiples of 8 and O 16-byte aligned", what);
  if (!al16(Q) || !al16(K) || !al16(VT) || (((uintptr_t)n_keys) & 3))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: Q, K, VT must be 16-byte aligned and n_keys 4-byte aligned", what);
  const int NQpad = (NQ + 31) / 32 * 32;
  const void* kern = NQ > 32 ? (const void*)resampler_attn_kernel<2> : (const void*)resampler_attn_kernel<4>;
  const int rc = x2i_ensure_dynamic_smem(kern, RS_LDS);
  if (rc) return rc;
  const dim3 grid((unsigned)(B * H));
  if (NQ > 32)
    hipLaunchKernelGGL(resampler_attn_kernel<2>, grid, dim3(256), RS_LDS, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)VT,
                       (const int*)n_keys, (bf16_t*)O, H, NQ, NQpad, L, Lpad, scale * LOG2E, (long long)ldo, (long long)o_batch_stride);
  else
    hipLaunchKernelGGL(resampler_attn_kernel<4>, grid, dim3(256), RS_LDS, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)VT,
                       (const int*)n_keys, (bf16_t*)O, H, NQ, NQpad, L, Lpad, scale * LOG2E, (long long)ldo, (long long)o_batch_stride);
  return x2i_check_launch(what);
}

int x2i_resampler_ln_pos_bf16(const void* X, int64_t ldx, const void* weight, const void* bias, float eps, const int32_t* ids, const void* pos,
                              int32_t n_pos, void* XV, int64_t ldv, void* XK, int64_t ldk, int64_t rows, int32_t D, x2i_stream_t stream) {
  const char* what = "resampler_ln_pos";
  if (!X || !weight || !bias || !ids || !pos || !XV || !XK) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", what);
  if (rows <= 0 || n_pos <= 0 || D <= 0 || D % 8 || D > 64 * 8 * RS_LN_MAXV || (rows + 3) / 4 > 0x7fffffffLL)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: D=%d must be a positive multiple of 8 and <= %d (rows=%lld n_pos=%d)", what, D, 64 * 8 * RS_LN_MAXV,
                         (long long)rows, n_pos);
  if (!(eps >= 0.f) || !isfinite(eps)) return x2i_set_error(X2I_ERR_ARG, "%s: eps must be finite and >= 0", what);
  if (ldx < D || ldv < D || ldk < D || ldx % 8 || ldv % 8 || ldk % 8 || !al16(X) || !al16(XV) || !al16(XK) || !al16(weight) || !al16(bias) ||
      !al16(pos) || (((uintptr_t)ids) & 3))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: row strides must be multiples of 8 and >= D, X, XV, XK, weight, bias and pos 16-byte aligned, ids 4-byte aligned", what);
  const long long ex = (rows - 1) * ldx + D, ev = (rows - 1) * ldv + D, ek = (rows - 1) * ldk + D;
  if (overlap(X, ex, XV, ev) || overlap(X, ex, XK, ek) || XV == XK) return x2i_set_error(X2I_ERR_ARG, "%s: X may alias neither output, and XV is not XK", what);
  hipLaunchKernelGGL(resampler_ln_pos_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, (long long)ldx,
                     (const bf16_t*)weight, (const bf16_t*)bias, eps, (const int*)ids, (const bf16_t*)pos, n_pos, (bf16_t*)XV, (long long)ldv,
                     (bf16_t*)XK, (long long)ldk, (long long)rows, D);
  return x2i_check_launch(what);
}

int x2i_resampler_kv_split_bf16(const void* Kr, int64_t ldk, const void* Vr, int64_t ldv, void* K, void* VT, int32_t B, int32_t L, int32_t Lpad,
                                int32_t H, x2i_stream_t stream) {
  const char* what = "resampler_kv_split";
  if (!Kr || !Vr || !K || !VT) return x2i_set_error(X2I_ERR_ARG, "%s: null pointer", what);
  if (B <= 0 || L <= 0 || H <= 0 || Lpad < L || Lpad % 8 || H > 65535 || B > 65535)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: bad shape (B=%d L=%d Lpad=%d H=%d)", what, B, L, Lpad, H);
  if (ldk < 128LL * H || ldv < 128LL * H || ldk % 8 || ldv % 8 || !al16(Kr) || !al16(Vr) || !al16(K) || !al16(VT))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: ldk and ldv must be multiples of 8 and >= 128*H, pointers 16-byte aligned", what);
  hipLaunchKernelGGL(resampler_kv_split_kernel, dim3((L + 63) / 64, H, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)Kr, (long long)ldk,
                     (const bf16_t*)Vr, (long long)ldv, (bf16_t*)K, (bf16_t*)VT, L, Lpad, H);
  return x2i_check_launch(what);
}

}  // extern "C"
