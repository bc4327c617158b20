// Sampled token selection of Qwen2 decoding (include/ext/sample/x2i_sample.h): temperature, top-k, top-p and one inverse-CDF draw over the
// f32 scores that the head launch (qwen_head.hip) left, in the place of that file's greedy select.
//   One workgroup of 1024 lanes per sample.  Every pass reads the sample's row of scores (600 KB at V = 151 936, from L2) and none writes it.
//   The two thresholds come from a most-significant-digit-first radix select over the order-preserving integer image of the scores:
//   four passes of one 8-bit digit, a 256-bin LDS histogram per pass -- of counts for top-k, of mass for top-p -- and wave 0 picks the bin.
//   The keys are those of p, not of s = p / temperature: the division is monotone, so the k-th largest p gives the k-th largest s, and the
//   passes that only count do not divide (one CU's vector rate, not its loads, is what a pass costs).  Distinct p can share one s, and
//   equal s are kept together: a threshold found among the p is widened to the smallest p with the same s, by bisection over the keys.
//   Mass is integer fixed point (round(exp(s - s_max) * 2^34), 64-bit sums): integer addition is associative, so LDS atomics, the lanes'
//   run-length combining and the scans below give the same bits in any order.  No floating-point value is ever summed.
//   The draw: per-segment masses in ascending token order (one wave per segment, a plain store each), an integer scan over the segments, and
//   wave 0 walks the one segment that holds u * Z.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "qwen_head_book.h"
#include "../../include/ext/sample/x2i_sample.h"

#include <cmath>

namespace {

using head_book::HDR;
using head_book::NO_STEP;
typedef unsigned long long u64;

constexpr int NT = 1024, NW = NT / 64;
constexpr int MAXSEG = 2048;          // segments of the draw: 16 KB of LDS
constexpr float MASS_ONE = (float)(1ull << X2I_SAMPLE_MASS_BITS);
constexpr float TWO64 = 18446744073709551616.f;
static_assert(X2I_SAMPLE_MASS_BITS + 29 <= 63, "2^29 weights of at most one unit each fit 64 bits");

struct SampleArgs {
  const float* logits; long long ldl;
  const float* ws; int nwg;
  float temperature; int top_k; float top_p;
  const u64* rng; const float* u_in; float* diag;
  int32_t* step; long long* token; long long* sequences; long long ld_seq; int ncols; long long* lengths; uint8_t* done;
  const long long* eos; int n_eos; long long pad; uint8_t* seen; long long ld_seen; int V;
};

// larger float <=> larger key (-0 lies below +0: widen() below joins what compares equal after the division)
__device__ inline uint32_t key_of(float s) {
  const uint32_t u = __float_as_uint(s);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ inline float val_of(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
__device__ inline float score(float p, float t) {
  const float s = __fdiv_rn(p, t);
  return s == 0.f ? 0.f : s;
}
__device__ inline u64 mass_of(float s, float smax) {
  float d = s - smax;
  d = d < 0.f ? d : 0.f;                                        // (a maximum the workspace got wrong, or a NaN: one unit, never more)
  return __float2ull_rn(expf(d) * MASS_ONE);
}
// x in [0, 1) as the 64-bit fraction floor(x * 2^64); exact for every f32 x >= 2^-40
__device__ inline u64 frac64(float x) {
  if (!(x > 0.f)) return 0;
  if (x >= 1.f) return ~0ull;
  return __float2ull_rz(x * TWO64);
}

__device__ inline u64 wave_incl_scan(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ inline uint32_t philox_word0(u64 seed, u64 ctr, uint32_t b) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = b, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// f(p) for every score of the row, each exactly once, in no particular order.  A lane has UNROLL loads in flight: one workgroup reads the row,
// and with one load per wave in flight a pass is nothing but 37 L2 latencies in a row.
constexpr int UNROLL = 8;
template <class F>
__device__ inline void for_each_score(const float* __restrict__ row, int V, bool vec, F f) {
  if (vec) {
    const float4* r4 = (const float4*)row;
    const int n4 = V >> 2;
    int i = threadIdx.x;
    for (; i + (UNROLL - 1) * NT < n4; i += UNROLL * NT) {
      float4 v[UNROLL];
#pragma unroll
      for (int q = 0; q < UNROLL; ++q) v[q] = r4[i + q * NT];
#pragma unroll
      for (int q = 0; q < UNROLL; ++q) { f(v[q].x); f(v[q].y); f(v[q].z); f(v[q].w); }
    }
    for (; i < n4; i += NT) {
      const float4 v = r4[i];
      f(v.x); f(v.y); f(v.z); f(v.w);
    }
  } else {
    int n = threadIdx.x;
    for (; n + (UNROLL - 1) * NT < V; n += UNROLL * NT) {
      float v[UNROLL];
#pragma unroll
      for (int q = 0; q < UNROLL; ++q) v[q] = row[n + q * NT];
#pragma unroll
      for (int q = 0; q < UNROLL; ++q) f(v[q]);
    }
    for (; n < V; n += NT) f(row[n]);
  }
}

// The radix select over the keys of p.  COUNT (MASS = false): -> the k-th largest key; `target` is k.  MASS: -> the smallest key K such that
// the mass of the keys > K among those >= floor_key is < top_p * Zk, Zk the mass of all keys >= floor_key; `target` is frac64(top_p).
// In both, with `base` what lies above the prefix's range: the digit is the first bin from the top with base + (inclusive sum) >= goal,
// the lowest bin if there is none, and base grows by the bins above it.
template <bool MASS>
__device__ uint32_t radix_select(const float* __restrict__ row, int V, bool vec, float t, float smax, uint32_t floor_key, u64 target, u64* hist,
                                 u64* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t prefix = 0;
  if (threadIdx.x == 0) { sh[0] = 0; sh[1] = target; }           // base, goal
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    uint32_t run_d = 0;
    u64 run_a = 0;                                              // a lane adds a run of equal digits once: the top digits of scores repeat
    for_each_score(row, V, vec, [&](float p) {
      const uint32_t k = key_of(p);
      if ((pass == 0 || (k >> (shift + 8)) == prefix) && (!MASS || k >= floor_key)) {
        const uint32_t d = (k >> shift) & 255u;
        if (d != run_d) {
          if (run_a) atomicAdd(&hist[run_d], run_a);
          run_d = d;
          run_a = 0;
        }
        run_a += MASS ? mass_of(score(p, t), smax) : 1ull;
      }
    });
    if (run_a) atomicAdd(&hist[run_d], run_a);
    __syncthreads();
    if (wave == 0) {                                            // lane L holds the bins 255 - 4 L - e, e = 0..3: from the top
      u64 c[4], tot = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) { c[e] = hist[255 - 4 * lane - e]; tot += c[e]; }
      const u64 incl = wave_incl_scan(tot, lane);
      const u64 base = sh[0];
      u64 goal = sh[1];
      if (MASS && pass == 0) {                                  // goal = ceil(top_p * Zk): an integer m is < top_p * Zk exactly when m < goal
        const u64 zk = __shfl(incl, 63);
        goal = __umul64hi(zk, target) + ((zk * target) != 0 ? 1 : 0);
      }
      const u64 hit = __ballot(base + incl >= goal);
      const int first = hit ? __ffsll((long long)hit) - 1 : 63;
      if (lane == first) {
        u64 above = base + incl - tot;
        int e = 0;
        for (; e < 3; ++e) {
          if (hit && above + c[e] >= goal) break;
          above += c[e];
        }
        if (!hit) e = 3;                                        // (above then holds everything but bin 0)
        sh[0] = above;
        sh[1] = goal;
        sh[2] = (u64)(255 - 4 * lane - e);
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (uint32_t)sh[2];
  }
  __syncthreads();
  return prefix;
}

// The smallest key of p whose s = p / temperature is not below the s of key `hi`: every p that shares the threshold's s is kept with it.
// score() is monotone over the keys up to hi (below -inf lie the negative NaNs, for which the test is false), so this is a bisection.
__device__ inline uint32_t widen(uint32_t hi, float t) {
  const float thr = score(val_of(hi), t);
  uint32_t lo = 0;                                              // the answer is in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (score(val_of(mid), t) >= thr) hi = mid;
    else lo = mid + 1;
  }
  return hi;
}

__global__ __launch_bounds__(NT) void sample_select_kernel(SampleArgs a) {
  __shared__ u64 hist[256];
  __shared__ u64 segsum[MAXSEG];
  __shared__ u64 sh[4];
  __shared__ u64 wtot[NW];
  __shared__ u64 sh_excl;
  __shared__ uint32_t sh_kmax, sh_kmin;
  __shared__ int sh_cnt, sh_nmax, sh_seg, sh_tok;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
  const float* __restrict__ row = a.logits + (long long)b * a.ldl;
  const bool vec = ((((uintptr_t)row) & 15) == 0) && (V & 3) == 0;
  const float t = a.temperature;

  if (tid == 0) { sh_kmax = 0; sh_kmin = 0xffffffffu; sh_cnt = 0; sh_nmax = -1; sh_seg = -1; sh_tok = -1; }
  __syncthreads();
  {                                                             // the softmax's maximum: the largest partial of the head launch
    const float2* part = (const float2*)(a.ws + HDR) + (long long)b * a.nwg;
    uint32_t km = 0;
    for (int g = tid; g < a.nwg; g += NT) {
      const uint32_t k = key_of(part[g].x);
      km = k > km ? k : km;
    }
    atomicMax(&sh_kmax, km);
  }
  __syncthreads();
  const float smax = score(val_of(sh_kmax), t);
  const int col = __float_as_int(a.ws[0]);

  float u;
  if (a.u_in) {
    u = a.u_in[b];
    u = u >= 0.f ? (u < 1.f ? u : 0x1.fffffep-1f) : 0.f;
  } else {
    const u64 c = a.rng[1] + (u64)(long long)(col == NO_STEP ? 0 : col);
    u = (float)(philox_word0(a.rng[0], c, (uint32_t)b) >> 8) * 0x1p-24f;
  }

  uint32_t thr_key = 0;
  const int k = a.top_k < V ? a.top_k : V;
  if (a.top_k > 0 && k < V) thr_key = widen(radix_select<false>(row, V, vec, t, smax, 0u, (u64)k, hist, sh), t);
  if (a.top_p < 1.f) {
    const uint32_t tp = widen(radix_select<true>(row, V, vec, t, smax, thr_key, frac64(a.top_p), hist, sh), t);
    thr_key = tp > thr_key ? tp : thr_key;
  }

  // the kept set in ascending token order: a segment is 256 m consecutive tokens, a unit of it one wave-wide load
  const int per = vec ? 4 : 1, unit_len = 64 * per;
  const int seg_len = 256 * (int)(((long long)V + 256ll * MAXSEG - 1) / (256ll * MAXSEG));
  const int nseg = (V + seg_len - 1) / seg_len, units = seg_len / unit_len;
  auto kept_mass = [&](float p) -> u64 { return key_of(p) >= thr_key ? mass_of(score(p, t), smax) : 0ull; };
  {
    int cnt = 0, nmax = -1;
    uint32_t kmin = 0xffffffffu;
    auto take = [&](int n, float p, u64& sum) {
      const uint32_t ky = key_of(p);
      if (ky >= thr_key) {
        sum += mass_of(score(p, t), smax);
        ++cnt;
        kmin = ky < kmin ? ky : kmin;
        nmax = n > nmax ? n : nmax;
      }
    };
    constexpr int SEGS = 4;                                     // a wave has the loads of four segments in flight
    for (int seg0 = wave; seg0 < nseg; seg0 += SEGS * NW) {
      u64 sum[SEGS] = {0, 0, 0, 0};
      for (int j = 0; j < units; ++j) {
        float4 v[SEGS];
        int n0[SEGS];
#pragma unroll
        for (int q = 0; q < SEGS; ++q) {
          const int seg = seg0 + q * NW;
          n0[q] = seg < nseg ? seg * seg_len + j * unit_len + lane * per : V;
          if (n0[q] < V) {
            if (vec) v[q] = *(const float4*)(row + n0[q]);
            else v[q].x = row[n0[q]];
          }
        }
#pragma unroll
        for (int q = 0; q < SEGS; ++q) {
          if (n0[q] < V) {
            take(n0[q], v[q].x, sum[q]);
            if (vec) { take(n0[q] + 1, v[q].y, sum[q]); take(n0[q] + 2, v[q].z, sum[q]); take(n0[q] + 3, v[q].w, sum[q]); }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < SEGS; ++q) {
        const u64 total = wave_sum(sum[q]);
        if (lane == 0 && seg0 + q * NW < nseg) segsum[seg0 + q * NW] = total;
      }
    }
    if (cnt) {
      atomicAdd(&sh_cnt, cnt);
      atomicMin(&sh_kmin, kmin);
      atomicMax(&sh_nmax, nmax);
    }
  }
  __syncthreads();

  // the segment that holds u * Z: thread t scans the segments 2 t and 2 t + 1
  const u64 a0 = 2 * tid < nseg ? segsum[2 * tid] : 0, a1 = 2 * tid + 1 < nseg ? segsum[2 * tid + 1] : 0;
  const u64 incl = wave_incl_scan(a0 + a1, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  u64 before = 0, Z = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    before += w < wave ? wtot[w] : 0;
    Z += wtot[w];
  }
  const u64 goal = __umul64hi(Z, frac64(u));                      // an integer m is > u * Z exactly when m > floor(u * Z); goal < Z where Z > 0
  const u64 e0 = before + incl - (a0 + a1), e1 = e0 + a0;
  if (a0 && e0 <= goal && goal < e0 + a0) { sh_seg = 2 * tid; sh_excl = e0; }
  if (a1 && e1 <= goal && goal < e1 + a1) { sh_seg = 2 * tid + 1; sh_excl = e1; }
  __syncthreads();

  if (wave == 0 && sh_seg >= 0) {
    const int seg = sh_seg;
    u64 cum = sh_excl;
    for (int j = 0; j < units; ++j) {
      const int n0 = seg * seg_len + j * unit_len + lane * per;
      u64 m[4] = {0, 0, 0, 0};
      if (n0 < V) {
        if (vec) {
          const float4 v = *(const float4*)(row + n0);
          m[0] = kept_mass(v.x); m[1] = kept_mass(v.y); m[2] = kept_mass(v.z); m[3] = kept_mass(v.w);
        } else {
          m[0] = kept_mass(row[n0]);
        }
      }
      const u64 mine = m[0] + m[1] + m[2] + m[3];
      const u64 upto = cum + wave_incl_scan(mine, lane);
      const u64 hit = __ballot(upto > goal);
      if (hit) {
        if (lane == __ffsll((long long)hit) - 1) {
          u64 runsum = upto - mine;
          int e = 0;
          for (; e < 3; ++e) {
            runsum += m[e];
            if (runsum > goal) break;
          }
          sh_tok = n0 + e;
        }
        break;
      }
      cum = __shfl(upto, 63);
    }
  }
  __syncthreads();
  if (tid != 0) return;
  if (a.diag) {
    float* d = a.diag + 4 * b;
    d[0] = (float)sh_cnt;
    d[1] = score(val_of(sh_kmin), t);
    d[2] = (float)Z * (1.f / MASS_ONE);
    d[3] = u;
  }
  const int pick = sh_tok >= 0 ? sh_tok : sh_nmax;              // rounding left none: the largest kept index
  head_book::generated_token(b, pick, col, V, a.step, a.token, a.sequences, a.ld_seq, a.ncols, a.lengths, a.done, a.eos, a.n_eos, a.pad, a.seen,
                             a.ld_seen);
}

}  // namespace

extern "C" {

int x2i_sample_select_f32(const float* logits, int64_t ldl, const float* ws, int64_t ws_floats, float temperature, int32_t top_k, float top_p,
                          const void* rng, const float* u_in, float* diag, int32_t* step, int64_t* token, int64_t* sequences, int64_t ld_seq,
                          int32_t ncols, int64_t* lengths, uint8_t* done, const int64_t* eos, int32_t n_eos, int64_t pad, uint8_t* seen,
                          int64_t ld_seen, int32_t B, int32_t V, x2i_stream_t stream) {
  if (!logits || !ws || !step || !token || !sequences || !lengths || !done) return x2i_set_error(X2I_ERR_ARG, "sample_select: null pointer");
  if (!rng && !u_in) return x2i_set_error(X2I_ERR_ARG, "sample_select: null pointer (one of rng and u_in is needed)");
  if (B < 1 || B > 8) return x2i_set_error(X2I_ERR_SHAPE, "sample_select: B=%d is not in 1..8", B);
  if (V <= 0 || V > (1 << 29)) return x2i_set_error(X2I_ERR_SHAPE, "sample_select: V=%d is not in 1..2^29", V);
  if (!(temperature > 0.f) || !std::isfinite(temperature))
    return x2i_set_error(X2I_ERR_ARG, "sample_select: the temperature must be positive and finite");
  if (top_k < 0) return x2i_set_error(X2I_ERR_ARG, "sample_select: top_k=%d is negative", top_k);
  if (!(top_p > 0.f) || !(top_p <= 1.f)) return x2i_set_error(X2I_ERR_ARG, "sample_select: top_p=%g is not in (0, 1]", (double)top_p);
  if (n_eos < 0 || n_eos > 8) return x2i_set_error(X2I_ERR_ARG, "sample_select: n_eos=%d is not in 0..8", n_eos);
  if (n_eos > 0 && !eos) return x2i_set_error(X2I_ERR_ARG, "sample_select: null pointer (eos with n_eos=%d)", n_eos);
  if (pad < 0 || pad >= V) return x2i_set_error(X2I_ERR_ARG, "sample_select: pad=%lld is not a token of the vocabulary [0, %d)", (long long)pad, V);
  if (ldl < V || ncols < 0 || ld_seq < ncols || (seen && ld_seen < V))
    return x2i_set_error(X2I_ERR_SHAPE, "sample_select: need ldl >= V, ncols >= 0, ld_seq >= ncols and ld_seen >= V (ldl=%lld, ncols=%d)",
                         (long long)ldl, ncols);
  if (!al16(ws) || (((uintptr_t)step) & 3) || (((uintptr_t)token) & 7) || (((uintptr_t)sequences) & 7) || (((uintptr_t)lengths) & 7) ||
      (((uintptr_t)eos) & 7) || (((uintptr_t)rng) & 7) || (((uintptr_t)logits) & 3) || (((uintptr_t)u_in) & 3) || (((uintptr_t)diag) & 3))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "sample_select: ws must be 16-byte, rng, token, sequences, lengths and eos 8-byte, logits, u_in, diag and step 4-byte "
                         "aligned");
  const int64_t need = X2I_SAMPLE_HEAD_WS_FLOATS(B, V);
  if (ws_floats < need)
    return x2i_set_error(X2I_ERR_SHAPE, "sample_select: workspace too small (%lld f32 given, %lld needed)", (long long)ws_floats, (long long)need);
  SampleArgs a;
  a.logits = logits; a.ldl = ldl; a.ws = ws; a.nwg = (V + 15) / 16;
  a.temperature = temperature; a.top_k = top_k; a.top_p = top_p;
  a.rng = (const u64*)rng; a.u_in = u_in; a.diag = diag;
  a.step = step; a.token = (long long*)token; a.sequences = (long long*)sequences; a.ld_seq = ld_seq; a.ncols = ncols;
  a.lengths = (long long*)lengths; a.done = done; a.eos = (const long long*)eos; a.n_eos = n_eos; a.pad = pad; a.seen = seen; a.ld_seen = ld_seen;
  a.V = V;
  hipLaunchKernelGGL(sample_select_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, a);
  return x2i_check_launch("sample_select");
}

}  // extern "C"
