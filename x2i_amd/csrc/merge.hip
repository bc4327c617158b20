// The prompt merge in front of the Qwen2 decoder stack (include/x2i_merge.h): layer 0's input of a multimodal prompt, written where it is used.
//   merge_rank     the exclusive rank of every placeholder row of the flattened ids (two launches: per-chunk counts, then offsets + ranks)
//   embed_merge    per prompt row either a (scaled) row of the token table or a row of one of two feature arrays, into slab[:, 0]
// They stand behind MiniCPM-o's get_vllm_embedding / get_omni_embedding scatters, InternVL's masked assignment and the per-sample
// index_select of Qwen2DecoderStack.  No workgroup waits on another and there is no atomic: a chunk's count is written by one workgroup of
// the first rank launch and read by the second launch; the merge's error flag is only stored to, always with the value 1.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_merge.h"

#include <cmath>

namespace {

constexpr int CHUNK = X2I_MERGE_RANK_CHUNK;
constexpr int STEPS = CHUNK / 256;        // 64-row steps of one wave
static_assert(CHUNK == 2048 && STEPS == 8, "four waves of eight 64-row steps");

__device__ __forceinline__ int popc64(unsigned long long m) { return __popcll(m); }

// The ballots of this wave's eight steps: wave w of workgroup g owns the rows [g * CHUNK + w * 512, + 512), lane l of step k the row + 64 k + l.
// -> the wave's placeholder count (wave-uniform)
__device__ __forceinline__ int rank_ballots(const long long* __restrict__ ids, long long n, long long ph, unsigned long long (&m)[STEPS]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * CHUNK + wave * (STEPS * 64) + lane;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const long long r = r0 + k * 64;
    const bool hit = r < n && ids[r] == ph;
    m[k] = __ballot(hit);
    cnt += popc64(m[k]);
  }
  return cnt;
}

__global__ __launch_bounds__(256) void merge_rank_count_kernel(const long long* __restrict__ ids, long long n, long long ph, int32_t* __restrict__ ws) {
  __shared__ int wcnt[4];
  unsigned long long m[STEPS];
  const int cnt = rank_ballots(ids, n, ph, m);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(256) void merge_rank_offset_kernel(const long long* __restrict__ ids, long long n, long long ph, const int32_t* __restrict__ ws,
                                                                int32_t* __restrict__ src, int32_t* __restrict__ total) {
  __shared__ int wcnt[4];
  __shared__ int before[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long m[STEPS];
  const int cnt = rank_ballots(ids, n, ph, m);
  int part = 0;                                           // the counts of the chunks before this one, in a fixed order
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += 256) part += ws[i];
#pragma unroll
  for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) { wcnt[wave] = cnt; before[wave] = part; }
  __syncthreads();
  int run = before[0] + before[1] + before[2] + before[3];
  for (int w = 0; w < wave; ++w) run += wcnt[w];
  const long long r0 = (long long)blockIdx.x * CHUNK + wave * (STEPS * 64) + lane;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < STEPS; ++k) {
    const long long r = r0 + k * 64;
    if (r < n) src[r] = ((m[k] >> lane) & 1ull) ? run + popc64(m[k] & below) : -1;
    run += popc64(m[k]);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    *total = before[0] + before[1] + before[2] + before[3] + wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// One thread per 16-byte piece.  A workgroup's first piece is split into (row, piece) once, in 64-bit scalar arithmetic; its threads divide 32-bit numbers.
__global__ __launch_bounds__(256) void embed_merge_kernel(const long long* __restrict__ ids, const int32_t* __restrict__ src,
                                                          const bf16_t* __restrict__ table, long long ldt, int V, float scale,
                                                          const bf16_t* __restrict__ feat0, long long ldf0, int n0,
                                                          const bf16_t* __restrict__ feat1, long long ldf1, int n1, bf16_t* __restrict__ out,
                                                          long long ldo, long long obs, int32_t* __restrict__ err, int rows, int S, int nc) {
  const long long first = (long long)blockIdx.x * 256;
  const long long row0 = first / nc;
  const int t = (int)(first - row0 * nc) + (int)threadIdx.x;
  const int dr = t / nc;
  const int c = t - dr * nc;
  const long long row64 = row0 + dr;
  if (row64 >= rows) return;
  const int row = (int)row64;
  const int sv = src ? src[row] : -1;
  if (sv < 0 && !table) return;                           // overwrite mode: not a feature row, not touched
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  bool bad = false;
  if (sv >= 0) {
    const int arr = (sv >> X2I_MERGE_SRC_ARRAY_BIT) & 1, k = sv & X2I_MERGE_SRC_ROW_MASK;
    const bf16_t* f = arr ? feat1 : feat0;
    const long long ldf = arr ? ldf1 : ldf0;
    if (k < (arr ? n1 : n0)) v = *(const uint4*)(f + (long long)k * ldf + c * 8);      // (a missing array has a count of 0)
    else bad = true;
  } else {
    const long long id = ids[row];
    if (id >= 0 && id < V) {
      v = *(const uint4*)(table + id * ldt + c * 8);
      if (scale != 1.0f) {
        float x[8];
        unpack8(v, x);
        v = make_uint4(pack_bf16x2(__fmul_rn(x[0], scale), __fmul_rn(x[1], scale)), pack_bf16x2(__fmul_rn(x[2], scale), __fmul_rn(x[3], scale)),
                       pack_bf16x2(__fmul_rn(x[4], scale), __fmul_rn(x[5], scale)), pack_bf16x2(__fmul_rn(x[6], scale), __fmul_rn(x[7], scale)));
      }
    } else {
      bad = true;
    }
  }
  const int b = row / S, s = row - b * S;
  *(uint4*)(out + b * obs + s * ldo + c * 8) = v;
  if (bad && c == 0) *err = 1;
}

inline bool al(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int x2i_merge_rank_i32(const int64_t* ids, int64_t n, int64_t placeholder, int32_t* src, int32_t* total, int32_t* ws, int64_t ws_ints,
                       x2i_stream_t stream) {
  if (!ids || !src || !total || !ws) return x2i_set_error(X2I_ERR_ARG, "merge_rank: null pointer");
  if (n < 1 || n > (1 << 24)) return x2i_set_error(X2I_ERR_SHAPE, "merge_rank: n=%lld is not in 1..2^24", (long long)n);
  if (!al(ids, 8) || !al(src, 4) || !al(total, 4) || !al(ws, 4))
    return x2i_set_error(X2I_ERR_ALIGN, "merge_rank: ids must be 8-byte, src, total and ws 4-byte aligned");
  const int64_t need = X2I_MERGE_RANK_WS_INTS(n);
  if (ws_ints < need)
    return x2i_set_error(X2I_ERR_SHAPE, "merge_rank: workspace too small (%lld int32 given, %lld needed)", (long long)ws_ints, (long long)need);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(merge_rank_count_kernel, dim3((unsigned)need), dim3(256), 0, st, (const long long*)ids, (long long)n, (long long)placeholder, ws);
  hipLaunchKernelGGL(merge_rank_offset_kernel, dim3((unsigned)need), dim3(256), 0, st, (const long long*)ids, (long long)n, (long long)placeholder,
                     (const int32_t*)ws, src, total);
  return x2i_check_launch("merge_rank");
}

int x2i_embed_merge_bf16(const int64_t* ids, const int32_t* src, const void* table, int64_t ldt, int32_t V, float scale, const void* feat0,
                         int64_t ldf0, int32_t n0, const void* feat1, int64_t ldf1, int32_t n1, void* out, int64_t ldo, int64_t out_batch_stride,
                         int32_t* err, int32_t B, int32_t S, int32_t H, x2i_stream_t stream) {
  if (!out || !err) return x2i_set_error(X2I_ERR_ARG, "embed_merge: null pointer");
  if (table && !ids) return x2i_set_error(X2I_ERR_ARG, "embed_merge: null pointer (ids with a table)");
  if (!table && !src) return x2i_set_error(X2I_ERR_ARG, "embed_merge: overwrite mode (no table) needs src");
  if (B < 1 || S < 1 || (int64_t)B * S > (1 << 30)) return x2i_set_error(X2I_ERR_SHAPE, "embed_merge: B=%d, S=%d: need B, S > 0 and B * S <= 2^30", B, S);
  if (H < 8 || H % 8) return x2i_set_error(X2I_ERR_SHAPE, "embed_merge: H=%d must be a positive multiple of 8", H);
  if (table && V < 1) return x2i_set_error(X2I_ERR_SHAPE, "embed_merge: V=%d is not positive", V);
  if (n0 < 0 || n1 < 0 || n0 > (1 << 30) || n1 > (1 << 30) || (!feat0 && n0) || (!feat1 && n1))
    return x2i_set_error(X2I_ERR_SHAPE, "embed_merge: feature counts n0=%d, n1=%d must be in [0, 2^30], and 0 without an array", n0, n1);
  if (!std::isfinite(scale)) return x2i_set_error(X2I_ERR_ARG, "embed_merge: the scale must be finite");
  if ((table && (ldt < H || ldt % 8)) || (feat0 && (ldf0 < H || ldf0 % 8)) || (feat1 && (ldf1 < H || ldf1 % 8)) || ldo < H || ldo % 8 ||
      out_batch_stride % 8 || (B > 1 && out_batch_stride < (int64_t)(S - 1) * ldo + H))
    return x2i_set_error(X2I_ERR_ALIGN,
                         "embed_merge: every row stride must be a multiple of 8 and >= H=%d, out_batch_stride a multiple of 8 that holds S rows", H);
  if (!al16(table) || !al16(feat0) || !al16(feat1) || !al16(out) || !al(ids, 8) || !al(src, 4) || !al(err, 4))
    return x2i_set_error(X2I_ERR_ALIGN, "embed_merge: table, feat0, feat1 and out must be 16-byte, ids 8-byte, src and err 4-byte aligned");
  const int rows = B * S, nc = H / 8;
  const long long pieces = (long long)rows * nc;
  const long long blocks = (pieces + 255) / 256;
  if (blocks > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "embed_merge: B * S * H / 8 = %lld pieces are too many for one launch", pieces);
  hipLaunchKernelGGL(embed_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, src, (const bf16_t*)table,
                     (long long)ldt, (int)V, scale, (const bf16_t*)feat0, (long long)ldf0, (int)n0, (const bf16_t*)feat1, (long long)ldf1, (int)n1,
                     (bf16_t*)out, (long long)ldo, (long long)out_batch_stride, err, rows, (int)S, nc);
  return x2i_check_launch("embed_merge");
}

}  // extern "C"
