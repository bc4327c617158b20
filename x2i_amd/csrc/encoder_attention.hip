// The one flash-attention kernel of the encoder extensions: T5's relative-position-bias attention (include/x2i_t5.h), the causal attention
// of the CLIP text encoder and the Qwen2 decoder prefill (include/x2i_clip.h, include/x2i_qwen.h) and the segmented attention of the
// Qwen2.5-VL vision tower (include/x2i_vit.h); the Qwen2 prompt extension's attention over a kept cache (include/x2i_qwen_extend.h) is CAUSAL
// with a first row.  The extern "C" entry points stay in t5.hip, clip.hip, qwen.hip, vit.hip and qwen_extend.hip and come here
// through the launchers at the end (x2i_kernels.h).  bf16 in and out, f32 arithmetic.
//
// The mapping is that of attention.hip (its 4-wave plain-HIP kernel) with the head width as a template parameter
//   * one workgroup = 4 waves, each wave owns 32 query rows; K / V^T stream through LDS in 64-key tiles, double-buffered LDS-DMA
//   * swapped QK^T (S^T = K Q^T, v_mfma_f32_32x32x16_bf16): a lane holds 32 scores of ONE query row, neighbouring lanes hold neighbouring
//     rows; the kvmap row permutation makes P^T directly the B operand of the PV MFMA
//   * K tile rows are 2 DK bytes (64 / 128 / 256): 16 / DK*8 rows share one 256-byte bank row, and the XOR swizzle is
//     chunk ^= (row / rows_per_bank_row) & (chunks_per_row - 1) -- a ds_read_b128 group's 16 lanes read rows that are distinct mod 16, hence
//     16 distinct 16-byte slots for every DK.  V^T tile rows are 128 bytes for every DK: chunk ^= (row >> 1) & 7, as attention.hip has it
//   * the trip count, every DMA issue, every s_waitcnt and every barrier are uniform across the workgroup in every mode; a wave that has
//     nothing to compute in a tile walks the loop (stage, wait, barrier) without MFMAs or exponentials
//
// RELBIAS (T5): no scale, every key tile, every wave computes every tile
//   * the head's bias table (2R + 1 floats, pre-multiplied by log2 e) sits in LDS behind the tiles; a score's bias is one ds_read_b32 at
//     clamp(key - query, -R, R) + R -- consecutive addresses across the lanes of a half-wave, one address inside the clamped region -- and a
//     (wave's query rows, key tile) pair wholly beyond +-R takes one uniform value instead
//   * keys >= S of a ragged last tile are masked by index; tile 0 holds key 0 < S, so every row's running maximum is a real score from its
//     first tile on (the defer-max test m_new - m_run <= THR fails against NEG_BIG there)
//
// CAUSAL (Qwen2): scale * log2 e is one multiply on the f32 scores
//   * grouped heads: query head h streams the K / V^T tiles of key/value head h / rep (rep = Hq / Hkv); the XCD-aware block order keeps the
//     query heads of a group next to each other on one XCD, so that the group's tiles are served from that XCD's L2
//   * a key range [klo, khi) per sample (read from device memory, clamped into [0, S]; [0, S) without the arrays); key j counts for row i
//     iff klo <= j <= min(i, khi - 1)
//   * a workgroup (query rows r0 .. r0+127) walks the key tiles klo / 64 .. min((min(S, r0 + 128) - 1) / 64, (khi - 1) / 64) only -- none when
//     the range is empty or starts after its last row
//   * a wave (rows q0 .. q0+31) computes a tile only when the tile starts at or before q0 (kv0 is a multiple of 64 and q0 of 32, so a tile
//     that starts after q0 starts after q0 + 31 too and is wholly in that wave's future), when q0 < S and when one of its rows reaches the
//     range (q0 + 31 >= klo).  Rows i >= S (never written) behave as row S - 1 at most, so that no lane of a computing wave is special
//   * the mask is by index: in a tile that reaches past min(q0, khi - 1) or starts before klo, a score of a key that does not count becomes
//     NEG_BIG before the maximum and the sum see it, whatever K and V^T hold there; exp2(NEG_BIG - m) is exactly 0
//   * rows with no counted key.  With klo inside a wave's 32 rows, the rows before klo of a computing wave see only masked scores.  A
//     running maximum that started AT NEG_BIG would stay there in such a row, exponentiate every masked score to exp2(0) = 1 and give the
//     plain average of whatever V^T holds.  So the running maximum starts at M_FLOOR = -1e15, far above NEG_BIG = -1e30 and far below any
//     score: a masked score gives exp2(NEG_BIG - m) = 0 against a real maximum and against the floor alike, such a row's sum stays exactly
//     0, and the epilogue selects the zero row on that sum (l == 0), which waves that never computed a tile share.  Without ranges no such
//     row exists: tile 0, the first tile of every computing wave, holds key 0 <= i, a row's first real score leaves the floor by far more
//     than THR exactly as it would leave NEG_BIG, and l > 0 in every written row
//
// CAUSAL_PLAIN (CLIP, 64-wide heads): CAUSAL with rep = 1 and the range [0, S) known at compile time; the same values bit for bit
//
// CAUSAL_EXT (the Qwen2 prompt extension, include/x2i_qwen_extend.h): CAUSAL in absolute rows with a first row.  The n query rows row0 ..
// row0 + n - 1 of a cache that already holds the keys before them; S = row0 + n, khi = S, and row0 travels in the kernel argument R, which
// only RELBIAS reads otherwise, so that the other instantiations' argument list is what it was
//   * the grid covers the 128-row query blocks that intersect [row0, S): block qt of the launch is block row0 / 128 + qt of the rows
//   * a wave computes only when one of its rows is live (q0 + 31 >= row0); a row is stored iff row0 <= q < S, at output row q - row0
//   * the defer-max test is per wave, so what the dead rows of a computing wave hold decides roundings of the live ones: they take the Q of
//     the nearest live row (rows < row0 that of row0, rows >= S that of S - 1) and no stale row of Q is read.  A dead row >= S is then row
//     S - 1 again, score for score; a dead row < row0 sees a prefix of row0's counted keys.  A live row's result is a function of the
//     chunk's Q rows and of the K / V^T slots [klo, S) alone
//   * a wave whose 32 rows are all >= row0 walks and masks exactly as CAUSAL does at S = row0 + n, Spad = cap, khi = S: the same values bit for
//     bit wherever that launch's own rows >= S do not move a rescale (they read Q rows >= S, which this mode does not)
//
// SEGMENT (the Qwen2.5-VL vision tower): bidirectional, a key range [rlo, rhi) per QUERY ROW (device memory [B][S], clamped into [0, S];
// [0, S) without the arrays): the windows and frames of one packed sequence, whose boundaries fall anywhere inside a tile, a wave or a
// workgroup.  CAUSAL's scale, M_FLOOR and zero rows
//   * a lane owns one query row, so the range is two integers per lane; the wave reduces them to the union of its rows' non-empty ranges and
//     to their intersection, the workgroup reduces the four unions through LDS: the walk runs from min(rlo) / 64 to (max(rhi) - 1) / 64 and
//     is derived here, not taken from the host and not assumed monotonic in the row
//   * a wave computes a tile only between the first and the last tile of its union; in a tile that is not wholly inside the intersection
//     the scores outside the lane's own range become NEG_BIG before the maximum and the sum see them (a ragged last tile: rhi <= S)
//   * the defer-max test is per row here, not per wave: the rows of a wave belong to different segments, and a row's result is a function
//     of its own range alone, bit for bit (encoder_attention_tile.inc)
//   * heads of 80 (DW = 80 in DK = 128): Q / K rows and the V^T head are 128 wide, and the tiles are staged whole; the score product takes
//     the 5 of 8 d-steps that hold data and the P V product 3 of 4 d-blocks, so columns 80..127 of Q / K and rows 96..127 of V^T never
//     reach an MFMA; rows 80..95 of V^T give rows 80..95 of O^T -- an MFMA's output row depends on that row of V^T alone -- which the
//     epilogue does not store.  The result does not depend on what the padding holds
#include "encoder_common.h"
#include "x2i_kernels.h"
#include <type_traits>

namespace {

enum { RELBIAS = 0, CAUSAL = 1, CAUSAL_PLAIN = 2, SEGMENT = 3, CAUSAL_EXT = 4 };

// DW: the head's width of data inside rows of DK elements (SEGMENT's 80-wide heads stored 128 wide); DW == DK everywhere else
template <int DK, int MODE, int DW = DK>
__global__ __launch_bounds__(256, 2) void encoder_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                              const bf16_t* __restrict__ VT, const float* __restrict__ tab,
                                                              const int* __restrict__ k_lo, const int* __restrict__ k_hi,
                                                              bf16_t* __restrict__ O, int H, int rep, int S, int Spad, int R, float scale2,
                                                              int ldo, long long o_bs, int nbatch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][K tile | V^T tile] | RELBIAS: bias table f32 [2R+1]
  constexpr int NT = 256;
  constexpr int KTILE = KVB * DK * 2;   // [64 keys][DK]
  constexpr int VTILE = DK * KVB * 2;   // [DK][64 keys]
  constexpr int CK = DK / 8;            // 16-byte chunks per K row
  constexpr int RPB = 16 / CK;          // K rows per 256-byte bank row
  constexpr int CH = DK / 32;           // chunks per thread per tile (64 * CK / 256)
  constexpr int NDS = DW / 16;          // d-steps of the score product (those that hold data)
  constexpr int NDB = (DW + 31) / 32;   // 32-wide d-blocks of O^T (the last one of DW = 80 is half data; its other half is never stored)
  static_assert(DW <= DK && DW % 16 == 0 && (MODE == SEGMENT || DW == DK), "a narrower head is SEGMENT's");
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
  [[maybe_unused]] const int row0 = MODE == CAUSAL_EXT ? R : 0;   // CAUSAL_EXT: the first live row
  const int qt = bid % nqt + (MODE == CAUSAL_EXT ? row0 / 128 : 0), h = (bid / nqt) % H, b = bid / (nqt * H);
  const int q0 = qt * 128 + wave * 32;
  const long long bh = (long long)b * H + h;
  constexpr bool RANGED = MODE == CAUSAL || MODE == CAUSAL_EXT;   // grouped heads and a key range per sample
  long long bg = bh;   // the key/value head
  if constexpr (RANGED) bg = (long long)b * (H / rep) + h / rep;   // repeat_kv: query head h reads key/value head h / rep
  const bf16_t* Qh = Q + bh * Spad * DK;
  const bf16_t* Kh = K + bg * Spad * DK;
  const bf16_t* Vh = VT + bg * DK * Spad;
  float* tl = (float*)(smem + 2 * (KTILE + VTILE));
  int klo = 0, khi = S;
  // SEGMENT only.  rlo, rhi: this lane's key range.  Wave-uniform: w_lomax / w_himin, the range that every row of the wave shares (a tile
  // inside it needs no mask), and tw_lo, the first tile the wave computes (t_wave below is the last)
  [[maybe_unused]] int rlo = 0, rhi = 0, w_lomax = 0, w_himin = 0, tw_lo = 0, seg_lo = 0, seg_hi = 0, seg_wave = -1;
  if constexpr (MODE == SEGMENT) {
    // the row's key range (k_lo / k_hi are [B][S] here), clamped into [0, S]: the host never sees these values, and no tile outside
    // [0, Spad) may be staged.  Rows >= S (never written) take row S - 1's, so that no lane of a computing wave is special
    const long long ri = (long long)b * S + min(q0 + li, S - 1);
    rlo = k_lo ? min(max(k_lo[ri], 0), S) : 0;
    rhi = k_hi ? min(max(k_hi[ri], 0), S) : S;
    // union (an empty row adds nothing to it) and intersection over the wave's 32 rows; both half-waves hold the same rows
    int ulo = rhi > rlo ? rlo : S, uhi = rhi > rlo ? rhi : 0, ilo = rlo, ihi = rhi;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      ulo = min(ulo, __shfl_xor(ulo, o));
      uhi = max(uhi, __shfl_xor(uhi, o));
      ilo = max(ilo, __shfl_xor(ilo, o));
      ihi = min(ihi, __shfl_xor(ihi, o));
    }
    ulo = __builtin_amdgcn_readfirstlane(ulo);
    uhi = __builtin_amdgcn_readfirstlane(uhi);
    w_lomax = __builtin_amdgcn_readfirstlane(ilo);
    w_himin = __builtin_amdgcn_readfirstlane(ihi);
    if (q0 >= S) { ulo = S; uhi = 0; }   // (wave-uniform) a wave past S computes nothing and asks for no tile
    if (uhi > ulo) { tw_lo = ulo / KVB; seg_wave = (uhi - 1) / KVB; }
    // the workgroup's walk: the union over its four waves, through LDS (behind the tiles, which nothing has touched yet)
    int* red = (int*)tl;
    if (lane == 0) { red[wave] = ulo; red[4 + wave] = uhi; }
    __syncthreads();
    seg_lo = min(min(red[0], red[1]), min(red[2], red[3]));
    seg_hi = max(max(red[4], red[5]), max(red[6], red[7]));
    seg_lo = __builtin_amdgcn_readfirstlane(seg_lo);
    seg_hi = __builtin_amdgcn_readfirstlane(seg_hi);
  } else if constexpr (MODE == RELBIAS) {
    // the head's bias table into LDS, in the exp2 domain
    for (int i = tid; i < 2 * R + 1; i += NT) tl[i] = tab[(long long)h * (2 * R + 1) + i] * LOG2E;
  } else if constexpr (RANGED) {
    // the sample's key range, clamped into [0, S]: the host never sees these values, and no tile outside [0, Spad) may be staged
    klo = k_lo ? min(max(__builtin_amdgcn_readfirstlane(k_lo[b]), 0), S) : 0;
    khi = k_hi ? min(max(__builtin_amdgcn_readfirstlane(k_hi[b]), 0), S) : S;
  }

  // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[q0+li][ds*16 + hi*8 .. +8]; rows past Spad (Spad % 128 != 0) read the last row
  bf16x8_t qf[NDS];
  {
    int qrow = min(q0 + li, Spad - 1);
    if constexpr (MODE == CAUSAL_EXT) qrow = min(max(q0 + li, row0), S - 1);   // a dead row takes the nearest live row's Q
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
  float m_run = MODE == RELBIAS ? NEG_BIG : M_FLOOR, l_run = 0.f;

  // workgroup-uniform: the key tiles t_lo .. t_lo + ntiles - 1.  RELBIAS: all of them.  Causal: from the tile that holds klo up to this query
  // block's diagonal and the tile that holds khi - 1 (ntiles <= 0: nothing to walk; every row of the block is a zero row)
  int t_lo = 0, ntiles = (S + KVB - 1) / KVB;
  const int q = q0 + li;
  // causal modes only.  t_wave (wave-uniform): the last tile this wave computes (the one its first row lies in), and none for a wave past S or
  // wholly before klo.  qlim: the last key of this lane's row
  [[maybe_unused]] int t_wave = 0, qlim = 0;
  if constexpr (MODE == SEGMENT) {
    t_lo = seg_lo / KVB;
    ntiles = seg_hi > seg_lo ? (seg_hi - 1) / KVB - t_lo + 1 : 0;
    t_wave = seg_wave;
  } else if constexpr (MODE != RELBIAS) {
    t_lo = klo / KVB;
    const int t_hi = (min(min(S, qt * 128 + 128), khi) - 1) / KVB;
    ntiles = khi > klo ? t_hi - t_lo + 1 : 0;
    t_wave = (q0 < S && q0 + 31 >= klo && (MODE != CAUSAL_EXT || q0 + 31 >= row0)) ? q0 / KVB : -1;
    qlim = min(q, khi - 1);
  }

  // ---- the walk over the key tiles.  The step (encoder_attention_tile.inc) is written once and stands in two frames, because the two
  // frames compile differently and each mode is held to what it was measured at on the MI355X.  RELBIAS: a lambda, with the last tile peeled
  // at compile time so that neither the staging test nor the ragged-tail mask stands in the loop (unpeeled, the T5-XXL launch takes 1 %
  // longer).  Causal modes: the step inline in one loop that tests n at run time (as a lambda, the 64-wide launch takes 2 % longer).
  if (MODE == RELBIAS || ntiles > 0) {   // (workgroup-uniform; RELBIAS: S >= 1)
    stage(0, t_lo * KVB);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // the first tile (and the bias table) is in LDS
    if constexpr (MODE == RELBIAS) {
      auto kv_tile = [&](int n, auto last_c) {
        constexpr bool LAST = decltype(last_c)::value;
#include "encoder_attention_tile.inc"
      };
      for (int n = 0; n < ntiles - 1; ++n) kv_tile(n, std::false_type{});
      kv_tile(ntiles - 1, std::true_type{});
    } else {
      for (int n = 0; n < ntiles; ++n) {
        constexpr bool LAST = false;
#include "encoder_attention_tile.inc"
      }
    }
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane (q = li, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3)
  l_run = xhalf_sum(l_run);
  // CAUSAL: the zero row, selected on a row sum that no counted key entered: rows before klo, an empty range, and waves that computed no tile
  // (their accumulators are still 0; 0 * finite V^T is 0 in the rows of a computing wave)
  const float inv = (MODE == RELBIAS || l_run > 0.f) ? 1.f / l_run : 0.f;
  bf16_t* orow = O + (long long)b * o_bs + (long long)q * ldo + h * DW;
  if constexpr (MODE == CAUSAL_EXT) orow -= (long long)row0 * ldo;   // output row q - row0; only the rows row0 <= q < S are written
  if ((((uintptr_t)O) & 15) == 0 && (ldo & 7) == 0 && (o_bs & 7) == 0) {
    // half-wave exchange: two 8-byte fragments of neighbouring d-groups become one 16-byte store per lane
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; g += 2) {
        if (db * 32 + 8 * g >= DW) continue;   // (compile time) the padding of a narrower head
        const uint32_t a0 = pack_bf16x2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv);
        const uint32_t a1 = pack_bf16x2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
        const uint32_t b0 = pack_bf16x2(oacc[db][4 * g + 4] * inv, oacc[db][4 * g + 5] * inv);
        const uint32_t b1 = pack_bf16x2(oacc[db][4 * g + 6] * inv, oacc[db][4 * g + 7] * inv);
        const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        if (q < S && (MODE != CAUSAL_EXT || q >= row0)) *(uint4*)(orow + db * 32 + 8 * (g + hi)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
  } else if (q < S && (MODE != CAUSAL_EXT || q >= row0)) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (db * 32 + 8 * g >= DW) continue;   // (compile time)
        const int d = db * 32 + 8 * g + 4 * hi;
        *(uint2*)(orow + d) = make_uint2(pack_bf16x2(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv),
                                         pack_bf16x2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv));
      }
  }
}

template <int DK, int MODE, int DW = DK>
int launch(const char* what, const void* Q, const void* K, const void* VT, const float* tab, const int* k_lo, const int* k_hi, void* O, int B, int H,
           int rep, int S, int Spad, int R, float scale2, int ldo, long long o_bs, hipStream_t stream) {
  // R: RELBIAS's clamp distance; CAUSAL_EXT's first row (the grid is the query blocks from that row's on)
  constexpr int TILES = 2 * 2 * KVB * DK * 2;
  constexpr int TAIL = MODE == SEGMENT ? 32 : 0;   // SEGMENT: the four waves' key ranges
  const int rc = x2i_ensure_dynamic_smem((const void*)encoder_attn_kernel<DK, MODE, DW>, TILES + TAIL + (MODE == RELBIAS ? (2 * RELBIAS_RMAX + 2) * 4 : 0));
  if (rc) return rc;
  const size_t shm = TILES + TAIL + (MODE == RELBIAS ? (size_t)((2 * R + 1 + 3) & ~3) * 4 : 0);
  const dim3 grid((unsigned)(((S + 127) / 128 - (MODE == CAUSAL_EXT ? R / 128 : 0)) * H * B));
  hipLaunchKernelGGL((encoder_attn_kernel<DK, MODE, DW>), grid, dim3(256), shm, stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)VT, tab, k_lo,
                     k_hi, (bf16_t*)O, H, rep, S, Spad, R, scale2, ldo, o_bs, B);
  return x2i_check_launch(what);
}

}  // namespace

int x2i_encoder_attention_refuse_shape(const char* name, int B, int H, int S, int Spad) {
  if (B <= 0 || H <= 0 || S <= 0 || Spad < S || Spad % 64)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: need Spad %% 64 == 0 and Spad >= S (S=%d Spad=%d)", name, S, Spad);
  return X2I_OK;
}

int x2i_encoder_attention_refuse_launch(const char* name, const char* heads, const char* align_tail, const void* Q, const void* K, const void* VT,
                                        const void* k_lo, const void* k_hi, const void* O, int B, int H, int S, int dk, int ldo, long long o_bs) {
  if ((long long)((S + 127) / 128) * H * B > 0x7fffffffLL) return x2i_set_error(X2I_ERR_SHAPE, "%s: too many work items", name);
  if (ldo < (long long)H * dk || ldo % 4 || o_bs % 4 || (((uintptr_t)O) & 7))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: output rows must hold %s*dk elements and be 8-byte aligned", name, heads);
  if (!al16(Q) || !al16(K) || !al16(VT) || (((uintptr_t)k_lo) & 3) || (((uintptr_t)k_hi) & 3))
    return x2i_set_error(X2I_ERR_ALIGN, "%s: Q, K, VT must be 16-byte aligned%s", name, align_tail);
  return X2I_OK;
}

int x2i_launch_encoder_attention_relbias(const void* Q, const void* K, const void* VT, const float* tab, void* O, int B, int H, int S, int Spad,
                                         int dk, int R, int ldo, long long o_bs, hipStream_t stream) {
  const char* what = "t5_attention";
  if (dk == 32) return launch<32, RELBIAS>(what, Q, K, VT, tab, nullptr, nullptr, O, B, H, 1, S, Spad, R, 0.f, ldo, o_bs, stream);
  if (dk == 64) return launch<64, RELBIAS>(what, Q, K, VT, tab, nullptr, nullptr, O, B, H, 1, S, Spad, R, 0.f, ldo, o_bs, stream);
  return launch<128, RELBIAS>(what, Q, K, VT, tab, nullptr, nullptr, O, B, H, 1, S, Spad, R, 0.f, ldo, o_bs, stream);
}

int x2i_launch_encoder_attention_causal(const void* Q, const void* K, const void* VT, const int* k_lo, const int* k_hi, void* O,
                                        int B, int Hq, int Hkv, int S, int Spad, int dk, float scale, int ldo, long long o_bs, hipStream_t stream) {
  const char* what = "qwen_attention";
  if (dk == 64) return launch<64, CAUSAL>(what, Q, K, VT, nullptr, k_lo, k_hi, O, B, Hq, Hq / Hkv, S, Spad, 0, scale * LOG2E, ldo, o_bs, stream);
  return launch<128, CAUSAL>(what, Q, K, VT, nullptr, k_lo, k_hi, O, B, Hq, Hq / Hkv, S, Spad, 0, scale * LOG2E, ldo, o_bs, stream);
}

// The Qwen2 prompt extension: rows row0 .. row0 + n - 1 of a cache of cap slots per head; k_lo [B] or null
int x2i_launch_encoder_attention_causal_ext(const void* Q, const void* K, const void* VT, const int* k_lo, void* O, int B, int Hq, int Hkv, int row0,
                                            int n, int cap, int dk, float scale, int ldo, long long o_bs, hipStream_t stream) {
  const char* what = "qwen_extend_attention";
  if (dk == 64)
    return launch<64, CAUSAL_EXT>(what, Q, K, VT, nullptr, k_lo, nullptr, O, B, Hq, Hq / Hkv, row0 + n, cap, row0, scale * LOG2E, ldo, o_bs, stream);
  return launch<128, CAUSAL_EXT>(what, Q, K, VT, nullptr, k_lo, nullptr, O, B, Hq, Hq / Hkv, row0 + n, cap, row0, scale * LOG2E, ldo, o_bs, stream);
}

// The CLIP text encoder's launch (64-wide ungrouped heads, the whole prefix) is short enough for CAUSAL's range and group arithmetic to show:
// 5.6 against 5.1 us at B = 16, H = 12, S = 77 on the MI355X.  CAUSAL_PLAIN folds both away and gives the same values, bit for bit
// (tests/test_clip_gpu.py compares the two entry points).
int x2i_launch_encoder_attention_causal_plain(const void* Q, const void* K, const void* VT, void* O, int B, int H, int S, int Spad, float scale,
                                              int ldo, long long o_bs, hipStream_t stream) {
  return launch<64, CAUSAL_PLAIN>("clip_attention", Q, K, VT, nullptr, nullptr, nullptr, O, B, H, 1, S, Spad, 0, scale * LOG2E, ldo, o_bs, stream);
}

// The Qwen2.5-VL vision tower: bidirectional, a key range per query row (row_lo, row_hi: [B][S], or both null for [0, S)); heads of 80 are
// the 128-wide tile with 5 of its 8 d-steps and 3 of its 4 d-blocks
int x2i_launch_encoder_attention_segment(const void* Q, const void* K, const void* VT, const int* row_lo, const int* row_hi, void* O, int B, int H,
                                         int S, int Spad, int dk, float scale, int ldo, long long o_bs, hipStream_t stream) {
  const char* what = "vit_attention";
  if (dk == 64) return launch<64, SEGMENT>(what, Q, K, VT, nullptr, row_lo, row_hi, O, B, H, 1, S, Spad, 0, scale * LOG2E, ldo, o_bs, stream);
  if (dk == 80) return launch<128, SEGMENT, 80>(what, Q, K, VT, nullptr, row_lo, row_hi, O, B, H, 1, S, Spad, 0, scale * LOG2E, ldo, o_bs, stream);
  return launch<128, SEGMENT>(what, Q, K, VT, nullptr, row_lo, row_hi, O, B, H, 1, S, Spad, 0, scale * LOG2E, ldo, o_bs, stream);
}
