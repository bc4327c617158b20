// Block-wise 8-bit AdamW (the reference's --use_8bit_adam, train/train_qwenvl.py:437-447, lightcontrol/train_lightcontrol.py:559-569):
// AdamW on bf16 parameters and f32 gradients whose two moments are kept as one uint8 code per element plus one f32 absmax per block of
// 256 consecutive elements of ONE parameter.  A code indexes a sorted 256-entry map of values in [-1, 1] (first moment, signed) or [0, 1]
// (second moment, unsigned), x2i_amd/optim.py: dynamic_map; the moment it stands for is map[code] * absmax.  DESIGN.md section 4 has the format.
//
//   g' = coef g;  m = b1 (map_s[c_m] absmax_m) + (1 - b1) g';  v = b2 (map_u[c_v] absmax_v) + (1 - b2) g'^2
//   p  = p (1 - lr wd) - lr (m / bc1) / (sqrt(v / bc2) + eps)          from the UNQUANTISED m and v, rounded once to bf16
//   absmax_m' = max |m|, absmax_v' = max v over the block's valid elements;  c' = index of the entry nearest to m / absmax_m' (v / absmax_v');
//   an absmax of 0 gives the zero entry; a positive v never takes the zero entry but the smallest positive one (the stated deviation from
//   bitsandbytes: a block whose gradients span more than ~3 decades would otherwise lose its small second moments, and the next update of
//   those elements is m / eps-sized).
//
// ONE launch updates every block of every parameter.  A wave owns a block at a time (grid-stride over blocks), a lane four consecutive elements:
// 16-byte gradient load, 8-byte parameter load / store, 4-byte code loads / stores, ~12 B of HBM traffic per element; the two block maxima are
// a wave reduction (no barrier, no LDS).  Gradients, codes and absmax are flat and block-aligned (block b: elements [256 b, 256 b + 256) of g
// and of the code arrays, padded by the caller); only p is indirect, because the parameters stay the modules' own separate tensors.
//
// The block table is PER BLOCK, int64 [num_blocks][2] = {address of the block's first parameter element, number of valid elements 1..256}:
// a wave finds its block with one 16-byte load and no search, at 16 B per 256 elements (0.5 % of the 3 KB the block moves).  A per-parameter
// segment table would be smaller (hundreds of rows for the 19 control nets) but every wave would have to search it for its block first -- a
// dependent chain of loads in front of the block's own -- and a block's first element address would still have to be derived from the row.
// Lanes beyond the valid count read and write nothing; a lane that holds the ragged end, or a block whose address is not 8-byte aligned,
// takes 2-byte parameter accesses and 1-byte code stores.
//
// Nearest entry: the 255 midpoints between neighbouring entries, 0.5f * (map[k] + map[k + 1]), are laid out in LDS as an implicit binary
// search tree in breadth-first order (node i's children are 2 i and 2 i + 1): the rank of x among the midpoints is its code.  Level l of the
// tree is 2^l consecutive words, so the lanes of a ds_read_b32 touch distinct banks (or the same address: a broadcast) down to level 5 and
// only the last two of the eight levels can conflict -- a search over the sorted array itself would collide on every level
// (MI355X_MICROARCH.md, LDS: 32 banks per 32-lane group).  A value on a midpoint takes the lower entry.
//
// Every f32 operation of the update is spelled out (no contraction left to the compiler): tests/adam8_ref.py bounds each output by them.
#include "x2i_common.h"
#include "x2i_kernels.h"

namespace {

constexpr int A8_BLOCK = 256;        // elements per quantisation block
constexpr int A8_ZERO_SIGNED = 127;  // index of 0 in the signed map (127 negative entries below it); 0 in the unsigned map
constexpr int A8_MAX_WG = 2048;      // workgroups of four waves: blocks beyond 8192 are reached by the grid stride

__device__ __forceinline__ float wave_max8(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// rank of x among the 255 midpoints held as a breadth-first tree in t[1..255] = number of midpoints < x = index of the nearest map entry
__device__ __forceinline__ int nearest_code(const float* t, float x) {
  int i = 1;
#pragma unroll
  for (int l = 0; l < 8; ++l) i = 2 * i + (x > t[i] ? 1 : 0);
  return i - 256;
}

__global__ __launch_bounds__(256) void adamw8_kernel(const long long* __restrict__ table, const float* __restrict__ g,
                                                     unsigned char* __restrict__ cm, unsigned char* __restrict__ cv, float* __restrict__ am,
                                                     float* __restrict__ av, const float* __restrict__ map_s, const float* __restrict__ map_u,
                                                     long long nblocks, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2,
                                                     const float* __restrict__ coef) {
  __shared__ float ms[256], mu[256], ts[256], tu[256];
  {
    const int i = threadIdx.x;
    ms[i] = map_s[i];
    mu[i] = map_u[i];
    // tree node i (1..255) at level l = floor(log2 i), j-th of its level, is midpoint (2 j + 1) 2^(7 - l) - 1 of the sorted order
    if (i > 0) {
      const int l = 31 - __clz(i), j = i - (1 << l), k = ((2 * j + 1) << (7 - l)) - 1;
      ts[i] = __fmul_rn(0.5f, __fadd_rn(map_s[k], map_s[k + 1]));
      tu[i] = __fmul_rn(0.5f, __fadd_rn(map_u[k], map_u[k + 1]));
    } else {
      ts[0] = tu[0] = 0.f;
    }
  }
  __syncthreads();
  const float cf = coef ? coef[0] : 1.f;
  const float omb1 = __fsub_rn(1.f, b1), omb2 = __fsub_rn(1.f, b2), decay = __fsub_rn(1.f, __fmul_rn(lr, wd));
  const int lane = threadIdx.x & 63, e0 = 4 * lane;
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblocks; b += (long long)gridDim.x * 4) {
    const long long addr = table[2 * b];
    const int cnt = (int)table[2 * b + 1];
    const int nv = min(4, max(0, cnt - e0));   // this lane's valid elements
    bf16_t* pp = (bf16_t*)addr + e0;
    const bool wide = nv == 4 && (addr & 7) == 0;
    float mm[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
    float amax = 0.f, vmax = 0.f;
    if (nv > 0) {
      const long long o = b * A8_BLOCK + e0;
      const f32x4_t gv = *(const f32x4_t*)(g + o);
      const uint32_t c4m = *(const uint32_t*)(cm + o), c4v = *(const uint32_t*)(cv + o);
      const float sm = am[b], sv = av[b];
      float pw[4] = {0.f, 0.f, 0.f, 0.f};
      if (wide) {
        const uint2 pv = *(const uint2*)pp;
        pw[0] = __uint_as_float(pv.x << 16); pw[1] = __uint_as_float(pv.x & 0xFFFF0000u);
        pw[2] = __uint_as_float(pv.y << 16); pw[3] = __uint_as_float(pv.y & 0xFFFF0000u);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nv) pw[j] = bf16_to_f32(pp[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nv) {
          const float gg = __fmul_rn(cf, gv[j]);
          const float dm = __fmul_rn(ms[(c4m >> (8 * j)) & 255], sm), dv = __fmul_rn(mu[(c4v >> (8 * j)) & 255], sv);
          mm[j] = __builtin_fmaf(b1, dm, __fmul_rn(omb1, gg));
          vv[j] = __builtin_fmaf(b2, dv, __fmul_rn(__fmul_rn(omb2, gg), gg));
          const float den = __fadd_rn(__fsqrt_rn(__fdiv_rn(vv[j], bc2)), eps);
          const float upd = __fdiv_rn(__fmul_rn(lr, __fdiv_rn(mm[j], bc1)), den);
          pw[j] = __builtin_fmaf(pw[j], decay, -upd);
          amax = fmaxf(amax, fabsf(mm[j]));
          vmax = fmaxf(vmax, vv[j]);
        }
      }
      if (wide) {
        uint2 pv;
        pv.x = pack_bf16x2(pw[0], pw[1]);
        pv.y = pack_bf16x2(pw[2], pw[3]);
        *(uint2*)pp = pv;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nv) pp[j] = f32_to_bf16(pw[j]);
      }
    }
    amax = wave_max8(amax);
    vmax = wave_max8(vmax);
    if (nv > 0) {
      const float rm = amax > 0.f ? __fdiv_rn(1.f, amax) : 0.f, rv = vmax > 0.f ? __fdiv_rn(1.f, vmax) : 0.f;
      uint32_t o4m = 0, o4v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int km = amax > 0.f ? nearest_code(ts, __fmul_rn(mm[j], rm)) : A8_ZERO_SIGNED;
        int kv = nearest_code(tu, __fmul_rn(vv[j], rv));
        if (vv[j] > 0.f) kv = max(kv, 1);   // a positive second moment never quantises to 0
        o4m |= (uint32_t)km << (8 * j);
        o4v |= (uint32_t)kv << (8 * j);
      }
      const long long o = b * A8_BLOCK + e0;
      if (nv == 4) {
        *(uint32_t*)(cm + o) = o4m;
        *(uint32_t*)(cv + o) = o4v;
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < nv) {
            cm[o + j] = (unsigned char)(o4m >> (8 * j));
            cv[o + j] = (unsigned char)(o4v >> (8 * j));
          }
      }
      if (lane == 0) {
        am[b] = amax;
        av[b] = vmax;
      }
    }
  }
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

int x2i_launch_adamw8(const long long* table, const float* g, void* cm, void* cv, float* am, float* av, const float* map_s, const float* map_u,
                      long long nblocks, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, const float* coef,
                      hipStream_t stream) {
  if (!table || !g || !cm || !cv || !am || !av || !map_s || !map_u || nblocks <= 0)
    return x2i_set_error(X2I_ERR_ARG, "adamw8: null pointer or no blocks");
  if (!al(table, 16) || !al(g, 16) || !al(cm, 4) || !al(cv, 4) || !al(am, 4) || !al(av, 4) || !al(map_s, 4) || !al(map_u, 4) || (coef && !al(coef, 4)))
    return x2i_set_error(X2I_ERR_ARG, "adamw8: block table and gradients must be 16-byte aligned, codes, absmax and maps 4-byte aligned");
  const long long wgs = (nblocks + 3) / 4;
  hipLaunchKernelGGL(adamw8_kernel, dim3((unsigned)(wgs < A8_MAX_WG ? wgs : A8_MAX_WG)), dim3(256), 0, stream, table, g, (unsigned char*)cm,
                     (unsigned char*)cv, am, av, map_s, map_u, nblocks, lr, b1, b2, eps, wd, bc1, bc2, coef);
  return x2i_check_launch("adamw8");
}
