// The two kernels of the VAE encoder (diffusers AutoencoderKL.encode; lightcontrol/train_lightcontrol.py:678-679) that the implicit-GEMM
// convolutions do not cover:
//
// * the image stem, Conv2d(Cin <= 4 -> Cout, 3 x 3, stride 1, padding 1) at the full image resolution (Encoder.conv_in, 3 -> 128).  Its
//   input is tiny (6 MiB per 1024^2 image) and its output is the encoder's largest tensor (256 MiB), so the kernel is a write stream with a
//   matrix core on the side: the 9 Cin taps, zero-padded to K = 32 per step, are ONE v_mfma_f32_16x16x32_bf16 per 16 output channels and 16
//   pixels.  Output channels ride in the MFMA's rows, 16 neighbouring pixels of an image row in its columns (as in conv_narrow.hip); the rows
//   of MFMA block cb are a permutation of the channels chosen so that a lane ends up holding eight CONSECUTIVE channels of its pixel from
//   blocks 2p and 2p + 1 -- one 16-byte store, four lanes filling a pixel's 64-byte segment.  The taps are gathered straight from the NCHW bf16
//   planes (k = ci * 9 + ky * 3 + kx: the nn.Conv2d weight [Cout][Cin][3][3] is the A operand as it is).  Optionally the epilogue leaves the
//   channel-quad moments in the layout of x2i_conv_desc.moments: per-workgroup partial sums (fixed lane / wave order) reduced by the
//   convolutions' own slab / finish kernels (gemm.hip), so block 0's first GroupNorm reads its input once.
//
// * the diagonal-Gaussian posterior (diffusers DiagonalGaussianDistribution.mode / .sample): one thread per OUTPUT element, so the writes are
//   coalesced along pixels for the NCHW latent and along the features for FLUX's packed tokens; fp32 arithmetic, one rounding to bf16.
#include "gemm_device.h"   // row16_sum: the conv epilogues' fixed-order DPP sum over 16 lanes

namespace {

constexpr int STEM_WAVES = 4;   // a workgroup: four strips of 16 pixel columns side by side

// MFMA block cb, row r (0 .. 15) -> output channel.  Pairs of blocks (2p, 2p + 1) cover channels 32p .. 32p + 31 with lane group g = r >> 2
// holding 32p + 8g .. 32p + 8g + 7 (block 2p: the first four, 2p + 1: the last four); a final unpaired block (Cout / 16 odd) is plain.
template <int NB>
__device__ __forceinline__ int stem_channel(int cb, int r) {
  constexpr int PAIRS = NB / 2;
  const int g = r >> 2, i = r & 3;
  return cb < 2 * PAIRS ? 32 * (cb >> 1) + 8 * g + 4 * (cb & 1) + i : 16 * cb + r;
}

template <int NB, int KS, bool MOM>
__global__ __launch_bounds__(256) void conv3x3_image_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                            const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, float* __restrict__ part,
                                                            int Cin, int H, int W, int rows_per_block, int blocks_per_img) {
  constexpr int COUT = NB * 16, PAIRS = NB / 2, NQ = NB;   // a lane's quads: two per pair, one for the odd block
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int x0 = (blockIdx.x * STEM_WAVES + wave) * 16, xc = x0 + n;
  const bool active = x0 < W;                              // (wave-uniform; inactive waves still join the moments reduction)
  const int y0 = blockIdx.y * rows_per_block, nrows = min(rows_per_block, H - y0);
  const long long HW = (long long)H * W;
  const bf16_t* xb = x + (long long)blockIdx.z * Cin * HW;
  bf16_t* yb = y + (long long)blockIdx.z * HW * COUT;
  const int K = 9 * Cin;

  // A fragments: row n = output channel stem_channel(cb, n), k = 32 ks + 8 g + j
  bf16x8_t wf[NB][KS];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) {
    const bf16_t* wr = w + (long long)stem_channel<NB>(cb, n) * K;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * ks + 8 * g + j;
        wf[cb][ks][j] = k < K ? (short)wr[k] : (short)0;
      }
    }
  }
  // this lane's B taps: k = 32 ks + 8 g + j -> (plane offset, dy, dx); k >= 9 Cin is zero padding
  int toff[KS][8], tdy[KS][8], tdx[KS][8];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * ks + 8 * g + j, ci = k / 9, t = k - 9 * ci;
      tdy[ks][j] = k < K ? t / 3 - 1 : -1000000;               // (an invalid tap: no row passes the bounds test)
      tdx[ks][j] = t % 3 - 1;
      toff[ks][j] = k < K ? ci * (int)HW + tdx[ks][j] : 0;
    }
  // bias of the channels this lane holds after the MFMA (rows 4 g + i of every block)
  float bv[NB][4];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[cb][i] = bias ? bf16_to_f32(bias[stem_channel<NB>(cb, 4 * g + i)]) : 0.f;
  float ms[NQ], mq[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) ms[q] = mq[q] = 0.f;

  if (active) {
    for (int o = 0; o < nrows; ++o) {
      const int yy = y0 + o;
      bf16x8_t bfr[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int sy = yy + tdy[ks][j], sx = xc + tdx[ks][j];
          const bool ok = sy >= 0 && sy < H && sx >= 0 && sx < W;
          bfr[ks][j] = ok ? (short)xb[toff[ks][j] + (long long)sy * W + xc] : (short)0;
        }
      f32x4_t acc[NB];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        acc[cb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[cb][ks], bfr[ks], acc[cb], 0, 0, 0);
      }
      const bool px_ok = xc < W;
      bf16_t* dst = yb + ((long long)yy * W + xc) * COUT;
#pragma unroll
      for (int p = 0; p < PAIRS; ++p) {
        const uint32_t u0 = pack_bf16x2(acc[2 * p][0] + bv[2 * p][0], acc[2 * p][1] + bv[2 * p][1]);
        const uint32_t u1 = pack_bf16x2(acc[2 * p][2] + bv[2 * p][2], acc[2 * p][3] + bv[2 * p][3]);
        const uint32_t u2 = pack_bf16x2(acc[2 * p + 1][0] + bv[2 * p + 1][0], acc[2 * p + 1][1] + bv[2 * p + 1][1]);
        const uint32_t u3 = pack_bf16x2(acc[2 * p + 1][2] + bv[2 * p + 1][2], acc[2 * p + 1][3] + bv[2 * p + 1][3]);
        if (px_ok) {
          *(uint4*)(dst + 32 * p + 8 * g) = make_uint4(u0, u1, u2, u3);
          if constexpr (MOM) {
            const uint32_t u[4] = {u0, u1, u2, u3};
#pragma unroll
            for (int h = 0; h < 2; ++h) {   // quad 8 p + 2 g + h: channels 32 p + 8 g + 4 h .. + 3
              float s = 0.f, s2 = 0.f;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float v = __uint_as_float(e & 1 ? (u[2 * h + (e >> 1)] & 0xffff0000u) : (u[2 * h + (e >> 1)] << 16));
                s += v;
                s2 = __builtin_fmaf(v, v, s2);
              }
              ms[2 * p + h] += s;
              mq[2 * p + h] += s2;
            }
          }
        }
      }
      if constexpr (NB & 1) {
        constexpr int cb = NB - 1;
        const uint32_t u0 = pack_bf16x2(acc[cb][0] + bv[cb][0], acc[cb][1] + bv[cb][1]);
        const uint32_t u1 = pack_bf16x2(acc[cb][2] + bv[cb][2], acc[cb][3] + bv[cb][3]);
        if (px_ok) {
          *(uint2*)(dst + 16 * cb + 4 * g) = make_uint2(u0, u1);
          if constexpr (MOM) {
            const float v[4] = {__uint_as_float(u0 << 16), __uint_as_float(u0 & 0xffff0000u), __uint_as_float(u1 << 16),
                                __uint_as_float(u1 & 0xffff0000u)};
            float s = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              s += v[e];
              s2 = __builtin_fmaf(v[e], v[e], s2);
            }
            ms[NQ - 1] += s;
            mq[NQ - 1] += s2;
          }
        }
      }
    }
  }
  if constexpr (MOM) {
    // the 16 pixel columns of a lane group (DPP row, fixed order), then the four waves in order: partial f32 [batch][blocks][Cout / 4][2]
    __shared__ float red[STEM_WAVES][COUT / 4][2];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float s = x2i_gemm::row16_sum(ms[q]), s2 = x2i_gemm::row16_sum(mq[q]);
      const int quad = (2 * PAIRS > q) ? 8 * (q >> 1) + 2 * g + (q & 1) : 4 * (NB - 1) + g;
      if (n == 0) red[wave][quad][0] = s, red[wave][quad][1] = s2;
    }
    __syncthreads();
    if ((int)threadIdx.x < COUT / 2) {
      const int quad = threadIdx.x >> 1, c = threadIdx.x & 1;
      float v = red[0][quad][c];
#pragma unroll
      for (int wv = 1; wv < STEM_WAVES; ++wv) v += red[wv][quad][c];
      part[((long long)blockIdx.z * blocks_per_img + blockIdx.y * gridDim.x + blockIdx.x) * (COUT / 2) + threadIdx.x] = v;
    }
  }
}

// z = mean (+ exp(0.5 clamp(logvar, -30, 20)) eps) (then (z - shift) * scale), fp32, one rounding; PACKED: the output is FLUX's token
// layout [B][(h / 2)(w / 2)][4 C] (feature c * 4 + dy * 2 + dx of token (i, j) = pixel (2 i + dy, 2 j + dx)), else NCHW [B][C][h][w]
template <bool PACKED>
__global__ __launch_bounds__(256) void vae_posterior_kernel(const bf16_t* __restrict__ params, const bf16_t* __restrict__ eps, bf16_t* __restrict__ out,
                                                            int C, int h, int w, int ldp, long long total, int scale_shift, float shift, float scale) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long chw = (long long)C * h * w;
  const int b = (int)(idx / chw);
  const long long r = idx - b * chw;
  int c, py, px;
  if (PACKED) {
    const int f4 = 4 * C, tok = (int)(r / f4), f = (int)(r - (long long)tok * f4);
    const int wt = w >> 1;
    c = f >> 2;
    py = 2 * (tok / wt) + ((f >> 1) & 1);
    px = 2 * (tok % wt) + (f & 1);
  } else {
    c = (int)(r / ((long long)h * w));
    const int pix = (int)(r - (long long)c * h * w);
    py = pix / w;
    px = pix - py * w;
  }
  const bf16_t* pp = params + ((long long)b * h * w + (long long)py * w + px) * ldp;
  float z = bf16_to_f32(pp[c]);
  if (eps) {
    const float lv = fminf(fmaxf(bf16_to_f32(pp[C + c]), -30.f), 20.f);
    z = __builtin_fmaf(expf(0.5f * lv), bf16_to_f32(eps[(long long)b * chw + (long long)c * h * w + (long long)py * w + px]), z);
  }
  if (scale_shift) z = (z - shift) * scale;
  out[idx] = f32_to_bf16(z);
}

}  // namespace

int x2i_launch_conv3x3_image(const void* x, const void* w, const void* bias, void* y, int B, int Cin, int H, int W, int Cout, float* moments,
                             float* moments_scratch, hipStream_t stream) {
  if (!x || !w || !y) return x2i_set_error(X2I_ERR_ARG, "conv3x3_image: null pointer (x, w and y are required)");
  if (moments && !moments_scratch) return x2i_set_error(X2I_ERR_ARG, "conv3x3_image: moments without moments_scratch (x2i_conv_moments_scratch_floats)");
  if (B <= 0 || H <= 0 || W <= 0 || Cin < 1 || Cin > 4 || Cout < 16 || Cout > 128 || (Cout & 15))
    return x2i_set_error(X2I_ERR_SHAPE, "conv3x3_image: serves 1 <= Cin <= 4 and Cout a multiple of 16 in 16 .. 128 (B=%d Cin=%d H=%d W=%d Cout=%d)", B, Cin, H,
                         W, Cout);
  if ((long long)Cin * H * W >= 0x7f000000LL || (long long)H * W * Cout >= 0x7f000000LL)
    return x2i_set_error(X2I_ERR_SHAPE, "conv3x3_image: image too large (H=%d W=%d)", H, W);
  if ((((uintptr_t)y) & 15) || (((uintptr_t)moments_scratch) & 15) || (((uintptr_t)x) & 1) || (((uintptr_t)w) & 1))
    return x2i_set_error(X2I_ERR_ALIGN, "conv3x3_image: y and moments_scratch need 16-byte alignment, x / w 2-byte");
  const int strips = (W + 16 * STEM_WAVES - 1) / (16 * STEM_WAVES);
  int rb = 64;   // rows per workgroup: enough workgroups to fill the chip twice over (as conv_narrow.hip)
  while (rb > 8 && (long long)strips * ((H + rb - 1) / rb) * B < 2 * 2 * x2i_num_cus()) rb >>= 1;
  // the moments' partial rows must fit the scratch of x2i_conv_moments_scratch_floats(H * W, Cout, B): 2 ceil(H W / 128) per image
  const long long cap = ((long long)H * W + 127) / 128 * 2;
  while ((long long)strips * ((H + rb - 1) / rb) > cap) rb *= 2;
  const int blocks = strips * ((H + rb - 1) / rb);
  dim3 grid(strips, (H + rb - 1) / rb, B);
  float* part = moments ? moments_scratch : nullptr;
#define X2I_STEM(NB, KS)                                                                                                                     \
  hipLaunchKernelGGL((moments ? conv3x3_image_kernel<NB, KS, true> : conv3x3_image_kernel<NB, KS, false>), grid, dim3(64 * STEM_WAVES), 0, \
                     stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)y, part, Cin, H, W, rb, blocks)
#define X2I_STEM_KS(NB) \
  if (Cin <= 3) X2I_STEM(NB, 1); else X2I_STEM(NB, 2)
  switch (Cout / 16) {
    case 1: X2I_STEM_KS(1); break;
    case 2: X2I_STEM_KS(2); break;
    case 3: X2I_STEM_KS(3); break;
    case 4: X2I_STEM_KS(4); break;
    case 5: X2I_STEM_KS(5); break;
    case 6: X2I_STEM_KS(6); break;
    case 7: X2I_STEM_KS(7); break;
    default: X2I_STEM_KS(8); break;
  }
#undef X2I_STEM_KS
#undef X2I_STEM
  int rc = x2i_check_launch("conv3x3_image");
  if (rc || !moments) return rc;
  return x2i_conv_moments_reduce(moments_scratch, moments, B, blocks, Cout, 0, stream);
}

int x2i_launch_vae_posterior(const void* params, int ldp, const void* eps, void* out_nchw, void* out_packed, int B, int C, int h, int w, int scale_shift,
                             float shift, float scale, hipStream_t stream) {
  if (!params || (!out_nchw && !out_packed)) return x2i_set_error(X2I_ERR_ARG, "vae_posterior: null pointer (params and at least one output are required)");
  if (scale_shift != 0 && scale_shift != 1) return x2i_set_error(X2I_ERR_ARG, "vae_posterior: scale_shift must be 0 or 1, got %d", scale_shift);
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || ldp < 2 * C)
    return x2i_set_error(X2I_ERR_SHAPE, "vae_posterior: bad shape B=%d C=%d h=%d w=%d ldp=%d (ldp >= 2 C)", B, C, h, w, ldp);
  if (out_packed && ((h & 1) || (w & 1))) return x2i_set_error(X2I_ERR_SHAPE, "vae_posterior: packed tokens need even h and w (h=%d w=%d)", h, w);
  if ((((uintptr_t)params) | ((uintptr_t)eps) | ((uintptr_t)out_nchw) | ((uintptr_t)out_packed)) & 1)
    return x2i_set_error(X2I_ERR_ALIGN, "vae_posterior: bf16 pointers need 2-byte alignment");
  const long long total = (long long)B * C * h * w;
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (out_nchw) {
    hipLaunchKernelGGL(vae_posterior_kernel<false>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)params, (const bf16_t*)eps, (bf16_t*)out_nchw, C, h, w,
                       ldp, total, scale_shift, shift, scale);
    const int rc = x2i_check_launch("vae_posterior");
    if (rc) return rc;
  }
  if (out_packed) {
    hipLaunchKernelGGL(vae_posterior_kernel<true>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)params, (const bf16_t*)eps, (bf16_t*)out_packed, C, h, w,
                       ldp, total, scale_shift, shift, scale);
    return x2i_check_launch("vae_posterior (packed)");
  }
  return X2I_OK;
}
