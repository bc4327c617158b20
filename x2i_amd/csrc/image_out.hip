// The image back end (abi/backend/x2i_image_out.h): the two ends of the VAE decode.  x2i_latents_to_vae turns the packed latents of the
// sampling call into the decoder's conv_in input (unpack, / scaling_factor + shift_factor, NHWC, channels padded to 64) in one launch;
// x2i_image_to_u8 turns the decoder's NHWC output into the uint8 pixels that are saved (/ 2 + 0.5, clamp, * 255, round).  Plain C++ and
// vector stores: no LDS, no atomics, no allocation; the launchers enqueue on the caller's stream and return.
#include "x2i_common.h"
#include "../../abi/backend/x2i_image_out.h"

namespace {

// float -> bf16 as torch's c10::BFloat16 rounds on this device (round_to_nearest_even): every NaN is 0x7FC0, everything else takes the
// integer carry, subnormals included.  f32_to_bf16 of x2i_common.h keeps a NaN's sign and payload, and the contract here is the bits of
// the torch expression for all 65536 inputs.
__device__ __forceinline__ bf16_t bf16_rne_torch(float f) {
  if (f != f) return 0x7FC0;
  const uint32_t u = __float_as_uint(f);
  return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// One lane per 16-byte piece of the output: piece k of a pixel holds channels 8 k .. 8 k + 7, so the eight lanes of a pixel and the
// pixels of a row store consecutive addresses (1 KiB per wave and store).  The lanes of pieces below Cz read their eight values 8 bytes
// apart from the packed row: pieces 0 and 1 of the two pixels (b = 0, 1) of one packed row together read 64 bytes of it, the wave of
// the image row below (a = 1) the other 64.  The pad pieces store zeros and read nothing.
__global__ __launch_bounds__(256) void latents_to_vae_kernel(const bf16_t* __restrict__ lat, long long ld_lat, uint4* __restrict__ out,
                                                             long long pieces, int h, int w, int Cz, float r, float shift) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= pieces) return;
  const int k = (int)(q & 7);
  uint32_t d[4] = {0u, 0u, 0u, 0u};
  if (k * 8 < Cz) {
    const long long p = q >> 3;                       // the pixel among B * h * w
    const int x = (int)(p % w);
    const long long ny = p / w;
    const int y = (int)(ny % h);
    const long long n = ny / h;
    const int hw2 = w >> 1;
    const bf16_t* row = lat + ((n * (h >> 1) + (y >> 1)) * hw2 + (x >> 1)) * ld_lat + (y & 1) * 2 + (x & 1);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int c = k * 8 + m;
      bf16_t o = 0;
      if (c < Cz) {
        const float t = bf16_to_f32(bf16_rne_torch(__fmul_rn(bf16_to_f32(row[c * 4]), r)));
        o = bf16_rne_torch(__fadd_rn(t, shift));
      }
      d[m >> 1] |= (uint32_t)o << ((m & 1) * 16);
    }
  }
  out[q] = make_uint4(d[0], d[1], d[2], d[3]);
}

__device__ __forceinline__ uint32_t to_u8(bf16_t v) {
  const float f = __builtin_fmaf(bf16_to_f32(v), 0.5f, 0.5f);            // (v * 0.5 is exact: the sum rounds once, as / 2 + 0.5 does)
  return (uint32_t)rintf(__fmul_rn(fminf(fmaxf(f, 0.0f), 1.0f), 255.0f));   // fmaxf(NaN, 0) = 0: a NaN gives 0
}

// One lane per four pixels of a row (quads = ceil(W / 4) lanes a row): four 8-byte loads of the pixels' first four channels, twelve
// bytes out.  3 * 4 pixels are a multiple of 4 bytes, so a quad is 4-byte aligned exactly where its row starts so: then three dword
// stores, lanes 12 bytes apart; a row that starts unaligned and the ragged last quad of a row go out byte by byte.
template <int LDY>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const bf16_t* __restrict__ y, uint8_t* __restrict__ out, long long image_pitch,
                                                          long long row_pitch, long long lanes, int H, int W, int quads) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= lanes) return;
  const int qd = (int)(t % quads);
  const long long nr = t / quads;                     // the row among B * H
  const int r = (int)(nr % H);
  const long long n = nr / H;
  const int x0 = qd * 4, np = min(4, W - x0);
  const uint2* src = (const uint2*)(y + (nr * W + x0) * LDY);
  uint32_t b[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint2 v = make_uint2(0u, 0u);
    if (i < np) v = src[i * (LDY / 4)];
    b[3 * i] = to_u8((bf16_t)(v.x & 0xFFFFu));
    b[3 * i + 1] = to_u8((bf16_t)(v.x >> 16));
    b[3 * i + 2] = to_u8((bf16_t)(v.y & 0xFFFFu));
  }
  uint8_t* dst = out + n * image_pitch + r * row_pitch + 3 * x0;
  if (np == 4 && ((uintptr_t)dst & 3) == 0) {
    uint32_t* d4 = (uint32_t*)dst;
#pragma unroll
    for (int j = 0; j < 3; ++j) d4[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * np) dst[j] = (uint8_t)b[j];
  }
}

constexpr long long MAX_BLOCKS = 0x7FFFFFFFLL;

}  // namespace

extern "C" {

int x2i_latents_to_vae(const void* latents, int64_t ld_lat, void* out, int32_t B, int32_t h, int32_t w, int32_t Cz, float scaling_factor,
                       float shift_factor, x2i_stream_t stream) {
  const char* what = "latents_to_vae";
  if (!latents || !out) return x2i_set_error(X2I_ERR_ARG, "%s: null latents or out", what);
  if (B < 1) return x2i_set_error(X2I_ERR_SHAPE, "%s: B=%d must be at least 1", what, B);
  if (h < 2 || w < 2 || (h & 1) || (w & 1))
    return x2i_set_error(X2I_ERR_SHAPE, "%s: h=%d and w=%d must be even and at least 2 (2 x 2 latent pixels per packed row)", what, h, w);
  if (Cz < 1 || Cz > 16) return x2i_set_error(X2I_ERR_SHAPE, "%s: Cz=%d must lie in 1..16", what, Cz);
  if (!(scaling_factor * 0.0f == 0.0f) || scaling_factor == 0.0f || !(shift_factor * 0.0f == 0.0f))   // (x * 0 == 0 exactly for finite x)
    return x2i_set_error(X2I_ERR_ARG, "%s: scaling_factor=%g must be finite and not 0, shift_factor=%g finite", what, (double)scaling_factor,
                         (double)shift_factor);
  if (ld_lat < 4 * Cz) return x2i_set_error(X2I_ERR_SHAPE, "%s: ld_lat=%lld must be at least 4 * Cz = %d", what, (long long)ld_lat, 4 * Cz);
  const long long hw = (long long)h * w;              // two int32 factors; B * hw only once hw is known to be below 2^31
  if (hw > MAX_BLOCKS || B * hw > MAX_BLOCKS)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: B * h * w = %d * %d * %d must not exceed 2^31 - 1", what, B, h, w);
  const long long pixels = B * hw;
  if (ld_lat > INT64_MAX / pixels)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: ld_lat=%lld times the %lld packed rows does not fit 63 bits", what, (long long)ld_lat, pixels / 4);
  if ((uintptr_t)latents & 1) return x2i_set_error(X2I_ERR_ALIGN, "%s: latents must be 2-byte aligned", what);
  if ((uintptr_t)out & 15) return x2i_set_error(X2I_ERR_ALIGN, "%s: out must be 16-byte aligned", what);
  const long long pieces = pixels * 8;
  const dim3 grid((unsigned)((pieces + 255) / 256));
  hipLaunchKernelGGL(latents_to_vae_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)latents, (long long)ld_lat, (uint4*)out,
                     pieces, h, w, Cz, 1.0f / scaling_factor, shift_factor);
  return x2i_check_launch(what);
}

int x2i_image_to_u8(const void* y, int32_t ldy, void* out, int64_t image_pitch, int64_t row_pitch, int32_t B, int32_t H, int32_t W,
                    x2i_stream_t stream) {
  const char* what = "image_to_u8";
  if (!y || !out) return x2i_set_error(X2I_ERR_ARG, "%s: null y or out", what);
  if (B < 1 || H < 1 || W < 1) return x2i_set_error(X2I_ERR_SHAPE, "%s: B=%d, H=%d and W=%d must be at least 1", what, B, H, W);
  if (ldy != 4 && ldy != 8) return x2i_set_error(X2I_ERR_SHAPE, "%s: ldy=%d must be 4 or 8", what, ldy);
  if (row_pitch < 3LL * W) return x2i_set_error(X2I_ERR_SHAPE, "%s: row_pitch=%lld must be at least 3 W = %lld", what, (long long)row_pitch, 3LL * W);
  // (H - 1) * row_pitch is never formed (it could pass 2^63): image_pitch - 3 W >= (H - 1) * row_pitch as a quotient
  if (image_pitch < 3LL * W || (H > 1 && (image_pitch - 3LL * W) / (H - 1) < row_pitch))
    return x2i_set_error(X2I_ERR_SHAPE, "%s: image_pitch=%lld must be at least (H - 1) * row_pitch + 3 W (H=%d, row_pitch=%lld, W=%d)", what,
                         (long long)image_pitch, H, (long long)row_pitch, W);
  const int quads = (W + 3) / 4;
  const long long rows = (long long)B * H;            // two int32 factors: below 2^62
  if (rows > MAX_BLOCKS || rows * quads > MAX_BLOCKS)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: B * H * ceil(W / 4) = %d * %d * %d must not exceed 2^31 - 1", what, B, H, quads);
  // the last image must end inside the address space too: (B - 1) * image_pitch as a quotient
  if (B > 1 && image_pitch > INT64_MAX / B)
    return x2i_set_error(X2I_ERR_SHAPE, "%s: B * image_pitch = %d * %lld does not fit 63 bits", what, B, (long long)image_pitch);
  if ((uintptr_t)y & 7) return x2i_set_error(X2I_ERR_ALIGN, "%s: y must be 8-byte aligned", what);
  const long long lanes = rows * quads;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if (ldy == 4)
    hipLaunchKernelGGL((image_to_u8_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, (uint8_t*)out, (long long)image_pitch,
                       (long long)row_pitch, lanes, H, W, quads);
  else
    hipLaunchKernelGGL((image_to_u8_kernel<8>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, (uint8_t*)out, (long long)image_pitch,
                       (long long)row_pitch, lanes, H, W, quads);
  return x2i_check_launch(what);
}

}  // extern "C"
