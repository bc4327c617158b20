/* x2i_image_out.h -- extension header of libx2i_hip.so: the image back end (csrc/image_out.hip), the two ends of the VAE decode that
 * close a sampling call: packed latents to the decoder's conv_in input, and the decoder's output to the uint8 pixels that are saved.
 *
 * Everything x2i.h says holds here: the conventions (device pointers owned by the caller, `stream` a hipStream_t passed as void* and
 * the last argument, work enqueued and never synchronised, no allocation, no atomics, no LDS, 0 or a negative X2I_ERR_* code with the
 * message in x2i_last_error(); every argument is validated before any launch).  The header stands in a top-level directory of its own
 * because the sets of headers under include/ are closed; the binding is x2i_amd/image_out_binding.py, the host module
 * x2i_amd/image_out.py (ImageBackEnd, ImageWriter), the caller in the model AutoencoderKL.decode_to_uint8 (x2i_amd/vae.py).
 *
 * bf16(f) below is one rounding of a float32 to bf16, to nearest even, every NaN becoming 0x7FC0: the rounding of torch's .to(bfloat16).
 */
#ifndef X2I_IMAGE_OUT_H
#define X2I_IMAGE_OUT_H
#include "../../include/x2i.h"
#ifdef __cplusplus
extern "C" {
#endif

/* latents: bf16, B items of (h / 2) * (w / 2) packed rows of ld_lat elements, dense: row (i, j) of item n starts at element
 * ((n * (h / 2) + i) * (w / 2) + j) * ld_lat and holds 4 * Cz values, FluxPipeline._pack_latents' order (channel, a, b).
 * out: bf16 [B, h, w, 64] NHWC, dense, the input of the decoder's conv_in with the latent channels padded to one K-step:
 *   out[n][2 i + a][2 j + b][c] = bf16(float(bf16(float(v) * r)) + shift_factor),  v = latents[n][i * (w / 2) + j][c * 4 + a * 2 + b],  c < Cz
 *   out[n][y][x][c] = +0 for Cz <= c < 64
 * with r = 1.0f / scaling_factor, a float32 division made on the host: `x / scaling_factor + shift_factor` of a bf16 tensor as PyTorch
 * computes it on the GPU (both host scalars reach its kernels as float32 and the division is a multiplication by the float32
 * reciprocal; its CPU kernels divide and round shift_factor to bf16 first, which moves about 2 % of the bf16 inputs by one bf16 step:
 * tests/golden/image_out_scalar_forms.json), two roundings to bf16, products and sums not contracted.  All of out is written and nothing else; a relaunch gives
 * the same bits.  One lane writes one 16-byte piece of a pixel (eight lanes a pixel, consecutive lanes consecutive addresses).
 * Refused: a null latents or out, a scaling_factor that is 0 or not finite, a shift_factor that is not finite (X2I_ERR_ARG); B < 1, h or w below 2 or odd, Cz outside 1..16, ld_lat < 4 * Cz, B * h * w above 2^31 - 1, an ld_lat
 * whose product with the row count passes 63 bits (X2I_ERR_SHAPE); latents not 2-byte aligned or out not 16-byte aligned (X2I_ERR_ALIGN). */
int x2i_latents_to_vae(const void* latents, int64_t ld_lat, void* out, int32_t B, int32_t h, int32_t w, int32_t Cz, float scaling_factor,
                       float shift_factor, x2i_stream_t stream);

/* y: bf16 [B, H, W, ldy] NHWC, dense, the decoder's output: ldy = 4 as x2i_conv3x3_narrow_bf16 leaves it, ldy = 8 as the implicit-GEMM
 * form does.  Channels 0 .. 2 of a pixel are read, the others never.
 * out: uint8; pixel (n, r, x) is the three bytes at out + n * image_pitch + r * row_pitch + 3 x (pitches in bytes):
 *   out[..][c] = (uint8) rint(min(max(float(y[n][r][x][c]) * 0.5f + 0.5f, 0.0f), 1.0f) * 255.0f)
 * in float32 with rint to nearest even: VaeImageProcessor.postprocess(image, "pil")'s arithmetic, (image / 2 + 0.5).clamp(0, 1), then
 * (arr * 255).round().astype("uint8").  A NaN gives 0: postprocess leaves that case undefined (a NaN cast to uint8), this is the one
 * defined extension.  Nothing outside the 3 W bytes of a row is written: not the rest of a pitch, nothing between the images.  A
 * relaunch gives the same bits.  A lane takes four pixels of a row and writes three dwords where the row starts 4-byte aligned; the
 * ragged end of a row and rows that start unaligned are written byte by byte.
 * Refused: a null y or out (X2I_ERR_ARG); B, H or W < 1, ldy not 4 or 8, row_pitch < 3 W, image_pitch < (H - 1) * row_pitch + 3 W,
 * B * H * ceil(W / 4) above 2^31 - 1 (X2I_ERR_SHAPE); y not 8-byte aligned (X2I_ERR_ALIGN).  out needs no alignment. */
int x2i_image_to_u8(const void* y, int32_t ldy, void* out, int64_t image_pitch, int64_t row_pitch, int32_t B, int32_t H, int32_t W,
                    x2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
