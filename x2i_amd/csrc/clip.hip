// The CLIP text encoder's kernels (include/x2i_clip.h): the token + position embedding, the quick-GELU of the MLP and the pooled output (the
// hidden state at each sample's end-of-text token); the causal attention for 64-wide heads is encoder_attention.hip's CAUSAL_PLAIN mode
// (CAUSAL with ungrouped heads and no key ranges).  They stand behind `transformers`' CLIPAttention (under the text model's causal mask) /
// CLIPTextEmbeddings / CLIPMLP / CLIPTextModel's pooling as the reference uses them (infer/inference_*.py:
// `clip_model(ids, output_hidden_states=False).pooler_output`, train/train_qwenvl.py:665,778).  bf16 in and out, f32 arithmetic; every
// launcher enqueues on the caller's stream and returns.
#include "encoder_common.h"
#include "x2i_kernels.h"
#include "../../include/x2i_clip.h"

namespace {

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

}  // namespace

extern "C" {

int x2i_clip_attention_bf16(const void* Q, const void* K, const void* VT, void* O, int32_t B, int32_t H, int32_t S, int32_t Spad, int32_t dk,
                            float scale, int32_t ldo, int64_t o_batch_stride, x2i_stream_t stream) {
  if (!Q || !K || !VT || !O) return x2i_set_error(X2I_ERR_ARG, "clip_attention: null pointer");
  if (dk != 64) return x2i_set_error(X2I_ERR_SHAPE, "clip_attention: head width dk=%d is not 64", dk);
  if (const int rc = x2i_encoder_attention_refuse_shape("clip_attention", B, H, S, Spad)) return rc;
  if (!(scale > 0.f) || !(scale < 1.0e30f)) return x2i_set_error(X2I_ERR_ARG, "clip_attention: scale must be positive and finite");
  if (const int rc = x2i_encoder_attention_refuse_launch("clip_attention", "H", "", Q, K, VT, nullptr, nullptr, O, B, H, S, dk, ldo, o_batch_stride)) return rc;
  return x2i_launch_encoder_attention_causal_plain(Q, K, VT, O, B, H, S, Spad, scale, ldo, o_batch_stride, (hipStream_t)stream);
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
  return launch_row_act<QuickGeluAct, false>("clip_quick_gelu", X, ldx, Y, ldy, rows, F, (hipStream_t)stream);
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
