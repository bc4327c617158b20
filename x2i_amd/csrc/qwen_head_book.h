// What the two token-selection launches share (qwen_head.hip: the greedy select, qwen_sample.hip: the sampled one): the layout of the head
// workspace's header and the bookkeeping of one generated token.
#pragma once
#include <cstdint>

namespace head_book {

constexpr int HDR = 4;        // f32 words in front of the partials: word 0 is the snapshot of the step counter
constexpr int NO_STEP = -0x7fffffff - 1;   // the snapshot of a logits call without a counter

// Sample b's chosen token `pick` (any int: it is clamped into [0, V)) and col, the counter's snapshot: done / pad, token, sequences[col] with the
// bounds skip, lengths, eos, seen, *step = col + 1, in this order.  One thread of sample b's workgroup calls it.
__device__ inline void generated_token(int b, int pick, int col, int V, int32_t* step, long long* token, long long* sequences, long long ld_seq,
                                       int ncols, long long* lengths, uint8_t* done, const long long* __restrict__ eos, int n_eos, long long pad,
                                       uint8_t* seen, long long ld_seen) {
  pick = pick < 0 ? 0 : (pick >= V ? V - 1 : pick);             // whatever the buffers held: the next step's gather stays inside the table
  const bool was_done = done[b] != 0;
  const long long tok = was_done ? pad : (long long)pick;
  token[b] = tok;
  if (col >= 0 && col < ncols) sequences[(long long)b * ld_seq + col] = tok;
  if (!was_done) lengths[b] += 1;
  bool hit = false;
  for (int e = 0; e < n_eos; ++e) hit |= eos[e] == tok;
  done[b] = (was_done || hit) ? 1 : 0;
  if (seen) seen[(long long)b * ld_seen + tok] = 1;
  if (b == 0 && col != NO_STEP && col != 0x7fffffff) *step = col + 1;
}

}  // namespace head_book
