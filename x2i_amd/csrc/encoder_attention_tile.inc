// The key-tile step of encoder_attn_kernel (encoder_attention.hip), included there once per way of walking the tiles: tile n of the walk,
// with LAST (a compile-time bool) set where the walk knows that this is the last tile.  Not a translation unit of its own.
// Names it takes from the including scope:
//   the frame's     n (index of the tile in the walk), LAST
//   template        DK, MODE; constants KTILE, VTILE, NDS, NDB, THR, RANGED (and KVB, NEG_BIG, LOG2E, RELBIAS, SEGMENT of the file)
//   read            smem, tl, qf, stage, t_lo, ntiles, t_wave, q0, q, qlim, klo, khi, S, R, scale2, hi, k_row_off, k_swz, v_row_off, v_swz
//                   SEGMENT: tw_lo, rlo, rhi, w_lomax, w_himin
//   read and written  oacc, m_run, l_run
    const int t = t_lo + n;
    const int buf = n & 1;
    if (MODE == RELBIAS ? !LAST : n + 1 < ntiles) stage(buf ^ 1, (t + 1) * KVB);   // (workgroup-uniform)
    if (MODE == RELBIAS || (t <= t_wave && (MODE != SEGMENT || t >= tw_lo))) {   // (wave-uniform)
      const char* kb = smem + buf * (KTILE + VTILE);
      const char* vb = kb + KTILE;

      // ---- S^T = K Q^T: two 32-key sub-tiles, alternating accumulators
      f32x16_t sacc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[u][r] = 0.f;
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bf16x8_t kf = *(const bf16x8_t*)(kb + u * 32 * (2 * DK) + k_row_off + (((ds * 2 + hi) ^ k_swz) << 4));
          sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ds], sacc[u], 0, 0, 0);
        }
      // lane (q = li, hi), sub-tile u, reg r  <->  key = kv0 + u*32 + 16*(r>>3) + 8*hi + (r&7)
      const int kv0 = t * KVB;
      if constexpr (MODE == RELBIAS) {
        // ---- scores into the exp2 domain, plus the bias of key offset key - q
        if (kv0 - (q0 + 31) >= R || kv0 + (KVB - 1) - q0 <= -R) {   // (wave-uniform) the whole 32 x 64 patch lies in one clamped region
          const float bias = tl[kv0 > q0 ? 2 * R : 0];
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[u][r] = __builtin_fmaf(sacc[u][r], LOG2E, bias);
        } else {
          const int rel0 = kv0 + 8 * hi - q;
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rel = rel0 + u * 32 + 16 * (r >> 3) + (r & 7);
              sacc[u][r] = __builtin_fmaf(sacc[u][r], LOG2E, tl[min(max(rel, -R), R) + R]);
            }
        }
        if (LAST && kv0 + KVB > S) {  // ragged last tile: keys >= S are masked by index
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int key = kv0 + u * 32 + 16 * (r >> 3) + 8 * hi + (r & 7);
              if (key >= S) sacc[u][r] = NEG_BIG;
            }
        }
      } else if constexpr (MODE == SEGMENT) {
        // ---- scores into the exp2 domain: one multiply by scale * log2 e
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[u][r] *= scale2;
        if (kv0 < w_lomax || kv0 + KVB > w_himin) {   // (wave-uniform) the tile is not wholly inside every row's range (a ragged last tile: rhi <= S)
          const int dn = rlo - kv0 - 8 * hi;
          const int up = rhi - kv0 - 8 * hi;
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = u * 32 + 16 * (r >> 3) + (r & 7);
              if (c < dn || c >= up) sacc[u][r] = NEG_BIG;
            }
        }
      } else {
        // ---- scores into the exp2 domain: one multiply by scale * log2 e
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[u][r] *= scale2;
        if (kv0 + (KVB - 1) > min(q0, khi - 1) || (RANGED && kv0 < klo)) {   // (wave-uniform) the tile holds a key that does not count for one of this wave's rows
          const int up = qlim - kv0 - 8 * hi;
          const int dn = klo - kv0 - 8 * hi;
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = u * 32 + 16 * (r >> 3) + (r & 7);
              if (c > up || (RANGED && c < dn)) sacc[u][r] = NEG_BIG;
            }
        }
      }
      // ---- online softmax
      float mx = NEG_BIG;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[u][r]);
      mx = xhalf_max(mx);
      // defer-max: keep the old running max while no row of this wave grew by more than THR, so that the O rescale is skipped on most tiles.
      // (A row's first real score leaves NEG_BIG or M_FLOOR by far more than THR, so the test fails and m_new is real; a CAUSAL row that has
      // seen no counted key keeps M_FLOOR, against which a masked score still exponentiates to 0.)
      float m_new = fmaxf(m_run, mx);
      if constexpr (MODE == SEGMENT) {
        // per ROW: the rows of a wave belong to different segments, and a wave-wide test would let the scores of one segment decide which
        // reference another segment's rows exponentiate against -- the same value, other roundings.  A row's result is a function of its
        // own range alone, bit for bit; the rescale below is still skipped when no row moved (and multiplies the others by exactly 1)
        if (m_new - m_run <= (float)THR) m_new = m_run;
      } else if (__all(m_new - m_run <= (float)THR)) m_new = m_run;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float psum = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u)
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
      bf16x8_t pf[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          union { bf16x8_t v; uint32_t w[4]; } cv;
#pragma unroll
          for (int j = 0; j < 4; ++j) cv.w[j] = pack_bf16x2(sacc[u][kt * 8 + 2 * j], sacc[u][kt * 8 + 2 * j + 1]);
          pf[u][kt] = cv.v;
        }
      // ---- O^T += V^T P^T
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const int u = g >> 1, kt = g & 1;
          const bf16x8_t vf = *(const bf16x8_t*)(vb + db * 32 * 128 + v_row_off + (((4 * u + 2 * kt + hi) ^ v_swz) << 4));
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[u][kt], oacc[db], 0, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next tile's DMA (issued by this wave) has landed
    __syncthreads();
