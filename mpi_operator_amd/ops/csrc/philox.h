// Counter-based random numbers for the dropout kernels: Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11),
// written from its definition, and the one scheme every dropout kernel and
// ops/reference.py philox_dropout_mask share, so the CPU reference
// reproduces each mask bit:
//
//   key     = (seed_lo, seed_hi)
//   counter = (octet, site, offset_lo, offset_hi)
//     octet  = flat element index / 8 (one Philox call serves 8 elements)
//     site   = the caller's call-site number
//     offset = the 64-bit step counter, read from DEVICE memory
//   element j of the octet draws r_j = (w[j >> 1] >> 16 * (j & 1)) & 0xffff
//   and is kept iff r_j >= thr, thr = round(p * 65536);
//   p_eff = thr / 65536 and the survivors are scaled by 1 / (1 - p_eff).
//
// Seed and offset live in an int64[2] device tensor (seed, offset) that
// rng_tick_k advances: a kernel captured into a graph reads them on every
// replay, where a launch argument would be frozen at capture.
#pragma once
#include <math.h>

#include "common.h"

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// c[0..3] <- Philox4x32-10(counter c, key (k0, k1))
DEV_INLINE void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
    uint32_t hi1 = __umulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += PHILOX_W0; // the key is bumped after each round
    k1 += PHILOX_W1;
  }
}

// (seed, offset) as the key and the upper counter words; wave-uniform loads.
// site, thr and scale are launch arguments (p is a hyperparameter); seed and
// offset are NOT: every kernel reads them through its state pointer.
struct DropState {
  uint32_t k0, k1, off_lo, off_hi;
};

DEV_INLINE DropState drop_state(const int64_t *__restrict__ state) {
  uint64_t seed = (uint64_t)state[0], off = (uint64_t)state[1];
  return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)off,
          (uint32_t)(off >> 32)};
}

// keep bits of one octet: bit j set = element j survives
DEV_INLINE uint32_t drop_keep8(const DropState &st, uint32_t site,
                               uint32_t thr, uint32_t octet) {
  uint32_t w[4] = {octet, site, st.off_lo, st.off_hi};
  philox4x32_10(w, st.k0, st.k1);
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint32_t r = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    bits |= (r >= thr ? 1u : 0u) << j;
  }
  return bits;
}

// ---- attention-probability dropout (attention.hip, flash_attention.hip) ----
// The mask of P[bh, i, j] (bh = b·H + h, query row i, key column j), in
// layout-free terms; ops/reference.py attn_dropout_keep mirrors it:
//
//   u = i & 15, band = i >> 4, half = (u >> 2) & 1,
//   slot = (u & 3) + 4·(u >> 3), NB = ceil(S / 16)
//   call = ((bh·NB + band)·2 + half)·S + j          counter word 0
//   counter = (call, site, offset_lo, offset_hi), key = (seed_lo, seed_hi)
//   r = (w[slot >> 1] >> 16·(slot & 1)) & 0xffff,  kept iff r >= thr
//
// One call serves the 8 rows {4·half + (s & 3) + 8·(s >> 2)} of one 16-row
// band at one column: exactly what one lane holds of a 32×32 MFMA result
// (row (r&3) + 8·(r>>2) + 4·(lane>>5) of the wave's 32, column lane&31) in
// registers r = 8k..8k+7, k the band within the wave's rows, with slot =
// r & 7 and half = lane >> 5. No draw is wasted and no lane exchanges bits.
//
// Packed (varlen) batches — N sequence slots in one [T, ...] buffer, lengths
// in cu_seqlens, grid sized by max_seqlen — use the SAME scheme with
//   bh = n·H + h (n the slot), S = max_seqlen (so NB = ceil(max_seqlen/16)),
//   i, j = row and column WITHIN the sequence (0 .. L−1), not packed rows.
// So element (i, j) of sequence n, head h draws the bit that a dense
// [N, max_seqlen] batch draws for (b = n, h, i, j): attn_dropout_keep(seed,
// offset, site, N, H, max_seqlen, p)[n, h, :L, :L] is its mask. Calls of
// different slots are disjoint whatever the lengths are, the masks do not
// depend on where a sequence sits in the buffer, and the host checks
// attn_dropout_shape_ok(N, H, max_seqlen).
struct AttnDrop {
  DropState st;
  uint32_t site, thr;
  float rs;      // 1 / (1 - p_eff)
  uint32_t bhnb; // bh·NB
  uint32_t S;
};

// launch arguments of the DROP kernels (unused where DROP is false)
struct AttnDropArgs {
  const int64_t *state;
  uint32_t site, thr;
  float rs;
};

DEV_INLINE AttnDrop attn_drop_init(const AttnDropArgs &a, int bh, int S) {
  uint32_t nb = (uint32_t)(S + 15) >> 4;
  return {drop_state(a.state), a.site, a.thr, a.rs, (uint32_t)bh * nb,
          (uint32_t)S};
}

// keep bits of the 16 C-layout registers of one lane at key column j: bit r
// set = register r survives. band0 = (first of the wave's 32 rows) >> 4.
DEV_INLINE uint32_t attn_drop_keep16(const AttnDrop &d, uint32_t band0,
                                     uint32_t half, uint32_t j) {
  uint32_t c0 = ((d.bhnb + band0) * 2 + half) * d.S + j;
  uint32_t c1 = c0 + 2 * d.S; // band0 + 1
  return drop_keep8(d.st, d.site, d.thr, c0) |
         (drop_keep8(d.st, d.site, d.thr, c1) << 8);
}

// 32-bit call counter: B·H·NB·2·S calls
static inline bool attn_dropout_shape_ok(long B, long H, long S) {
  if (B < 1 || H < 1 || S < 1) return false;
  long nb = (S + 15) / 16;
  return B * H * nb * 2 * S < (1L << 32);
}

// Host side: p -> (thr, scale). False when p is outside [0, 1) or rounds to
// thr = 65536 (everything dropped, scale infinite). nearbyint rounds half to
// even, as Python's round() does in the reference.
static inline bool dropout_thr_scale(double p, uint32_t *thr, float *scale) {
  if (!(p >= 0.0 && p < 1.0)) return false;
  double t = nearbyint(p * 65536.0);
  if (t > 65535.0) return false;
  *thr = (uint32_t)t;
  *scale = 1.0f / (1.0f - (float)*thr / 65536.0f);
  return true;
}

// One Philox call per octet and a 32-bit octet counter
static inline bool dropout_numel_ok(long n) {
  return n > 0 && n % 8 == 0 && n / 8 < (1L << 32);
}
