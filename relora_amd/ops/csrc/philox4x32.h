// Philox4x32-10 with a full four-word counter, and the stochastic
// fp32 -> bf16 rounding rule built on it (docs/KERNELS.md, "AdamW number
// formats"). Counter-based: the bits depend only on (key, counter), never
// on grid shape, so any kernel that agrees on the counter layout agrees on
// the bits. The reference implementation is relora_amd/ops/philox.py.
#pragma once

#include "common.h"

struct Philox4 { uint32_t w[4]; };

DEV_INLINE Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                 uint32_t c2, uint32_t c3) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {  // the key advances between rounds: nine bumps for ten rounds
      k0 += W0;
      k1 += W1;
    }
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  Philox4 out;
  out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
  return out;
}

// The optimizer's counter layout: key = halves of the 64-bit seed, counter =
// (element index low, element index high, step, tensor ordinal).
DEV_INLINE Philox4 philox_for_element(uint32_t seed_lo, uint32_t seed_hi, long index,
                                      uint32_t step, uint32_t ordinal) {
  const unsigned long idx = (unsigned long)index;
  return philox4x32_10(seed_lo, seed_hi, (uint32_t)idx, (uint32_t)(idx >> 32), step, ordinal);
}

// 16 random bits per destination, one Philox call per element:
// lane 0 = parameter, lane 1 = exp_avg, lane 2 = exp_avg_sq.
DEV_INLINE uint32_t philox_lane16(const Philox4& r, int lane) {
  return lane == 0 ? (r.w[0] & 0xFFFFu) : lane == 1 ? (r.w[0] >> 16) : (r.w[1] & 0xFFFFu);
}

// Stochastic rounding: upper 16 bits of (bits(x) + r16). The magnitude rounds
// up with probability low16/65536, exact values never move, and a carry out of
// the largest finite exponent gives inf. inf/nan take the nearest conversion.
DEV_INLINE __hip_bfloat16 stochastic_round_bf16(float x, uint32_t r16) {
  const uint32_t u = __float_as_uint(x);
  if (((u >> 23) & 0xFFu) == 0xFFu) return from_f32<__hip_bfloat16>(x);
  const unsigned short hi = (unsigned short)((u + r16) >> 16);
  __hip_bfloat16 out;
  __builtin_memcpy(&out, &hi, sizeof(hi));
  return out;
}
