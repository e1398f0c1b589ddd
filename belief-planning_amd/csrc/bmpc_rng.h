// bmpc_rng.h -- the closed loops' counter-based random draws (bmpc_set_obstacle_sampling).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): a keyed
// bijection of a 128-bit counter, no state.  A draw is addressed, never consumed -- counter
//   {lo32(g), hi32(g), epoch, purpose},  key {lo32(seed), hi32(seed)},
// g the ego's global index (the plan's ego_base + its ego e), epoch = t / hold, purpose 0 the
// obstacle's backup policy -- so the launch path, the split of a loop over calls and the shard an
// ego lives in cannot change it.  Plain integer arithmetic, the same on host and device;
// bmpc/rng.py restates it in NumPy.
#pragma once

#include "bmpc_core.h"

namespace bmpc {

enum { RNG_PURPOSE_OBSTACLE_POLICY = 0 };   // other purposes are reserved

// out = Philox4x32-10(counter c, key k)
BMPC_HD void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += W0;
    k1 += W1;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// 53 bits of two output words as a double in [0, 1): exact, the same double everywhere
BMPC_HD double rng_uniform53(uint32_t o0, uint32_t o1) {
  const uint64_t bits = ((uint64_t)(o0 >> 5) << 26) | (uint64_t)(o1 >> 6);
  return (double)bits * (1.0 / 9007199254740992.0);
}

// the uniform of (seed, global ego g, epoch) for one purpose
BMPC_HD double rng_draw(uint64_t seed, uint64_t g, uint32_t epoch, uint32_t purpose) {
  const uint32_t c[4] = {(uint32_t)g, (uint32_t)(g >> 32), epoch, purpose};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  philox4x32_10(c, k, o);
  return rng_uniform53(o[0], o[1]);
}
BMPC_HD double obstacle_uniform(uint64_t seed, uint64_t g, uint32_t epoch) {
  return rng_draw(seed, g, epoch, RNG_PURPOSE_OBSTACLE_POLICY);
}

// Inverse CDF over m weights: p_j = w_j / sum with the sum taken in order j = 0, 1, ...; the
// smallest j with u < p_0 + ... + p_j (partial sums in that order), m - 1 if none.
BMPC_HD int rng_inverse_cdf(const double* w, int m, double u) {
  double sum = 0.0;
  for (int j = 0; j < m; ++j) sum += w[j];
  double acc = 0.0;
  for (int j = 0; j < m; ++j) {
    acc += w[j] / sum;
    if (u < acc) return j;
  }
  return m - 1;
}

}  // namespace bmpc
