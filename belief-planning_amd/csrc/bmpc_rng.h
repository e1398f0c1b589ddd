// bmpc_rng.h -- the closed loops' counter-based random draws (bmpc_set_obstacle_sampling,
// bmpc_set_disturbance, bmpc_set_observation).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): a keyed
// bijection of a 128-bit counter, no state.  A draw is addressed, never consumed -- counter
//   {lo32(g), hi32(g), epoch, purpose},  key {lo32(seed), hi32(seed)},
// g the ego's global index (the plan's ego_base + its ego e), epoch = t / hold, purpose 0 the
// obstacle's backup policy -- so the launch path, the split of a loop over calls and the shard an
// ego lives in cannot change it.  The actuation disturbance (rng_disturbance below) is addressed the
// same way, by the step t itself and one purpose per vehicle and input component, and so is the
// observation noise (rng_observe_state), with one purpose per vehicle and state component.  Plain
// integer arithmetic, the same on host and device; bmpc/rng.py restates it in NumPy.
#pragma once

#include "bmpc_core.h"

namespace bmpc {

// counter word 3: 0 the obstacle's policy, 1 the resampling draw (bmpc_resample.h), 8 + c / 12 + c
// component c of the obstacle's / the ego's actuation disturbance (c < BMPC_MAX_D), 16 + c / 24 + c
// component c of the observed obstacle / ego state (c < BMPC_MAX_N); 2-7 are reserved
enum {
  RNG_PURPOSE_OBSTACLE_POLICY = 0,
  RNG_PURPOSE_DISTURB_OBSTACLE = 8,
  RNG_PURPOSE_DISTURB_EGO = 12,
  RNG_PURPOSE_OBSERVE_OBSTACLE = 16,
  RNG_PURPOSE_OBSERVE_EGO = 24
};

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

// The actuation disturbance's variate (bmpc_set_disturbance, law BMPC_DISTURB_IH4): the centred sum
// of the four output words, an exact integer |s| < 2^34, times sqrt(3) / 2^32 -- one rounding, so the
// same double on host, device and in NumPy.  Irwin-Hall with four terms: mean 0, variance 1 - 2^-64,
// kurtosis 2.7, |xi| <= 2 sqrt(3).
BMPC_HD double rng_ih4(const uint32_t o[4]) {
  const int64_t s = (int64_t)o[0] + (int64_t)o[1] + (int64_t)o[2] + (int64_t)o[3] - 2 * (int64_t)0xFFFFFFFFu;
  return (double)s * 0x1.bb67ae8584caap-32;
}
// xi of (seed, global ego g, closed-loop step t) for one purpose (RNG_PURPOSE_DISTURB_* or
// RNG_PURPOSE_OBSERVE_* + component)
BMPC_HD double rng_disturbance(uint64_t seed, uint64_t g, uint32_t t, uint32_t purpose) {
  const uint32_t c[4] = {(uint32_t)g, (uint32_t)(g >> 32), t, purpose};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  philox4x32_10(c, k, o);
  return rng_ih4(o);
}
// out[c] = v[c] + sigma[c] * xi(seed, g, t, purpose0 + c) for c < n, the product rounded before it is
// added; a component with sigma == 0 makes no draw and passes v[c] through to the bit.  The one loop
// behind the disturbed inputs and the observed states.
BMPC_HD void rng_add_noise(uint64_t seed, uint64_t g, uint32_t t, uint32_t purpose0, const double* sigma, int n,
                           const double* v, double* out) {
  for (int c = 0; c < n; ++c)
    if (sigma[c] != 0.0) {
#pragma clang fp contract(off)
      const double dv = sigma[c] * rng_disturbance(seed, g, t, purpose0 + c);
      out[c] = v[c] + dv;
    } else {
      out[c] = v[c];
    }
}
// The input a vehicle applies at step t under the disturbance D (null or law NONE: u itself):
// out[c] = u[c] + sigma[c] * xi(g, t, purpose0 + c) (rng_add_noise).  ego: the ego's input (sigma_ego,
// purposes 12 + c) or the obstacle's (sigma_obs, 8 + c); e: the ego's index in the plan; d <= BMPC_MAX_D.
BMPC_HD void rng_disturb_input(const bmpc_disturbance* D, bool ego, long long e, int t, int d, const double* u,
                               double* out) {
  if (!D || D->law != BMPC_DISTURB_IH4) {
    for (int c = 0; c < d; ++c) out[c] = u[c];
    return;
  }
  rng_add_noise(D->seed, (uint64_t)(D->ego_base + e), (uint32_t)t,
                ego ? RNG_PURPOSE_DISTURB_EGO : RNG_PURPOSE_DISTURB_OBSTACLE, ego ? D->sigma_ego : D->sigma_obs, d, u, out);
}
// The state the solve of step t is handed under the perception model O (bmpc_set_observation; null or
// law NONE: v itself): out[c] = v[c] + sigma[c] * xi(g, t, purpose0 + c) (rng_add_noise).  ego: the
// ego's own state (sigma_x, purposes 24 + c) or the obstacle's (sigma_z, 16 + c); e: the ego's index
// in the plan; n <= BMPC_MAX_N.  v is the truth and is not written.
BMPC_HD void rng_observe_state(const bmpc_observation* O, bool ego, long long e, int t, int n, const double* v,
                               double* out) {
  if (!O || O->law != BMPC_OBSERVE_IH4) {
    for (int c = 0; c < n; ++c) out[c] = v[c];
    return;
  }
  rng_add_noise(O->seed, (uint64_t)(O->ego_base + e), (uint32_t)t,
                ego ? RNG_PURPOSE_OBSERVE_EGO : RNG_PURPOSE_OBSERVE_OBSTACLE, ego ? O->sigma_x : O->sigma_z, n, v, out);
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
