// obstacle_sampling_host.cpp -- TEST-ONLY host build of the sampled obstacle (csrc/bmpc_rng.h and the
// sampled rule of csrc/bmpc_env.h / bmpc_env_quad.h; bmpc_set_obstacle_sampling).
//
// A stand-alone program under the address and undefined-behaviour sanitizers
// (tests/test_obstacle_sampling.py): the generator's known answers, the uniform's bounds, 64-bit egos
// and seeds, the inverse CDF's edges.  The CPU tests drive the draws and the scene functions with a
// sampler through tests/hostsim/scene_host.cpp.  Never loaded by the belief-planning_amd package.
#include <stdio.h>

#include "bmpc_env_quad.h"

using namespace bmpc;

static int failures = 0;
#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      printf("line %d: %s\n", __LINE__, #c);               \
      ++failures;                                          \
    }                                                      \
  } while (0)

static bool philox_is(const uint32_t (&c)[4], const uint32_t (&k)[2], const uint32_t (&want)[4]) {
  uint32_t o[4];
  philox4x32_10(c, k, o);
  return o[0] == want[0] && o[1] == want[1] && o[2] == want[2] && o[3] == want[3];
}

int main() {
  // the generator's known answers
  CHECK(philox_is({0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}));
  CHECK(philox_is({0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
                  {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}));
  CHECK(philox_is({0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
                  {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}));
  // the uniform: 0 at the all-zero words, the largest double below 1 at the all-ones words, and
  // only the 27 + 26 leading bits count
  CHECK(rng_uniform53(0, 0) == 0.0);
  CHECK(rng_uniform53(0xffffffffu, 0xffffffffu) == 0x1.fffffffffffffp-1);
  CHECK(rng_uniform53(0xffffffffu, 0xffffffffu) < 1.0);
  CHECK(rng_uniform53(0x1fu, 0x3fu) == 0.0);
  CHECK(rng_uniform53(0x20u, 0) == 0x1p-27 && rng_uniform53(0, 0x40u) == 0x1p-53);
  // a draw's counter is {lo32(g), hi32(g), epoch, 0} and its key {lo32(seed), hi32(seed)}: an ego
  // and a seed beyond 2^32 reach the high words (ego 2^33 + 5, seed 2^40 + 1, epoch 3)
  const uint64_t g = (1ull << 33) + 5, seed = (1ull << 40) + 1;
  CHECK(philox_is({5, 2, 3, 0}, {1, 256}, {0xf2b311b9u, 0x3bcbc246u, 0x3963fcdbu, 0x66f6cdafu}));
  CHECK(obstacle_uniform(seed, g, 3) == rng_uniform53(0xf2b311b9u, 0x3bcbc246u));
  CHECK(obstacle_uniform(seed, g, 3) == 0x1.e566234ef2f09p-1);
  CHECK(obstacle_uniform(seed, g, 3) != obstacle_uniform(seed, 5, 3));          // hi32(g) counts
  CHECK(obstacle_uniform(seed, g, 3) != obstacle_uniform(1, g, 3));             // hi32(seed) counts
  CHECK(obstacle_uniform(seed, g, 3) != obstacle_uniform(seed, g, 4));
  CHECK(obstacle_uniform(seed, g, 3) != rng_draw(seed, g, 3, 1));               // the purpose word counts
  for (uint64_t e = 0; e < 4096; ++e) {
    const double u = obstacle_uniform(7, e + (e % 3) * (1ull << 40), (uint32_t)(e % 5));
    CHECK(u >= 0.0 && u < 1.0);
  }
  // the inverse CDF: weights 1 2 1 -> partial sums 0.25, 0.75, 1 (exact in doubles)
  const double w[3] = {1.0, 2.0, 1.0};
  CHECK(rng_inverse_cdf(w, 3, 0.0) == 0);
  CHECK(rng_inverse_cdf(w, 3, 0x1.fffffffffffffp-3) == 0);    // just below 0.25
  CHECK(rng_inverse_cdf(w, 3, 0.25) == 1);                    // at a partial sum: the next policy
  CHECK(rng_inverse_cdf(w, 3, 0x1.7ffffffffffffp-1) == 1);    // just below 0.75
  CHECK(rng_inverse_cdf(w, 3, 0.75) == 2);
  CHECK(rng_inverse_cdf(w, 3, 0x1.fffffffffffffp-1) == 2);
  // no j qualifies (partial sums that stay at or below u: thirds summing to less than u; NaN
  // weights): m - 1
  const double third[3] = {1.0 / 3, 1.0 / 3, 1.0 / 3};
  CHECK(rng_inverse_cdf(third, 3, 1.0) == 2);
  const double zero[2] = {0.0, 0.0};
  CHECK(rng_inverse_cdf(zero, 2, 0.5) == 1);
  const double one[1] = {3.0};
  CHECK(rng_inverse_cdf(one, 1, 0.0) == 0 && rng_inverse_cdf(one, 1, 0x1.fffffffffffffp-1) == 0);
  // inside an epoch the scene keeps the row's last choice, clamped to a policy
  bmpc_obstacle_sampling S = {BMPC_OBS_SAMPLE_MODEL, 3, 7, 0};
  const double mc[8] = {4.0, 2.5, 2.0, 3.0};
  const bmpc_policy pol[3] = {{BMPC_POL_MAINTAIN, 0, {0.1}}, {BMPC_POL_BRAKE, 0, {0.1}},
                              {BMPC_POL_LC, 0, {0, 5.4, 20, 0}}};
  const double x[4] = {0, 1.8, 20, 0}, z[4] = {5, 5.4, 20, 0};
  CHECK(env_sampled_choice<Highway>(S, 0, mc, 0.1, 6, 3, 1, pol, x, z, 2.0) == 2);
  CHECK(env_sampled_choice<Highway>(S, 0, mc, 0.1, 6, 3, 2, pol, x, z, 1.0) == 1);
  CHECK(env_sampled_choice<Highway>(S, 0, mc, 0.1, 6, 3, 1, pol, x, z, 9.0) == 2);
  CHECK(env_sampled_choice<Highway>(S, 0, mc, 0.1, 6, 3, 1, pol, x, z, -4.0) == 0);
  const int c0 = env_sampled_choice<Highway>(S, 0, mc, 0.1, 6, 3, 3, pol, x, z, 0.0);
  CHECK(c0 >= 0 && c0 < 3);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
