// disturbance_host.cpp -- TEST-ONLY host build of the actuation disturbance (csrc/bmpc_rng.h's
// rng_ih4 / rng_disturbance / rng_disturb_input and the three scene functions' post(t-1);
// bmpc_set_disturbance).
//
// A stand-alone program under the address and undefined-behaviour sanitizers
// (tests/test_disturbance.py): the variate's known answers, its two extremes, 64-bit egos and seeds,
// sigma = 0.  The CPU tests drive the draws and the three scene functions with a disturbance through
// tests/hostsim/scene_host.cpp.  Never loaded by the belief-planning_amd package.
#include <stdio.h>

#include "bmpc_env_merge.h"
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

int main() {
  // known answers of xi (bmpc/rng.py's disturbance): purposes 12, 13 at (seed 7, ego 0, step 3) and
  // 8, 9, 10 at (7, 1, 3)
  CHECK(rng_disturbance(7, 0, 3, RNG_PURPOSE_DISTURB_EGO) == 0x1.46d85550b5cdfp+1);
  CHECK(rng_disturbance(7, 0, 3, RNG_PURPOSE_DISTURB_EGO + 1) == -0x1.167cc2e809c2fp+0);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_DISTURB_OBSTACLE) == 0x1.3ce0a09bb3364p-1);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_DISTURB_OBSTACLE + 1) == -0x1.27098008c1499p+0);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_DISTURB_OBSTACLE + 2) == 0x1.f3a0675fcfdb3p-3);
  CHECK(RNG_PURPOSE_DISTURB_OBSTACLE == 8 && RNG_PURPOSE_DISTURB_EGO == 12);
  // the two extremes: -+ 2 (2^32 - 1) K at the all-zero / all-ones output words, inside 2 sqrt(3);
  // the centre, and one unit of the integer sum
  const uint32_t zeros[4] = {0, 0, 0, 0}, ones[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  CHECK(rng_ih4(zeros) == -0x1.bb67ae83c962fp+1 && rng_ih4(ones) == 0x1.bb67ae83c962fp+1);
  CHECK(rng_ih4(ones) == 8589934590.0 * 0x1.bb67ae8584caap-32 && rng_ih4(ones) < 0x1.bb67ae8584caap+1);
  const uint32_t mid[4] = {0xffffffffu, 0, 0xffffffffu, 0}, unit[4] = {0xffffffffu, 1, 0xffffffffu, 0};
  CHECK(rng_ih4(mid) == 0.0 && rng_ih4(unit) == 0x1.bb67ae8584caap-32);
  // g and seed beyond 2^32 reach the counter's and the key's high words (ego 2^33 + 5, seed 2^40 + 1)
  const uint64_t g = (1ull << 33) + 5, seed = (1ull << 40) + 1;
  {
    const uint32_t c[4] = {5, 2, 3, 12}, k[2] = {1, 256};
    uint32_t o[4];
    philox4x32_10(c, k, o);
    CHECK(o[0] == 89502319u && o[1] == 1683228240u && o[2] == 3711361203u && o[3] == 2075856137u);
    CHECK(rng_disturbance(seed, g, 3, 12) == rng_ih4(o));
  }
  CHECK(rng_disturbance(seed, g, 3, 12) == -0x1.a956107fba1b8p-2);
  CHECK(rng_disturbance(seed, g, 3, 15) == 0x1.191ca9232a4a8p+0);
  CHECK(rng_disturbance(~0ull, 1ull << 32, 4, 8) == -0x1.223920708af30p+0);
  CHECK(rng_disturbance(seed, g, 3, 12) != rng_disturbance(seed, 5, 3, 12));   // hi32(g) counts
  CHECK(rng_disturbance(seed, g, 3, 12) != rng_disturbance(1, g, 3, 12));      // hi32(seed) counts
  CHECK(rng_disturbance(seed, g, 3, 12) != rng_disturbance(seed, g, 4, 12));
  CHECK(rng_disturbance(seed, g, 3, 12) != rng_disturbance(seed, g, 3, 8));    // the purpose word counts
  for (uint64_t e = 0; e < 4096; ++e) {
    const double xi = rng_disturbance(7, e + (e % 3) * (1ull << 40), (uint32_t)(e % 5), 8 + (uint32_t)(e % 8));
    CHECK(xi >= -0x1.bb67ae8584caap+1 && xi <= 0x1.bb67ae8584caap+1);
  }
  // the applied input: null, law NONE and sigma = 0 pass the input through to the bit (-0.0 too);
  // a non-zero sigma adds sigma * xi of (ego_base + e, t, purpose + c), component by component
  const double u[3] = {1.25, -0.0, 3.0};
  double out[3];
  bmpc_disturbance D = {};
  D.law = BMPC_DISTURB_IH4;
  D.seed = 7;
  D.ego_base = 1;
  rng_disturb_input(nullptr, true, 0, 3, 3, u, out);
  CHECK(out[0] == 1.25 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0);
  rng_disturb_input(&D, true, 0, 3, 3, u, out);   // all sigmas zero
  CHECK(out[0] == 1.25 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0);
  D.sigma_obs[0] = 0.5;
  D.sigma_obs[2] = 2.0;
  D.sigma_ego[1] = 0.25;
  rng_disturb_input(&D, false, 0, 3, 3, u, out);   // global ego 1, step 3, purposes 8 and 10
  CHECK(out[0] == 1.25 + 0.5 * 0x1.3ce0a09bb3364p-1 && out[1] == 0.0 && std::signbit(out[1]));
  CHECK(out[2] == 3.0 + 2.0 * 0x1.f3a0675fcfdb3p-3);
  rng_disturb_input(&D, true, -1, 3, 3, u, out);   // global ego 0, purpose 13 only
  CHECK(out[0] == 1.25 && out[1] == -0.0 + 0.25 * -0x1.167cc2e809c2fp+0 && out[2] == 3.0);
  D.law = BMPC_DISTURB_NONE;
  rng_disturb_input(&D, false, 0, 3, 3, u, out);
  CHECK(out[0] == 1.25 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0);
  // a scene step: sigma = 0 and law NONE leave the Euler step as it is, a non-zero sigma moves it and
  // keeps the row's nominal obstacle input
  {
    const bmpc_merge_env_desc E = {};
    const double tab[6] = {0.0, 100.0, 1.8, 1.8, 0.0, 0.0}, bxp[4] = {5.95, -1.25, 0.25, 0.25}, u0[2] = {0.5, 0.01};
    const MergeRef R{tab, 2};
    double a[ENV_STRIDE] = {0, 1.8, 20, 0, 10, 5.4, 19, 0.01, 0.3, -0.001}, b[ENV_STRIDE], c[ENV_STRIDE];
    for (int i = 0; i < ENV_STRIDE; ++i) b[i] = c[i] = a[i];
    double x[4], z[4], xr[4], S[16], bx[4];
    bmpc_disturbance Z = {};
    Z.law = BMPC_DISTURB_IH4;
    merge_env_step_ego(E, R, bxp, 4, 0.1, 1, a, u0, x, z, xr, S, bx);
    merge_env_step_ego(E, R, bxp, 4, 0.1, 1, b, u0, x, z, xr, S, bx, &Z, 3);
    for (int i = 0; i < ENV_STRIDE; ++i) CHECK(a[i] == b[i]);
    Z.sigma_obs[0] = 0.5;
    merge_env_step_ego(E, R, bxp, 4, 0.1, 1, c, u0, x, z, xr, S, bx, &Z, 3);
    for (int i = 0; i < 4; ++i) CHECK(c[ENV_X + i] == a[ENV_X + i]);
    CHECK(c[ENV_Z + 2] == 19.0 + (0.3 + 0.5 * rng_disturbance(0, 3, 0, 8)) * 0.1 && c[ENV_Z + 2] != a[ENV_Z + 2]);
    CHECK(c[ENV_UOBS] == 0.5 * (E.v0 - c[ENV_Z + 2]));
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
