// observation_host.cpp -- TEST-ONLY host build of the observation noise (csrc/bmpc_rng.h's
// rng_observe_state and the three scene functions' x_out / z_out; bmpc_set_observation).
//
// Two uses of one file.  As a stand-alone program under the address and undefined-behaviour sanitizers
// (tests/test_observation.py): the variate's known answers at the two purpose bases, its two
// extremes, 64-bit egos and seeds, sigma = 0, and one scene step of each scene with every array at
// its exact size.  As a shared library (tests/observation_common.py): the three scene steps over a
// batch with every argument the kernels pass, the observation model last -- scene_host.h's wrappers
// keep the argument list the scene functions had before it.  Never loaded by the belief-planning_amd
// package.
#include <stdio.h>

#include <cmath>

#include "bmpc_env_merge.h"
#include "bmpc_env_quad.h"

using namespace bmpc;

extern "C" {

// One overtake scene step of `batch` egos as k_env runs it (scene_host.h's sh_env_step with obs)
int oh_env_step(const bmpc_env_desc* env, const double* mc, double dt, int N, int m, int t, int batch, double* scene,
                bmpc_policy* pol, const double* upred, int upred_stride, double* x, double* z, double* xref,
                const bmpc_obstacle_sampling* smp, const bmpc_obstacle_proposal* prop, const bmpc_disturbance* dist,
                const bmpc_observation* obs) {
  if (m < 1 || m > BMPC_MAX_M) return -22;
  if (smp && smp->mode >= BMPC_OBS_SAMPLE_TILTED && !prop) return -22;
  for (int e = 0; e < batch; ++e)
    env_step_ego(*env, dt, N, m, t, scene + (size_t)e * ENV_STRIDE, pol + (size_t)e * m,
                 upred ? upred + (size_t)e * upred_stride : nullptr, x + (size_t)e * 4, z + (size_t)e * 4,
                 xref + (size_t)e * 4, smp, mc, e, prop, dist, obs);
  return 0;
}

// One merge scene step as k_env_merge runs it (sh_merge_env_step with obs)
int oh_merge_env_step(const bmpc_merge_env_desc* env, int nref, const double* ref, const double* bx_plan, int nbx,
                      double dt, int t, int batch, double* scene, const double* upred, int upred_stride, const double* J,
                      const int32_t* status, const int32_t* iters, double* x, double* z, double* xref, double* S,
                      double* bx, double* stats, const bmpc_disturbance* dist, const bmpc_observation* obs) {
  const MergeRef R{ref, nref};
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    if (t > 0 && stats && J && status && iters)
      env_accumulate(st, J[e], status[e], iters[e], true, stats + (size_t)e * ENVS_STRIDE);
    merge_env_step_ego(*env, R, bx_plan, nbx, dt, t, st, upred ? upred + (size_t)e * upred_stride : nullptr,
                       x + (size_t)e * 4, z + (size_t)e * 4, xref + (size_t)e * 4, S + (size_t)e * 16,
                       bx + (size_t)e * nbx, dist, e, obs);
  }
  return 0;
}

// One quadruped scene step as k_env_quad runs it (sh_quad_env_step with obs)
int oh_quad_env_step(const bmpc_quad_env_desc* env, const double* mc, double dt, int N, int m, int t, int batch,
                     double* scene, const bmpc_policy* pol, const double* upred, int upred_stride, const double* J,
                     const int32_t* status, const int32_t* iters, double* x, double* z, double* xref, double* stats,
                     const bmpc_obstacle_sampling* smp, const bmpc_obstacle_proposal* prop,
                     const bmpc_disturbance* dist, const bmpc_observation* obs) {
  if (m < 1 || m > BMPC_MAX_M) return -22;
  if (smp && smp->mode >= BMPC_OBS_SAMPLE_TILTED && !prop) return -22;
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    if (t > 0 && stats && J && status && iters)
      env_accumulate(st, J[e], status[e], iters[e], false, stats + (size_t)e * ENVS_STRIDE);
    quad_env_step_ego(*env, mc, dt, N, m, t, st, pol + (size_t)e * m, upred ? upred + (size_t)e * upred_stride : nullptr,
                      x + (size_t)e * 3, z + (size_t)e * 3, xref + (size_t)e * 3, smp, e, prop, dist, obs);
  }
  return 0;
}

}  // extern "C"

static int failures = 0;
#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      printf("line %d: %s\n", __LINE__, #c);               \
      ++failures;                                          \
    }                                                      \
  } while (0)

int main() {
  // known answers of xi at the two purpose bases (bmpc/rng.py's observation): purposes 24..27 at
  // (seed 7, ego 0, step 3) and 16..19 at (7, 1, 3)
  CHECK(RNG_PURPOSE_OBSERVE_OBSTACLE == 16 && RNG_PURPOSE_OBSERVE_EGO == 24);
  CHECK(RNG_PURPOSE_OBSERVE_OBSTACLE + BMPC_MAX_N == RNG_PURPOSE_OBSERVE_EGO);   // (8 components each)
  CHECK(RNG_PURPOSE_DISTURB_EGO + BMPC_MAX_D == RNG_PURPOSE_OBSERVE_OBSTACLE);   // (no purpose shared)
  CHECK(rng_disturbance(7, 0, 3, RNG_PURPOSE_OBSERVE_EGO) == -0x1.01c6e2f7f0efdp-1);
  CHECK(rng_disturbance(7, 0, 3, RNG_PURPOSE_OBSERVE_EGO + 1) == -0x1.269c7a8300863p-1);
  CHECK(rng_disturbance(7, 0, 3, RNG_PURPOSE_OBSERVE_EGO + 2) == 0x1.bc74b8e2cc824p-1);
  CHECK(rng_disturbance(7, 0, 3, RNG_PURPOSE_OBSERVE_EGO + 3) == -0x1.88420a06a48a6p+0);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_OBSERVE_OBSTACLE) == -0x1.fb612af7eee0fp-2);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_OBSERVE_OBSTACLE + 1) == -0x1.5d417cb0ecdbdp-1);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_OBSERVE_OBSTACLE + 2) == 0x1.930824c42bcc6p-2);
  CHECK(rng_disturbance(7, 1, 3, RNG_PURPOSE_OBSERVE_OBSTACLE + 3) == 0x1.23601648abf31p+0);
  // the two extremes: -+ 2 (2^32 - 1) K at the all-zero / all-ones output words, inside 2 sqrt(3)
  const uint32_t zeros[4] = {0, 0, 0, 0}, ones[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  CHECK(rng_ih4(zeros) == -8589934590.0 * 0x1.bb67ae8584caap-32 && rng_ih4(ones) == 8589934590.0 * 0x1.bb67ae8584caap-32);
  CHECK(rng_ih4(ones) == 0x1.bb67ae83c962fp+1 && rng_ih4(ones) < 0x1.bb67ae8584caap+1);
  // g and seed beyond 2^32 reach the counter's and the key's high words (ego 2^33 + 5, seed 2^40 + 1)
  const uint64_t g = (1ull << 33) + 5, seed = (1ull << 40) + 1;
  {
    const uint32_t c[4] = {5, 2, 3, 16}, k[2] = {1, 256};
    uint32_t o[4];
    philox4x32_10(c, k, o);
    CHECK(o[0] == 1692862641u && o[1] == 4188569856u && o[2] == 1281722131u && o[3] == 2629544381u);
    CHECK(rng_disturbance(seed, g, 3, 16) == rng_ih4(o));
  }
  CHECK(rng_disturbance(seed, g, 3, 16) == 0x1.f0af6eecf9eb4p-2);
  CHECK(rng_disturbance(seed, g, 3, 23) == -0x1.835d0049c2acap+0);   // the last obstacle purpose
  CHECK(rng_disturbance(seed, g, 3, 24) == -0x1.6bbf1de882afep-2);
  CHECK(rng_disturbance(seed, g, 3, 31) == -0x1.7b27443a6dd28p-2);   // the last ego purpose
  CHECK(rng_disturbance(~0ull, 1ull << 32, 4, 16) == 0x1.54ce2a521d122p+0);
  CHECK(rng_disturbance(seed, g, 3, 16) != rng_disturbance(seed, 5, 3, 16));   // hi32(g) counts
  CHECK(rng_disturbance(seed, g, 3, 16) != rng_disturbance(1, g, 3, 16));      // hi32(seed) counts
  CHECK(rng_disturbance(seed, g, 3, 16) != rng_disturbance(seed, g, 4, 16));
  CHECK(rng_disturbance(seed, g, 3, 16) != rng_disturbance(seed, g, 3, 8));    // not the disturbance's draw
  CHECK(rng_disturbance(seed, g, 3, 24) != rng_disturbance(seed, g, 3, 12));
  for (uint64_t e = 0; e < 4096; ++e) {
    const double xi = rng_disturbance(7, e + (e % 3) * (1ull << 40), (uint32_t)(e % 5), 16 + (uint32_t)(e % 16));
    CHECK(xi >= -0x1.bb67ae8584caap+1 && xi <= 0x1.bb67ae8584caap+1);
  }
  // the observed state: null, law NONE and sigma = 0 pass the state through to the bit (-0.0 too); a
  // non-zero sigma adds sigma * xi of (ego_base + e, t, purpose + c), component by component, and the
  // truth is not written
  const double v[4] = {1.25, -0.0, 3.0, -7.5};
  double out[4];
  bmpc_observation O = {};
  O.law = BMPC_OBSERVE_IH4;
  O.seed = 7;
  O.ego_base = 1;
  rng_observe_state(nullptr, true, 0, 3, 4, v, out);
  CHECK(out[0] == 1.25 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0 && out[3] == -7.5);
  rng_observe_state(&O, false, 0, 3, 4, v, out);   // all sigmas zero
  CHECK(out[0] == 1.25 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0 && out[3] == -7.5);
  O.sigma_z[0] = 0.5;
  O.sigma_z[3] = 2.0;
  O.sigma_x[1] = 0.25;
  rng_observe_state(&O, false, 0, 3, 4, v, out);   // global ego 1, step 3, purposes 16 and 19
  CHECK(out[0] == 1.25 + 0.5 * -0x1.fb612af7eee0fp-2 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0);
  CHECK(out[3] == -7.5 + 2.0 * 0x1.23601648abf31p+0);
  rng_observe_state(&O, true, -1, 3, 4, v, out);   // global ego 0, purpose 25 only
  CHECK(out[0] == 1.25 && out[1] == -0.0 + 0.25 * -0x1.269c7a8300863p-1 && out[2] == 3.0 && out[3] == -7.5);
  CHECK(v[0] == 1.25 && std::signbit(v[1]) && v[2] == 3.0 && v[3] == -7.5);
  O.law = BMPC_OBSERVE_NONE;
  rng_observe_state(&O, false, 0, 3, 4, v, out);
  CHECK(out[0] == 1.25 && out[1] == 0.0 && std::signbit(out[1]) && out[2] == 3.0 && out[3] == -7.5);
  {
    // the last component of a full-width state draws at purposes 23 / 31
    bmpc_observation W = {};
    W.law = BMPC_OBSERVE_IH4;
    W.seed = seed;
    W.sigma_x[7] = W.sigma_z[7] = 1.0;
    const double w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double o8[8];
    rng_observe_state(&W, false, (long long)g, 3, 8, w, o8);
    CHECK(o8[7] == -0x1.835d0049c2acap+0 && o8[6] == 0.0);
    rng_observe_state(&W, true, (long long)g, 3, 8, w, o8);
    CHECK(o8[7] == -0x1.7b27443a6dd28p-2 && o8[0] == 0.0);
  }
  // a merge scene step: sigma = 0 and law NONE leave every output as it is; a non-zero sigma_z moves
  // z_out at that component only and leaves the row, x_out, x_ref, S and bx alone
  {
    const bmpc_merge_env_desc E = {};
    const double tab[6] = {0.0, 100.0, 1.8, 1.8, 0.0, 0.0}, bxp[4] = {5.95, -1.25, 0.25, 0.25}, u0[2] = {0.5, 0.01};
    const MergeRef R{tab, 2};
    double a[ENV_STRIDE] = {0, 1.8, 20, 0, 10, 5.4, 19, 0.01, 0.3, -0.001}, b[ENV_STRIDE], c[ENV_STRIDE];
    for (int i = 0; i < ENV_STRIDE; ++i) b[i] = c[i] = a[i];
    double x[4], z[4], xr[4], S[16], bx[4], x2[4], z2[4], xr2[4], S2[16], bx2[4];
    bmpc_observation Z = {};
    Z.law = BMPC_OBSERVE_IH4;
    merge_env_step_ego(E, R, bxp, 4, 0.1, 1, a, u0, x, z, xr, S, bx);
    merge_env_step_ego(E, R, bxp, 4, 0.1, 1, b, u0, x2, z2, xr2, S2, bx2, nullptr, 3, &Z);
    for (int i = 0; i < ENV_STRIDE; ++i) CHECK(a[i] == b[i]);
    for (int i = 0; i < 4; ++i) CHECK(x[i] == x2[i] && z[i] == z2[i]);
    Z.sigma_z[2] = 0.5;
    merge_env_step_ego(E, R, bxp, 4, 0.1, 1, c, u0, x2, z2, xr2, S2, bx2, nullptr, 3, &Z);
    for (int i = 0; i < ENV_STRIDE; ++i) CHECK(a[i] == c[i]);
    for (int i = 0; i < 4; ++i) CHECK(x[i] == x2[i] && xr[i] == xr2[i] && bx[i] == bx2[i] && (i == 2 || z[i] == z2[i]));
    for (int i = 0; i < 16; ++i) CHECK(S[i] == S2[i]);
    CHECK(z2[2] == c[ENV_Z + 2] + 0.5 * rng_disturbance(0, 3, 1, 18) && z2[2] != z[2]);   // step t = 1 itself
  }
  // an overtake and a quadruped scene step through the batch wrappers, one ego, arrays at their exact sizes
  {
    bmpc_env_desc E = {};
    E.n_lane = 4, E.L = 4.0, E.W = 2.5, E.Kpsi = 0.1, E.v0 = 20.0, E.vlen = 4.0, E.vwid = 2.4;
    const double mc[8] = {4.0, 2.5, 2.0, 4.0, 0, 0, 0, 0}, u0[2] = {0.5, 0.01};
    double a[ENV_STRIDE] = {0, 1.8, 20, 0, 10, 5.4, 19, 0.01}, b[ENV_STRIDE];
    for (int i = 0; i < ENV_STRIDE; ++i) b[i] = a[i];
    bmpc_policy pa[2] = {}, pb[2] = {};
    double x[4], z[4], xr[4], x2[4], z2[4], xr2[4];
    bmpc_observation Z = {};
    Z.law = BMPC_OBSERVE_IH4;
    Z.sigma_x[3] = 0.125;
    CHECK(oh_env_step(&E, mc, 0.1, 4, 2, 1, 1, a, pa, u0, 2, x, z, xr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(oh_env_step(&E, mc, 0.1, 4, 2, 1, 1, b, pb, u0, 2, x2, z2, xr2, nullptr, nullptr, nullptr, &Z) == 0);
    for (int i = 0; i < ENV_STRIDE; ++i) CHECK(a[i] == b[i]);
    for (int i = 0; i < 4; ++i) CHECK(z[i] == z2[i] && xr[i] == xr2[i] && (i == 3 || x[i] == x2[i]));
    CHECK(x2[3] == b[ENV_X + 3] + 0.125 * rng_disturbance(0, 0, 1, 27) && x2[3] != x[3]);
  }
  {
    const bmpc_quad_env_desc E = {0.5, 5.0, 0.1};
    const double mc[8] = {0.5, 0.5, 1.0, 1.0, 1.0, 1.0, 0, 0}, u0[3] = {0.1, 0.0, 0.05};
    double a[ENV_STRIDE] = {0, 0, 0, 2, 1, 0.5, 0, 0, 0, 5, -3, 0}, b[ENV_STRIDE];
    for (int i = 0; i < ENV_STRIDE; ++i) b[i] = a[i];
    const bmpc_policy pol[2] = {};
    double x[3], z[3], xr[3], x2[3], z2[3], xr2[3];
    bmpc_observation Z = {};
    Z.law = BMPC_OBSERVE_IH4;
    Z.ego_base = 9;
    Z.sigma_z[0] = 0.02;
    CHECK(oh_quad_env_step(&E, mc, 0.1, 4, 2, 1, 1, a, pol, u0, 3, nullptr, nullptr, nullptr, x, z, xr, nullptr, nullptr,
                           nullptr, nullptr, nullptr) == 0);
    CHECK(oh_quad_env_step(&E, mc, 0.1, 4, 2, 1, 1, b, pol, u0, 3, nullptr, nullptr, nullptr, x2, z2, xr2, nullptr,
                           nullptr, nullptr, nullptr, &Z) == 0);
    for (int i = 0; i < ENV_STRIDE; ++i) CHECK(a[i] == b[i]);
    for (int i = 0; i < 3; ++i) CHECK(x[i] == x2[i] && xr[i] == xr2[i] && (i == 0 || z[i] == z2[i]));
    CHECK(z2[0] == b[QENV_Z] + 0.02 * rng_disturbance(0, 9, 1, 16) && z2[0] != z[0]);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
