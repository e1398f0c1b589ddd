// obstacle_proposal_host.cpp -- TEST-ONLY host build of the weighted obstacle modes (the tilted and the
// scripted rule of csrc/bmpc_env.h / bmpc_env_quad.h; bmpc_set_obstacle_proposal).
//
// A stand-alone program under the address and undefined-behaviour sanitizers
// (tests/test_obstacle_proposal.py): a tilt of ones against mode 1, the log-weight of a tilted and of
// a scripted choice, the script's clamps at a table of exactly its size, the epochs' untouched steps,
// and whole scene steps of both scenes in both modes through scene_host.h's wrappers -- the ones the
// CPU tests drive as a shared library (tests/hostsim/scene_host.cpp).  Never loaded by the
// belief-planning_amd package.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "scene_host.h"

using namespace bmpc;

static int failures = 0;
#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      printf("line %d: %s\n", __LINE__, #c);               \
      ++failures;                                          \
    }                                                      \
  } while (0)

static bmpc_obstacle_proposal proposal(double b0, double b1, double b2, const int32_t* script, int epochs, int epoch0) {
  bmpc_obstacle_proposal q = {};
  q.tilt[0] = b0, q.tilt[1] = b1, q.tilt[2] = b2, q.tilt[3] = 1.0;
  q.script = script, q.script_epochs = epochs, q.epoch0 = epoch0;
  return q;
}

int main() {
  const double mc[8] = {4.0, 2.5, 2.0, 3.0};
  const bmpc_policy pol[3] = {{BMPC_POL_MAINTAIN, 0, {0.1}}, {BMPC_POL_BRAKE, 0, {0.1}},
                              {BMPC_POL_LC, 0, {0, 5.4, 20, 0}}};
  const double x[4] = {0, 1.8, 20, 0}, z[4] = {5, 5.4, 20, 0};
  double w[3], sw = 0.0;
  op_weights(0, mc, 0.1, 6, 3, 1, pol, x, z, w);
  for (int j = 0; j < 3; ++j) sw += w[j];
  CHECK(w[0] > 0 && w[1] > 0 && w[2] > 0);

  // a tilt of ones is mode 1: the same choice at every ego and epoch, and exactly + 0.0
  const bmpc_obstacle_proposal ones = proposal(1, 1, 1, nullptr, 0, 0);
  for (int e = 0; e < 256; ++e) {
    const bmpc_obstacle_sampling S1 = {BMPC_OBS_SAMPLE_MODEL, 2, 7, 0}, S2 = {BMPC_OBS_SAMPLE_TILTED, 2, 7, 0};
    double lw = 0.0;
    const int a = env_sampled_choice<Highway>(S1, e, mc, 0.1, 6, 3, 2 * (e % 5), pol, x, z, 0.0);
    const int b = env_sampled_choice<Highway>(S2, e, mc, 0.1, 6, 3, 2 * (e % 5), pol, x, z, 0.0, &ones, &lw);
    CHECK(a == b);
    CHECK(lw == 0.0 && !signbit(lw));
  }

  // a tilted choice: the inverse CDF of w b at the draw, and + log(sum w b / (b_j sum w))
  const bmpc_obstacle_proposal tilt = proposal(1, 4, 0.25, nullptr, 0, 0);
  const double wb[3] = {w[0] * 1, w[1] * 4, w[2] * 0.25};
  const double swb = wb[0] + wb[1] + wb[2];
  int seen[3] = {0, 0, 0};
  for (int e = 0; e < 256; ++e) {
    const bmpc_obstacle_sampling S = {BMPC_OBS_SAMPLE_TILTED, 3, 11, 40};
    double lw = 0.5;
    const int j = env_sampled_choice<Highway>(S, e, mc, 0.1, 6, 3, 3, pol, x, z, 0.0, &tilt, &lw);
    CHECK(j == rng_inverse_cdf(wb, 3, obstacle_uniform(11, 40 + (uint64_t)e, 1)));
    CHECK(fabs(lw - (0.5 + log(swb / (tilt.tilt[j] * sw)))) < 1e-15);
    ++seen[j];
    // inside the epoch: the row's choice, clamped, and the weight untouched
    double lw2 = 0.75;
    CHECK(env_sampled_choice<Highway>(S, e, mc, 0.1, 6, 3, 4, pol, x, z, 9.0, &tilt, &lw2) == 2 && lw2 == 0.75);
  }
  CHECK(seen[0] > 0 && seen[1] > seen[0] && seen[1] > seen[2]);   // the brake is drawn most under b = (1, 4, 1/4)

  // a script, in a heap table of exactly batch x epochs entries (the sanitizer sees a read past it):
  // followed from its column t / hold - epoch0, entries clamped to a policy, + log p_j, no draw
  {
    const int batch = 3, epochs = 2, epoch0 = 3, hold = 2;
    std::vector<int32_t> table = {0, 1, 2, 9, -4, 1};
    const bmpc_obstacle_proposal q = proposal(1, 1, 1, table.data(), epochs, epoch0);
    const int want[3][2] = {{0, 1}, {2, 2}, {0, 1}};
    for (int e = 0; e < batch; ++e)
      for (int c = 0; c < epochs; ++c) {
        const int t = (epoch0 + c) * hold;
        double lw = -1.0, keep = 0.125;
        for (uint64_t seed = 0; seed < 3; ++seed) {   // (the seed is ignored)
          const bmpc_obstacle_sampling S = {BMPC_OBS_SCRIPT, hold, seed, 5};
          lw = -1.0;
          CHECK(env_sampled_choice<Highway>(S, e, mc, 0.1, 6, 3, t, pol, x, z, 0.0, &q, &lw) == want[e][c]);
          CHECK(fabs(lw - (-1.0 + log(w[want[e][c]] / sw))) < 1e-15);
          CHECK(env_sampled_choice<Highway>(S, e, mc, 0.1, 6, 3, t + 1, pol, x, z, 1.0, &q, &keep) == 1);
          CHECK(keep == 0.125);
        }
      }
    // an epoch outside the table (the entry points refuse it on the host) reads its nearest column
    const bmpc_obstacle_sampling S = {BMPC_OBS_SCRIPT, hold, 0, 0};
    double lw = 0.0;
    CHECK(env_sampled_choice<Highway>(S, 2, mc, 0.1, 6, 3, 0, pol, x, z, 0.0, &q, &lw) == 0);
    CHECK(env_sampled_choice<Highway>(S, 2, mc, 0.1, 6, 3, 40, pol, x, z, 0.0, &q, &lw) == 1);
    // the probabilities of the m prescribed choices sum to one
    double total = 0.0;
    for (int j = 0; j < 3; ++j) total += exp(log(w[j] / sw));
    CHECK(fabs(total - 1.0) < 1e-15);
  }

  // whole scene steps of both scenes, modes 2 and 3, three egos, six steps with hold 2
  {
    const int batch = 3, steps = 6, hold = 2;
    std::vector<int32_t> table = {0, 1, 2, 2, 1, 0, 1, 1, 1};
    const bmpc_obstacle_proposal q = proposal(1, 4, 0.25, table.data(), 3, 0);
    bmpc_env_desc E = {};
    E.n_lane = 4, E.L = 4.0, E.W = 2.5, E.Kpsi = 0.1, E.v0 = 20.0, E.vlen = 4.0, E.vwid = 2.4;
    E.target[0] = 0.5, E.target[1] = 1.8, E.target[2] = 15.0;
    const bmpc_quad_env_desc QE = {0.5, 5.0, 0.1};
    const double qmc[8] = {0.5, 0.3, 1.0, 0.6, 0.2, 2.0};
    const bmpc_policy qpol1[2] = {{BMPC_POL_FORWARD, 0, {0.2}}, {BMPC_POL_STOP, 0, {0}}};
    for (int mode = BMPC_OBS_SAMPLE_TILTED; mode <= BMPC_OBS_SCRIPT; ++mode) {
      const bmpc_obstacle_sampling S = {mode, hold, 3, 0};
      std::vector<double> scene(batch * ENV_STRIDE, 0.0), qscene(batch * ENV_STRIDE, 0.0);
      std::vector<bmpc_policy> p, qp;
      for (int e = 0; e < batch; ++e) {
        for (int i = 0; i < 4; ++i) scene[e * ENV_STRIDE + ENV_X + i] = x[i], scene[e * ENV_STRIDE + ENV_Z + i] = z[i];
        const double qs[12] = {0, 1.8, 0, 2.5, 2.5, -1.5707963267948966, 0, 0, 0, 5, -3, 0};
        for (int i = 0; i < 12; ++i) qscene[e * ENV_STRIDE + i] = qs[i];
        p.insert(p.end(), pol, pol + 3);
        qp.insert(qp.end(), qpol1, qpol1 + 2);
      }
      std::vector<double> xo(batch * 4), zo(batch * 4), xr(batch * 4), up(batch * 3, 0.05);
      for (int t = 0; t < steps; ++t) {
        CHECK(sh_env_step(&E, mc, 0.1, 6, 3, t, batch, scene.data(), p.data(), t ? up.data() : nullptr, 3, xo.data(),
                          zo.data(), xr.data(), &S, &q, nullptr, 0) == 0);
        CHECK(sh_quad_env_step(&QE, qmc, 0.2, 6, 2, t, batch, qscene.data(), qp.data(), t ? up.data() : nullptr, 3,
                               nullptr, nullptr, nullptr, xo.data(), zo.data(), xr.data(), nullptr, &S, &q, nullptr,
                               0) == 0);
        for (int e = 0; e < batch; ++e) {
          const double c = scene[e * ENV_STRIDE + ENV_OBSPOL], qc = qscene[e * ENV_STRIDE + ENV_OBSPOL];
          CHECK(c >= 0 && c <= 2 && qc >= 0 && qc <= 1);
          if (mode == BMPC_OBS_SCRIPT) {
            const int s = table[e * 3 + t / hold];
            CHECK(c == s && qc == (s > 1 ? 1 : s));
            CHECK(scene[e * ENV_STRIDE + ENV_LOGW] < 0.0 && qscene[e * ENV_STRIDE + ENV_LOGW] < 0.0);
          }
          CHECK(isfinite(scene[e * ENV_STRIDE + ENV_LOGW]) && isfinite(qscene[e * ENV_STRIDE + ENV_LOGW]));
          CHECK(scene[e * ENV_STRIDE + ENV_STEPS] == t + 1);
        }
      }
    }
    // the modes without a proposal never touch the slot
    const bmpc_obstacle_sampling S1 = {BMPC_OBS_SAMPLE_MODEL, 1, 3, 0};
    std::vector<double> scene(ENV_STRIDE, 0.0), xo(4), zo(4), xr(4);
    for (int i = 0; i < 4; ++i) scene[ENV_X + i] = x[i], scene[ENV_Z + i] = z[i];
    scene[ENV_LOGW] = -7777.25;
    bmpc_policy p1[3] = {pol[0], pol[1], pol[2]};
    CHECK(sh_env_step(&E, mc, 0.1, 6, 3, 0, 1, scene.data(), p1, nullptr, 0, xo.data(), zo.data(), xr.data(), &S1,
                      nullptr, nullptr, 0) == 0);
    CHECK(sh_env_step(&E, mc, 0.1, 6, 3, 0, 1, scene.data(), p1, nullptr, 0, xo.data(), zo.data(), xr.data(), nullptr,
                      &q, nullptr, 0) == 0);
    CHECK(scene[ENV_LOGW] == -7777.25);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
