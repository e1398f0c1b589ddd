// scene_host.h -- TEST-ONLY host build of the three scene steps (csrc/bmpc_env.h, bmpc_env_merge.h,
// bmpc_env_quad.h): one wrapper per scene that runs the per-ego scene function the kernels call
// (k_env / k_env_merge / k_env_quad and the k_loops) over a batch, with every argument the kernels
// pass -- the obstacle's sampler and proposal, the disturbance, upred_stride.
//
// arglist selects the scene function's argument list, so that a test can compare a null option with
// the list the function had before that option existed:
//   0  every argument;
//   1  the list before the disturbance        (overtake / quadruped: smp, prop; merge: none of them);
//   2  the list before the proposal           (smp only);
//   3  the list before the sampler            (the scene function's required arguments alone).
// Included by tests/hostsim/scene_host.cpp (the shared library libbmpc_hostsim_scene.so) and by the
// stand-alone sanitizer programs whose main() calls a wrapper.  Never loaded by the package.
#pragma once

#include "bmpc_env_merge.h"
#include "bmpc_env_quad.h"

extern "C" {

// One overtake scene step of `batch` egos as k_env runs it (no statistics: hostsim.cpp's hs_env_step
// has them).  pol [batch][m]; upred [batch][upred_stride], its first two doubles uPred[0].
int sh_env_step(const bmpc_env_desc* env, const double* mc, double dt, int N, int m, int t, int batch, double* scene,
                bmpc_policy* pol, const double* upred, int upred_stride, double* x, double* z, double* xref,
                const bmpc_obstacle_sampling* smp, const bmpc_obstacle_proposal* prop, const bmpc_disturbance* dist,
                int arglist) {
  using namespace bmpc;
  if (m < 1 || m > BMPC_MAX_M) return -22;
  if (arglist < 2 && smp && smp->mode >= BMPC_OBS_SAMPLE_TILTED && !prop) return -22;
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    bmpc_policy* p = pol + (size_t)e * m;
    const double* u0 = upred ? upred + (size_t)e * upred_stride : nullptr;
    double *xe = x + (size_t)e * 4, *ze = z + (size_t)e * 4, *re = xref + (size_t)e * 4;
    if (arglist == 3)
      env_step_ego(*env, dt, N, m, t, st, p, u0, xe, ze, re);
    else if (arglist == 2)
      env_step_ego(*env, dt, N, m, t, st, p, u0, xe, ze, re, smp, mc, e);
    else if (arglist == 1)
      env_step_ego(*env, dt, N, m, t, st, p, u0, xe, ze, re, smp, mc, e, prop);
    else
      env_step_ego(*env, dt, N, m, t, st, p, u0, xe, ze, re, smp, mc, e, prop, dist);
  }
  return 0;
}

// One merge scene step, as k_env_merge runs it: the statistics of the last solve (t > 0, all of J /
// status / iters / stats given), then the scene step.  ref = grid | refY | refpsi; S [batch][16] and
// bx [batch][nbx] stand in for the egos' transform slots.  arglist: 0, or 1 (before the disturbance).
int sh_merge_env_step(const bmpc_merge_env_desc* env, int nref, const double* ref, const double* bx_plan, int nbx,
                      double dt, int t, int batch, double* scene, const double* upred, int upred_stride, const double* J,
                      const int32_t* status, const int32_t* iters, double* x, double* z, double* xref, double* S,
                      double* bx, double* stats, const bmpc_disturbance* dist, int arglist) {
  using namespace bmpc;
  const MergeRef R{ref, nref};
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    const double* u0 = upred ? upred + (size_t)e * upred_stride : nullptr;
    double *xe = x + (size_t)e * 4, *ze = z + (size_t)e * 4, *re = xref + (size_t)e * 4;
    if (t > 0 && stats && J && status && iters)
      env_accumulate(st, J[e], status[e], iters[e], true, stats + (size_t)e * ENVS_STRIDE);
    if (arglist)
      merge_env_step_ego(*env, R, bx_plan, nbx, dt, t, st, u0, xe, ze, re, S + (size_t)e * 16, bx + (size_t)e * nbx);
    else
      merge_env_step_ego(*env, R, bx_plan, nbx, dt, t, st, u0, xe, ze, re, S + (size_t)e * 16, bx + (size_t)e * nbx,
                         dist, e);
  }
  return 0;
}

// One quadruped scene step, as k_env_quad runs it: the statistics of the last solve (an OSQP-class
// controller's status), then the scene step.  upred's first three doubles per ego are uPred[0].
int sh_quad_env_step(const bmpc_quad_env_desc* env, const double* mc, double dt, int N, int m, int t, int batch,
                     double* scene, const bmpc_policy* pol, const double* upred, int upred_stride, const double* J,
                     const int32_t* status, const int32_t* iters, double* x, double* z, double* xref, double* stats,
                     const bmpc_obstacle_sampling* smp, const bmpc_obstacle_proposal* prop,
                     const bmpc_disturbance* dist, int arglist) {
  using namespace bmpc;
  if (m < 1 || m > BMPC_MAX_M) return -22;
  if (arglist < 2 && smp && smp->mode >= BMPC_OBS_SAMPLE_TILTED && !prop) return -22;
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    const bmpc_policy* p = pol + (size_t)e * m;
    const double* u0 = upred ? upred + (size_t)e * upred_stride : nullptr;
    double *xe = x + (size_t)e * 3, *ze = z + (size_t)e * 3, *re = xref + (size_t)e * 3;
    if (t > 0 && stats && J && status && iters)
      env_accumulate(st, J[e], status[e], iters[e], false, stats + (size_t)e * ENVS_STRIDE);
    if (arglist == 3)
      quad_env_step_ego(*env, mc, dt, N, m, t, st, p, u0, xe, ze, re);
    else if (arglist == 2)
      quad_env_step_ego(*env, mc, dt, N, m, t, st, p, u0, xe, ze, re, smp, e);
    else if (arglist == 1)
      quad_env_step_ego(*env, mc, dt, N, m, t, st, p, u0, xe, ze, re, smp, e, prop);
    else
      quad_env_step_ego(*env, mc, dt, N, m, t, st, p, u0, xe, ze, re, smp, e, prop, dist);
  }
  return 0;
}

// the model weights w [batch][m] the obstacle's rule forms at the states x, z [batch][n] under pol [batch][m]
void op_weights(int quadruped, const double* mc, double dt, int N, int m, int batch, const bmpc_policy* pol,
                const double* x, const double* z, double* w) {
  using namespace bmpc;
  const int n = quadruped ? 3 : 4;
  for (int e = 0; e < batch; ++e)
    for (int j = 0; j < m; ++j) {
      const bmpc_policy* p = pol + (size_t)e * m;
      const double *xe = x + (size_t)e * n, *ze = z + (size_t)e * n;
      w[(size_t)e * m + j] = quadruped ? Quadruped::prob_weight(mc, Quadruped::bf_traj(mc, dt, N, p[0], p[j], xe, ze))
                                       : Highway::prob_weight(mc, Highway::bf_traj(mc, dt, N, p[0], p[j], xe, ze));
    }
}

}  // extern "C"
