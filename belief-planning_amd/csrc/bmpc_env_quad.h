// bmpc_env_quad.h -- the closed-loop quadruped scene, one scene per ego.
//
// Restates quadruped_env.Quad_env.step (quadruped_env.py:67-130; the package's quadruped_env.py
// :44-104 is its host restatement) for the two-robot scene of main_quadruped (the controlled ego
// and one obstacle).  One quad_env_step_ego advances one ego's scene by one control step around
// the controller solve:
//   post(t-1): Euler step of the ego with uPred[0] of the last solve and of the obstacle with
//              the backup input chosen at t-1 (robot.step :34-37, used at :121-127);
//   pre(t):    the obstacle's backup choice -- the ego rolled forward under policy 0 (x1), the
//              obstacle under every policy (zpred_eval :82-84), hi[j] the minimum over the horizon
//              of the NumPy robot_col clearance (quadruped_branch_dyn.py:147-150, Euclidean), policy
//              0 while hi[0] > switch_clearance, else np.argmax(hi) (:92-101) --, its input (the
//              NumPy branch of the backup, :103), and the x_ref rule towards the ego's x_des
//              (:107-118): the inputs of the next solve.
// The reference has no collision rule for this scene (Robot_sim sets `collision = False` and never
// tests it), so ENV_COLL stays 0 and the statistics' collision columns stay 0.
// The scene state reuses bmpc_env.h's stride and its ENV_COLL / ENV_OBSPOL / ENV_STEPS slots; the
// three-component states move the rest: x 0-2, z 3-5, the obstacle's input 6-8, x_des 9-11.
#pragma once

#include "bmpc_env.h"

namespace bmpc {

enum {
  QENV_X = 0,      // ego state (X, Y, theta)
  QENV_Z = 3,      // obstacle state
  QENV_UOBS = 6,   // obstacle input chosen by pre(t), applied by post(t)
  QENV_XDES = 9    // the ego's goal x_des (written by the caller, never by the scene)
};
static_assert(QENV_XDES + 3 <= ENV_COLL, "the quadruped slots end before the shared ones");

// NumPy robot_col (quadruped_branch_dyn.py:147-150), one row: ||a - b||_2 - (L1 + L2) / 2 - tol.
// Quadruped::robot_col is the SX branch (the 1-norm) the controller's rows use; the scene calls
// the function with arrays and so takes this one.  mc = L1 W1 L2 W2 tol s1.
BMPC_HD double quad_env_robot_col(const double* mc, double a0, double a1, double b0, double b1) {
  const double dx = a0 - b0, dy = a1 - b1;
  return sqrt(dx * dx + dy * dy) - (mc[0] + mc[2]) / 2.0 - mc[4];
}

// One scene step of one ego (see the header comment).  st: ENV_STRIDE doubles; mc: the plan's
// model constants; pol: the ego's m model policies; u0: uPred[0] of the last solve (unused at
// t == 0); x_out, z_out, xref_out: the next solve's inputs (3 doubles each).  smp: the plan's
// obstacle sampler or null (null and mode BMPC_OBS_ARGMAX are the reference's rule); e: the ego's
// index in the plan; prop: the plan's obstacle proposal (the weighted modes, bmpc_env.h); dist: the
// plan's actuation disturbance or null (bmpc_set_disturbance, as in env_step_ego); obs: the plan's
// observation model or null (bmpc_set_observation: x_out and z_out only; xref_out is the true state's).
BMPC_HD void quad_env_step_ego(const bmpc_quad_env_desc& E, const double* mc, double dt, int N, int m, int t,
                               double* st, const bmpc_policy* pol, const double* u0, double* x_out, double* z_out,
                               double* xref_out, const bmpc_obstacle_sampling* smp = nullptr, long long e = 0,
                               const bmpc_obstacle_proposal* prop = nullptr,
                               const bmpc_disturbance* dist = nullptr, const bmpc_observation* obs = nullptr) {
  double* x = st + QENV_X;
  double* z = st + QENV_Z;
  if (t > 0) {   // post(t-1): robot.step of ego and obstacle
    double xp[3], zp[3], ue[3], uo[3];
    rng_disturb_input(dist, true, e, t - 1, 3, u0, ue);
    rng_disturb_input(dist, false, e, t - 1, 3, st + QENV_UOBS, uo);
    step<Quadruped>(dt, x, ue, xp);
    step<Quadruped>(dt, z, uo, zp);
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = xp[i], z[i] = zp[i];
  }
  int best = 0;
  if (env_samples(smp)) {
    best = env_sampled_choice<Quadruped>(*smp, e, mc, dt, N, m, t, pol, x, z, st[ENV_OBSPOL], prop, st + ENV_LOGW);
  } else {
    // clearance of every obstacle backup against the ego's policy-0 rollout (the ego's backupidx
    // is never changed): the rollouts of zpred_eval, row by row (rollout<> of one step, in place)
    double hi[BMPC_MAX_M], zo[BMPC_MAX_M][3], xe[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) xe[i] = x[i];
    for (int j = 0; j < m; ++j) {
      hi[j] = 1e300;
#pragma unroll
      for (int i = 0; i < 3; ++i) zo[j][i] = z[i];
    }
    for (int k = 0; k < N; ++k) {
      rollout<Quadruped>(dt, 1, pol[0], xe, xe, 3);
      for (int j = 0; j < m; ++j) {
        rollout<Quadruped>(dt, 1, pol[j], zo[j], zo[j], 3);
        hi[j] = fmin(hi[j], quad_env_robot_col(mc, xe[0], xe[1], zo[j][0], zo[j][1]));
      }
    }
    if (!(hi[0] > E.switch_clearance))
      for (int j = 1; j < m; ++j)
        if (hi[j] > hi[best]) best = j;   // np.argmax: the first maximum
  }
  st[ENV_OBSPOL] = (double)best;
  Quadruped::policy(pol[best], z, st + QENV_UOBS);
  // x_ref rule (:107-118): `lookahead` metres towards x_des; the heading along the way, wrapped
  // towards x_des[2], or the ego's own within `near` of the goal
  const double* xd = st + QENV_XDES;
  double d0 = xd[0] - x[0], d1 = xd[1] - x[1];
  const double nrm = sqrt(d0 * d0 + d1 * d1);
  const double len = fmin(nrm, E.lookahead);
  d0 = d0 / nrm * len;
  d1 = d1 / nrm * len;
  double psi = x[2];
  if (sqrt(d0 * d0 + d1 * d1) > E.near) {
    const double pi = 3.141592653589793;
    psi = atan2(d1, d0);
    // the reference's two while loops; atan2 is within pi of 0, so they turn |x_des[2]| / 2 pi
    // times -- the count is capped so that a goal heading left uninitialised cannot hang a wave
    for (int i = 0; i < 64 && psi - xd[2] > pi; ++i) psi -= 2.0 * pi;
    for (int i = 0; i < 64 && psi - xd[2] < -pi; ++i) psi += 2.0 * pi;
  }
  rng_observe_state(obs, true, e, t, 3, x, x_out);
  rng_observe_state(obs, false, e, t, 3, z, z_out);
  xref_out[0] = x[0] + d0;
  xref_out[1] = x[1] + d1;
  xref_out[2] = psi;
  st[ENV_STEPS] += 1.0;
}

}  // namespace bmpc
