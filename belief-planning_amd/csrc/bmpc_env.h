// bmpc_env.h -- the closed-loop highway overtake scene, one scene per ego.
//
// Restates Highway_env_branch.Highway_env.step (Highway_env_branch.py:83-184) and the
// collision rule of Highway_sim (:421-429) for the two-vehicle sim_overtake scene
// (:719-725); oracle/env.py is its CPU oracle.  One env_step_ego advances one ego's scene
// by one control step around the controller solve:
//   post(t-1): Euler step of the ego with uPred[0] of the last solve and of the obstacle with
//              the backup input chosen at t-1 (vehicle.step :39-41, used at :170-182);
//   collision: Highway_sim's sticky flag, tested before env.step(t) (:421-429);
//   pre(t):    the obstacle's backup choice -- argmax over the model's backup rollouts of the
//              clipped NumPy veh_col / lane_bdry_h safety value (:137-149) --, the lane
//              bookkeeping with the update_backup re-targeting of the lane-change policy
//              (:93-118), and the x_ref rule (:153-167): the inputs of the next solve.
// The obstacle's input uses the env's construction-time backup list (NumPy branches, :60,
// :149); the rollouts use the model's list as it was before this step's update (SX
// branches, zpred_eval at :95 precedes update_backup at :118).
#pragma once

#include "bmpc_model.h"
#include "bmpc_rng.h"

namespace bmpc {

// per-ego scene state (doubles), resident on the device between steps
enum {
  ENV_X = 0,        // ego state (X, Y, v, psi)
  ENV_Z = 4,        // obstacle state
  ENV_UOBS = 8,     // obstacle input chosen by pre(t), applied by post(t)
  ENV_LANE0 = 10,   // laneidx of the ego / of the obstacle (:96-101)
  ENV_LANE1 = 11,
  ENV_COLL = 12,    // Highway_sim collision flag (sticky)
  ENV_OBSPOL = 13,  // obstacle backup index chosen by the last pre()
  ENV_STEPS = 14,   // control steps taken
  ENV_LOGW = BMPC_ENV_LOGW,   // running log-weight of the weighted obstacle modes (also the quadruped scene's)
  ENV_STRIDE = BMPC_ENV_STRIDE
};

// per-ego closed-loop statistics (doubles, accumulated over the steps)
enum {
  ENVS_J = 0, ENVS_J2, ENVS_INFEAS, ENVS_ITERS, ENVS_SOLVES, ENVS_COLL_STEPS, ENVS_COLLIDED,
  ENVS_STRIDE = BMPC_ENV_NSTAT
};

// NumPy veh_col (highway_branch_dyn.py:243-254): rows clipped to +-5, alpha = 1
BMPC_HD double env_veh_col(double a0, double a1, double b0, double b1, double s0, double s1) {
  const double dx = fmin(fmax(fabs(a0 - b0) - s0, -5.0), 5.0);
  const double dy = fmin(fmax(fabs(a1 - b1) - s1, -5.0), 5.0);
  const double ex = exp(dx), ey = exp(dy);
  return (dx * ex + dy * ey) / (ex + ey);
}

// NumPy lane_bdry_h (highway_branch_dyn.py:195-214): softmin_5([y - lb, ub - y])
BMPC_HD double env_lane_bdry(double y, double lb, double ub) {
  const double a = y - lb, b = ub - y;
  const double ea = exp(-5.0 * a), eb = exp(-5.0 * b);
  return (ea * a + eb * b) / (ea + eb);
}

// NumPy branches of the env's backup list (highway_branch_dyn.py:67, :121, :148)
BMPC_HD void env_policy_u(int kind, const double* x, double Kpsi, const double* target, double* u) {
  if (kind == 0) {
    u[0] = 0.0;
    u[1] = -Kpsi * x[3];
  } else if (kind == 1) {   // softmax([-5, -v], 3)
    const double a = -5.0, b = -x[2];
    const double ea = exp(3.0 * a), eb = exp(3.0 * b);
    u[0] = (ea * a + eb * b) / (ea + eb);
    u[1] = -Kpsi * x[3];
  } else {
    u[0] = -0.8558 * (x[2] - target[2]);
    u[1] = -0.3162 * (x[1] - target[1]) - 3.9889 * (x[3] - target[3]);
  }
}

// The sampled backup choice of step t (bmpc_set_obstacle_sampling, BMPC_OBS_SAMPLE_MODEL) of the
// plan's ego e at the pre-step state (x, z): at an epoch start, t % hold == 0, the inverse CDF of
// the model's own branch distribution -- branch_eval's p_j = prob_weight(bf_traj_j) / sum, in plain
// doubles, no Jacobian -- at the draw of (seed, ego_base + e, t / hold); otherwise `prev`, the scene
// row's choice of the step before (clamped to a policy: a sampler attached mid-episode, or a row
// the caller wrote, keeps it until the next epoch boundary).  mc: the plan's model constants.
//
// The weighted modes (bmpc_set_obstacle_proposal; Q the plan's proposal, logw the scene row's
// ENV_LOGW slot) choose at the same epoch starts from the same weights w_j and add the log-weight of
// their choice to *logw; inside an epoch they too return `prev` and leave *logw alone.
//   BMPC_OBS_SAMPLE_TILTED: the inverse CDF of w_j b_j (b = Q->tilt) at the same draw, and
//     log((sum w_k b_k) / (b_j sum w_k)) = log(p_j / q_j) -- with b == 1 the products are the w_j
//     themselves, so the choice is the untilted one and the quotient is exactly 1: + 0.0;
//   BMPC_OBS_SCRIPT: Q->script[e][t / hold - epoch0] clamped to a policy, no draw, and
//     log(w_j / sum w_k) = log p_j.  (The entry points check on the host that the script covers
//     the epochs of their steps; the column is clamped here all the same, so that a table is never
//     read outside its rows.)
// All sums run in the order k = 0, 1, ...
template <class M>
BMPC_HD int env_sampled_choice(const bmpc_obstacle_sampling& S, long long e, const double* mc, double dt, int N,
                               int m, int t, const bmpc_policy* pol, const double* x, const double* z, double prev,
                               const bmpc_obstacle_proposal* Q = nullptr, double* logw = nullptr) {
  if (t % S.hold != 0) return prev >= (double)(m - 1) ? m - 1 : prev > 0.0 ? (int)prev : 0;
  double w[BMPC_MAX_M];
  for (int j = 0; j < m; ++j) w[j] = M::prob_weight(mc, M::bf_traj(mc, dt, N, pol[0], pol[j], x, z));
  if (S.mode == BMPC_OBS_SCRIPT) {
    int c = t / S.hold - Q->epoch0;
    c = c >= Q->script_epochs ? Q->script_epochs - 1 : c > 0 ? c : 0;
    int j = Q->script[(size_t)e * (size_t)Q->script_epochs + (size_t)c];
    j = j >= m - 1 ? m - 1 : j > 0 ? j : 0;
    double sw = 0.0;
    for (int k = 0; k < m; ++k) sw += w[k];
    *logw += log(w[j] / sw);
    return j;
  }
  const double u = obstacle_uniform(S.seed, (uint64_t)(S.ego_base + e), (uint32_t)(t / S.hold));
  if (S.mode != BMPC_OBS_SAMPLE_TILTED) return rng_inverse_cdf(w, m, u);
  double wb[BMPC_MAX_M], sw = 0.0, swb = 0.0;
  {
#pragma clang fp contract(off)   // (w_k b_k rounded before it is added, in every kernel that inlines this)
    for (int k = 0; k < m; ++k) wb[k] = w[k] * Q->tilt[k];
    for (int k = 0; k < m; ++k) sw += w[k], swb += wb[k];
  }
  const int j = rng_inverse_cdf(wb, m, u);
  *logw += log(swb / (Q->tilt[j] * sw));
  return j;
}
BMPC_HD bool env_samples(const bmpc_obstacle_sampling* smp) { return smp && smp->mode != BMPC_OBS_ARGMAX; }

// What a plan has attached to its scenes beyond the sampler, as one device block behind one pointer
// (null: nothing attached): the obstacle proposal (bmpc_set_obstacle_proposal; read only in the
// sampler modes that need one, which the host admits only while one is attached) followed by the
// actuation disturbance (bmpc_set_disturbance; law BMPC_DISTURB_NONE while none is attached) and the
// observation model (bmpc_set_observation; law BMPC_OBSERVE_NONE while none is attached).
struct SceneOptions {
  bmpc_obstacle_proposal prop;
  bmpc_disturbance dist;
  bmpc_observation obs;
};
BMPC_HD const bmpc_obstacle_proposal* scene_prop(const SceneOptions* o) { return o ? &o->prop : nullptr; }
BMPC_HD const bmpc_disturbance* scene_dist(const SceneOptions* o) { return o ? &o->dist : nullptr; }
BMPC_HD const bmpc_observation* scene_obs(const SceneOptions* o) { return o ? &o->obs : nullptr; }

// One scene step of one ego (see the header comment).  st: ENV_STRIDE doubles; pol: the
// ego's m model policies (the lane-change target is re-targeted in place, update_backup);
// u0: uPred[0] of the last solve (unused at t == 0); x_out, z_out, xref_out: the next
// solve's inputs.  smp: the plan's obstacle sampler or null (null and mode BMPC_OBS_ARGMAX are the
// reference's argmax rule), with mc, the plan's model constants, and e, the ego's index in the plan;
// prop: the plan's obstacle proposal (read in modes BMPC_OBS_SAMPLE_TILTED and BMPC_OBS_SCRIPT only);
// dist: the plan's actuation disturbance or null (bmpc_set_disturbance: the inputs post(t-1) applies,
// rng_disturb_input; the row's ENV_UOBS keeps the nominal input); obs: the plan's observation model or
// null (bmpc_set_observation: x_out and z_out only, rng_observe_state at step t; the row, the choice,
// the bookkeeping and xref_out stay on the true states).
BMPC_HD void env_step_ego(const bmpc_env_desc& E, double dt, int N, int m, int t, double* st,
                          bmpc_policy* pol, const double* u0, double* x_out, double* z_out,
                          double* xref_out, const bmpc_obstacle_sampling* smp = nullptr,
                          const double* mc = nullptr, long long e = 0,
                          const bmpc_obstacle_proposal* prop = nullptr,
                          const bmpc_disturbance* dist = nullptr, const bmpc_observation* obs = nullptr) {
  double* x = st + ENV_X;
  double* z = st + ENV_Z;
  if (t > 0) {   // post(t-1): vehicle.step of ego and obstacle
    double xp[4], zp[4], ue[2], uo[2];
    rng_disturb_input(dist, true, e, t - 1, 2, u0, ue);
    rng_disturb_input(dist, false, e, t - 1, 2, st + ENV_UOBS, uo);
    step<Highway>(dt, x, ue, xp);
    step<Highway>(dt, z, uo, zp);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = xp[i], z[i] = zp[i];
  }
  if (st[ENV_COLL] == 0.0) {   // Highway_sim, before env.step(t)
    const double dis = fmax(fabs(x[0] - z[0]) - E.vlen, fabs(x[1] - z[1]) - E.vwid);
    if (dis < 0.0) st[ENV_COLL] = 1.0;
  }
  int best = 0;
  if (env_samples(smp)) {   // (the policies in force before this step's re-targeting below)
    best = env_sampled_choice<Highway>(*smp, e, mc, dt, N, m, t, pol, x, z, st[ENV_OBSPOL], prop, st + ENV_LOGW);
  } else {
    // safety value of every obstacle backup against the ego's backup-0 rollout (the ego's
    // backupidx is never changed): min over the rows of veh_col and lane_bdry_h of the ego
    const double s0 = E.L + 1.0, s1 = E.W + 0.2;
    const double lb = E.W / 2.0, ub = E.n_lane * 3.6 - E.W / 2.0;
    double hi[BMPC_MAX_M], zo[BMPC_MAX_M][4], xe[4];
    double lane_min = 1e300;
#pragma unroll
    for (int i = 0; i < 4; ++i) xe[i] = x[i];
    for (int j = 0; j < m; ++j) {
      hi[j] = 1e300;
#pragma unroll
      for (int i = 0; i < 4; ++i) zo[j][i] = z[i];
    }
    for (int k = 0; k < N; ++k) {
      double ue[2], fe[4];
      Highway::policy(pol[0], xe, ue);
      Highway::f(xe, ue, fe);
#pragma unroll
      for (int i = 0; i < 4; ++i) xe[i] = xe[i] + fe[i] * dt;
      lane_min = fmin(lane_min, env_lane_bdry(xe[1], lb, ub));
      for (int j = 0; j < m; ++j) {
        double uo[2], fo[4];
        Highway::policy(pol[j], zo[j], uo);
        Highway::f(zo[j], uo, fo);
#pragma unroll
        for (int i = 0; i < 4; ++i) zo[j][i] = zo[j][i] + fo[i] * dt;
        hi[j] = fmin(hi[j], env_veh_col(xe[0], xe[1], zo[j][0], zo[j][1], s0, s1));
      }
    }
    for (int j = 0; j < m; ++j) {
      hi[j] = fmin(hi[j], lane_min);
      if (hi[j] > hi[best]) best = j;   // np.argmax: the first maximum
    }
  }
  // lane bookkeeping (Python round = half to even = rint) and update_backup re-targeting
  for (int i = 0; i < 2; ++i) {
    const double* v = i == 0 ? x : z;
    const double nl = rint((v[1] - 1.8) / 3.6);
    double& lane = st[ENV_LANE0 + i];
    if (t == 0 || (nl != lane && fabs(v[1] - 1.8 - 3.6 * nl) < 1.4)) {
      lane = nl;
      if (i == 1) {
        const double l0 = st[ENV_LANE0], l1 = st[ENV_LANE1];
        const double tl = l0 < l1 ? l1 - 1.0 : l0 > l1 ? l1 + 1.0 : l1 > 0.0 ? l1 - 1.0 : l1 + 1.0;
        for (int j = 0; j < m; ++j)
          if (pol[j].kind == BMPC_POL_LC) {
            pol[j].p[0] = 0.0;
            pol[j].p[1] = 1.8 + 3.6 * tl;
            pol[j].p[2] = E.v0;
            pol[j].p[3] = 0.0;
          }
      }
    }
  }
  st[ENV_OBSPOL] = (double)best;
  env_policy_u(best, z, E.Kpsi, E.target, st + ENV_UOBS);
  // x_ref rule (:153-167)
  const double Ydes = x[0] < z[0] ? 1.8 + st[ENV_LANE0] * 3.6 : z[1];
  const double vdes = (fabs(x[1] - Ydes) < 1.0 && x[0] > z[0] + 3.0) ? E.v0 : z[2] + (z[0] + 1.5 - x[0]);
  rng_observe_state(obs, true, e, t, 4, x, x_out);
  rng_observe_state(obs, false, e, t, 4, z, z_out);
  xref_out[0] = 0.0;
  xref_out[1] = Ydes;
  xref_out[2] = vdes;
  xref_out[3] = 0.0;
  st[ENV_STEPS] += 1.0;
}

// statistics of the last solve and of the scene (bench / closed-loop summaries)
BMPC_HD void env_accumulate(const double* st, double J, int status, int iters, bool cvar, double* acc) {
  acc[ENVS_J] += J;
  acc[ENVS_J2] += J * J;
  acc[ENVS_INFEAS] += (cvar ? status < 0 : status != 1) ? 1.0 : 0.0;
  acc[ENVS_ITERS] += (double)iters;
  acc[ENVS_SOLVES] += 1.0;
  acc[ENVS_COLL_STEPS] += st[ENV_COLL];
  acc[ENVS_COLLIDED] = st[ENV_COLL];
}

}  // namespace bmpc
