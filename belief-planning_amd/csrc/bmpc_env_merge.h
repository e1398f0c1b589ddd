// bmpc_env_merge.h -- the closed-loop merge scene, one scene per ego.
//
// Restates Highway_env_branch.Highway_env_merge.step (Highway_env_branch.py:317-380) and the
// collision rule of Highway_sim (:421-429) for the two-vehicle sim_merge scene (the ego on the
// ramp, the obstacle on the main road).  One merge_env_step_ego advances one ego's scene by one
// control step around the controller solve:
//   post(t-1): Euler step of the ego with uPred[0] of the last solve and of the obstacle with
//              the input chosen at t-1 (vehicle.step :39-41, used at :370-377);
//   collision: Highway_sim's sticky flag, tested before env.step(t) (:421-429);
//   pre(t):    the lane flag -- a vehicle past merge_s + 8 has left the ramp for good (:328-329);
//              the obstacle's input -- the reference overwrites its argmax with backup 0 (:345-347),
//              so it is always backup 0 of the main-road list, the NumPy branch of
//              backup_maintain_trackV (highway_branch_dyn.py:80-96), and no rollout is needed --;
//              and the S / x_ref / bx the scene passes to the solve (:350-361).
// The scene state reuses the slots of bmpc_env.h; ENV_LANE0 holds "the ego has merged" (0 on the
// ramp), so a zero-initialised scene with x and z written is the reference's laneID = [1, 0].
// The obstacle starts on the main road and can only stay there (ENV_LANE1 is unused).
#pragma once

#include "bmpc_env.h"

namespace bmpc {

enum { ENV_MERGED = ENV_LANE0 };

// the scene's lane references refY(X), refpsi(X): linear interpolants on one shared grid
// (Highway_env_branch.py:308-309); tab = grid | refY | refpsi, n points each
struct MergeRef {
  const double* tab;
  int n;
};

// One scene step of one ego (see the header comment).  st: ENV_STRIDE doubles; bx_plan: the
// plan's state bound (mpc.param.bx, nbx entries); u0: uPred[0] of the last solve (unused at
// t == 0); x_out, z_out, xref_out: the next solve's inputs; S_out [4][4] and bx_out [nbx]: the
// solve's state transformation and state bound (nbx >= 4 on the ramp's rule).  dist: the plan's
// actuation disturbance or null (bmpc_set_disturbance, as in env_step_ego), with e, the ego's index
// in the plan; obs: the plan's observation model or null (bmpc_set_observation: x_out and z_out only;
// xref_out, S_out and bx_out are those of the true state).
BMPC_HD void merge_env_step_ego(const bmpc_merge_env_desc& E, const MergeRef& R, const double* bx_plan, int nbx,
                                double dt, int t, double* st, const double* u0, double* x_out, double* z_out,
                                double* xref_out, double* S_out, double* bx_out,
                                const bmpc_disturbance* dist = nullptr, long long e = 0,
                                const bmpc_observation* obs = nullptr) {
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
  if (x[0] > E.merge_s + 8.0) st[ENV_MERGED] = 1.0;
  // obstacle: backup 0 of the main-road list, u = [0.5 (v0 - v), -Kpsi psi]
  st[ENV_OBSPOL] = 0.0;
  st[ENV_UOBS] = 0.5 * (E.v0 - z[2]);
  st[ENV_UOBS + 1] = -E.Kpsi * z[3];
#pragma unroll
  for (int i = 0; i < 16; ++i) S_out[i] = (i % 5 == 0) ? 1.0 : 0.0;
  if (st[ENV_MERGED] != 0.0) {   // main road: S = I (on), the last lane's centre, the plan's bound
    xref_out[0] = 0.0;
    xref_out[1] = (E.n_lane - 0.5) * 3.6;
    xref_out[2] = E.v0;
    xref_out[3] = 0.0;
    for (int i = 0; i < nbx; ++i) bx_out[i] = bx_plan[i];
  } else {   // ramp: the tangent transformation and bounds of the lane reference at X
    const LaneRef RY{R.tab, R.tab + R.n, R.n}, RP{R.tab, R.tab + 2 * R.n, R.n};
    const double y0 = lref_eval(RY, x[0]), psi0 = lref_eval(RP, x[0]);
    const double tn = tan(psi0);
    S_out[4] = -tn;
    xref_out[0] = 0.0;
    xref_out[1] = -tn * x[0] + y0 + 1.8;
    xref_out[2] = E.v0;
    xref_out[3] = psi0;
    for (int i = 4; i < nbx; ++i) bx_out[i] = bx_plan[i];
    bx_out[0] = -tn * x[0] + y0 + 3.6 * E.merge_lane - E.W / 2.0;
    bx_out[1] = tn * x[0] - y0 - E.W / 2.0;
    bx_out[2] = psi0 + E.psimax;
    bx_out[3] = -psi0 + E.psimax;
  }
  rng_observe_state(obs, true, e, t, 4, x, x_out);
  rng_observe_state(obs, false, e, t, 4, z, z_out);
  st[ENV_STEPS] += 1.0;
}

}  // namespace bmpc
