// bmpc_k_highway_qp_loop.hip -- the fused closed loop of the overtake scene under BranchMPC and robustMPC (bmpc_loop_device): k_loop of the highway model with the overtake scene step and the QP solver.
#include "bmpc_dev.h"

namespace bmpc {
namespace dev {

hipError_t launch_loop_highway_qp(const SolveLaunch& a, const bmpc_env_desc& env, int t0, int nsteps, double* scene,
                                  double* stats) {
  return launch_loop<Highway>(a, OvertakeQpScene{env, a.smp, a.opt}, t0, nsteps, scene, stats);
}

}  // namespace dev
}  // namespace bmpc
