// bmpc_k_quad_loop.hip -- the fused closed loop of the quadruped scene (bmpc_quad_loop_device): k_loop of the quadruped model with the quadruped scene step and the QP solver.
#include "bmpc_dev.h"

namespace bmpc {
namespace dev {

hipError_t launch_loop_quad(const SolveLaunch& a, const bmpc_quad_env_desc& env, int t0, int nsteps, double* scene,
                            double* stats) {
  return launch_loop<Quadruped>(a, QuadScene{env, a.smp, a.opt}, t0, nsteps, scene, stats);
}

}  // namespace dev
}  // namespace bmpc
