// bmpc_k_merge_loop.hip -- the fused closed loop of the merge scene (bmpc_merge_loop_device): k_loop of the merge-scene model with the merge scene step.
#include "bmpc_dev.h"

namespace bmpc {
namespace dev {

hipError_t launch_loop_merge(const SolveLaunch& a, const bmpc_merge_env_desc& env, const MergeRef& ref, int t0,
                             int nsteps, double* scene, double* stats) {
  return launch_loop<HighwayMerge>(a, MergeScene{env, ref, a.opt}, t0, nsteps, scene, stats);
}

}  // namespace dev
}  // namespace bmpc
