// merge_env_host.cpp -- TEST-ONLY host build of the merge scene step (csrc/bmpc_env_merge.h).
//
// Compiles the per-ego scene function the kernels call (k_env_merge, the merge k_loop) with g++,
// so the CPU tests can drive it against the reference's recording.  Exports its own `ms_*`
// symbol; never loaded by the belief-planning_amd package.
#include "bmpc_env_merge.h"

using namespace bmpc;

extern "C" {

// One scene step of `batch` egos, as k_env_merge runs it: the statistics of the last solve (t > 0,
// all of J / status / iters / stats given), then the scene step.  ref = grid | refY | refpsi;
// S [batch][16] and bx [batch][nbx] stand in for the egos' transform slots.
int ms_env_step(const bmpc_merge_env_desc* env, int nref, const double* ref, const double* bx_plan, int nbx, double dt,
                int t, int batch, double* scene, const double* upred, int upred_stride, const double* J,
                const int32_t* status, const int32_t* iters, double* x, double* z, double* xref, double* S, double* bx,
                double* stats) {
  const MergeRef R{ref, nref};
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    if (t > 0 && stats && J && status && iters)
      env_accumulate(st, J[e], status[e], iters[e], true, stats + (size_t)e * ENVS_STRIDE);
    merge_env_step_ego(*env, R, bx_plan, nbx, dt, t, st, upred ? upred + (size_t)e * upred_stride : nullptr,
                       x + (size_t)e * 4, z + (size_t)e * 4, xref + (size_t)e * 4, S + (size_t)e * 16,
                       bx + (size_t)e * nbx);
  }
  return 0;
}

}  // extern "C"
