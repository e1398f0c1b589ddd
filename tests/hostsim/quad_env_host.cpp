// quad_env_host.cpp -- TEST-ONLY host build of the quadruped scene step (csrc/bmpc_env_quad.h).
//
// Compiles the per-ego scene function the kernels call (k_env_quad, the quadruped k_loop) with
// g++, so the CPU tests can drive it against the reference's recording.  Exports its own `qs_*`
// symbol; never loaded by the belief-planning_amd package.
#include "bmpc_env_quad.h"

using namespace bmpc;

extern "C" {

// One scene step of `batch` egos, as k_env_quad runs it: the statistics of the last solve (t > 0,
// all of J / status / iters / stats given; an OSQP-class controller's status), then the scene step.
// pol [batch][m]; upred [batch][upred_stride], its first three doubles uPred[0].
int qs_env_step(const bmpc_quad_env_desc* env, const double* mc, double dt, int N, int m, int t, int batch,
                double* scene, const bmpc_policy* pol, const double* upred, int upred_stride, const double* J,
                const int32_t* status, const int32_t* iters, double* x, double* z, double* xref, double* stats) {
  if (m < 1 || m > BMPC_MAX_M) return -22;
  for (int e = 0; e < batch; ++e) {
    double* st = scene + (size_t)e * ENV_STRIDE;
    if (t > 0 && stats && J && status && iters)
      env_accumulate(st, J[e], status[e], iters[e], false, stats + (size_t)e * ENVS_STRIDE);
    quad_env_step_ego(*env, mc, dt, N, m, t, st, pol + (size_t)e * m, upred ? upred + (size_t)e * upred_stride : nullptr,
                      x + (size_t)e * 3, z + (size_t)e * 3, xref + (size_t)e * 3);
  }
  return 0;
}

}  // extern "C"
