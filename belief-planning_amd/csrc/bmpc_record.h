// bmpc_record.h -- the closed loops' per-step recorder (bmpc_set_loop_record): where a step's row
// lies in the caller's columns and the copy of one ego's row.  Written once for the fused k_loop
// (an out-of-line call at the end of each step, bmpc_dev.h), the per-step launches' k_loop_record
// (bmpc_hip.hip) and the host (tests/hostsim/loop_record_host.cpp): the same code, so the same bits.
//
// A row is in the device scene's own convention -- state and inputs OF step t: the scene row as
// step t's solve saw it (after the scene step of t, before the Euler step of t + 1), that solve's
// x_ref, its outputs and its tree.  Highway_sim's post-step state_rec[t] is row t + 1's x.
#pragma once

#include "bmpc_core.h"

namespace bmpc {

// doubles (int32 for status / iters) per row of each column
struct RecordDims {
  int32_t n, d, T, U, nbw;   // nbw = nbranch - 1 branch weights
};

// where one ego's row comes from: the scene row [BMPC_ENV_STRIDE], the solve's x_ref [n] and uPred
// [U][d], its cost, exit code and iteration count, and its predictions xPred [T][n], the tree's
// obstacle predictions [T][n] and branch weights [nbw] (read only for columns that are attached)
struct RecordSrc {
  const double *scene, *xref, *upred, *J;
  const int32_t *status, *iters;
  const double *xpred, *zpred, *bw;
};

// Offset of row (e, r)'s first entry in a column of `width` entries per row.  size_t throughout:
// batch * capacity * T * n passes 2^32 at Monte-Carlo sizes.
BMPC_HD size_t record_offset(size_t e, size_t capacity, size_t r, size_t width) {
  return (e * capacity + r) * width;
}

// The row of closed-loop step t, or false when no recorder is attached or t lies outside
// [t_base, t_base + capacity): such a step is not recorded and touches nothing.
BMPC_HD bool record_row_of(const bmpc_loop_record& R, int t, size_t* r) {
  if (R.capacity < 1) return false;
  const long long k = (long long)t - (long long)R.t_base;
  if (k < 0 || k >= (long long)R.capacity) return false;
  *r = (size_t)k;
  return true;
}

// One row (index `row` = e * capacity + r, record_offset(e, capacity, r, 1)) of the core columns,
// cooperatively by the `nlanes` lanes of one executor (this is lane `lane`; the host runs it with
// every lane in turn): the scene row, x_ref, u and the scalars go out on the first lanes.  Plain
// stores only.  (Columns and sources as separate arguments: the fused k_loop calls this out of line
// with every argument in a register, bmpc_dev.h.)
BMPC_HD void record_write_core(double* scene, double* xref, double* u, double* J, int32_t* status, int32_t* iters,
                               size_t row, int n, int d, int lane, int nlanes, const double* s_scene,
                               const double* s_xref, const double* s_upred, const double* s_J,
                               const int32_t* s_status, const int32_t* s_iters) {
  for (int i = lane; i < BMPC_ENV_STRIDE; i += nlanes) scene[row * BMPC_ENV_STRIDE + i] = s_scene[i];
  for (int i = lane; i < n; i += nlanes) xref[row * (size_t)n + i] = s_xref[i];
  for (int i = lane; i < d; i += nlanes) u[row * (size_t)d + i] = s_upred[i];
  if (lane == 0) {
    J[row] = *s_J;
    status[row] = *s_status;
    iters[row] = *s_iters;
  }
}

// The same row of the optional columns, each strided over all lanes; NULL columns are skipped.
BMPC_HD void record_write_wide(double* upred, double* xpred, double* zpred, double* branch_w, size_t row,
                               const RecordDims& D, int lane, int nlanes, const double* s_upred,
                               const double* s_xpred, const double* s_zpred, const double* s_bw) {
  if (upred) {
    const int cnt = D.U * D.d;
    double* out = upred + row * (size_t)cnt;
    for (int i = lane; i < cnt; i += nlanes) out[i] = s_upred[i];
  }
  if (xpred) {
    const int cnt = D.T * D.n;
    double* out = xpred + row * (size_t)cnt;
    for (int i = lane; i < cnt; i += nlanes) out[i] = s_xpred[i];
  }
  if (zpred) {
    const int cnt = D.T * D.n;
    double* out = zpred + row * (size_t)cnt;
    for (int i = lane; i < cnt; i += nlanes) out[i] = s_zpred[i];
  }
  if (branch_w && D.nbw > 0) {
    double* out = branch_w + row * (size_t)D.nbw;
    for (int i = lane; i < D.nbw; i += nlanes) out[i] = s_bw[i];
  }
}

// Ego e's whole row r: the two parts above.
BMPC_HD void record_write_row(const bmpc_loop_record& R, const RecordDims& D, size_t e, size_t r, int lane, int nlanes,
                              const RecordSrc& S) {
  const size_t row = record_offset(e, (size_t)R.capacity, r, 1);
  record_write_core(R.scene, R.xref, R.u, R.J, R.status, R.iters, row, D.n, D.d, lane, nlanes, S.scene, S.xref,
                    S.upred, S.J, S.status, S.iters);
  record_write_wide(R.upred, R.xpred, R.zpred, R.branch_w, row, D, lane, nlanes, S.upred, S.xpred, S.zpred, S.bw);
}

}  // namespace bmpc
