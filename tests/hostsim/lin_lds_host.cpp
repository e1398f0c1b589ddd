// lin_lds_host.cpp -- the host build of the solver (hostsim.cpp and the two plan builders) with three
// entry points more, for tests/test_lin_lds_host.py: what the plan carved for the linearisation cache
// (BMPC_LIN_LDS, csrc/bmpc_core.h), and a solve in its two halves -- the tree step, then the IPM --
// so that a test can read and change the slab between them (hs_ws_ptr).  The halves are the calls
// hs_solve makes (solve_ego = tree_step + solve_ego_ipm) with the same executors.
#include "bmpc_plan.cpp"
#include "bmpc_qpplan.cpp"
#include "hostsim.cpp"

extern "C" {

// out[0..6]: nlds_rich, nlin_a, tab16, nlds, ntab, lin.na, BMPC_LIN_LDS
int hs_lin_info(void* p, int32_t* out) {
  const Plan& P = ((HS*)p)->hp.plan;
  const int v[7] = {P.nlds_rich, P.nlin_a, P.tab16, P.nlds, P.ntab, P.lin.na, BMPC_LIN_LDS};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return 0;
}

// the tree step of every ego (CVaR plans of the highway models)
int hs_tree_only(void* p, const double* x, const double* z, const double* xref) {
  HS* h = (HS*)p;
  const Plan& P = h->hp.plan;
  const Layout& L = h->hp.lay;
  HostExec ex;
  HostExecT<true> exm;
  for (int e = 0; e < h->batch; ++e) {
    EgoView E{h->ws.data() + L.stride * e, h->pol.data() + (size_t)e * P.m};
    const double *xe = x + e * P.n, *ze = z + e * P.n, *re = xref + e * P.n;
    if (P.desc.model == BMPC_MODEL_HIGHWAY_MERGE) tree_step<HostExecT<true>, HighwayMerge>(exm, P, L, E, xe, ze, re);
    else if (P.desc.flags & BMPC_PLAN_TRANSFORM) tree_step<HostExecT<true>, HighwayT>(exm, P, L, E, xe, ze, re);
    else tree_step<HostExec, Highway>(ex, P, L, E, xe, ze, re);
  }
  return 0;
}

// the IPM and the unpacking of every ego over the slab as it stands; lean: the slab coupling system
int hs_ipm_only(void* p, int lean, double* upred, double* xpred, double* J, int32_t* status, int32_t* iters) {
  HS* h = (HS*)p;
  const Plan& P = h->hp.plan;
  const Layout& L = h->hp.lay;
  HostExec ex;
  HostExecT<true> exm;
  HostExecT<false, false> exl;
  std::vector<double> lds(P.nlds), eco(ECO_COUNT);
  for (int i = 0; i < P.nconst; ++i) lds[P.lds_w + i] = plan_const(P, i);
  ex.lds = exm.lds = exl.lds = lds.data();
  ex.tab = exm.tab = exl.tab = P.t.br_depth;
  exm.eco = eco.data();
  for (int e = 0; e < h->batch; ++e) {
    EgoView E{h->ws.data() + L.stride * e, h->pol.data() + (size_t)e * P.m};
    IpmResult r;
    if (P.desc.model == BMPC_MODEL_HIGHWAY_MERGE) r = solve_ego_ipm<HostExecT<true>, HighwayMerge>(exm, P, L, E);
    else if (P.desc.flags & BMPC_PLAN_TRANSFORM) r = solve_ego_ipm<HostExecT<true>, HighwayT>(exm, P, L, E);
    else if (lean) r = solve_ego_ipm<HostExecT<false, false>, Highway>(exl, P, L, E);
    else r = solve_ego_ipm<HostExec, Highway>(ex, P, L, E);
    const double* ws = E.ws;
    memcpy(upred + (size_t)e * P.U * P.d, ws + L.upred, sizeof(double) * P.U * P.d);
    memcpy(xpred + (size_t)e * P.T * P.n, ws + L.xpred, sizeof(double) * P.T * P.n);
    J[e] = ws[L.sol + P.oJ];
    status[e] = r.exit_flag;
    iters[e] = r.iters;
  }
  return 0;
}

}  // extern "C"
