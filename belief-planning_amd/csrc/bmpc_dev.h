// bmpc_dev.h -- the solver kernels of libbmpc.so (gfx950) and their launchers.
//
// Mapping: one 64-lane wavefront (one 64-thread workgroup) per ego.  k_tree rebuilds the ego's
// scenario tree (warm start, rollouts, linearisation, collision rows); k_ipm / k_qp run the
// structured interior-point solve and unpack the solution.  All per-ego state lives in one
// contiguous slab of HBM (Layout), so every strided lane loop reads and writes contiguous
// 512-byte segments.  Each predictive model's kernels are instantiated in a translation unit of
// their own (bmpc_k_*.hip, compiled in parallel); bmpc_hip.hip holds the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "bmpc_env_merge.h"
#include "bmpc_env_quad.h"
#include "bmpc_hmm.h"
#include "bmpc_plan.h"
#include "bmpc_qp.h"
#include "bmpc_qpplan.h"
#include "bmpc_record.h"
#include "bmpc_solve.h"

namespace bmpc {
namespace dev {

#ifndef BMPC_WPE
#define BMPC_WPE 4   // waves per SIMD the IPM kernel is register-limited to (4 = all 4096 egos resident)
#endif


#ifndef BMPC_DPP_REDUCE
// wave butterflies on DPP / permlane swaps instead of __shfl_xor (ds_bpermute): 1 in the multi-wave
// small-batch executor (latency-bound: one ego N=20 NB=1 10.11 -> 9.44 ms, N=8 NB=2 19.00 -> 18.78,
// bit-identical), 0 in the one-wave k_ipm (bandwidth-bound: +1.3% time and +1.2% bytes at 4,096
// headline egos from the extra registers, +0.3% on config 3; profiles/r06/r06d_*); 2 both, 0 neither
#define BMPC_DPP_REDUCE 1
#endif
constexpr bool kDppWave = BMPC_DPP_REDUCE == 2;                              // DevExecT (k_ipm, k_qp, k_tree)
constexpr bool kDppBlock = BMPC_DPP_REDUCE == 1 || BMPC_DPP_REDUCE == 2;     // DevBlockExecT (k_solve_blk)

// LA, LN: the IPM reads A of the solve's linearisation from the wave's LDS cache (bmpc_ipm.h
// lin_A), through the model's description LN of it -- the launch's choice, like TL (bmpc_hip.hip
// choose_launch).  k_tree, k_qp and the tools' kernels take the defaults.
template <bool TR, bool TL = true, bool LA = false, class LN = NoLin>
struct DevExecT {
  static constexpr bool kTransform = TR;   // per-ego S / bx constants in LDS (merge plans)
  static constexpr bool kLinA = LA;
  using Lin = LN;
  // LDS-rich launch (TL): topology tables copied to LDS and the coupling system in LDS;
  // lean launch: tables read from the plan's blob, coupling system in the slab
  static constexpr bool kCoupLds = TL;
  // (with the cache the LDS copy of the tables is 16-bit: what makes its room at 16 egos per CU)
  using tab_ptr = typename std::conditional<TL, typename std::conditional<LA, lint16*, lint*>::type, gint*>::type;
  int lane;
  ldouble* lds;  // this wave's LDS scratch (Plan::nlds doubles; k_ipm / k_qp only)
  tab_ptr tab;   // topology tables (k_ipm / k_qp only)
  ldouble* eco;  // per-ego constants of the solve (ECO_*; kTransform only)
  static constexpr int nlanes = 64;
  // one wave runs a band QP: blocked factorisation and sweeps on wave broadcasts (bmpc_bandqp.h)
  static constexpr bool kBqpWave = true;
  static constexpr bool kInlineG = true;    // apply_G inline (bmpc_ipm.h)
  // small dense systems with a lane per row (bmpc_ipm.h, small_lu_solve_rows)
  static constexpr bool kRowLanes = true;
  // lane l's v, wave-uniform (l uniform)
  __device__ double rlane(double v, int l) const {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                            __builtin_amdgcn_readlane(__double2loint(v), l));
  }
  // task groups of 4 lanes (one DPP quad) for the tree sweeps
  static constexpr int kTaskLanes = 4;
  // cone rows per lane the fused IPM passes hold in registers (bmpc_ipm.h, cone_regs)
  static constexpr int kConeRegRows = 8;
  __device__ double tsum(double v) const {
    v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
    return v;
  }
  template <int S>
  __device__ double tget(double v) const { return dpp_d<S | (S << 2) | (S << 4) | (S << 6)>(v); }
  // sum over aligned groups of g lanes (g a power of two)
  __device__ double gsum(double v, int g) const { return group_reduce<0, kDppWave>(v, g); }
  __device__ double gmax(double v, int g) const { return group_reduce<1, kDppWave>(v, g); }
  __device__ double gmin(double v, int g) const { return group_reduce<2, kDppWave>(v, g); }
  __device__ void sync() const { __syncthreads(); }
  // a wave-uniform flag as a scalar: branches on it (and the calls they guard) run with the
  // full exec mask instead of an exec mask derived from a VGPR the compiler cannot prove uniform
  __device__ bool uniform(bool b) const { return __builtin_amdgcn_readfirstlane((int)b) != 0; }
  // a wave-uniform double as a scalar pair: an SGPR operand of the lane loops that use it
  __device__ double uniform(double v) const {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
  }
  // the IPM's iteration record in this wave's LDS (bmpc_ipm.h, IterRec; Plan::lds_it): one wave per
  // workgroup, so a slot written by every lane is read back by every lane without a barrier
  static constexpr bool kIterLds = BMPC_ITER_RECORD != 0;
  __device__ double sum(double v) const { return wave_reduce<0, kDppWave>(v); }
  __device__ double max(double v) const { return wave_reduce<1, kDppWave>(v); }
  __device__ double min(double v) const { return wave_reduce<2, kDppWave>(v); }
  // K sums / minima at once (in place)
  template <int K>
  __device__ void sum_n(double* v) const {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sum(v[k]);
  }
  template <int K>
  __device__ void min_n(double* v) const {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = min(v[k]);
  }
};

using DevExec = DevExecT<false>;
// the IPM's one-wave executor of model M, with the cache or without (then the default executor's type)
template <class M, bool TL, bool LA>
using IpmExecT = DevExecT<M::kTransform, TL, LA, typename std::conditional<LA, typename M::Lin, NoLin>::type>;
// a model's launches are compiled with the cache where it has a description
template <class M>
constexpr bool kHasLin = BMPC_LIN_LDS && M::Lin::NA > 0;

#ifndef BMPC_BLK_RED2
#define BMPC_BLK_RED2 1   // whole-executor reductions with one barrier (two buffers in turn)
#endif
// Multi-wave executor: one ego on NW waves of one workgroup (batch-1 / small-batch callers --
// main_branch's one solve per step): the same phase templates with 64*NW lanes, so the tree
// solve's tasks, the cone groups and every lane loop spread over NW waves.  Wave-level
// operations (DPP quads, cone-group shuffles) are unchanged; whole-executor reductions go
// through LDS (`red`: K*NW doubles of one of two buffers) and one barrier.
template <bool TR, bool TL, int NW>
struct DevBlockExecT {
  static constexpr bool kTransform = TR;
  static constexpr bool kCoupLds = TL;
  using tab_ptr = typename std::conditional<TL, lint*, gint*>::type;
  int lane;
  ldouble* lds;
  tab_ptr tab;
  ldouble* eco;
  ldouble* red;   // reduction scratch: 2 * kRedMax * NW doubles, then NW turn slots
  static constexpr int nlanes = 64 * NW;
  static constexpr int kBatchDiv = NW;   // lane batches NW times narrower (bmpc_core.h, lane_batch)
  static constexpr bool kRowLanes = true;
  static constexpr int kTaskLanes = 4;
  // wider cone groups than one wave's (exec_cgrp): fewer rows per lane in the fused cone passes
  // and the cone groups' strided loops (4 waves: a 122-row cone on 64 lanes holds 2 rows a lane)
  static constexpr int kConeRegRows = NW == 4 ? 4 : 8;
  static constexpr int kConeBatch = NW == 4 ? 2 : 4;
  static constexpr int kRedMax = 16;
  static constexpr bool kIterRecord = false;   // the IPM loop with its state in locals (bmpc_ipm.h, ipm_solve)
  static constexpr bool kLinA = false;   // A from the slab -- or from its LDS-resident span (k_solve_blk)
  using Lin = NoLin;
  __device__ double tsum(double v) const {
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    return v;
  }
  template <int S>
  __device__ double tget(double v) const { return dpp_d<S | (S << 2) | (S << 4) | (S << 6)>(v); }
  __device__ double gsum(double v, int g) const { return group_reduce<0, kDppBlock>(v, g); }
  __device__ double gmax(double v, int g) const { return group_reduce<1, kDppBlock>(v, g); }
  __device__ double gmin(double v, int g) const { return group_reduce<2, kDppBlock>(v, g); }
  __device__ void sync() const { __syncthreads(); }
  __device__ bool uniform(bool b) const { return __builtin_amdgcn_readfirstlane((int)b) != 0; }
  // OP 0 sum, 1 max, 2 min of K values per lane over all lanes (in place)
  template <int OP, int K>
  __device__ void reduce(double* v) const {
    static_assert(K <= kRedMax, "reduction scratch");
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_reduce<OP, kDppBlock>(v[k]);
    const int wv = lane >> 6;
#if BMPC_BLK_RED2
    // two buffers used in turn (each wave's turn kept in its LDS slot: every wave runs the same
    // reductions in the same order): a wave writing reduction r + 2 into the buffer of r has
    // passed r + 1's barrier, which every wave reaches only after reading r -- one barrier each
    ldouble* turn = red + 2 * kRedMax * NW + wv;
    const int odd = __builtin_amdgcn_readfirstlane((int)*turn);
    ldouble* buf = red + (odd ? kRedMax * NW : 0);
    if ((lane & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) buf[k * NW + wv] = v[k];
      *turn = odd ? 0.0 : 1.0;
    }
#else
    ldouble* buf = red;
    __syncthreads();   // the previous reduction's readers are done with red
    if ((lane & 63) == 0)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * NW + wv] = v[k];
#endif
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double a = buf[k * NW];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const double b = buf[k * NW + w];
        a = OP == 0 ? a + b : OP == 1 ? fmax(a, b) : fmin(a, b);
      }
      v[k] = a;
    }
  }
  __device__ double sum(double v) const { reduce<0, 1>(&v); return v; }
  __device__ double max(double v) const { reduce<1, 1>(&v); return v; }
  __device__ double min(double v) const { reduce<2, 1>(&v); return v; }
  template <int K>
  __device__ void sum_n(double* v) const { reduce<0, K>(v); }
  template <int K>
  __device__ void min_n(double* v) const { reduce<2, K>(v); }
};

struct Bundle {
  Plan P;
  Layout L;
};

// Dynamic LDS of the solver kernels: Plan::nlds_rich / nlds_lean doubles of scratch, then a copy of the
// topology tables (Plan::ntab int32; tab16: of 16 bits, the launches with the linearisation cache), then
// (transform-capable models) ECO_COUNT doubles of
// per-ego constants.  The table copy is one batched pass at kernel start; every later tree /
// cone / node-index lookup of the solve is an LDS read.
// lin: a launch that reads the linearisation cache -- Plan::nlin_a doubles behind the others, its table copy 16-bit
__host__ __device__ inline size_t solver_lds_bytes(const Plan& P, bool transform, bool rich, bool lin = false) {
  const size_t tab = rich ? ((lin ? sizeof(int16_t) : sizeof(int32_t)) * (size_t)P.ntab + 7) & ~(size_t)7 : 0;
  return sizeof(double) * (size_t)((rich ? P.nlds_rich : P.nlds_lean) + (lin ? P.nlin_a : 0)) + tab +
         (transform ? sizeof(double) * ECO_COUNT : 0);
}
template <bool TR, bool TL, bool LA = false, class LN = NoLin>
__device__ __forceinline__ DevExecT<TR, TL, LA, LN> solver_exec(const Plan& P, double* lds_dyn) {
  const int32_t* gtab = (const int32_t*)P.t.br_depth;   // blob base (the first table)
  double* eco = lds_dyn + (solver_lds_bytes(P, false, TL, LA) / sizeof(double));
  // W1 | Wu | Fx | Fu for the IPM passes' per-lane row lookups
  for (int i = threadIdx.x; i < P.nconst; i += 64) lds_dyn[P.lds_w + i] = plan_const(P, i);
  if constexpr (TL) {
    using TT = typename std::conditional<LA, int16_t, int32_t>::type;
    TT* tabl = reinterpret_cast<TT*>(lds_dyn + P.nlds_rich + (LA ? P.nlin_a : 0));
    for (int i = threadIdx.x; i < P.ntab; i += 64) tabl[i] = (TT)gtab[i];   // (16 bits: in range, Plan::tab16)
    __syncthreads();
    return DevExecT<TR, TL, LA, LN>{(int)threadIdx.x, (ldouble*)lds_dyn, (const BMPC_AS_LDS TT*)tabl, (ldouble*)eco};
  } else {
    __syncthreads();
    return DevExecT<TR, TL, LA, LN>{(int)threadIdx.x, (ldouble*)lds_dyn, (gint*)gtab, (ldouble*)eco};
  }
}

// waves per ego of the small-batch solver kernel (k_solve_blk): 4, or 8 for trees of at least
// BMPC_BLK_WIDE_T state nodes (measured at one ego, profiles/r03/r03x_blk_waves.log: N=8 NB=2
// 22 ms on 4 waves, 24 on 8, 38 on 16, 30 on one; N=20 NB=1 12-14 / 14-17 / 20-22 / 14-16;
// N=30 NB=2 48-54 / 44-49 / 62-65 / 61-65)
#ifndef BMPC_BLK_WIDE_T
#define BMPC_BLK_WIDE_T 256
#endif
#define BMPC_BLK_WAVES_MAX 8

// LDS of a multi-wave solver launch: the wave launch's, then the reduction scratch
__host__ __device__ inline size_t solver_lds_bytes_blk(const Plan& P, bool transform, int nw) {
  return ((solver_lds_bytes(P, transform, true) + 7) & ~(size_t)7) + sizeof(double) * (2 * 16 + 1) * (size_t)nw;
}
template <bool TR, int NW>
__device__ __forceinline__ DevBlockExecT<TR, true, NW> solver_exec_blk(const Plan& P, double* lds_dyn) {
  const int t = threadIdx.x, nt = 64 * NW;
  for (int i = t; i < P.nconst; i += nt) lds_dyn[P.lds_w + i] = plan_const(P, i);
  const int32_t* gtab = (const int32_t*)P.t.br_depth;
  int32_t* tabl = reinterpret_cast<int32_t*>(lds_dyn + P.nlds_rich);
  for (int i = t; i < P.ntab; i += nt) tabl[i] = gtab[i];
  double* eco = lds_dyn + (solver_lds_bytes(P, false, true) / sizeof(double));
  double* red = lds_dyn + ((solver_lds_bytes(P, TR, true) + 7) & ~(size_t)7) / sizeof(double);
  if (t < NW) red[2 * 16 * NW + t] = 0.0;   // each wave's reduction turn (BMPC_BLK_RED2)
  __syncthreads();
  return DevBlockExecT<TR, true, NW>{t, (ldouble*)lds_dyn, (lint*)tabl, (ldouble*)eco, (ldouble*)red};
}

// The solver kernels' epilogue: ego e's predictions out of its slab w (strided over the NT
// lanes of the workgroup), then the cost (*Jsrc: the IPM's slot of the solution, or the QP's
// primal cost), the exit code and the iteration count on lane 0.  Null outputs are skipped.
template <int NT>
__device__ __forceinline__ void write_outputs(const Plan& P, const Layout& L, const double* w, int e,
                                              const double* Jsrc, const IpmResult& r, double* upred, double* xpred,
                                              double* bw, double* J, int32_t* status, int32_t* iters) {
  const int lane = threadIdx.x;
  if (upred)
    for (int i = lane; i < P.U * P.d; i += NT) upred[(size_t)e * P.U * P.d + i] = w[L.upred + i];
  if (xpred)
    for (int i = lane; i < P.T * P.n; i += NT) xpred[(size_t)e * P.T * P.n + i] = w[L.xpred + i];
  if (bw)
    for (int i = lane; i < P.nbranch - 1; i += NT) bw[(size_t)e * (P.nbranch - 1) + i] = w[L.w + 1 + i];
  if (lane == 0) {
    if (J) J[e] = *Jsrc;
    if (status) status[e] = r.exit_flag;
    if (iters) iters[e] = r.iters;
  }
}

// One ego per workgroup of NW waves (small batches: every wave of the chip on few egos);
// QP: the OSQP-class controllers' k_qp path, else the CVaR IPM.
//
// LDS-resident arrays (lay != NULL; translation units with BMPC_FLAT_SLAB only): lay[e] is ego e's
// copy of the layout in which spans of the IPM's own arrays (written before they are read within a
// solve: the NT scaling, the node factors and tree-solve vectors, z / s / lambda) are offset from
// the ego's slab to this workgroup's LDS at hot_off doubles (flat addresses: LDS aperture + offset,
// bmpc_hip.hip blk_layouts); the tree's linearisation (A, B and dh, written by k_tree) is copied
// in when its span is relocated.  A layout that does not land in this workgroup's LDS fails the
// solve with EXIT_GUARD.
template <class M, bool QP, int NW>
__global__ __launch_bounds__(64 * NW) void k_solve_blk(const Bundle* __restrict__ B, double* __restrict__ ws,
                                                      const bmpc_policy* __restrict__ pol, double* upred,
                                                      double* xpred, double* bw, double* J, int32_t* status,
                                                      int32_t* iters, int batch, const Layout* __restrict__ lay,
                                                      size_t hot_off) {
  const int e = blockIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L0 = B->L;
  const Layout& L = lay ? lay[e] : L0;
  constexpr bool TR = QP ? false : M::kTransform;
  extern __shared__ double lds_dyn[];
  const auto ex = solver_exec_blk<TR, NW>(P, lds_dyn);
  using X = DevBlockExecT<TR, true, NW>;
#if defined(BMPC_FLAT_SLAB)
  // the slab pointer through readfirstlane: the compiler cannot infer from the kernel argument
  // that the arrays behind it are global memory, so every slab access is a flat access (LDS or
  // global by address)
  EgoView E{uniform_ptr(ws + L0.stride * (size_t)e), pol + (size_t)e * P.m};
#else
  EgoView E{ws + L0.stride * (size_t)e, pol + (size_t)e * P.m};
#endif
  IpmResult r;
#if defined(BMPC_FLAT_SLAB)
  if (lay) {
    const int t = threadIdx.x, nt = 64 * NW;
    double* w = E.ws;
    if ((uintptr_t)(w + L.dl) != (uintptr_t)(lds_dyn + hot_off)) {   // the first relocated span
      if (t == 0) {
        if (status) status[e] = EXIT_GUARD;
        if (iters) iters[e] = 0;
      }
      return;
    }
    if (L.Ad != L0.Ad)
      for (size_t i = t; i < L0.Cd - L0.Ad; i += nt) w[L.Ad + i] = w[L0.Ad + i];
    if (L.dh != L0.dh)
      for (size_t i = t; i < L0.h0 - L0.dh; i += nt) w[L.dh + i] = w[L0.dh + i];
    __syncthreads();
  }
#endif
  if constexpr (QP) r = solve_ego_qp<X, M>(ex, P, L, E);
  else r = solve_ego_ipm<X, M>(ex, P, L, E);
  const double* w = E.ws;
  write_outputs<64 * NW>(P, L, w, e, QP ? &r.pcost : w + L.sol + P.oJ, r, upred, xpred, bw, J, status, iters);
}

#if defined(BMPC_BLK2)
// Tools-only A/B (-DBMPC_BLK2, BMPC_IPM_W2=1): the large-batch CVaR IPM with one ego on TWO waves
// (the small-batch kernel's executor at 128 lanes, slab arrays in global memory, the register
// budget of k_ipm) -- 8 egos per CU instead of 16, each on twice the lanes.
template <class M>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(BMPC_WPE))) void k_ipm_w2(
    const Bundle* __restrict__ B, double* __restrict__ ws, const bmpc_policy* __restrict__ pol, double* upred,
    double* xpred, double* bw, double* J, int32_t* status, int32_t* iters, int batch) {
  const int e = blockIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  extern __shared__ double lds_dyn[];
  const auto ex = solver_exec_blk<M::kTransform, 2>(P, lds_dyn);
  EgoView E{ws + L.stride * (size_t)e, pol + (size_t)e * P.m};
  IpmResult r = solve_ego_ipm<DevBlockExecT<M::kTransform, true, 2>, M>(ex, P, L, E);
  write_outputs<128>(P, L, E.ws, e, E.ws + L.sol + P.oJ, r, upred, xpred, bw, J, status, iters);
}
#endif

#ifndef BMPC_TREE_WPE
#define BMPC_TREE_WPE 4   // k_tree's register budget in batches beyond 2 waves per SIMD (r05ad: 1.23 -> 0.99 ms at 4,096 egos; 3: 1.30)
#endif
// WPE: waves per SIMD the register budget allows (1: 2 waves, the compiler's own choice of 220 VGPRs).  The
// budget pays where the batch has more egos than 2 waves per SIMD hold (launch_tree); a one-ego
// launch is faster without its spills.
template <class M, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE > 1 ? WPE : 2))) void k_tree(const Bundle* __restrict__ B, double* __restrict__ ws,
                                             const bmpc_policy* __restrict__ pol,
                                             const double* __restrict__ x, const double* __restrict__ z,
                                             const double* __restrict__ xref, int batch) {
  const int e = blockIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  DevExec ex{(int)threadIdx.x, nullptr, nullptr, nullptr};
  EgoView E{ws + L.stride * (size_t)e, pol + (size_t)e * P.m};
  BMPC_PROF(E.ws, L, PROF_TREE);
  tree_step<DevExec, M>(ex, P, L, E, x + e * P.n, z + e * P.n, xref + e * P.n);
}

template <class M, bool TL, bool LA = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BMPC_WPE))) void k_ipm(const Bundle* __restrict__ B, double* __restrict__ ws,
                                            const bmpc_policy* __restrict__ pol, double* upred,
                                            double* xpred, double* bw, double* J, int32_t* status,
                                            int32_t* iters, int batch) {
  const int e = blockIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  extern __shared__ double lds_dyn[];
  using X = IpmExecT<M, TL, LA>;
  const auto ex = solver_exec<M::kTransform, TL, LA, typename X::Lin>(P, lds_dyn);
  EgoView E{ws + L.stride * (size_t)e, pol + (size_t)e * P.m};
  IpmResult r = solve_ego_ipm<X, M>(ex, P, L, E);
  write_outputs<64>(P, L, E.ws, e, E.ws + L.sol + P.oJ, r, upred, xpred, bw, J, status, iters);
}

template <class M, bool TL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BMPC_WPE))) void k_qp(
    const Bundle* __restrict__ B, double* __restrict__ ws, const bmpc_policy* __restrict__ pol, double* upred,
    double* xpred, double* bw, double* J, int32_t* status, int32_t* iters, int batch) {
  const int e = blockIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  extern __shared__ double lds_dyn[];
  const auto ex = solver_exec<false, TL>(P, lds_dyn);
  EgoView E{ws + L.stride * (size_t)e, pol + (size_t)e * P.m};
  IpmResult r = solve_ego_qp<DevExecT<false, TL>, M>(ex, P, L, E);
  write_outputs<64>(P, L, E.ws, e, &r.pcost, r, upred, xpred, bw, J, status, iters);
}

// The three parts of a k_loop step as calls of their own: each gets its registers allocated
// apart from the others' (the scene step's and the tree step's private arrays and live values
// stay out of the IPM loop's 128-VGPR budget).
template <class X, class M>
__device__ __attribute__((noinline)) void loop_tree_step(const X ex, const Plan& P, const Layout& L, EgoView E,
                                                          const double* x, const double* z, const double* xref) {
  tree_step<X, M>(ex, P, L, E, x, z, xref);
}
template <class X, class M>
__device__ __attribute__((noinline)) IpmResult loop_ipm(const X ex, const Plan& P, const Layout& L, EgoView E) {
  return solve_ego_ipm<X, M>(ex, P, L, E);
}
// (smp: the plan's obstacle sampler, bmpc_set_obstacle_sampling, by reference out of the kernel
// argument like env -- two argument registers; the sampled rule lives in here, on lane 0, under a
// branch on its mode, so the solve's register budget never sees it.  e: the wave's ego.  prop: the
// plan's device block of scene options (bmpc_env.h SceneOptions: its obstacle proposal,
// bmpc_set_obstacle_proposal, then its disturbance, bmpc_set_disturbance, then its observation model,
// bmpc_set_observation) or null -- one pointer; the proposal is read by the weighted modes only, the
// disturbance's and the observation's law once per step.)
__device__ __attribute__((noinline)) void loop_env_step(const bmpc_env_desc& env, double dt, int N, int m, int t,
                                                        double* st, bmpc_policy* pol, const double* up, double* x,
                                                        double* z, double* xr, double Jv, int status, int iters,
                                                        double* stats, const bmpc_obstacle_sampling& smp,
                                                        const double* mc, int e, const SceneOptions* opt) {
  if (t > 0 && stats) env_accumulate(st, Jv, status, iters, true, stats);
  env_step_ego(env, dt, N, m, t, st, pol, up, x, z, xr, &smp, mc, e, scene_prop(opt), scene_dist(opt),
               scene_obs(opt));
}

// One merge-scene step of one ego into its slab (k_env_merge and the merge k_loop): the scene
// function writes S and bx straight into the ego's transform slots and marks them set (S on),
// which is all bmpc_set_transform would have scattered there.  opt: the plan's scene options or null
// (the merge scene reads the disturbance and the observation model: its obstacle never chooses), e: the
// ego's index.
__device__ __forceinline__ void merge_env_step_slab(const bmpc_merge_env_desc& env, const MergeRef& R, const Plan& P,
                                                    const Layout& L, int t, double* st, double* ws, const double* up,
                                                    double* x, double* z, double* xr, const SceneOptions* opt, int e) {
  double* xf = ws + L.xform;
  merge_env_step_ego(env, R, P.desc.bx, P.nFx, P.desc.dt, t, st, up, x, z, xr, xf + XF_S, xf + XF_BX,
                     scene_dist(opt), e, scene_obs(opt));
  xf[XF_SON] = 1.0;
  xf[XF_BXSET] = 1.0;
}
__device__ __attribute__((noinline)) void loop_merge_env_step(const bmpc_merge_env_desc& env, const MergeRef& R,
                                                              const Plan& P, const Layout& L, int t, double* st,
                                                              double* ws, const double* up, double* x, double* z,
                                                              double* xr, double Jv, int status, int iters,
                                                              double* stats, const SceneOptions* opt, int e) {
  if (t > 0 && stats) env_accumulate(st, Jv, status, iters, true, stats);
  merge_env_step_slab(env, R, P, L, t, st, ws, up, x, z, xr, opt, e);
}

// The overtake scene's step for the OSQP-class controllers (BranchMPC, robustMPC; OvertakeQpScene):
// loop_env_step with the statistics reading their status (1 = solved), the rule k_env applies to a
// plan that is not CVaR.
__device__ __attribute__((noinline)) void loop_env_step_qp(const bmpc_env_desc& env, double dt, int N, int m, int t,
                                                           double* st, bmpc_policy* pol, const double* up, double* x,
                                                           double* z, double* xr, double Jv, int status, int iters,
                                                           double* stats, const bmpc_obstacle_sampling& smp,
                                                           const double* mc, int e, const SceneOptions* opt) {
  if (t > 0 && stats) env_accumulate(st, Jv, status, iters, false, stats);
  env_step_ego(env, dt, N, m, t, st, pol, up, x, z, xr, &smp, mc, e, scene_prop(opt), scene_dist(opt),
               scene_obs(opt));
}

// The quadruped loop's solve and scene step as calls (OSQP-class controllers: env_accumulate reads
// their status, 1 = solved).
template <class X, class M>
__device__ __attribute__((noinline)) IpmResult loop_qp(const X ex, const Plan& P, const Layout& L, EgoView E) {
  return solve_ego_qp<X, M>(ex, P, L, E);
}
__device__ __attribute__((noinline)) void loop_quad_env_step(const bmpc_quad_env_desc& env, const Plan& P, int t,
                                                             double* st, const bmpc_policy* pol, const double* up,
                                                             double* x, double* z, double* xr, double Jv, int status,
                                                             int iters, double* stats,
                                                             const bmpc_obstacle_sampling& smp, int e,
                                                             const SceneOptions* opt) {
  if (t > 0 && stats) env_accumulate(st, Jv, status, iters, false, stats);
  quad_env_step_ego(env, P.desc.mc, P.desc.dt, P.N, P.m, t, st, pol, up, x, z, xr, &smp, e, scene_prop(opt),
                    scene_dist(opt), scene_obs(opt));
}

// Ego e's row r of the closed loops' recorder (bmpc_record.h), by the 64 lanes of one wave: the
// scene row st, the solve's x_ref xr, its uPred up, cost and exit code from the loop's own buffers,
// the predictions, the tree's obstacle predictions and the branch weights out of the ego's slab w
// through the plan's base layout -- the offsets bmpc_get_tree and write_outputs read (none of them
// lies in a span the small-batch kernel relocates to LDS, bmpc_hip.hip blk_layouts).
__device__ __forceinline__ void record_ego_row(const bmpc_loop_record& R, const Plan& P, const Layout& L, int e,
                                               size_t r, const double* w, const double* st, const double* xr,
                                               const double* up, const double* J, const int32_t* status,
                                               const int32_t* iters) {
  const RecordDims D{P.n, P.d, P.T, P.U, P.nbranch - 1};
  const RecordSrc S{st, xr, up, J, status, iters, w + L.xpred, w + L.zbar, w + L.w + 1};
  record_write_row(R, D, (size_t)e, r, (int)threadIdx.x, 64, S);
}
// ... as calls of their own at the end of a k_loop step: their registers are allocated apart from
// the solve's (the IPM / QP loop's 128-VGPR budget never sees the copy loops; DESIGN §5b on what
// inlining into that budget costs), and a loop without a recorder branches around them.  Two calls
// of scalar arguments, not one taking the struct: an 88-byte struct goes to a callee through the
// caller's stack frame, which every k_loop launch would pay as scratch, recorder or not (§5e);
// each of these fits the 32 argument registers.  `row` = e * capacity + r.
__device__ __attribute__((noinline)) void loop_record_core(double* scene, double* xref, double* u, double* J,
                                                           int32_t* status, int32_t* iters, size_t row,
                                                           const Plan& P, const double* st, const double* xr,
                                                           const double* up, const double* Je, const int32_t* ste,
                                                           const int32_t* ite) {
  record_write_core(scene, xref, u, J, status, iters, row, P.n, P.d, (int)threadIdx.x, 64, st, xr, up, Je, ste, ite);
}
__device__ __attribute__((noinline)) void loop_record_wide(double* upred, double* xpred, double* zpred, double* bw,
                                                           size_t row, const Plan& P, const Layout& L,
                                                           const double* w, const double* up) {
  const RecordDims D{P.n, P.d, P.T, P.U, P.nbranch - 1};
  record_write_wide(upred, xpred, zpred, bw, row, D, (int)threadIdx.x, 64, up, w + L.xpred, w + L.zbar, w + L.w + 1);
}

#ifndef BMPC_MERGE_LOOP_INLINE_IPM
#define BMPC_MERGE_LOOP_INLINE_IPM 1
#endif
#ifndef BMPC_QUAD_LOOP_INLINE_QP
#define BMPC_QUAD_LOOP_INLINE_QP 1
#endif
#ifndef BMPC_OVERTAKE_QP_LOOP_INLINE_QP
#define BMPC_OVERTAKE_QP_LOOP_INLINE_QP 1
#endif
// The scene of a k_loop (its kernel argument): one ego's scene step on lane 0, through an
// out-of-line call.  The overtake scene re-targets the ego's policies, the merge scene writes the
// ego's transform slots, the quadruped scene neither.  The overtake and the quadruped scene carry the
// plan's obstacle sampler (mode 0: none); the merge scene's obstacle never chooses.  All three carry
// a pointer to the plan's scene options (null: none): the proposal, the disturbance and the observation
// model.  kQp: the step's
// solve is the OSQP-class controllers' solve_ego_qp (k_qp's) instead of the CVaR IPM.  kInlineIpm: the solve inlined into
// the kernel as k_ipm / k_qp have it (the tree and scene steps stay calls) instead of a call of
// its own -- as a callee the IPM's frame grows from k_ipm's ~590 to ~1,490 bytes per lane (merge
// loop: 2,528 bytes of scratch against 1,648), the QP's loop from 1,152 to 1,280
// (§5d).  The overtake loop keeps the form it was measured in (§5b).
struct OvertakeScene {
  static constexpr bool kQp = false;
  static constexpr bool kInlineIpm = false;
  bmpc_env_desc env;
  bmpc_obstacle_sampling smp;
  const SceneOptions* opt;
  __device__ void step(const Plan& P, const Layout&, int t, double* st, bmpc_policy* pe, double*, const double* up,
                       double* x, double* z, double* xr, double Jv, int status, int iters, double* stats) const {
    loop_env_step(env, P.desc.dt, P.N, P.m, t, st, pe, up, x, z, xr, Jv, status, iters, stats, smp, P.desc.mc,
                  (int)blockIdx.x, opt);
  }
};
// The overtake scene under BranchMPC or robustMPC (bmpc_k_highway_qp_loop.hip): OvertakeScene's step
// with the QP solver and the OSQP-class statistics (both forms of the solve measured).
struct OvertakeQpScene {
  static constexpr bool kQp = true;
  static constexpr bool kInlineIpm = BMPC_OVERTAKE_QP_LOOP_INLINE_QP != 0;
  bmpc_env_desc env;
  bmpc_obstacle_sampling smp;
  const SceneOptions* opt;
  __device__ void step(const Plan& P, const Layout&, int t, double* st, bmpc_policy* pe, double*, const double* up,
                       double* x, double* z, double* xr, double Jv, int status, int iters, double* stats) const {
    loop_env_step_qp(env, P.desc.dt, P.N, P.m, t, st, pe, up, x, z, xr, Jv, status, iters, stats, smp, P.desc.mc,
                     (int)blockIdx.x, opt);
  }
};
struct MergeScene {
  static constexpr bool kQp = false;
  static constexpr bool kInlineIpm = BMPC_MERGE_LOOP_INLINE_IPM != 0;
  bmpc_merge_env_desc env;
  MergeRef ref;
  const SceneOptions* opt;
  __device__ void step(const Plan& P, const Layout& L, int t, double* st, bmpc_policy*, double* ws, const double* up,
                       double* x, double* z, double* xr, double Jv, int status, int iters, double* stats) const {
    loop_merge_env_step(env, ref, P, L, t, st, ws, up, x, z, xr, Jv, status, iters, stats, opt, (int)blockIdx.x);
  }
};
struct QuadScene {
  static constexpr bool kQp = true;
  static constexpr bool kInlineIpm = BMPC_QUAD_LOOP_INLINE_QP != 0;   // (both forms measured)
  bmpc_quad_env_desc env;
  bmpc_obstacle_sampling smp;
  const SceneOptions* opt;
  __device__ void step(const Plan& P, const Layout&, int t, double* st, bmpc_policy* pe, double*, const double* up,
                       double* x, double* z, double* xr, double Jv, int status, int iters, double* stats) const {
    loop_quad_env_step(env, P, t, st, pe, up, x, z, xr, Jv, status, iters, stats, smp, (int)blockIdx.x, opt);
  }
};

// nsteps closed-loop steps of one ego per wave (bmpc_loop_device, bmpc_merge_loop_device,
// bmpc_quad_loop_device): the scene step of k_env / k_env_merge / k_env_quad (lane 0), k_tree's tree
// step and k_ipm's (SC::kQp: k_qp's) solve + unpack, in
// that order, per step -- the same per-ego functions the three launches run, so the same bits --
// with no device-wide boundary between the steps: the egos' loops are independent, and a wave
// whose ego needs few IPM iterations in one step starts its next step instead of idling until the
// slowest ego of the batch finishes.  REC: the kernel can record (bmpc_set_loop_record) -- the one
// instantiation the product launches, with or without a recorder; a build with
// -DBMPC_LOOP_RECORD_TEMPLATE=1 launches the REC = false instantiation, which compiles as the kernel
// did before the recorder, whenever none is attached (the A/B of DESIGN §5e).
#ifndef BMPC_LOOP_RECORD_TEMPLATE
#define BMPC_LOOP_RECORD_TEMPLATE 0
#endif
template <class M, bool TL, class SC, bool REC, bool LA = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BMPC_WPE))) void k_loop(
    const Bundle* __restrict__ B, double* __restrict__ ws, bmpc_policy* __restrict__ pol, SC sc, int t0,
    int nsteps, double* scene, double* upred, double* xs, double* zs, double* xrefs, double* J, int32_t* status,
    int32_t* iters, double* stats, int batch, bmpc_loop_record rec) {
  const int e = blockIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  extern __shared__ double lds_dyn[];
  constexpr bool TR = SC::kQp ? false : M::kTransform;   // (k_qp's executor takes no transform)
  using X = typename std::conditional<SC::kQp, DevExecT<false, TL>, IpmExecT<M, TL, LA>>::type;
  const auto ex = solver_exec<TR, TL, X::kLinA, typename X::Lin>(P, lds_dyn);
  bmpc_policy* pe = pol + (size_t)e * P.m;
  EgoView E{ws + L.stride * (size_t)e, pe};
  double* st = scene + (size_t)e * ENV_STRIDE;
  double* up = upred + (size_t)e * P.U * P.d;
  double* x = xs + (size_t)e * P.n;
  double* z = zs + (size_t)e * P.n;
  double* xr = xrefs + (size_t)e * P.n;
  const int lane = threadIdx.x;
  for (int s = 0; s < nsteps; ++s) {
    const int t = t0 + s;
    if (lane == 0)   // k_env / k_env_merge
      sc.step(P, L, t, st, pe, E.ws, up, x, z, xr, J[e], status[e], iters[e],
              stats ? stats + (size_t)e * ENVS_STRIDE : nullptr);
    __syncthreads();
    loop_tree_step<X, M>(ex, P, L, E, x, z, xr);   // k_tree
    IpmResult r;   // k_ipm / k_qp
    if constexpr (SC::kQp) {
      if constexpr (SC::kInlineIpm) r = solve_ego_qp<X, M>(ex, P, L, E);
      else r = loop_qp<X, M>(ex, P, L, E);
    } else {
      if constexpr (SC::kInlineIpm) r = solve_ego_ipm<X, M>(ex, P, L, E);
      else r = loop_ipm<X, M>(ex, P, L, E);
    }
    const double* w = E.ws;
    for (int i = lane; i < P.U * P.d; i += 64) up[i] = w[L.upred + i];
    if (lane == 0) {
      if constexpr (SC::kQp) J[e] = r.pcost;
      else J[e] = w[L.sol + P.oJ];
      status[e] = r.exit_flag;
      iters[e] = r.iters;
    }
    // the step's row of the recorder (a kernel argument: a wave-uniform scalar branch); each lane
    // reads back what it stored above itself, the rest was written before the solve's last barrier
    if constexpr (REC) {
      if (rec.capacity > 0) {
        size_t r;
        if (record_row_of(rec, t, &r)) {
          const size_t row = record_offset((size_t)e, (size_t)rec.capacity, r, 1);
          loop_record_core(rec.scene, rec.xref, rec.u, rec.J, rec.status, rec.iters, row, P, st, xr, up, J + e,
                           status + e, iters + e);
          if (rec.upred || rec.xpred || rec.zpred || rec.branch_w)
            loop_record_wide(rec.upred, rec.xpred, rec.zpred, rec.branch_w, row, P, L, w, up);
        }
      }
    }
    __syncthreads();
  }
}

// one solve launch of a plan (device pointers; the timing events are recorded by the caller
// between the two launches)
struct SolveLaunch {
  const Bundle* bundle;
  double* ws;
  const bmpc_policy* pol;
  const double *x, *z, *xref;
  double *upred, *xpred, *bw, *J;
  int32_t *status, *iters;
  int batch;
  size_t lds_bytes;   // dynamic LDS of the solver kernel (solver_lds_bytes)
  bool rich;          // LDS-rich solver launch (choose_lds_rich)
  bool qp;            // OSQP-class controller (k_qp) instead of the CVaR IPM (k_ipm)
  hipStream_t stream;
  int nw = 4;        // small-batch launch: waves per ego (4 or 8)
  const Layout* blk_lay = nullptr;   // ... per-ego layouts with LDS-resident spans (or NULL)
  int cus = 256;                     // compute units of the device (k_tree's register budget)
  const Plan* hplan = nullptr;       // the plan on the host (launch sizes)
  size_t blk_hot_off = 0;            // ... their LDS offset (doubles)
  const struct PhasedLaunch* ph = nullptr;   // tools-only builds (BMPC_WITH_PHASED, below)
  bmpc_loop_record rec = {};         // the fused closed loop's recorder (capacity 0: none)
  bmpc_obstacle_sampling smp = {};   // the fused closed loop's obstacle sampler (mode 0: none)
  const SceneOptions* opt = nullptr;   // ... and the plan's device block of scene options (null: none)
  bool lin = false;  // the IPM reads A from its LDS cache (choose_launch: the plan carved it)
};
using LaunchFn = hipError_t(const SolveLaunch&);

// dynamic LDS above 64 KB needs the kernel's opt-in (a driver call: nothing below that size)
inline hipError_t optin_lds(const void* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <class M>
hipError_t launch_tree(const SolveLaunch& a) {
  if (BMPC_TREE_WPE > 1 && a.batch > 2 * 4 * a.cus)
    hipLaunchKernelGGL((k_tree<M, (BMPC_TREE_WPE > 1 ? BMPC_TREE_WPE : 1)>), dim3(a.batch), dim3(64), 0, a.stream,
                       a.bundle, a.ws, a.pol, a.x, a.z, a.xref, a.batch);
  else
    hipLaunchKernelGGL((k_tree<M, 1>), dim3(a.batch), dim3(64), 0, a.stream, a.bundle, a.ws, a.pol, a.x, a.z, a.xref,
                     a.batch);
  return hipGetLastError();
}

// a kernel of the solver signature (k_ipm, k_qp, k_ipm_w2): one workgroup of nt lanes per ego
template <class K>
hipError_t launch_solver_kernel(K kernel, const SolveLaunch& a, int nt, size_t lds) {
  const hipError_t e = optin_lds((const void*)kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(a.batch), dim3(nt), lds, a.stream, a.bundle, a.ws, a.pol, a.upred, a.xpred, a.bw,
                     a.J, a.status, a.iters, a.batch);
  return hipGetLastError();
}

// WITH_QP: the model also serves the OSQP-class controllers (Prox, BranchMPC, robustMPC)
template <class M, bool WITH_QP>
hipError_t launch_solver(const SolveLaunch& a) {
  if constexpr (WITH_QP) {
    if (a.qp)
      return a.rich ? launch_solver_kernel(k_qp<M, true>, a, 64, a.lds_bytes)
                    : launch_solver_kernel(k_qp<M, false>, a, 64, a.lds_bytes);
  }
#if defined(BMPC_BLK2)
  if (const char* e = getenv("BMPC_IPM_W2"))
    if (atoi(e) == 1)
      return launch_solver_kernel(k_ipm_w2<M>, a, 128, solver_lds_bytes_blk(*a.hplan, M::kTransform, 2));
#endif
  if constexpr (kHasLin<M>) {
    if (a.lin)
      return a.rich ? launch_solver_kernel(k_ipm<M, true, true>, a, 64, a.lds_bytes)
                    : launch_solver_kernel(k_ipm<M, false, true>, a, 64, a.lds_bytes);
  }
  if (a.lin) return hipErrorInvalidValue;   // (no kernel of this model reads the cache the plan carved)
  return a.rich ? launch_solver_kernel(k_ipm<M, true>, a, 64, a.lds_bytes)
                : launch_solver_kernel(k_ipm<M, false>, a, 64, a.lds_bytes);
}

// the fused closed loop (k_loop): the one-wave IPM's LDS and register budget
template <class M, class SC>
hipError_t launch_loop(const SolveLaunch& a, const SC& sc, int t0, int nsteps, double* scene, double* stats) {
  void (*k)(const Bundle*, double*, bmpc_policy*, SC, int, int, double*, double*, double*, double*, double*, double*,
            int32_t*, int32_t*, double*, int, bmpc_loop_record) =
      a.rich ? k_loop<M, true, SC, true> : k_loop<M, false, SC, true>;
  if constexpr (BMPC_LOOP_RECORD_TEMPLATE != 0) {
    if (a.rec.capacity < 1) k = a.rich ? k_loop<M, true, SC, false> : k_loop<M, false, SC, false>;
  }
  if constexpr (!SC::kQp) {   // the IPM with its linearisation cache, as launch_solver
    if constexpr (kHasLin<M>) {
      if (a.lin) k = a.rich ? k_loop<M, true, SC, true, true> : k_loop<M, false, SC, true, true>;
    }
    if (a.lin && !kHasLin<M>) return hipErrorInvalidValue;
  }
  const hipError_t e = optin_lds((const void*)k, a.lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(a.batch), dim3(64), a.lds_bytes, a.stream, a.bundle, a.ws, const_cast<bmpc_policy*>(a.pol),
                     sc, t0, nsteps, scene, a.upred, const_cast<double*>(a.x), const_cast<double*>(a.z),
                     const_cast<double*>(a.xref), a.J, a.status, a.iters, stats, a.batch, a.rec);
  return hipGetLastError();
}

// the small-batch launch: one ego per NW-wave workgroup (solver_lds_bytes_blk of LDS)
template <class M, bool QP, int NW>
hipError_t launch_blk_kernel(const SolveLaunch& a) {
  // the opt-in is a driver call of its own (~1.5 ms per one-ego solve when made on every launch):
  // made once per device and size
  static size_t opted[16] = {};
  int dev = 0;
  if (a.lds_bytes > 64 * 1024 && hipGetDevice(&dev) == hipSuccess && a.lds_bytes > opted[dev & 15]) {
    const hipError_t e = optin_lds((const void*)k_solve_blk<M, QP, NW>, a.lds_bytes);
    if (e != hipSuccess) return e;
    opted[dev & 15] = a.lds_bytes;
  }
  hipLaunchKernelGGL((k_solve_blk<M, QP, NW>), dim3(a.batch), dim3(64 * NW), a.lds_bytes, a.stream, a.bundle, a.ws,
                     a.pol, a.upred, a.xpred, a.bw, a.J, a.status, a.iters, a.batch, a.blk_lay, a.blk_hot_off);
  return hipGetLastError();
}
#ifndef BMPC_BLK_ALLOW2
#define BMPC_BLK_ALLOW2 0
#endif
// tools-only A/B (-DBMPC_BLK_ALLOW2): BMPC_BLOCK_WAVES=2 runs the small-batch kernel on two waves per ego
constexpr bool kAllowTwoWaves = BMPC_BLK_ALLOW2 != 0;
// (the OSQP-class controllers never take this path: bmpc_hip.hip chooses it for the CVaR IPM only)
template <class M, bool WITH_QP>
hipError_t launch_solver_blk(const SolveLaunch& a) {
  if (a.qp) return hipErrorInvalidValue;
  if constexpr (kAllowTwoWaves) {
    if (a.nw == 2) return launch_blk_kernel<M, false, 2>(a);
  }
  return a.nw == 8 ? launch_blk_kernel<M, false, 8>(a) : launch_blk_kernel<M, false, 4>(a);
}

// The launchers of one model, as bmpc_hip.hip's launchers_for hands them out: the solve's tree and
// solver launches (bmpc_k_<model>.hip) and the small-batch solver (bmpc_kb_<model>.hip, built with
// BMPC_FLAT_SLAB).
struct ModelLaunchers {
  LaunchFn *tree, *solver, *solver_blk;
  LaunchFn* phased;   // the phase-per-kernel IPM of tools-only builds, or null
};
LaunchFn launch_tree_highway, launch_solver_highway, launch_solver_blk_highway;
LaunchFn launch_tree_highway_t, launch_solver_highway_t, launch_solver_blk_highway_t;
LaunchFn launch_tree_merge, launch_solver_merge, launch_solver_blk_merge;
LaunchFn launch_tree_quadruped, launch_solver_quadruped, launch_solver_blk_quadruped;
// the fused closed loops (bmpc_k_highway.hip, bmpc_k_merge_loop.hip, bmpc_k_quad_loop.hip,
// bmpc_k_highway_qp_loop.hip: the overtake scene under an OSQP-class controller)
hipError_t launch_loop_highway(const SolveLaunch& a, const bmpc_env_desc& env, int t0, int nsteps, double* scene,
                               double* stats);
hipError_t launch_loop_merge(const SolveLaunch& a, const bmpc_merge_env_desc& env, const MergeRef& ref, int t0,
                             int nsteps, double* scene, double* stats);
hipError_t launch_loop_quad(const SolveLaunch& a, const bmpc_quad_env_desc& env, int t0, int nsteps, double* scene,
                            double* stats);
hipError_t launch_loop_highway_qp(const SolveLaunch& a, const bmpc_env_desc& env, int t0, int nsteps, double* scene,
                                  double* stats);

#if defined(BMPC_WITH_PHASED)
// The phase-per-kernel CVaR IPM (experimental/bmpc_dev_ph.h, bmpc_kp_*.hip; tools-only builds with
// -DBMPC_WITH_PHASED): what a launch of it takes beyond SolveLaunch, and its per-model launchers.
constexpr int kMaxSub = 8;   // sub-batch streams
struct PhasedLaunch {
  int32_t* d_count = nullptr;   // egos going on per iteration [kMaxSub][maxit + 1]
  int32_t* h_count = nullptr;   // ... pinned read-back slots [kMaxSub]
  int maxit = 0;
  int ph_mode = 1;   // 1: one kernel per phase, 2: one kernel calling grouped out-of-line phases
  int nsub = 1;                   // mode 1: sub-batches, one stream each
  hipStream_t sub[kMaxSub] = {};   // their streams
  hipEvent_t sub_ev[kMaxSub + 1] = {};   // fork / join events
};
LaunchFn launch_ipm_phased_highway, launch_ipm_phased_highway_t, launch_ipm_phased_merge;
#endif

}  // namespace dev
}  // namespace bmpc
