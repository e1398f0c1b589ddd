// bmpc_hip.hip -- the C ABI of libbmpc.so (include/bmpc.h) and the small kernels (scene step,
// model / HMM evaluation, band QP, slab gather / scatter).  The solver kernels live in
// bmpc_dev.h / bmpc_k_*.hip.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "bmpc_dev.h"
#include "bmpc_resample.h"

using namespace bmpc;
using namespace bmpc::dev;

namespace {

// LDS-rich launch (topology tables and coupling system in LDS) only when it costs no
// resident ego: a workgroup's LDS bounds the egos per CU (160 KB / bytes, at most 16 with 4
// waves per SIMD).  Deep trees (N=30, NB=2: 17 KB of tables, a 20 KB coupling matrix) run
// lean, 16 egos per CU instead of 4, unless the batch is resident either way.  BMPC_LDS_RICH=0/1
// forces either.
// lin: the launch reads the linearisation cache (choose_launch): priced with it.
static bool choose_lds_rich(const Plan& P, bool transform, int batch, int cus, size_t lds_per_cu, bool lin) {
  if (const char* e = getenv("BMPC_LDS_RICH")) return atoi(e) != 0;
  auto egos = [&](size_t b) { return std::min<size_t>(16, lds_per_cu / std::max<size_t>(b, 1)); };
  const size_t rich = egos(solver_lds_bytes(P, transform, true, lin));
  // a batch that is resident either way (one CU per `rich` egos) runs rich: residency is not
  // what limits it
  return (size_t)batch <= (size_t)cus * rich || rich >= egos(solver_lds_bytes(P, transform, false, lin));
}

// one thread per ego: the closed-loop scene step (bmpc_env.h) around the solve.  smp: the plan's
// obstacle sampler (mode 0: the argmax rule), mc: the plan's model constants on the device, opt: the
// plan's device block of scene options (null: none; bmpc_env.h SceneOptions -- the obstacle proposal,
// read by the weighted modes only, the actuation disturbance and the observation model)
__global__ void k_env(bmpc_env_desc E, double dt, int N, int m, int U, int d, int t, int batch, double* scene,
                      bmpc_policy* pol, const double* upred, const double* J, const int32_t* status,
                      const int32_t* iters, int cvar, double* x, double* z, double* xref, double* stats,
                      bmpc_obstacle_sampling smp, const double* mc, const SceneOptions* opt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= batch) return;
  double* st = scene + (size_t)e * ENV_STRIDE;
  if (t > 0 && stats && J && status && iters)
    env_accumulate(st, J[e], status[e], iters[e], cvar != 0, stats + (size_t)e * ENVS_STRIDE);
  env_step_ego(E, dt, N, m, t, st, pol + (size_t)e * m, upred ? upred + (size_t)e * U * d : nullptr,
               x + (size_t)e * 4, z + (size_t)e * 4, xref + (size_t)e * 4, &smp, mc, e, scene_prop(opt),
               scene_dist(opt), scene_obs(opt));
}

// one thread per ego: the merge scene step (bmpc_env_merge.h) around the solve; S, bx and their
// flags go straight into the ego's transform slots (no bmpc_set_transform before the solve)
__global__ void k_env_merge(const Bundle* __restrict__ B, bmpc_merge_env_desc E, MergeRef R, int t, int batch,
                            double* scene, double* ws, const double* upred, const double* J, const int32_t* status,
                            const int32_t* iters, double* x, double* z, double* xref, double* stats,
                            const SceneOptions* opt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  double* st = scene + (size_t)e * ENV_STRIDE;
  if (t > 0 && stats && J && status && iters)
    env_accumulate(st, J[e], status[e], iters[e], true, stats + (size_t)e * ENVS_STRIDE);
  merge_env_step_slab(E, R, P, L, t, st, ws + L.stride * (size_t)e, upred ? upred + (size_t)e * P.U * P.d : nullptr,
                      x + (size_t)e * 4, z + (size_t)e * 4, xref + (size_t)e * 4, opt, e);
}

// one thread per ego: the quadruped scene step (bmpc_env_quad.h) around the solve of an OSQP-class
// controller (status 1 = solved)
__global__ void k_env_quad(const Bundle* __restrict__ B, bmpc_quad_env_desc E, int t, int batch, double* scene,
                           const bmpc_policy* pol, const double* upred, const double* J, const int32_t* status,
                           const int32_t* iters, double* x, double* z, double* xref, double* stats,
                           bmpc_obstacle_sampling smp, const SceneOptions* opt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= batch) return;
  const Plan& P = B->P;
  double* st = scene + (size_t)e * ENV_STRIDE;
  if (t > 0 && stats && J && status && iters)
    env_accumulate(st, J[e], status[e], iters[e], false, stats + (size_t)e * ENVS_STRIDE);
  quad_env_step_ego(E, P.desc.mc, P.desc.dt, P.N, P.m, t, st, pol + (size_t)e * P.m,
                    upred ? upred + (size_t)e * P.U * P.d : nullptr, x + (size_t)e * 3, z + (size_t)e * 3,
                    xref + (size_t)e * 3, &smp, e, scene_prop(opt), scene_dist(opt), scene_obs(opt));
}

// One wave per ego: step t's row of the closed loops' recorder after the per-step launches (run_loop)
// -- the fused k_loop's writer (record_ego_row) on the loop's buffers and the slab, so the same
// bits.  A wave per ego, not a flat grid over elements: the grid and the lane striding are the
// solver kernels' own, each row goes out in contiguous 512-byte segments, and the offsets are
// computed once per ego, not per element.  The host launches it only for a step inside the window.
__global__ __launch_bounds__(64) void k_loop_record(const Bundle* __restrict__ B, const double* __restrict__ ws,
                                                    bmpc_loop_record R, int t, int batch, const double* scene,
                                                    const double* xref, const double* upred, const double* J,
                                                    const int32_t* status, const int32_t* iters) {
  const int e = blockIdx.x;
  size_t r;
  if (e >= batch || !record_row_of(R, t, &r)) return;
  const Plan& P = B->P;
  const Layout& L = B->L;
  record_ego_row(R, P, L, e, r, ws + L.stride * (size_t)e, scene + (size_t)e * ENV_STRIDE, xref + (size_t)e * P.n,
                 upred + (size_t)e * P.U * P.d, J + e, status + e, iters + e);
}

__global__ void k_gather(const double* __restrict__ ws, size_t stride, size_t off, int count,
                         double* __restrict__ out, int batch) {
  const size_t tot = (size_t)batch * count;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i / count, j = i % count;
    out[i] = ws[e * stride + off + j];
  }
}

__global__ void k_scatter(double* __restrict__ ws, size_t stride, size_t off, int count,
                          const double* __restrict__ in, const uint8_t* __restrict__ mask, int batch) {
  const size_t tot = (size_t)batch * count;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i / count, j = i % count;
    if (!mask || mask[e]) ws[e * stride + off + j] = in[i];
  }
}

__global__ void k_reset(double* ws, size_t stride, size_t off, const uint8_t* mask, int batch) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < batch && (!mask || mask[e])) ws[e * stride + off + MISC_INIT] = 0.0;
}

// ---- population resampling (bmpc_resample.h holds the per-element rules) ---------------------------
// One workgroup of kPopThreads threads walks the population in tiles of kPopThreads egos (coalesced
// loads, a running carry between tiles): at most 2^20 egos, a handful of passes -- a second
// workgroup would need a device-wide boundary between the passes and buy nothing at these sizes.
constexpr int kPopThreads = 1024;
constexpr int kPopWaves = kPopThreads / 64;

// inclusive scan of v over the workgroup; *total = the workgroup's sum.  sh: kPopWaves slots.
__device__ __forceinline__ uint64_t pop_block_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = wave_scan_u64(v);
  __syncthreads();   // the previous use of sh is over
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int w = 0; w < kPopWaves; ++w) {
    const uint64_t s = sh[w];
    before += w < wave ? s : 0;
    all += s;
  }
  *total = all;
  return before + incl;
}

// the workgroup's max of v (NaN-free) in every thread.  sh: kPopThreads doubles.
__device__ __forceinline__ double pop_block_max(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kPopThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  return sh[0];
}

// the workgroup's sum of a 128-bit integer in every thread.  sh: 2 * kPopThreads uint64.
__device__ __forceinline__ u128 pop_block_sum128(u128 v, uint64_t* sh) {
  __syncthreads();
  sh[2 * threadIdx.x] = (uint64_t)v;
  sh[2 * threadIdx.x + 1] = (uint64_t)(v >> 64);
  __syncthreads();
  for (int s = kPopThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const u128 a = ((u128)sh[2 * threadIdx.x + 1] << 64) | sh[2 * threadIdx.x];
      const u128 b = ((u128)sh[2 * (threadIdx.x + s) + 1] << 64) | sh[2 * (threadIdx.x + s)];
      const u128 c = a + b;
      sh[2 * threadIdx.x] = (uint64_t)c;
      sh[2 * threadIdx.x + 1] = (uint64_t)(c >> 64);
    }
    __syncthreads();
  }
  return ((u128)sh[1] << 64) | sh[0];
}

// bmpc_population_ancestors: log-weights -> ancestors, the k used and the info vector.  C, Pk: scratch
// of `batch` uint64 each (the prefix sums of k, then of the packed (dead, surplus) pairs).
__global__ __launch_bounds__(kPopThreads) void k_pop_ancestors(bmpc_resample_desc D, int batch,
                                                               const double* __restrict__ logw, int stride,
                                                               int32_t* __restrict__ anc, uint64_t* __restrict__ weight,
                                                               double* __restrict__ info, uint64_t* C, uint64_t* Pk) {
  __shared__ uint64_t sh[2 * kPopThreads];
  const int tid = threadIdx.x;
  // pass 1: the maximum, and whether any log-weight refuses the resampling
  double mx = -INFINITY;
  uint64_t bad = 0;
  for (int i = tid; i < batch; i += kPopThreads) {
    const double lw = logw[(size_t)i * stride];
    bad += resample_bad_logw(lw) ? 1 : 0;
    mx = lw > mx && lw < INFINITY ? lw : mx;
  }
  const double M = pop_block_max(mx, reinterpret_cast<double*>(sh));
  const uint64_t nbad = (uint64_t)pop_block_sum128(bad, sh);
  uint64_t S = 0;
  double ess = 0.0, lw_new = 0.0;
  bool resampled = false;
  if (nbad == 0 && M > -INFINITY) {
    // pass 2: quantise, scan, sum of squares
    u128 q = 0;
    for (int base = 0; base < batch; base += kPopThreads) {
      const int i = base + tid;
      const uint64_t k = i < batch ? resample_quantise(logw[(size_t)i * stride], M) : 0;
      if (i < batch && weight) weight[i] = k;
      q += (u128)k * k;
      uint64_t total;
      const uint64_t incl = pop_block_scan(k, sh, &total);
      if (i < batch) C[i] = S + incl;
      S += total;
    }
    const u128 Q = pop_block_sum128(q, sh);
    ess = resample_ess(S, Q);
    lw_new = resample_new_logw(M, S, batch);
    resampled = ess < D.ess_fraction * (double)batch;
  } else if (weight) {
    for (int i = tid; i < batch; i += kPopThreads) weight[i] = 0;
  }
  uint64_t dead = 0;
  if (!resampled) {
    for (int i = tid; i < batch; i += kPopThreads) anc[i] = i;
  } else {
    // pass 3: children per slot from the prefix sums, the packed (dead, surplus) scan
    __syncthreads();   // C is complete
    const u128 U0 = resample_offset(resample_u53(D.seed, (uint64_t)D.ego_base, D.round), S);
    uint64_t carry = 0;
    for (int base = 0; base < batch; base += kPopThreads) {
      const int i = base + tid;
      uint64_t v = 0;
      if (i < batch) {
        const int hi = resample_children_below(C[i], S, U0, batch);
        const int lo = i ? resample_children_below(C[i - 1], S, U0, batch) : 0;
        v = resample_pack(hi - lo);
      }
      uint64_t total;
      const uint64_t incl = pop_block_scan(v, sh, &total);
      if (i < batch) Pk[i] = carry + incl;
      carry += total;
    }
    dead = carry >> 32;
    // pass 4: the arrangement
    __syncthreads();   // Pk is complete
    for (int i = tid; i < batch; i += kPopThreads) anc[i] = resample_arrange(Pk, batch, i);
  }
  if (tid == 0) {
    info[0] = resampled ? 1.0 : 0.0;
    info[1] = ess;
    info[2] = M;
    info[3] = lw_new;
    info[4] = (double)S;
    info[5] = (double)(batch - (int)dead);
    info[6] = (double)nbad;
    info[7] = 0.0;
  }
}

// bmpc_gather_egos, pass 1 and pass 2: one workgroup per ego (bmpc_resample.h, gather_stage_ego /
// gather_commit_ego).  flag: null, or the info vector of the resampling that made `anc` -- nothing
// moves when its "resampled" entry is 0.
__global__ __launch_bounds__(256) void k_ego_stage(GatherList G, const int32_t* __restrict__ anc,
                                                   uint32_t* __restrict__ stage, const double* flag) {
  if (flag && flag[0] == 0.0) return;
  gather_stage_ego(G, anc, stage, blockIdx.x, threadIdx.x, blockDim.x);
}
__global__ __launch_bounds__(256) void k_ego_commit(GatherList G, const int32_t* __restrict__ anc,
                                                    const uint32_t* __restrict__ stage, const double* flag) {
  if (flag && flag[0] == 0.0) return;
  gather_commit_ego(G, anc, stage, blockIdx.x, threadIdx.x, blockDim.x);
}

// bmpc_resample_device's last stage: the log of the mean weight into every ego's BMPC_ENV_LOGW
__global__ void k_pop_set_logw(double* scene, int batch, const double* info) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < batch && info[0] != 0.0) scene[(size_t)e * ENV_STRIDE + BMPC_ENV_LOGW] = info[3];
}

template <class M>
__global__ void k_model(bmpc_plan_desc D, const bmpc_policy* pol, int B, const double* x,
                        const double* u, const double* z, double* A, double* Bm, double* C,
                        double* xp, double* p, double* dp, double* zpred, double* h0, double* dh,
                        LaneRef R) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = D.n, d = D.d, m = D.m, N = D.N;
#define OFF(ptr, k) (ptr ? ptr + (size_t)b * (k) : nullptr)
  model_eval_point<M>(D, pol + (size_t)b * m, x + b * n, u + b * d, z + b * n, OFF(A, n * n),
                      OFF(Bm, n * d), OFF(C, n), OFF(xp, n), OFF(p, m), OFF(dp, m * n),
                      OFF(zpred, N * m * n), OFF(h0, 1), OFF(dh, n), R);
#undef OFF
}

bool is_psiref(int kind) {
  return kind == BMPC_POL_MAINTAIN_PSIREF || kind == BMPC_POL_MAINTAIN_TRACKV_PSIREF ||
         kind == BMPC_POL_BRAKE_PSIREF;
}

// a lane reference as bmpc_model_eval_ref / bmpc_set_lane_ref take it; "" when valid
std::string check_lane_ref(int nref, const double* grid, const double* values) {
  if (nref == 0) return "";
  if (nref < 2 || nref > BMPC_MAX_LANE_REF) return "lane reference: need 2 <= nref <= BMPC_MAX_LANE_REF";
  if (!grid || !values) return "lane reference: null grid / values";
  for (int i = 0; i + 1 < nref; ++i)
    if (!(grid[i + 1] > grid[i])) return "lane reference: the grid must be strictly increasing";
  for (int i = 0; i < nref; ++i)
    if (!std::isfinite(grid[i]) || !std::isfinite(values[i])) return "lane reference: non-finite entry";
  return "";
}

__global__ void k_hmm(int M, int m, const double* __restrict__ hc, int B, const double* xb, const double* u,
                      const double* xbackup, double* xbp, double* A, double* Bm, double* C, double* h0,
                      double* Jh) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const int nb = 4 + M * m;
#define OFF(ptr, k) (ptr ? ptr + (size_t)p * (k) : nullptr)
  hmm_linearize(M, m, hc, xb + (size_t)p * nb, u + (size_t)p * 2, xbackup + (size_t)p * M * m * 4, OFF(xbp, nb),
                OFF(A, nb * nb), OFF(Bm, nb * 2), OFF(C, nb), OFF(h0, M * m), OFF(Jh, M * m * nb));
#undef OFF
}

// one wave per QP of the batch (bmpc_bandqp.h); d's tables are device pointers
__global__ __launch_bounds__(64) void k_bandqp(BandQPDesc d, const double* __restrict__ vals,
                                               const double* __restrict__ cvals, double* __restrict__ ws,
                                               double* x, double* y, int32_t* status, int32_t* iters, int batch) {
  const int b = blockIdx.x;
  if (b >= batch) return;
  extern __shared__ double lds_dyn[];
  const DevExec ex{(int)threadIdx.x, (ldouble*)lds_dyn, nullptr, nullptr};
  const int st = bandqp_solve(ex, d, vals + (size_t)b * d.nvals, cvals + (size_t)b * d.ncvals, ws + d.stride * b,
                              x + (size_t)b * d.n, y + (size_t)b * d.m, iters ? iters + b : nullptr);
  if (threadIdx.x == 0) status[b] = st;
}

// plans whose solves take S / Fx / bx (bmpc_set_transform, bmpc_set_fx)
bool plan_takes_transform(const Plan& P) {
  return P.desc.model == BMPC_MODEL_HIGHWAY_MERGE ||
         (P.desc.model == BMPC_MODEL_HIGHWAY && (P.desc.flags & BMPC_PLAN_TRANSFORM));
}

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHECK(expr)                                                                      \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) return fail(-5, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// device buffer owned by the scope (every early return of a HIPCHECK frees it)
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// host array -> fresh device copy (or null when the host pointer is null)
hipError_t upload(DevBuf& b, const void* host, size_t bytes) {
  if (!host) return hipSuccess;
  hipError_t e = b.alloc(bytes);
  if (e != hipSuccess) return e;
  return hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice);
}

}  // namespace

namespace {
// A grow-only device buffer (reallocated only when a call needs more).
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() {
    if (p) hipFree(p);
  }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// bmpc_qp_solve's analyses, keyed by everything bandqp_analyse reads except the bound
// values: the pattern, the row classes, max_iter, eps and the factor-in-LDS choice.  A caller
// such as PredictiveControllers.MPC or Highway_env re-solves one pattern every control step:
// the ordering, the scatter lists and their device copy are made once.
struct QPCacheEntry {
  std::vector<int32_t> key;
  double eps = 0;
  HostBandQP h;
  GrowBuf tab;
  uint64_t used = 0;
};

// A plan's share of the phase-per-kernel IPM (experimental/bmpc_dev_ph.h: mode 1 one kernel per
// IPM phase, the factored coupling system re-read into LDS by every kernel that solves with it;
// modes 2 / 3 one kernel calling grouped phase functions).  Tools-only builds; the product's
// plans carry the empty stand-in.
#if defined(BMPC_WITH_PHASED)
#ifndef BMPC_IPM_PHASED_DEFAULT
#define BMPC_IPM_PHASED_DEFAULT 0
#endif
#ifndef BMPC_PH_STREAMS_DEFAULT
#define BMPC_PH_STREAMS_DEFAULT 4
#endif
#define BMPC_PHASED_FN(model) launch_ipm_phased_##model
struct PhasedPlan {
  PhasedLaunch l;
  int create(int maxit) {
    l.maxit = maxit;
    if (hipMalloc(&l.d_count, sizeof(int32_t) * kMaxSub * (size_t)(maxit + 1)) != hipSuccess ||
        hipHostMalloc(&l.h_count, sizeof(int32_t) * kMaxSub) != hipSuccess)
      return fail(-12, "hipMalloc failed (out of device memory?)");
    for (auto& q : l.sub)
      if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) return fail(-5, "hipStreamCreate failed");
    for (auto& e : l.sub_ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(-5, "hipEventCreate failed");
    return 0;
  }
  void destroy() {
    hipFree(l.d_count);
    if (l.h_count) hipHostFree(l.h_count);
    for (auto& q : l.sub)
      if (q) {
        hipStreamSynchronize(q);
        hipStreamDestroy(q);
      }
    for (auto& e : l.sub_ev)
      if (e) hipEventDestroy(e);
  }
  // The launch's phased part: BMPC_IPM_PHASED (0: monolithic k_ipm) and BMPC_PH_STREAMS (mode 1's
  // sub-batch streams; 1 = all on the solve's stream).  Large LDS-rich CVaR batches (`eligible`)
  // of a model that has it take the phased launcher instead of `solver`.
  void fill(SolveLaunch& a, bool eligible, LaunchFn*& solver, LaunchFn* phased) {
    const char* e = getenv("BMPC_IPM_PHASED");
    l.ph_mode = e ? atoi(e) : BMPC_IPM_PHASED_DEFAULT;
    e = getenv("BMPC_PH_STREAMS");
    l.nsub = e ? atoi(e) : BMPC_PH_STREAMS_DEFAULT;
    a.ph = &l;
    if (eligible && phased && l.ph_mode != 0) solver = phased;
  }
};
#else
#define BMPC_PHASED_FN(model) nullptr
struct PhasedPlan {
  int create(int) { return 0; }
  void destroy() {}
  void fill(SolveLaunch&, bool, LaunchFn*&, LaunchFn*) {}
};
#endif
}  // namespace

struct bmpc_ctx {
  int device;
  int cus;             // compute units (hipDeviceProp_t::multiProcessorCount)
  size_t lds_per_cu;   // LDS bytes per CU (maxSharedMemoryPerMultiProcessor)
  size_t lds_per_block = 0;      // LDS bytes one workgroup may opt in to (sharedMemPerBlockOptin)
  unsigned long long lds_flat0 = 0;   // flat address of LDS offset 0 (k_lds_aperture), 0 = not probed
  // bmpc_qp_solve: its own stream (synchronised alone, never the device), the analysis cache
  // and grow-only buffers reused across calls
  hipStream_t qstream = nullptr;
  static constexpr int kQPCache = 8;
  std::vector<std::unique_ptr<QPCacheEntry>> qcache;
  uint64_t qclock = 0;
  GrowBuf q_in, q_ws, q_out, q_aux;
  std::vector<double> q_host;
  // bmpc_hmm_eval / bmpc_qp_solve / bmpc_model_eval share the staging buffers, the stream and
  // the QP cache above; ctypes releases the GIL during a call, so calls from several host
  // threads on one context are serialised here
  std::mutex q_mu;
  // bmpc_population_ancestors: its scratch (the two scans) and the event that orders one call's use
  // of it before the next call's, whichever streams they run on
  GrowBuf r_scratch;
  hipEvent_t r_done = nullptr;
  ~bmpc_ctx() {
    if (r_done) hipEventDestroy(r_done);
    if (qstream) hipStreamDestroy(qstream);
  }
};

struct bmpc_plan {
  bmpc_ctx* ctx;
  HostPlan hp;
  int batch;
  Bundle* d_bundle = nullptr;
  int32_t* d_tables = nullptr;
  double* d_ws = nullptr;
  bmpc_policy* d_pol = nullptr;
  std::vector<bmpc_policy> h_pol;
  double* d_in = nullptr;     // x | z | xref staging
  double* d_out = nullptr;    // upred | xpred | bw | J staging
  int32_t* d_iout = nullptr;  // status | iters
  double* d_scratch = nullptr;
  size_t scratch_len = 0;
  hipStream_t stream = nullptr;
  hipStream_t user_stream = nullptr;
  bool timing = false;
  // timing ring: three events per instrumented solve, read back only when the ring is full
  // or bmpc_timing is called, so timed solves run without a host synchronisation
  static constexpr int kTimeSlots = 32;
  hipEvent_t ev[3 * kTimeSlots] = {};
  int t_pending = 0;
  double t_acc[2] = {0, 0};
  int t_cnt = 0;
  bool pol_on_device = false;   // bmpc_env_step re-targeted d_pol: h_pol is stale
  int last_kernel = BMPC_KERNEL_NONE;   // solver kernel of the last launch (BMPC_INFO_SOLVER)
  bool last_lin = false;                // ... and whether it read the linearisation cache (bmpc_last_lin_cache)
  double* d_lref = nullptr;   // lane reference of the *_PSIREF policies (grid | values)
  // small-batch kernel: per-ego layouts with LDS-resident spans (blk_layouts), built on the first
  // small-batch solve for this plan's LDS base
  Layout* d_blk_lay = nullptr;
  size_t blk_lay_base = 0, blk_hot_off = 0, blk_hot_bytes = 0;
  bool psiref = false;        // some policy in force tracks the lane reference
  // the merge scene (bmpc_set_merge_scene): its constants and lane references (grid | refY | refpsi)
  bmpc_merge_env_desc menv = {};
  double* d_mref = nullptr;
  int n_mref = 0;   // 0: no merge scene set
  bmpc_loop_record rec = {};   // the closed loops' recorder (bmpc_set_loop_record; capacity 0: none)
  bmpc_obstacle_sampling smp = {};   // the scenes' obstacle sampler (bmpc_set_obstacle_sampling; mode 0: none)
  // the obstacle proposal (bmpc_set_obstacle_proposal), the actuation disturbance (bmpc_set_disturbance)
  // and the observation model (bmpc_set_observation): the host copies, and the device block of the
  // three that the scene kernels read through one pointer (allocated at the first attach of any;
  // has_prop / has_dist / has_obs false: none attached -- the block's disturbance / observation then
  // has law NONE)
  bmpc_obstacle_proposal prop = {};
  bmpc_disturbance dist = {};
  bmpc_observation obs = {};
  SceneOptions* d_opt = nullptr;
  bool has_prop = false, has_dist = false, has_obs = false;
  uint64_t* d_rs = nullptr;   // bmpc_resample_device's scans (2 * batch uint64, allocated at the first call)
  PhasedPlan ph;   // (empty but in tools-only builds)
};

// the stream a call works on: the caller's, remembered for drain(), or the plan's own
static hipStream_t plan_stream(bmpc_plan* pl, void* stream) {
  if (stream) pl->user_stream = (hipStream_t)stream;
  return stream ? (hipStream_t)stream : pl->stream;
}

// waits for the plan's stream, then for the last caller stream: whoever rewrites device state
// that launches read (policies, lane references, scene tables) drains first
static int drain(bmpc_plan* pl) {
  HIPCHECK(hipStreamSynchronize(pl->stream));
  if (pl->user_stream) HIPCHECK(hipStreamSynchronize(pl->user_stream));
  return 0;
}

// the options pointer the scene kernels get: the plan's device block, or null when neither a proposal
// nor a disturbance nor an observation model is attached
static const SceneOptions* scene_options(const bmpc_plan* pl) {
  return pl->has_prop || pl->has_dist || pl->has_obs ? pl->d_opt : nullptr;
}

// the plan's host copies into its device block, allocated at the first call, after draining the
// plan's streams: no scene step in flight reads the old block
static int upload_scene_options(bmpc_plan* pl, const bmpc_obstacle_proposal& prop, const bmpc_disturbance& dist,
                                const bmpc_observation& obs) {
  HIPCHECK(hipSetDevice(pl->ctx->device));
  if (const int rc = drain(pl)) return rc;
  if (!pl->d_opt) HIPCHECK(hipMalloc(&pl->d_opt, sizeof(SceneOptions)));
  SceneOptions h;
  h.prop = prop;
  h.dist = dist;
  h.obs = obs;
  HIPCHECK(hipMemcpy(pl->d_opt, &h, sizeof(h), hipMemcpyHostToDevice));
  return 0;
}

// "" when the plan's sampler is not in mode BMPC_OBS_SCRIPT or its script covers every epoch of the
// closed-loop steps [t0, t0 + nsteps) (t0 >= 0, nsteps >= 1): checked on the host by every entry that
// steps a scene, before anything is enqueued
static std::string check_script_covers(const bmpc_plan* pl, int t0, int nsteps) {
  if (pl->smp.mode != BMPC_OBS_SCRIPT) return "";
  const long long first = t0 / pl->smp.hold, last = ((long long)t0 + nsteps - 1) / pl->smp.hold;
  const long long lo = pl->prop.epoch0, hi = lo + pl->prop.script_epochs;
  if (pl->has_prop && first >= lo && last < hi) return "";
  return "the script covers epochs " + std::to_string(lo) + ".." + std::to_string(hi - 1) + ", steps " +
         std::to_string(t0) + ".." + std::to_string((long long)t0 + nsteps - 1) + " need epochs " +
         std::to_string(first) + ".." + std::to_string(last) + " (bmpc_set_obstacle_proposal)";
}

// the plan's constants and layout, with the table and lane-reference pointers at their device
// copies, into the device Bundle the kernels read
static hipError_t upload_bundle(bmpc_plan* pl) {
  Bundle hb;
  hb.P = pl->hp.plan;
  hb.L = pl->hp.lay;
  HostPlan tmp = pl->hp;       // re-point the table pointers at the device copy
  tmp.point_tables(pl->d_tables);
  hb.P.t = tmp.plan.t;
  hb.P.lref = pl->d_lref;
  return hipMemcpy(pl->d_bundle, &hb, sizeof(Bundle), hipMemcpyHostToDevice);
}

extern "C" {

const char* bmpc_last_error(void) { return g_err.c_str(); }
int bmpc_abi_version(void) { return BMPC_ABI_VERSION; }
int bmpc_last_lin_cache(const bmpc_plan* pl) { return pl && pl->last_lin ? 1 : 0; }

int bmpc_open(int hip_device, bmpc_ctx** out) {
  if (!out) return fail(-22, "null output pointer");
  int ndev = 0;
  HIPCHECK(hipGetDeviceCount(&ndev));
  if (hip_device < 0 || hip_device >= ndev) return fail(-19, "no such HIP device");
  HIPCHECK(hipSetDevice(hip_device));
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, hip_device));
  const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const size_t lds = prop.maxSharedMemoryPerMultiProcessor > 0 ? prop.maxSharedMemoryPerMultiProcessor : 160 * 1024;
  bmpc_ctx* c = new bmpc_ctx;
  c->device = hip_device;
  c->cus = cus;
  c->lds_per_cu = lds;
  c->lds_per_block = prop.sharedMemPerBlockOptin > 0 ? std::min(prop.sharedMemPerBlockOptin, lds) : lds;
  *out = c;
  return 0;
}

int bmpc_close(bmpc_ctx* ctx) {
  delete ctx;
  return 0;
}

int bmpc_plan_create(bmpc_ctx* ctx, const bmpc_plan_desc* desc, int batch, bmpc_plan** out) {
  if (!ctx || !desc || !out) return fail(-22, "null argument");
  if (batch <= 0) return fail(-22, "batch must be positive");
  HIPCHECK(hipSetDevice(ctx->device));
  bmpc_plan* pl = new bmpc_plan();
  pl->ctx = ctx;
  pl->batch = batch;
  std::string err = build_plan(*desc, pl->hp);
  if (!err.empty()) {
    delete pl;
    return fail(-22, err);
  }
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  auto cleanup = [&](int rc) {
    bmpc_plan_destroy(pl);
    return rc;
  };
  if (hipMalloc(&pl->d_tables, pl->hp.blob.size() * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&pl->d_bundle, sizeof(Bundle)) != hipSuccess ||
      hipMalloc(&pl->d_ws, L.stride * (size_t)batch * sizeof(double)) != hipSuccess ||
      hipMalloc(&pl->d_pol, sizeof(bmpc_policy) * (size_t)batch * P.m) != hipSuccess ||
      hipMalloc(&pl->d_in, sizeof(double) * (size_t)batch * P.n * 3) != hipSuccess ||
      hipMalloc(&pl->d_out, sizeof(double) * (size_t)batch * ((size_t)P.U * P.d + (size_t)P.T * P.n + P.nbranch + 1)) != hipSuccess ||
      hipMalloc(&pl->d_iout, sizeof(int32_t) * (size_t)batch * 2) != hipSuccess)
    return cleanup(fail(-12, "hipMalloc failed (out of device memory?)"));
  if (hipMemcpy(pl->d_tables, pl->hp.blob.data(), pl->hp.blob.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(-5, "hipMemcpy tables failed"));
  if (upload_bundle(pl) != hipSuccess ||
      hipMemset(pl->d_ws, 0, L.stride * (size_t)batch * sizeof(double)) != hipSuccess)
    return cleanup(fail(-5, "plan upload failed"));
  pl->h_pol.assign((size_t)batch * P.m, bmpc_policy{});
  if (hipMemcpy(pl->d_pol, pl->h_pol.data(), sizeof(bmpc_policy) * pl->h_pol.size(), hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(-5, "policy upload failed"));
  if (hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(-5, "hipStreamCreate failed"));
  for (auto& e : pl->ev)
    if (hipEventCreate(&e) != hipSuccess) return cleanup(fail(-5, "hipEventCreate failed"));
  if (const int rc = pl->ph.create(P.desc.maxit)) return cleanup(rc);
  *out = pl;
  return 0;
}

int bmpc_plan_destroy(bmpc_plan* pl) {
  if (!pl) return 0;
  hipSetDevice(pl->ctx->device);
  if (pl->stream) hipStreamSynchronize(pl->stream);
  hipFree(pl->d_tables);
  hipFree(pl->d_bundle);
  hipFree(pl->d_ws);
  hipFree(pl->d_pol);
  hipFree(pl->d_in);
  hipFree(pl->d_out);
  hipFree(pl->d_iout);
  hipFree(pl->d_scratch);
  hipFree(pl->d_lref);
  hipFree(pl->d_mref);
  hipFree(pl->d_opt);
  hipFree(pl->d_rs);
  hipFree(pl->d_blk_lay);
  for (auto& e : pl->ev)
    if (e) hipEventDestroy(e);
  pl->ph.destroy();
  if (pl->stream) hipStreamDestroy(pl->stream);
  delete pl;
  return 0;
}

int bmpc_plan_info(const bmpc_plan* pl, int32_t* info) {
  if (!pl || !info) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  info[BMPC_INFO_T] = P.T;
  info[BMPC_INFO_U] = P.U;
  info[BMPC_INFO_BDIM] = P.bdim;
  info[BMPC_INFO_NBRANCH] = P.nbranch;
  info[BMPC_INFO_NV] = P.nv;
  info[BMPC_INFO_NEQ] = P.neq;
  info[BMPC_INFO_NROWS] = P.nrows;
  info[BMPC_INFO_NCONES] = P.ncones;
  info[BMPC_INFO_LP] = P.nlp;
  info[BMPC_INFO_BATCH] = pl->batch;
  info[BMPC_INFO_WS_DOUBLES] = (int32_t)pl->hp.lay.stride;
  info[BMPC_INFO_SOLVER] = pl->last_kernel;
  return 0;
}

int bmpc_set_policies(bmpc_plan* pl, const bmpc_policy* pol, const uint8_t* mask) {
  if (!pl || !pol) return fail(-22, "null argument");
  const int m = pl->hp.plan.m;
  for (int e = 0; e < pl->batch; ++e)
    for (int i = 0; i < m; ++i)
      if ((!mask || mask[e]) && is_psiref(pol[(size_t)e * m + i].kind) &&
          pl->hp.plan.desc.model != BMPC_MODEL_HIGHWAY_MERGE)
        return fail(-22, "lane-reference (psiref) policies need a HIGHWAY_MERGE plan");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  if (pl->pol_on_device && mask) {   // keep the device-side re-targets of unmasked egos
    if (const int rc = drain(pl)) return rc;
    HIPCHECK(hipMemcpy(pl->h_pol.data(), pl->d_pol, sizeof(bmpc_policy) * pl->h_pol.size(), hipMemcpyDeviceToHost));
  }
  pl->pol_on_device = false;
  for (int e = 0; e < pl->batch; ++e)
    if (!mask || mask[e])
      memcpy(&pl->h_pol[(size_t)e * m], pol + (size_t)e * m, sizeof(bmpc_policy) * m);
  pl->psiref = false;
  for (const bmpc_policy& q : pl->h_pol) pl->psiref = pl->psiref || is_psiref(q.kind);
  HIPCHECK(hipMemcpyAsync(pl->d_pol, pl->h_pol.data(), sizeof(bmpc_policy) * pl->h_pol.size(),
                          hipMemcpyHostToDevice, pl->stream));
  HIPCHECK(hipStreamSynchronize(pl->stream));
  return 0;
}

int bmpc_get_policies(bmpc_plan* pl, bmpc_policy* pol) {
  if (!pl || !pol) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  if (const int rc = drain(pl)) return rc;
  HIPCHECK(hipMemcpy(pol, pl->d_pol, sizeof(bmpc_policy) * pl->h_pol.size(), hipMemcpyDeviceToHost));
  return 0;
}

int bmpc_reset(bmpc_plan* pl, const uint8_t* mask) {
  if (!pl) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  DevBuf d_mask;
  HIPCHECK(upload(d_mask, mask, pl->batch));
  hipLaunchKernelGGL(k_reset, dim3((pl->batch + 255) / 256), dim3(256), 0, pl->stream, pl->d_ws,
                     pl->hp.lay.stride, pl->hp.lay.misc, d_mask.as<uint8_t>(), pl->batch);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(pl->stream));
  return 0;
}

// Scatter per-ego host rows [batch][cnt] into the slab at offset off (one staging copy;
// masked egos only).  The stream is drained before the staging buffers go out of scope.
static int scatter_rows(bmpc_plan* pl, const double* src, size_t off, int cnt, const uint8_t* d_mask) {
  if (!src || cnt <= 0) return 0;
  DevBuf buf;
  HIPCHECK(upload(buf, src, sizeof(double) * (size_t)pl->batch * cnt));
  hipLaunchKernelGGL(k_scatter, dim3(512), dim3(256), 0, pl->stream, pl->d_ws, pl->hp.lay.stride, off, cnt,
                     buf.as<double>(), d_mask, pl->batch);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(pl->stream));
  return 0;
}

// A warm start: host rows [batch][cnt] into the masked egos' slabs at their offsets (null rows
// are skipped), then those slabs' MISC_INIT flag.
struct SlabPart { const double* src; size_t off; int cnt; };
static int scatter_parts(bmpc_plan* pl, std::initializer_list<SlabPart> parts, const uint8_t* mask) {
  DevBuf dmask;
  HIPCHECK(upload(dmask, mask, pl->batch));
  for (const SlabPart& pt : parts)
    if (int rc = scatter_rows(pl, pt.src, pt.off, pt.cnt, dmask.as<uint8_t>())) return rc;
  const std::vector<double> ones(pl->batch, 1.0);
  return scatter_rows(pl, ones.data(), pl->hp.lay.misc + MISC_INIT, 1, dmask.as<uint8_t>());
}

// Reads back the pending timing events (waits for the last instrumented solve).  The ring is
// emptied on every exit path: a failed read-back drops the pending samples rather than leaving
// t_pending at kTimeSlots (the next launch would index past ev[]).
static int fold_timing(bmpc_plan* pl) {
  const int pending = pl->t_pending;
  pl->t_pending = 0;
  for (int k = 0; k < pending && k < bmpc_plan::kTimeSlots; ++k) {
    hipEvent_t* ev = pl->ev + 3 * k;
    HIPCHECK(hipEventSynchronize(ev[2]));
    float a = 0, b = 0;
    HIPCHECK(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIPCHECK(hipEventElapsedTime(&b, ev[1], ev[2]));
    pl->t_acc[0] += a;
    pl->t_acc[1] += b;
    pl->t_cnt += 1;
  }
  return 0;
}

// the flat (generic) address of LDS offset 0: the LDS aperture base every workgroup's LDS is
// addressed through (the same for every kernel of the process)
__global__ void k_lds_aperture(unsigned long long* out) {
  __shared__ double s[2];
  s[threadIdx.x & 1] = 0.0;
  if (threadIdx.x == 0) out[0] = (unsigned long long)(uintptr_t)(double*)s;
}

// LDS-resident spans of the small-batch kernel (bmpc_dev.h, k_solve_blk): ego e's layout with
// spans of the IPM's own arrays offset from the ego's slab (d_ws + e * stride) to the workgroup's
// LDS after the launch's own lds_base bytes.  Spans in priority order, each kept whole (code
// addresses several fields of a span from one base) and skipped when it does not fit: the NT
// scaling (dl .. vnt), the node factors (hx .. kff), the tree solve's l and x right-hand sides
// (lvec, qx0), z / s / lambda, the tree's A / B and dh (copied in by the kernel).  Every span
// holds arrays a solve writes before it reads them (or that the kernel copies in); the scaling's
// span must fit (the kernel's guard checks it).  Returns the extra LDS bytes (0: no layouts).
static int blk_layouts(bmpc_plan* pl, size_t lds_base) {
  bmpc_ctx* c = pl->ctx;
  if (pl->d_blk_lay && pl->blk_lay_base == lds_base) return 0;
  if (!c->lds_flat0) {
    unsigned long long* d = nullptr;
    HIPCHECK(hipMalloc(&d, sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_lds_aperture, dim3(1), dim3(64), 0, pl->stream, d);
    unsigned long long h = 0;
    hipError_t e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, pl->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(pl->stream);
    hipFree(d);
    HIPCHECK(e);
    if (!h) return fail(-5, "LDS aperture probe returned 0");
    c->lds_flat0 = h;
  }
  const Layout& L = pl->hp.lay;
  const size_t off0 = ((lds_base + 63) & ~(size_t)63) / sizeof(double);
  const size_t cap = c->lds_per_block / sizeof(double);
  struct Span { size_t Layout::*a; size_t Layout::*b; };
  const Span spans[] = {{&Layout::dl, &Layout::hx},   {&Layout::hx, &Layout::lvec}, {&Layout::lvec, &Layout::qx0},
                        {&Layout::qx0, &Layout::gk},  {&Layout::z, &Layout::z1},    {&Layout::Ad, &Layout::Cd},
                        {&Layout::dh, &Layout::h0}};
  const int nsp = sizeof(spans) / sizeof(spans[0]);
  size_t at[nsp];   // LDS offset (doubles) of each relocated span, 0 = stays in the slab
  size_t cur = off0;
  for (int k = 0; k < nsp; ++k) {
    const size_t a = L.*spans[k].a, b = L.*spans[k].b;
    at[k] = 0;
    if (b <= a) continue;
    const size_t len = (b - a + 7) & ~(size_t)7;
    if (cur + len <= cap) {
      at[k] = cur;
      cur += len;
    }
  }
  if (!at[0]) return 0;   // not even the scaling fits: the plain layout
  const int B = pl->batch;
  std::vector<Layout> lays(B, L);
  const size_t nf = offsetof(Layout, stride) / sizeof(size_t);
  for (int e = 0; e < B; ++e) {
    const int64_t ws_e = (int64_t)(uintptr_t)(pl->d_ws + (size_t)e * L.stride);
    size_t* f = reinterpret_cast<size_t*>(&lays[e]);
    const size_t* f0 = reinterpret_cast<const size_t*>(&L);
    for (int k = 0; k < nsp; ++k) {
      if (!at[k]) continue;
      const size_t a = L.*spans[k].a, b = L.*spans[k].b;
      // ws_e + 8 (off + delta) = LDS(at[k] + off - a) for every field offset off in [a, b)
      const int64_t delta = ((int64_t)c->lds_flat0 + 8 * (int64_t)at[k] - ws_e) / 8 - (int64_t)a;
      for (size_t i = 0; i < nf; ++i)
        if (f0[i] >= a && f0[i] < b) f[i] = (size_t)((int64_t)f0[i] + delta);
    }
  }
  if (!pl->d_blk_lay) {
    HIPCHECK(hipMalloc(&pl->d_blk_lay, sizeof(Layout) * (size_t)B));
  } else {
    // a rebuild (the launch's LDS base changed, e.g. BMPC_BLOCK_WAVES toggled between solves):
    // a small-batch kernel still in flight reads the old layouts, on whichever stream a caller
    // that alternates streams gave it -- let the device drain before the buffer is overwritten
    HIPCHECK(hipDeviceSynchronize());
  }
  HIPCHECK(hipMemcpy(pl->d_blk_lay, lays.data(), sizeof(Layout) * (size_t)B, hipMemcpyHostToDevice));
  pl->blk_lay_base = lds_base;
  pl->blk_hot_off = at[0];
  pl->blk_hot_bytes = (cur - off0) * sizeof(double);
  return 0;
}

// How a plan's solver launches (launch_solve and the fused loops ask here and nowhere else).
struct LaunchChoice {
  int nw;             // small-batch launch (k_solve_blk): waves per ego; 0: one wave per ego
  bool rich;          // LDS-rich or lean (choose_lds_rich; the small-batch kernel is rich)
  bool lin;           // the one-wave IPM reads A from its LDS cache (bmpc_ipm.h lin_A; the plan carved it)
  size_t lds_bytes;   // dynamic LDS of the solver kernel (before the small-batch kernel's spans)
  bool blk_lds;       // small-batch launch: the IPM's arrays in LDS (blk_layouts)
  bool fused_loop;    // a closed loop runs as one k_loop launch instead of launches per step
};

// Small batches of the CVaR IPM: one ego per multi-wave workgroup (k_solve_blk) when the batch
// leaves CUs idle -- 4 waves per ego, 8 for trees of BMPC_BLK_WIDE_T state nodes or more.
// Measured at one ego (profiles/r03/r03x_blk_waves.log): N=8 NB=2 22 ms vs 30 on one wave,
// N=20 NB=1 12-14 vs 14-16, N=30 NB=2 44-49 vs 61-65.  BMPC_BLOCK_EGOS: the largest batch that
// takes this path (default: one ego per CU; 0 disables it); BMPC_BLOCK_WAVES: 4 or 8;
// BMPC_BLK_LDS=0: the small-batch kernel keeps every array in the slab.
// Larger CVaR batches may fuse a closed loop into one launch, unless a policy tracks the lane
// reference or BMPC_LOOP_FUSED=0 asks for the per-step launches (A/B).  qp_loop: the caller's loop
// has a k_loop that runs the QP solver (the quadruped loop, the overtake loop) -- its OSQP-class
// plans fuse too, at any batch (they have no small-batch kernel), except the overtake loop's robust
// plans, which keep their launches per step unless BMPC_LOOP_FUSED=2 asks for every plan that has
// a k_loop to fuse.
static LaunchChoice choose_launch(const bmpc_plan* pl, bool xform, bool qp_loop = false) {
  const Plan& P = pl->hp.plan;
  const bmpc_ctx* c = pl->ctx;
  const bool cvar = P.desc.controller == BMPC_CTRL_CVAR;
  int blk_max = c->cus;
  if (const char* e = getenv("BMPC_BLOCK_EGOS")) blk_max = atoi(e);
  LaunchChoice ch{};
  if (cvar && pl->batch <= blk_max) {
    ch.nw = P.T >= BMPC_BLK_WIDE_T ? 8 : 4;
    if (const char* e = getenv("BMPC_BLOCK_WAVES")) ch.nw = atoi(e) == 8 ? 8 : kAllowTwoWaves && atoi(e) == 2 ? 2 : 4;
    ch.rich = true;
    ch.lds_bytes = solver_lds_bytes_blk(P, xform, ch.nw);
    const char* el = getenv("BMPC_BLK_LDS");
    ch.blk_lds = !(el && atoi(el) == 0);
    return ch;
  }
  // The IPM with its linearisation cache (A from LDS, 16-bit table copy), where the plan carved one,
  // for batches beyond 8 egos per CU, as k_tree's register budget (launch_tree): those are bound by
  // the bytes the cache saves; smaller ones by latency, where the cache's selects and the narrow
  // table loads cost more than the slab reads they replace (1,024 egos +1.2%).
  // BMPC_LIN_CACHE=0/1 forces either.
  ch.lin = BMPC_LIN_LDS && cvar && P.nlin_a > 0 && pl->batch > 8 * c->cus;
  if (const char* e = getenv("BMPC_LIN_CACHE")) ch.lin = BMPC_LIN_LDS && cvar && P.nlin_a > 0 && atoi(e) != 0;
  ch.rich = choose_lds_rich(P, xform, pl->batch, c->cus, c->lds_per_cu, ch.lin);
  ch.lds_bytes = solver_lds_bytes(P, xform, ch.rich, ch.lin);
  // occupancy experiments: BMPC_IPM_LDS_BYTES reserves at least that much LDS per workgroup
  // (fewer egos resident per CU => a smaller working set in L2 / Infinity Cache)
  if (const char* e = getenv("BMPC_IPM_LDS_BYTES")) {
    const size_t want = (size_t)atol(e);
    if (want > ch.lds_bytes && want <= c->lds_per_cu) ch.lds_bytes = want;
  }
  const char* ef = getenv("BMPC_LOOP_FUSED");
  const int fuse = ef ? atoi(ef) : 1;
  const bool per_step_default = P.desc.model == BMPC_MODEL_HIGHWAY && P.desc.controller == BMPC_CTRL_ROBUST;
  ch.fused_loop = (cvar || qp_loop) && !pl->psiref && fuse != 0 && (fuse == 2 || !per_step_default);
  return ch;
}

// one solve launch of the plan as chosen, on stream s
static SolveLaunch solve_launch(const bmpc_plan* pl, const LaunchChoice& ch, hipStream_t s, const double* d_x,
                                const double* d_z, const double* d_xref, double* d_upred, double* d_xpred,
                                double* d_bw, double* d_J, int32_t* d_status, int32_t* d_iters) {
  SolveLaunch a{pl->d_bundle, pl->d_ws, pl->d_pol, d_x, d_z, d_xref, d_upred, d_xpred, d_bw, d_J, d_status,
                d_iters, pl->batch, ch.lds_bytes, ch.rich, pl->hp.plan.desc.controller != BMPC_CTRL_CVAR, s};
  if (ch.nw) a.nw = ch.nw;
  a.lin = ch.lin;
  a.cus = pl->ctx->cus;
  a.hplan = &pl->hp.plan;
  return a;
}

// The timing bracket of an instrumented launch on s: mark 0 before the tree launch, 1 between the
// two, 2 after the solver (ev[3 slot + k]); mark 2 closes the ring slot and folds a full ring.
static int timing_mark(bmpc_plan* pl, hipStream_t s, int k) {
  if (!pl->timing) return 0;
  if (pl->t_pending < 0 || pl->t_pending >= bmpc_plan::kTimeSlots)
    return fail(-5, "timing ring out of range (t_pending = " + std::to_string(pl->t_pending) + ")");
  hipEvent_t* ev = pl->ev + 3 * pl->t_pending;
  HIPCHECK(hipEventRecord(ev[k], s));
  if (k == 2 && ++pl->t_pending == bmpc_plan::kTimeSlots) return fold_timing(pl);
  return 0;
}

static const ModelLaunchers& launchers_for(const Plan& P) {
  static const ModelLaunchers hw{launch_tree_highway, launch_solver_highway, launch_solver_blk_highway,
                                 BMPC_PHASED_FN(highway)},
      hwt{launch_tree_highway_t, launch_solver_highway_t, launch_solver_blk_highway_t, BMPC_PHASED_FN(highway_t)},
      mrg{launch_tree_merge, launch_solver_merge, launch_solver_blk_merge, BMPC_PHASED_FN(merge)},
      quad{launch_tree_quadruped, launch_solver_quadruped, launch_solver_blk_quadruped, nullptr};
  // HIGHWAY plans that take solve's S / Fx / bx run the transform path of the same model
  if (P.desc.model == BMPC_MODEL_HIGHWAY) return (P.desc.flags & BMPC_PLAN_TRANSFORM) ? hwt : hw;
  return P.desc.model == BMPC_MODEL_HIGHWAY_MERGE ? mrg : quad;
}

static int launch_solve(bmpc_plan* pl, const double* d_x, const double* d_z, const double* d_xref,
                        double* d_upred, double* d_xpred, double* d_bw, double* d_J,
                        int32_t* d_status, int32_t* d_iters, hipStream_t s) {
  const Plan& P = pl->hp.plan;
  const LaunchChoice ch = choose_launch(pl, plan_takes_transform(P));
  if (pl->psiref && P.nlref == 0)
    return fail(-22, "the plan's policies track a lane reference: set it first (bmpc_set_lane_ref)");
  SolveLaunch a = solve_launch(pl, ch, s, d_x, d_z, d_xref, d_upred, d_xpred, d_bw, d_J, d_status, d_iters);
  const ModelLaunchers& ml = launchers_for(P);
  LaunchFn* solver = ch.nw ? ml.solver_blk : ml.solver;
  if (ch.nw && ch.blk_lds) {
    if (const int rc = blk_layouts(pl, a.lds_bytes)) return rc;
    if (pl->d_blk_lay) {
      a.blk_lay = pl->d_blk_lay;
      a.blk_hot_off = pl->blk_hot_off;
      a.lds_bytes = pl->blk_hot_off * sizeof(double) + pl->blk_hot_bytes;
    }
  }
  pl->ph.fill(a, !ch.nw && !a.qp && ch.rich, solver, ml.phased);
  pl->last_lin = a.lin && !a.qp;
  pl->last_kernel = ch.nw   ? (ch.nw == 8 ? BMPC_KERNEL_IPM_BLK8 : BMPC_KERNEL_IPM_BLK4)
                    : a.qp  ? (ch.rich ? BMPC_KERNEL_QP_RICH : BMPC_KERNEL_QP_LEAN)
                            : (ch.rich ? BMPC_KERNEL_IPM_RICH : BMPC_KERNEL_IPM_LEAN);
  if (const int rc = timing_mark(pl, s, 0)) return rc;
  HIPCHECK(ml.tree(a));
  if (const int rc = timing_mark(pl, s, 1)) return rc;
  HIPCHECK(solver(a));
  return timing_mark(pl, s, 2);
}

extern "C++" {
// nsteps closed-loop steps of a scene (bmpc_loop_device, bmpc_merge_loop_device): one k_loop launch
// (`fused`) for batches that choose_launch lets fuse, otherwise the scene's step (`step`) + the
// solve launches per step -- same results either way.  retargets: the scene's step rewrites d_pol;
// qp_loop: the scene's k_loop runs the QP solver (choose_launch).  The plan's recorder
// (bmpc_set_loop_record) rides along either way: k_loop takes it as an argument; the per-step path
// launches k_loop_record after each solve whose step lies in the window.  The plan's obstacle sampler
// (bmpc_set_obstacle_sampling) reaches both paths: k_loop's scene argument carries it, and `step` is
// the single-step entry point, which passes it to k_env / k_env_quad; the pointer to the plan's scene
// options -- its obstacle proposal (bmpc_set_obstacle_proposal), its disturbance (bmpc_set_disturbance)
// and its observation model (bmpc_set_observation) -- travels beside it on both, to the merge scene too.
template <class Step, class Fused>
static int run_loop(bmpc_plan* pl, bool retargets, bool qp_loop, int t0, int nsteps, double* d_scene, double* d_upred,
                    double* d_x, double* d_z, double* d_xref, double* d_J, int32_t* d_status, int32_t* d_iters,
                    void* stream, Step step, Fused fused) {
  HIPCHECK(hipSetDevice(pl->ctx->device));
  hipStream_t s = plan_stream(pl, stream);
  const LaunchChoice ch = choose_launch(pl, plan_takes_transform(pl->hp.plan), qp_loop);
  if (!ch.fused_loop) {
    for (int k = 0; k < nsteps; ++k) {
      if (int rc = step(t0 + k)) return rc;
      if (int rc = launch_solve(pl, d_x, d_z, d_xref, d_upred, nullptr, nullptr, d_J, d_status, d_iters, s)) return rc;
      size_t row;
      if (record_row_of(pl->rec, t0 + k, &row)) {
        hipLaunchKernelGGL(k_loop_record, dim3(pl->batch), dim3(64), 0, s, pl->d_bundle, pl->d_ws, pl->rec, t0 + k,
                           pl->batch, d_scene, d_xref, d_upred, d_J, d_status, d_iters);
        HIPCHECK(hipGetLastError());
      }
    }
    return 0;
  }
  SolveLaunch a = solve_launch(pl, ch, s, d_x, d_z, d_xref, d_upred, nullptr, nullptr, d_J, d_status, d_iters);
  a.rec = pl->rec;
  a.smp = pl->smp;
  a.opt = scene_options(pl);
  pl->last_lin = a.lin && !qp_loop;
  pl->last_kernel = ch.rich ? BMPC_KERNEL_LOOP_RICH : BMPC_KERNEL_LOOP_LEAN;
  // (the whole fused launch is booked as the solver's time, none as the tree's)
  if (const int rc = timing_mark(pl, s, 0)) return rc;
  if (const int rc = timing_mark(pl, s, 1)) return rc;
  HIPCHECK(fused(a));
  if (retargets) pl->pol_on_device = true;
  return timing_mark(pl, s, 2);
}
}

int bmpc_solve(bmpc_plan* pl, const double* x, const double* z, const double* xref, double* upred,
               double* xpred, double* branch_w, double* J, int32_t* status, int32_t* iters) {
  if (!pl || !x || !z || !xref) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  const size_t B = pl->batch, n = P.n;
  hipStream_t s = pl->stream;
  double* dx = pl->d_in;
  double* dz = dx + B * n;
  double* dr = dz + B * n;
  HIPCHECK(hipMemcpyAsync(dx, x, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(dz, z, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(dr, xref, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
  double* up = pl->d_out;
  double* xp = up + B * P.U * P.d;
  double* bw = xp + B * P.T * P.n;
  double* jj = bw + B * (P.nbranch - 1);
  int32_t* st = pl->d_iout;
  int32_t* it = st + B;
  int rc = launch_solve(pl, dx, dz, dr, up, xp, bw, jj, st, it, s);
  if (rc) return rc;
  if (upred) HIPCHECK(hipMemcpyAsync(upred, up, sizeof(double) * B * P.U * P.d, hipMemcpyDeviceToHost, s));
  if (xpred) HIPCHECK(hipMemcpyAsync(xpred, xp, sizeof(double) * B * P.T * P.n, hipMemcpyDeviceToHost, s));
  if (branch_w) HIPCHECK(hipMemcpyAsync(branch_w, bw, sizeof(double) * B * (P.nbranch - 1), hipMemcpyDeviceToHost, s));
  if (J) HIPCHECK(hipMemcpyAsync(J, jj, sizeof(double) * B, hipMemcpyDeviceToHost, s));
  if (status) HIPCHECK(hipMemcpyAsync(status, st, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  if (iters) HIPCHECK(hipMemcpyAsync(iters, it, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

int bmpc_solve_device(bmpc_plan* pl, const double* d_x, const double* d_z, const double* d_xref,
                      double* d_upred, double* d_xpred, double* d_branch_w, double* d_J,
                      int32_t* d_status, int32_t* d_iters, void* stream) {
  if (!pl || !d_x || !d_z || !d_xref) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  hipStream_t s = plan_stream(pl, stream);
  return launch_solve(pl, d_x, d_z, d_xref, d_upred, d_xpred, d_branch_w, d_J, d_status, d_iters, s);
}

int bmpc_env_step(bmpc_plan* pl, const bmpc_env_desc* env, int t, double* d_scene, const double* d_upred,
                  const double* d_J, const int32_t* d_status, const int32_t* d_iters, double* d_x,
                  double* d_z, double* d_xref, double* d_stats, void* stream) {
  if (!pl || !env || !d_scene || !d_x || !d_z || !d_xref) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (P.desc.model != BMPC_MODEL_HIGHWAY || P.n != 4 || P.d != 2)
    return fail(-22, "bmpc_env_step: the overtake scene needs a highway plan (n = 4, d = 2)");
  if (t < 0 || (t > 0 && !d_upred)) return fail(-22, "bmpc_env_step: t > 0 needs the last uPred");
  if (env->n_lane < 1) return fail(-22, "bmpc_env_step: n_lane < 1");
  if (const std::string e = check_script_covers(pl, t, 1); !e.empty()) return fail(-22, "bmpc_env_step: " + e);
  HIPCHECK(hipSetDevice(pl->ctx->device));
  hipStream_t s = plan_stream(pl, stream);
  hipLaunchKernelGGL(k_env, dim3((pl->batch + 63) / 64), dim3(64), 0, s, *env, P.desc.dt, P.N, P.m, P.U, P.d, t,
                     pl->batch, d_scene, pl->d_pol, d_upred, d_J, d_status, d_iters,
                     P.desc.controller == BMPC_CTRL_CVAR ? 1 : 0, d_x, d_z, d_xref, d_stats, pl->smp,
                     pl->d_bundle->P.desc.mc, scene_options(pl));
  HIPCHECK(hipGetLastError());
  pl->pol_on_device = true;
  return 0;
}

int bmpc_loop_device(bmpc_plan* pl, const bmpc_env_desc* env, int t0, int nsteps, double* d_scene, double* d_upred,
                     double* d_x, double* d_z, double* d_xref, double* d_J, int32_t* d_status, int32_t* d_iters,
                     double* d_stats, void* stream) {
  if (!pl || !env || !d_scene || !d_upred || !d_x || !d_z || !d_xref || !d_J || !d_status || !d_iters)
    return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (P.desc.model != BMPC_MODEL_HIGHWAY || (P.desc.flags & BMPC_PLAN_TRANSFORM) || P.n != 4 || P.d != 2)
    return fail(-22, "bmpc_loop_device: the overtake scene needs a highway plan (n = 4, d = 2) without transform");
  const bool qp = P.desc.controller != BMPC_CTRL_CVAR;
  if (qp && P.desc.controller != BMPC_CTRL_QP && P.desc.controller != BMPC_CTRL_ROBUST)
    return fail(-22, "bmpc_loop_device: CVaR, BranchMPC (BMPC_CTRL_QP) or robust controllers only");
  if (nsteps < 1 || t0 < 0) return fail(-22, "bmpc_loop_device: nsteps >= 1 and t0 >= 0");
  if (env->n_lane < 1) return fail(-22, "bmpc_loop_device: n_lane < 1");
  if (const std::string e = check_script_covers(pl, t0, nsteps); !e.empty())
    return fail(-22, "bmpc_loop_device: " + e);
  return run_loop(
      pl, true, qp, t0, nsteps, d_scene, d_upred, d_x, d_z, d_xref, d_J, d_status, d_iters, stream,
      [&](int t) {
        return bmpc_env_step(pl, env, t, d_scene, d_upred, d_J, d_status, d_iters, d_x, d_z, d_xref, d_stats, stream);
      },
      [&](const SolveLaunch& a) {
        return qp ? launch_loop_highway_qp(a, *env, t0, nsteps, d_scene, d_stats)
                  : launch_loop_highway(a, *env, t0, nsteps, d_scene, d_stats);
      });
}

int bmpc_set_merge_scene(bmpc_plan* pl, const bmpc_merge_env_desc* desc, int nref, const double* grid,
                         const double* refY, const double* refpsi) {
  if (!pl || !desc) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (P.desc.model != BMPC_MODEL_HIGHWAY_MERGE || P.desc.controller != BMPC_CTRL_CVAR || P.n != 4 || P.d != 2 ||
      P.nFx != 4)
    return fail(-22, "bmpc_set_merge_scene: the merge scene needs a HIGHWAY_MERGE CVaR plan (n = 4, d = 2, nFx = 4)");
  if (nref < 2) return fail(-22, "bmpc_set_merge_scene: lane reference: need 2 <= nref <= BMPC_MAX_LANE_REF");
  for (const double* v : {refY, refpsi}) {
    const std::string e = check_lane_ref(nref, grid, v);
    if (!e.empty()) return fail(-22, "bmpc_set_merge_scene: " + e);
  }
  if (desc->n_lane < 1 || desc->merge_lane < 1) return fail(-22, "bmpc_set_merge_scene: n_lane, merge_lane >= 1");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  if (const int rc = drain(pl)) return rc;   // no scene step in flight reads the old tables
  DevBuf fresh;
  HIPCHECK(fresh.alloc(sizeof(double) * 3 * (size_t)nref));
  const double* parts[] = {grid, refY, refpsi};
  for (int k = 0; k < 3; ++k)
    HIPCHECK(hipMemcpy(fresh.as<double>() + (size_t)k * nref, parts[k], sizeof(double) * nref, hipMemcpyHostToDevice));
  hipFree(pl->d_mref);
  pl->d_mref = fresh.as<double>();
  fresh.p = nullptr;   // owned by the plan now
  pl->n_mref = nref;
  pl->menv = *desc;
  return 0;
}

int bmpc_merge_env_step(bmpc_plan* pl, int t, double* d_scene, const double* d_upred, const double* d_J,
                        const int32_t* d_status, const int32_t* d_iters, double* d_x, double* d_z, double* d_xref,
                        double* d_stats, void* stream) {
  if (!pl || !d_scene || !d_x || !d_z || !d_xref) return fail(-22, "null argument");
  if (!pl->n_mref) return fail(-22, "bmpc_merge_env_step: no merge scene (bmpc_set_merge_scene)");
  if (t < 0 || (t > 0 && !d_upred)) return fail(-22, "bmpc_merge_env_step: t > 0 needs the last uPred");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  hipStream_t s = plan_stream(pl, stream);
  hipLaunchKernelGGL(k_env_merge, dim3((pl->batch + 63) / 64), dim3(64), 0, s, pl->d_bundle, pl->menv,
                     MergeRef{pl->d_mref, pl->n_mref}, t, pl->batch, d_scene, pl->d_ws, d_upred, d_J, d_status, d_iters,
                     d_x, d_z, d_xref, d_stats, scene_options(pl));
  HIPCHECK(hipGetLastError());
  return 0;
}

int bmpc_merge_loop_device(bmpc_plan* pl, int t0, int nsteps, double* d_scene, double* d_upred, double* d_x,
                           double* d_z, double* d_xref, double* d_J, int32_t* d_status, int32_t* d_iters,
                           double* d_stats, void* stream) {
  if (!pl || !d_scene || !d_upred || !d_x || !d_z || !d_xref || !d_J || !d_status || !d_iters)
    return fail(-22, "null argument");
  if (!pl->n_mref) return fail(-22, "bmpc_merge_loop_device: no merge scene (bmpc_set_merge_scene)");
  if (nsteps < 1 || t0 < 0) return fail(-22, "bmpc_merge_loop_device: nsteps >= 1 and t0 >= 0");
  return run_loop(
      pl, false, false, t0, nsteps, d_scene, d_upred, d_x, d_z, d_xref, d_J, d_status, d_iters, stream,
      [&](int t) {
        return bmpc_merge_env_step(pl, t, d_scene, d_upred, d_J, d_status, d_iters, d_x, d_z, d_xref, d_stats, stream);
      },
      [&](const SolveLaunch& a) {
        return launch_loop_merge(a, pl->menv, MergeRef{pl->d_mref, pl->n_mref}, t0, nsteps, d_scene, d_stats);
      });
}

// "" for the plans the quadruped scene runs on
static std::string check_quad_scene_plan(const Plan& P) {
  if (P.desc.model != BMPC_MODEL_QUADRUPED || P.n != 3 || P.d != 3 || P.desc.controller == BMPC_CTRL_CVAR)
    return "the quadruped scene needs a QUADRUPED plan (n = d = 3) with an OSQP-class controller";
  return "";
}

int bmpc_quad_env_step(bmpc_plan* pl, const bmpc_quad_env_desc* env, int t, double* d_scene, const double* d_upred,
                       const double* d_J, const int32_t* d_status, const int32_t* d_iters, double* d_x, double* d_z,
                       double* d_xref, double* d_stats, void* stream) {
  if (!pl || !env || !d_scene || !d_x || !d_z || !d_xref) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (const std::string e = check_quad_scene_plan(P); !e.empty()) return fail(-22, "bmpc_quad_env_step: " + e);
  if (t < 0 || (t > 0 && !d_upred)) return fail(-22, "bmpc_quad_env_step: t >= 0, and t > 0 needs the last uPred");
  if (const std::string e = check_script_covers(pl, t, 1); !e.empty()) return fail(-22, "bmpc_quad_env_step: " + e);
  HIPCHECK(hipSetDevice(pl->ctx->device));
  hipStream_t s = plan_stream(pl, stream);
  hipLaunchKernelGGL(k_env_quad, dim3((pl->batch + 63) / 64), dim3(64), 0, s, pl->d_bundle, *env, t, pl->batch, d_scene,
                     pl->d_pol, d_upred, d_J, d_status, d_iters, d_x, d_z, d_xref, d_stats, pl->smp, scene_options(pl));
  HIPCHECK(hipGetLastError());
  return 0;
}

int bmpc_quad_loop_device(bmpc_plan* pl, const bmpc_quad_env_desc* env, int t0, int nsteps, double* d_scene,
                          double* d_upred, double* d_x, double* d_z, double* d_xref, double* d_J, int32_t* d_status,
                          int32_t* d_iters, double* d_stats, void* stream) {
  if (!pl || !env || !d_scene || !d_upred || !d_x || !d_z || !d_xref || !d_J || !d_status || !d_iters)
    return fail(-22, "null argument");
  if (const std::string e = check_quad_scene_plan(pl->hp.plan); !e.empty())
    return fail(-22, "bmpc_quad_loop_device: " + e);
  if (nsteps < 1 || t0 < 0) return fail(-22, "bmpc_quad_loop_device: nsteps >= 1 and t0 >= 0");
  if (const std::string e = check_script_covers(pl, t0, nsteps); !e.empty())
    return fail(-22, "bmpc_quad_loop_device: " + e);
  return run_loop(
      pl, false, true, t0, nsteps, d_scene, d_upred, d_x, d_z, d_xref, d_J, d_status, d_iters, stream,
      [&](int t) {
        return bmpc_quad_env_step(pl, env, t, d_scene, d_upred, d_J, d_status, d_iters, d_x, d_z, d_xref, d_stats,
                                  stream);
      },
      [&](const SolveLaunch& a) { return launch_loop_quad(a, *env, t0, nsteps, d_scene, d_stats); });
}

int bmpc_set_loop_record(bmpc_plan* pl, const bmpc_loop_record* rec) {
  if (!pl) return fail(-22, "null argument");
  if (!rec) {
    pl->rec = bmpc_loop_record{};
    return 0;
  }
  if (rec->capacity < 1) return fail(-22, "bmpc_set_loop_record: capacity must be at least 1");
  if (!rec->scene || !rec->xref || !rec->u || !rec->J || !rec->status || !rec->iters)
    return fail(-22, "bmpc_set_loop_record: null core column (scene, xref, u, J, status and iters are required)");
  if (rec->zpred && pl->hp.plan.desc.controller == BMPC_CTRL_ROBUST)
    return fail(-22, "bmpc_set_loop_record: a robustMPC plan's tree keeps no zbar: zpred must be NULL");
  pl->rec = *rec;
  return 0;
}

// "" for the plans whose scene has an obstacle that chooses: overtake and quadruped scene plans
static std::string check_obstacle_chooses(const Plan& P) {
  if (P.desc.model == BMPC_MODEL_HIGHWAY_MERGE) return "the merge scene's obstacle never chooses (always backup 0)";
  if (P.desc.flags & BMPC_PLAN_TRANSFORM) return "no closed loop runs on a plan with BMPC_PLAN_TRANSFORM";
  if (P.desc.model == BMPC_MODEL_QUADRUPED) return check_quad_scene_plan(P);
  if (P.desc.model != BMPC_MODEL_HIGHWAY || P.n != 4 || P.d != 2)
    return "the overtake scene needs a highway plan (n = 4, d = 2)";
  return "";
}

int bmpc_set_obstacle_sampling(bmpc_plan* pl, const bmpc_obstacle_sampling* smp) {
  if (!pl) return fail(-22, "null argument");
  if (!smp) {
    pl->smp = bmpc_obstacle_sampling{};
    return 0;
  }
  const Plan& P = pl->hp.plan;
  if (smp->mode < BMPC_OBS_ARGMAX || smp->mode > BMPC_OBS_SCRIPT)
    return fail(-22, "bmpc_set_obstacle_sampling: unknown mode (BMPC_OBS_ARGMAX, _SAMPLE_MODEL, _SAMPLE_TILTED or _SCRIPT)");
  if (smp->hold < 1) return fail(-22, "bmpc_set_obstacle_sampling: hold must be at least 1");
  if (smp->ego_base < 0) return fail(-22, "bmpc_set_obstacle_sampling: ego_base must not be negative");
  if (const std::string e = check_obstacle_chooses(P); !e.empty()) return fail(-22, "bmpc_set_obstacle_sampling: " + e);
  if (smp->mode >= BMPC_OBS_SAMPLE_TILTED && !pl->has_prop)
    return fail(-22, "bmpc_set_obstacle_sampling: modes BMPC_OBS_SAMPLE_TILTED and BMPC_OBS_SCRIPT need a proposal "
                     "(bmpc_set_obstacle_proposal)");
  if (smp->mode == BMPC_OBS_SCRIPT && pl->prop.script_epochs == 0)
    return fail(-22, "bmpc_set_obstacle_sampling: mode BMPC_OBS_SCRIPT needs a proposal with a script");
  pl->smp = *smp;
  return 0;
}

int bmpc_set_obstacle_proposal(bmpc_plan* pl, const bmpc_obstacle_proposal* q) {
  if (!pl) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (!q) {
    if (pl->smp.mode >= BMPC_OBS_SAMPLE_TILTED)
      return fail(-22, "bmpc_set_obstacle_proposal: the sampler's mode needs the proposal: detach or change the "
                       "sampler first (bmpc_set_obstacle_sampling)");
    pl->has_prop = false;   // (the device copy stays allocated: a loop in flight may still read it)
    pl->prop = bmpc_obstacle_proposal{};
    return 0;
  }
  if (const std::string e = check_obstacle_chooses(P); !e.empty()) return fail(-22, "bmpc_set_obstacle_proposal: " + e);
  for (int j = 0; j < P.m; ++j)
    if (!(std::isfinite(q->tilt[j]) && q->tilt[j] > 0.0))
      return fail(-22, "bmpc_set_obstacle_proposal: tilt[" + std::to_string(j) + "] must be finite and > 0");
  if (q->script_epochs < 0) return fail(-22, "bmpc_set_obstacle_proposal: script_epochs must not be negative");
  if (q->epoch0 < 0) return fail(-22, "bmpc_set_obstacle_proposal: epoch0 must not be negative");
  if (q->script_epochs > 0 && !q->script)
    return fail(-22, "bmpc_set_obstacle_proposal: script_epochs > 0 needs the device table (null script)");
  if (pl->smp.mode == BMPC_OBS_SCRIPT && q->script_epochs == 0)
    return fail(-22, "bmpc_set_obstacle_proposal: the sampler's mode BMPC_OBS_SCRIPT needs a proposal with a script");
  bmpc_obstacle_proposal h = *q;
  for (int j = P.m; j < BMPC_MAX_M; ++j) h.tilt[j] = 1.0;   // (never read)
  if (h.script_epochs == 0) h.script = nullptr;
  if (const int rc = upload_scene_options(pl, h, pl->dist, pl->obs)) return rc;
  pl->prop = h;
  pl->has_prop = true;
  return 0;
}

// "" for the plans one of the three scene entries accepts (bmpc_env_step, bmpc_set_merge_scene,
// bmpc_quad_env_step)
static std::string check_scene_plan(const Plan& P) {
  if (P.desc.model == BMPC_MODEL_QUADRUPED) return check_quad_scene_plan(P);
  if (P.desc.model == BMPC_MODEL_HIGHWAY_MERGE) {
    if (P.desc.controller != BMPC_CTRL_CVAR || P.n != 4 || P.d != 2 || P.nFx != 4)
      return "the merge scene needs a HIGHWAY_MERGE CVaR plan (n = 4, d = 2, nFx = 4)";
    return "";
  }
  if (P.desc.model != BMPC_MODEL_HIGHWAY || P.n != 4 || P.d != 2)
    return "the overtake scene needs a highway plan (n = 4, d = 2)";
  return "";
}

int bmpc_set_disturbance(bmpc_plan* pl, const bmpc_disturbance* d) {
  if (!pl) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (!d) {
    // (the block stays allocated: a loop in flight may still read it; where an attached proposal or
    // observation model keeps its pointer in use by the launches to come, the block's law is cleared)
    if (pl->has_dist && (pl->has_prop || pl->has_obs))
      if (const int rc = upload_scene_options(pl, pl->prop, bmpc_disturbance{}, pl->obs)) return rc;
    pl->has_dist = false;
    pl->dist = bmpc_disturbance{};
    return 0;
  }
  if (d->law != BMPC_DISTURB_NONE && d->law != BMPC_DISTURB_IH4)
    return fail(-22, "bmpc_set_disturbance: unknown law (BMPC_DISTURB_NONE or BMPC_DISTURB_IH4)");
  if (d->ego_base < 0) return fail(-22, "bmpc_set_disturbance: ego_base must not be negative");
  for (int v = 0; v < 2; ++v)
    for (int c = 0; c < BMPC_MAX_D; ++c) {
      const double sg = v == 0 ? d->sigma_ego[c] : d->sigma_obs[c];
      const std::string name = std::string(v == 0 ? "sigma_ego[" : "sigma_obs[") + std::to_string(c) + "]";
      if (!(std::isfinite(sg) && sg >= 0.0)) return fail(-22, "bmpc_set_disturbance: " + name + " must be finite and >= 0");
      if (c >= P.d && sg != 0.0)
        return fail(-22, "bmpc_set_disturbance: " + name + " must be 0: the plan's inputs have " + std::to_string(P.d) +
                             " components");
    }
  if (const std::string e = check_scene_plan(P); !e.empty()) return fail(-22, "bmpc_set_disturbance: " + e);
  bmpc_disturbance h = *d;
  h.reserved = 0;
  if (const int rc = upload_scene_options(pl, pl->prop, h, pl->obs)) return rc;
  pl->dist = h;
  pl->has_dist = true;
  return 0;
}

int bmpc_set_observation(bmpc_plan* pl, const bmpc_observation* o) {
  if (!pl) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (!o) {
    // (as bmpc_set_disturbance detaches: the law is cleared where another option keeps the pointer in use)
    if (pl->has_obs && (pl->has_prop || pl->has_dist))
      if (const int rc = upload_scene_options(pl, pl->prop, pl->dist, bmpc_observation{})) return rc;
    pl->has_obs = false;
    pl->obs = bmpc_observation{};
    return 0;
  }
  if (o->law != BMPC_OBSERVE_NONE && o->law != BMPC_OBSERVE_IH4)
    return fail(-22, "bmpc_set_observation: unknown law (BMPC_OBSERVE_NONE or BMPC_OBSERVE_IH4)");
  if (o->ego_base < 0) return fail(-22, "bmpc_set_observation: ego_base must not be negative");
  for (int v = 0; v < 2; ++v)
    for (int c = 0; c < BMPC_MAX_N; ++c) {
      const double sg = v == 0 ? o->sigma_x[c] : o->sigma_z[c];
      const std::string name = std::string(v == 0 ? "sigma_x[" : "sigma_z[") + std::to_string(c) + "]";
      if (!(std::isfinite(sg) && sg >= 0.0)) return fail(-22, "bmpc_set_observation: " + name + " must be finite and >= 0");
      if (c >= P.n && sg != 0.0)
        return fail(-22, "bmpc_set_observation: " + name + " must be 0: the plan's states have " + std::to_string(P.n) +
                             " components");
    }
  if (const std::string e = check_scene_plan(P); !e.empty()) return fail(-22, "bmpc_set_observation: " + e);
  bmpc_observation h = *o;
  h.reserved = 0;
  if (const int rc = upload_scene_options(pl, pl->prop, pl->dist, h)) return rc;
  pl->obs = h;
  pl->has_obs = true;
  return 0;
}

// "" for a resampling description and batch the ancestor rule takes
static std::string check_resample(const bmpc_resample_desc* d, int batch) {
  if (batch < 1 || batch > BMPC_RESAMPLE_MAX_BATCH) return "batch must lie in 1 .. BMPC_RESAMPLE_MAX_BATCH (2^20)";
  if (d->scheme != BMPC_RESAMPLE_SYSTEMATIC) return "unknown scheme (BMPC_RESAMPLE_SYSTEMATIC)";
  if (!(std::isfinite(d->ess_fraction) && d->ess_fraction >= 0.0)) return "ess_fraction must be finite and >= 0";
  if (d->ego_base < 0) return "ego_base must not be negative";
  return "";
}

// the ancestor kernel on s (scratch: 2 * batch uint64)
static int launch_ancestors(const bmpc_resample_desc& d, int batch, const double* d_logw, int stride,
                            int32_t* d_anc, uint64_t* d_weight, double* d_info, uint64_t* scratch, hipStream_t s) {
  hipLaunchKernelGGL(k_pop_ancestors, dim3(1), dim3(kPopThreads), 0, s, d, batch, d_logw, stride, d_anc, d_weight,
                     d_info, scratch, scratch + batch);
  HIPCHECK(hipGetLastError());
  return 0;
}

int bmpc_population_ancestors(bmpc_ctx* ctx, const bmpc_resample_desc* desc, int batch, const double* d_logw,
                              int stride, int32_t* d_ancestor, uint64_t* d_weight, double* d_info, void* stream) {
  if (!ctx || !desc || !d_logw || !d_ancestor || !d_info)
    return fail(-22, "bmpc_population_ancestors: null argument (ctx, desc, d_logw, d_ancestor and d_info are required)");
  if (stride < 1) return fail(-22, "bmpc_population_ancestors: stride must be at least 1");
  if (const std::string e = check_resample(desc, batch); !e.empty()) return fail(-22, "bmpc_population_ancestors: " + e);
  std::lock_guard<std::mutex> lock(ctx->q_mu);
  HIPCHECK(hipSetDevice(ctx->device));
  if (!ctx->qstream) HIPCHECK(hipStreamCreateWithFlags(&ctx->qstream, hipStreamNonBlocking));
  if (!ctx->r_done) HIPCHECK(hipEventCreateWithFlags(&ctx->r_done, hipEventDisableTiming));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->qstream;
  // (a reallocation frees the old scratch, which waits for the device; otherwise the last call's
  // kernel, on whichever stream, finishes with the scratch before this one starts)
  HIPCHECK(ctx->r_scratch.reserve(2 * sizeof(uint64_t) * (size_t)batch));
  HIPCHECK(hipStreamWaitEvent(s, ctx->r_done, 0));
  if (const int rc = launch_ancestors(*desc, batch, d_logw, stride, d_ancestor, d_weight, d_info,
                                      ctx->r_scratch.as<uint64_t>(), s))
    return rc;
  HIPCHECK(hipEventRecord(ctx->r_done, s));
  return 0;
}

// the gather of a plan's egos through `anc` on s, under `flag` (null: unconditionally)
static int launch_gather(bmpc_plan* pl, const int32_t* d_anc, const bmpc_ego_buffers* b, const double* flag,
                         hipStream_t s) {
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  GatherList G = {};
  G.batch = pl->batch;
  bool ok = true;
  const size_t n = P.n, ud = (size_t)P.U * P.d;
  if (b) {   // (words are 4 bytes: a double is 2)
    ok = ok && gather_add(G, b->scene, 2 * ENV_STRIDE, 0, 2 * ENV_STRIDE) && gather_add(G, b->upred, 2 * ud, 0, 2 * ud) &&
         gather_add(G, b->x, 2 * n, 0, 2 * n) && gather_add(G, b->z, 2 * n, 0, 2 * n) &&
         gather_add(G, b->xref, 2 * n, 0, 2 * n) && gather_add(G, b->J, 2, 0, 2) && gather_add(G, b->status, 1, 0, 1) &&
         gather_add(G, b->iters, 1, 0, 1) && gather_add(G, b->stats, 2 * ENVS_STRIDE, 0, 2 * ENVS_STRIDE);
  }
  static_assert(sizeof(bmpc_policy) % 4 == 0, "policy rows are copied as 4-byte words");
  const size_t polw = sizeof(bmpc_policy) / 4 * P.m;
  ok = ok && gather_add(G, pl->d_pol, polw, 0, polw);
  EgoSpan spans[EGO_MAX_SPANS];
  const int nsp = ego_state_spans(P, L, spans);
  for (int k = 0; k < nsp; ++k) ok = ok && gather_add(G, pl->d_ws, 2 * L.stride, 2 * spans[k].off, 2 * spans[k].len);
  if (!ok) return fail(-5, "bmpc_gather_egos: segment list overflow");
  const size_t need = ((size_t)pl->batch * G.row_words + 1) / 2;   // doubles of the plan's scratch
  if (need > pl->scratch_len) {
    hipFree(pl->d_scratch);   // (waits for the device: nothing in flight reads the old scratch)
    pl->d_scratch = nullptr;
    pl->scratch_len = 0;
    HIPCHECK(hipMalloc(&pl->d_scratch, need * sizeof(double)));
    pl->scratch_len = need;
  }
  uint32_t* stage = reinterpret_cast<uint32_t*>(pl->d_scratch);
  hipLaunchKernelGGL(k_ego_stage, dim3(pl->batch), dim3(256), 0, s, G, d_anc, stage, flag);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_ego_commit, dim3(pl->batch), dim3(256), 0, s, G, d_anc, stage, flag);
  HIPCHECK(hipGetLastError());
  pl->pol_on_device = true;   // policy rows moved on the device: h_pol is stale
  return 0;
}

int bmpc_gather_egos(bmpc_plan* pl, const int32_t* d_ancestor, const bmpc_ego_buffers* bufs, void* stream) {
  if (!pl || !d_ancestor) return fail(-22, "bmpc_gather_egos: null argument (plan and d_ancestor are required)");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  return launch_gather(pl, d_ancestor, bufs, nullptr, plan_stream(pl, stream));
}

int bmpc_resample_device(bmpc_plan* pl, const bmpc_resample_desc* desc, const bmpc_ego_buffers* bufs,
                         int32_t* d_ancestor, double* d_info, void* stream) {
  if (!pl || !desc || !bufs || !bufs->scene || !d_ancestor || !d_info)
    return fail(-22, "bmpc_resample_device: null argument (plan, desc, bufs->scene, d_ancestor and d_info are required)");
  if (const std::string e = check_obstacle_chooses(pl->hp.plan); !e.empty()) return fail(-22, "bmpc_resample_device: " + e);
  if (const std::string e = check_resample(desc, pl->batch); !e.empty()) return fail(-22, "bmpc_resample_device: " + e);
  HIPCHECK(hipSetDevice(pl->ctx->device));
  if (!pl->d_rs) HIPCHECK(hipMalloc(&pl->d_rs, 2 * sizeof(uint64_t) * (size_t)pl->batch));
  hipStream_t s = plan_stream(pl, stream);
  if (const int rc = launch_ancestors(*desc, pl->batch, bufs->scene + BMPC_ENV_LOGW, ENV_STRIDE, d_ancestor, nullptr,
                                      d_info, pl->d_rs, s))
    return rc;
  if (const int rc = launch_gather(pl, d_ancestor, bufs, d_info, s)) return rc;
  hipLaunchKernelGGL(k_pop_set_logw, dim3((pl->batch + 255) / 256), dim3(256), 0, s, bufs->scene, pl->batch, d_info);
  HIPCHECK(hipGetLastError());
  return 0;
}

static int gather(bmpc_plan* pl, size_t off, int count, double* host) {
  if (!host) return 0;
  const size_t need = (size_t)pl->batch * count;
  if (need > pl->scratch_len) {
    hipFree(pl->d_scratch);
    pl->d_scratch = nullptr;
    HIPCHECK(hipMalloc(&pl->d_scratch, need * sizeof(double)));
    pl->scratch_len = need;
  }
  hipLaunchKernelGGL(k_gather, dim3(1024), dim3(256), 0, pl->stream, pl->d_ws, pl->hp.lay.stride, off,
                     count, pl->d_scratch, pl->batch);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(host, pl->d_scratch, need * sizeof(double), hipMemcpyDeviceToHost, pl->stream));
  HIPCHECK(hipStreamSynchronize(pl->stream));
  return 0;
}

int bmpc_get_counters(bmpc_plan* pl, double* out) {
  if (!pl || !out) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  return gather(pl, pl->hp.lay.prof, PROF_COUNT, out);
}

int bmpc_get_warm_start(bmpc_plan* pl, double* uLin, double* p, double* jcons, double* old_input) {
  if (!pl) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  int rc;
  if ((rc = gather(pl, L.uLin, (P.U + 1) * P.d, uLin))) return rc;
  if (P.bdim * P.m > 0 && (rc = gather(pl, L.pprev, P.bdim * P.m, p))) return rc;
  if ((rc = gather(pl, L.misc + MISC_JCONS, 1, jcons))) return rc;
  if ((rc = gather(pl, L.misc + MISC_OLDU, P.d, old_input))) return rc;
  return 0;
}

int bmpc_set_warm_start(bmpc_plan* pl, const double* uLin, const double* p, const double* jcons,
                        const double* old_input, const uint8_t* mask) {
  if (!pl || !uLin) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  return scatter_parts(pl, {{uLin, L.uLin, (P.U + 1) * P.d}, {p, L.pprev, P.bdim * P.m},
                            {jcons, L.misc + MISC_JCONS, 1}, {old_input, L.misc + MISC_OLDU, P.d}}, mask);
}

int bmpc_get_robust_warm_start(bmpc_plan* pl, double* xLin, double* uLin, double* old_input) {
  if (!pl) return fail(-22, "null argument");
  if (pl->hp.plan.desc.controller != BMPC_CTRL_ROBUST) return fail(-22, "not a robustMPC plan");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  int rc;
  if (xLin && (rc = gather(pl, L.xlin, P.T * P.n, xLin))) return rc;
  if (uLin && (rc = gather(pl, L.uLin, P.U * P.d, uLin))) return rc;
  if (old_input && (rc = gather(pl, L.misc + MISC_OLDU, P.d, old_input))) return rc;
  return 0;
}

int bmpc_set_robust_warm_start(bmpc_plan* pl, const double* xLin, const double* uLin, const double* old_input,
                               const uint8_t* mask) {
  if (!pl) return fail(-22, "null argument");
  if (pl->hp.plan.desc.controller != BMPC_CTRL_ROBUST) return fail(-22, "not a robustMPC plan");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  return scatter_parts(pl, {{xLin, L.xlin, P.T * P.n}, {uLin, L.uLin, P.U * P.d}, {old_input, L.misc + MISC_OLDU, P.d}},
                       mask);
}

int bmpc_set_transform(bmpc_plan* pl, const double* S, const uint8_t* s_on, const double* bx, const uint8_t* mask) {
  if (!pl) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (!plan_takes_transform(P))
    return fail(-22, "bmpc_set_transform: only HIGHWAY_MERGE plans and HIGHWAY CVaR plans created with "
                     "BMPC_PLAN_TRANSFORM take a state transformation");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Layout& L = pl->hp.lay;
  const int B = pl->batch, n = P.n, nF = P.nFx;
  DevBuf dmask;
  HIPCHECK(upload(dmask, mask, B));
  // S (or zeros) and the "S is not None" flag of every masked ego
  std::vector<double> Sv((size_t)B * n * n, 0.0), on(B, 0.0);
  for (int e = 0; e < B; ++e) {
    if (S) {
      std::copy(S + (size_t)e * n * n, S + (size_t)(e + 1) * n * n, Sv.begin() + (size_t)e * n * n);
      on[e] = (!s_on || s_on[e]) ? 1.0 : 0.0;
    }
  }
  // the slab keeps S at row stride n (XF_S holds n*n values)
  if (int rc = scatter_rows(pl, Sv.data(), L.xform + XF_S, n * n, dmask.as<uint8_t>())) return rc;
  if (int rc = scatter_rows(pl, on.data(), L.xform + XF_SON, 1, dmask.as<uint8_t>())) return rc;
  if (bx) {
    std::vector<double> ones(B, 1.0);
    if (int rc = scatter_rows(pl, bx, L.xform + XF_BX, nF, dmask.as<uint8_t>())) return rc;
    if (int rc = scatter_rows(pl, ones.data(), L.xform + XF_BXSET, 1, dmask.as<uint8_t>())) return rc;
  }
  return 0;
}

int bmpc_set_fx(bmpc_plan* pl, const double* Fx, const uint8_t* mask) {
  if (!pl || !Fx) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (!plan_takes_transform(P))
    return fail(-22, "bmpc_set_fx: only HIGHWAY_MERGE plans and HIGHWAY CVaR plans created with "
                     "BMPC_PLAN_TRANSFORM take a per-solve Fx");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Layout& L = pl->hp.lay;
  const int B = pl->batch;
  DevBuf dmask;
  HIPCHECK(upload(dmask, mask, B));
  std::vector<double> ones(B, 1.0);
  if (int rc = scatter_rows(pl, Fx, L.xform + XF_FX, P.nFx * P.n, dmask.as<uint8_t>())) return rc;
  return scatter_rows(pl, ones.data(), L.xform + XF_FXSET, 1, dmask.as<uint8_t>());
}

int bmpc_get_transform(bmpc_plan* pl, double* S, double* bx, double* flags) {
  if (!pl) return fail(-22, "null argument");
  const Plan& P = pl->hp.plan;
  if (!plan_takes_transform(P)) return fail(-22, "bmpc_get_transform: the plan takes no state transformation");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  int rc;
  if ((rc = drain(pl))) return rc;
  const Layout& L = pl->hp.lay;
  if ((rc = gather(pl, L.xform + XF_S, P.n * P.n, S))) return rc;
  if ((rc = gather(pl, L.xform + XF_BX, P.nFx, bx))) return rc;
  static_assert(XF_BXSET == XF_SON + 1, "the two flags are gathered as one pair");
  return gather(pl, L.xform + XF_SON, 2, flags);
}

int bmpc_get_branch_dp(bmpc_plan* pl, double* dp) {
  if (!pl || !dp) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  if (P.bdim * P.m * P.n == 0) return 0;
  return gather(pl, pl->hp.lay.dp, P.bdim * P.m * P.n, dp);
}

int bmpc_get_tree(bmpc_plan* pl, double* xbar, double* ubar, double* zbar, double* w, double* p,
                  double* sol) {
  if (!pl) return fail(-22, "null argument");
  HIPCHECK(hipSetDevice(pl->ctx->device));
  const Plan& P = pl->hp.plan;
  const Layout& L = pl->hp.lay;
  int rc;
  if ((rc = gather(pl, L.xbar, P.T * P.n, xbar))) return rc;
  if ((rc = gather(pl, L.ubar, P.U * P.d, ubar))) return rc;
  if ((rc = gather(pl, L.zbar, P.T * P.n, zbar))) return rc;
  if ((rc = gather(pl, L.w, P.nbranch, w))) return rc;
  if (P.bdim * P.m > 0 && (rc = gather(pl, L.p, P.bdim * P.m, p))) return rc;
  if ((rc = gather(pl, L.sol, P.nv, sol))) return rc;
  return 0;
}

int bmpc_enable_timing(bmpc_plan* pl, int on) {
  if (!pl) return fail(-22, "null argument");
  pl->timing = on != 0;
  pl->t_pending = 0;
  pl->t_acc[0] = pl->t_acc[1] = 0;
  pl->t_cnt = 0;
  return 0;
}

int bmpc_timing(bmpc_plan* pl, double* ms, int32_t* count) {
  if (!pl) return fail(-22, "null argument");
  if (int rc = fold_timing(pl)) return rc;
  const int c = pl->t_cnt;
  if (ms) {
    ms[0] = c ? pl->t_acc[0] / c : 0.0;
    ms[1] = c ? pl->t_acc[1] / c : 0.0;
  }
  if (count) *count = c;
  pl->t_acc[0] = pl->t_acc[1] = 0;
  pl->t_cnt = 0;
  return 0;
}

// A packed evaluation call on the context's stream (bmpc_model_eval_ref, bmpc_hmm_eval; the caller
// holds q_mu): the inputs packed into q_host and uploaded in one copy to the grow-only q_aux, a
// device slot behind them for every output that has a host array, and -- after the caller's launch
// -- one read-back, unpacked.  The compat environments and the belief MPC call these once per
// control step: no allocation and no device-wide synchronisation per call.
struct PackedArg { const void* host; size_t bytes; };           // (packed as whole doubles)
struct PackedOut { double* host; size_t len; double* dev; };    // len doubles; dev is null when host is
struct PackedCall {
  bmpc_ctx* ctx;
  PackedOut* out;
  int nout;
  size_t tin = 0, tout = 0;
  int begin(const PackedArg* in, int nin, const double** din) {   // din[i]: in[i] on the device
    for (int i = 0; i < nin; ++i) tin += (in[i].bytes + sizeof(double) - 1) / sizeof(double);
    for (int i = 0; i < nout; ++i) tout += out[i].host ? out[i].len : 0;
    ctx->q_host.resize(tin + tout);
    HIPCHECK(ctx->q_aux.reserve((tin + tout) * sizeof(double)));
    if (!ctx->qstream) HIPCHECK(hipStreamCreateWithFlags(&ctx->qstream, hipStreamNonBlocking));
    double* cur = ctx->q_aux.as<double>();
    for (int i = 0; i < nin; ++i) {
      if (in[i].bytes) memcpy(ctx->q_host.data() + (cur - ctx->q_aux.as<double>()), in[i].host, in[i].bytes);
      din[i] = cur;
      cur += (in[i].bytes + sizeof(double) - 1) / sizeof(double);
    }
    HIPCHECK(hipMemcpyAsync(ctx->q_aux.p, ctx->q_host.data(), tin * sizeof(double), hipMemcpyHostToDevice, ctx->qstream));
    for (int i = 0; i < nout; ++i) {
      out[i].dev = out[i].host ? cur : nullptr;
      if (out[i].host) cur += out[i].len;
    }
    return 0;
  }
  int finish() {   // after the launch
    HIPCHECK(hipGetLastError());
    double* h = ctx->q_host.data() + tin;
    if (tout) HIPCHECK(hipMemcpyAsync(h, ctx->q_aux.as<double>() + tin, tout * sizeof(double), hipMemcpyDeviceToHost, ctx->qstream));
    HIPCHECK(hipStreamSynchronize(ctx->qstream));
    for (int i = 0; i < nout; h += out[i].host ? out[i].len : 0, ++i)
      if (out[i].host) memcpy(out[i].host, h, out[i].len * sizeof(double));
    return 0;
  }
};

int bmpc_model_eval(bmpc_ctx* ctx, const bmpc_plan_desc* desc, const bmpc_policy* policies, int B,
                    const double* x, const double* u, const double* z, double* A, double* Bm,
                    double* C, double* xp, double* p, double* dp, double* zpred, double* h0,
                    double* dh) {
  return bmpc_model_eval_ref(ctx, desc, policies, 0, nullptr, nullptr, B, x, u, z, A, Bm, C, xp, p, dp, zpred, h0,
                             dh);
}

int bmpc_model_eval_ref(bmpc_ctx* ctx, const bmpc_plan_desc* desc, const bmpc_policy* policies, int nref,
                        const double* grid, const double* values, int B, const double* x, const double* u,
                        const double* z, double* A, double* Bm, double* C, double* xp, double* p, double* dp,
                        double* zpred, double* h0, double* dh) {
  if (!ctx || !desc || !policies || !x || !u || !z || B <= 0) return fail(-22, "null argument");
  {
    const std::string e = check_lane_ref(nref, grid, values);
    if (!e.empty()) return fail(-22, e);
  }
  for (size_t i = 0; i < (size_t)B * (desc->m > 0 ? desc->m : 0); ++i)
    if (is_psiref(policies[i].kind) && (desc->model != BMPC_MODEL_HIGHWAY_MERGE || nref == 0))
      return fail(-22, "lane-reference (psiref) policies need the HIGHWAY_MERGE model and a lane reference");
  const int n = desc->n, d = desc->d, m = desc->m, N = desc->N;
  if (((desc->model == BMPC_MODEL_HIGHWAY || desc->model == BMPC_MODEL_HIGHWAY_MERGE) && (n != 4 || d != 2)) ||
      (desc->model == BMPC_MODEL_QUADRUPED && (n != 3 || d != 3)) ||
      (desc->model != BMPC_MODEL_HIGHWAY && desc->model != BMPC_MODEL_HIGHWAY_MERGE &&
       desc->model != BMPC_MODEL_QUADRUPED) || m < 1 || m > BMPC_MAX_M || N < 1)
    return fail(-22, "bad model dimensions");
  const size_t Bz = (size_t)B;
  const PackedArg in[] = {{policies, Bz * m * sizeof(bmpc_policy)}, {x, sizeof(double) * Bz * n},
                          {u, sizeof(double) * Bz * d},             {z, sizeof(double) * Bz * n},
                          {grid, sizeof(double) * nref},            {values, sizeof(double) * nref}};
  // (dp goes with p, dh with h0)
  PackedOut out[] = {{A, Bz * n * n}, {Bm, Bz * n * d},           {C, Bz * n},         {xp, Bz * n},
                     {p, Bz * m},     {p ? dp : nullptr, Bz * m * n}, {zpred, Bz * N * m * n}, {h0, Bz},
                     {h0 ? dh : nullptr, Bz * n}};
  const double* din[6];
  std::lock_guard<std::mutex> lock(ctx->q_mu);
  HIPCHECK(hipSetDevice(ctx->device));
  PackedCall pc{ctx, out, 9};
  if (const int rc = pc.begin(in, 6, din)) return rc;
  const LaneRef R{nref ? din[4] : nullptr, nref ? din[5] : nullptr, nref};
  const auto k = desc->model == BMPC_MODEL_HIGHWAY         ? k_model<Highway>
                 : desc->model == BMPC_MODEL_HIGHWAY_MERGE ? k_model<HighwayMerge>
                                                           : k_model<Quadruped>;
  hipLaunchKernelGGL(k, dim3((B + 63) / 64), dim3(64), 0, ctx->qstream, *desc, (const bmpc_policy*)din[0], B, din[1],
                     din[2], din[3], out[0].dev, out[1].dev, out[2].dev, out[3].dev, out[4].dev, out[5].dev, out[6].dev,
                     out[7].dev, out[8].dev, R);
  return pc.finish();
}

int bmpc_set_lane_ref(bmpc_plan* pl, int nref, const double* grid, const double* values) {
  if (!pl) return fail(-22, "null argument");
  if (pl->hp.plan.desc.model != BMPC_MODEL_HIGHWAY_MERGE) return fail(-22, "lane references are for HIGHWAY_MERGE plans");
  {
    const std::string e = check_lane_ref(nref, grid, values);
    if (!e.empty()) return fail(-22, e);
  }
  HIPCHECK(hipSetDevice(pl->ctx->device));
  if (const int rc = drain(pl)) return rc;   // no solve in flight reads the old reference
  // the new copy is built beside the old one and swapped in only once the device bundle points
  // at it: a failure on the way leaves the plan on its old, still allocated reference
  DevBuf fresh;
  if (nref) {
    HIPCHECK(fresh.alloc(sizeof(double) * 2 * (size_t)nref));
    HIPCHECK(hipMemcpy(fresh.as<double>(), grid, sizeof(double) * nref, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(fresh.as<double>() + nref, values, sizeof(double) * nref, hipMemcpyHostToDevice));
  }
  double* const old = pl->d_lref;
  const int old_n = pl->hp.plan.nlref;
  pl->d_lref = fresh.as<double>();
  pl->hp.plan.nlref = nref;
  pl->hp.plan.lref = nullptr;   // host copy unused; upload_bundle points the device copy at d_lref
  const hipError_t e = upload_bundle(pl);
  if (e != hipSuccess) {
    pl->d_lref = old;
    pl->hp.plan.nlref = old_n;
    return fail(-5, std::string("upload_bundle: ") + hipGetErrorString(e));
  }
  fresh.p = nullptr;   // owned by the plan now
  hipFree(old);
  return 0;
}

int bmpc_hmm_eval(bmpc_ctx* ctx, int M, int m, const double* hc, int B, const double* xb, const double* u,
                  const double* xbackup, double* xbp, double* A, double* Bm, double* C, double* h0,
                  double* Jh) {
  if (!ctx || !hc || !xb || !u || !xbackup || B <= 0) return fail(-22, "null argument");
  if (M < 1 || m < 1 || M > HMM_MAX_AGENTS || m > HMM_MAX_BACKUPS) return fail(-22, "M, m must be in 1..4");
  const size_t Bz = (size_t)B, nb = 4 + (size_t)M * m, Mm = (size_t)M * m;
  const PackedArg in[] = {{hc, sizeof(double) * 8}, {xb, sizeof(double) * Bz * nb}, {u, sizeof(double) * Bz * 2},
                          {xbackup, sizeof(double) * Bz * Mm * 4}};
  PackedOut out[] = {{xbp, Bz * nb}, {A, Bz * nb * nb}, {Bm, Bz * nb * 2}, {C, Bz * nb}, {h0, Bz * Mm}, {Jh, Bz * Mm * nb}};
  const double* din[4];
  std::lock_guard<std::mutex> lock(ctx->q_mu);
  HIPCHECK(hipSetDevice(ctx->device));
  PackedCall pc{ctx, out, 6};
  if (const int rc = pc.begin(in, 4, din)) return rc;
  hipLaunchKernelGGL(k_hmm, dim3((B + 63) / 64), dim3(64), 0, ctx->qstream, M, m, din[0], B, din[1], din[2], din[3],
                     out[0].dev, out[1].dev, out[2].dev, out[3].dev, out[4].dev, out[5].dev);
  return pc.finish();
}

int bmpc_qp_solve(bmpc_ctx* ctx, int n, int m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                  const int32_t* Ai, int batch, const double* Px, const double* q, const double* Ax, const double* l,
                  const double* u, int max_iter, double eps, double* x, double* y, int32_t* status, int32_t* iters,
                  int32_t* info) {
  if (!ctx || !q || !x || !status) return fail(-22, "null argument");
  if (n < 1 || m < 0 || batch < 1 || !Pp || !Ap) return fail(-22, "need n >= 1, m >= 0, batch >= 1 and a pattern");
  // the column pointers are checked before they size anything (the cache key below)
  if (Pp[0] != 0 || Ap[0] != 0) return fail(-22, "column pointers must start at 0");
  for (int j = 0; j < n; ++j)
    if (Pp[j + 1] < Pp[j] || Ap[j + 1] < Ap[j]) return fail(-22, "column pointers must be non-decreasing");
  if ((Pp[n] > 0 && !Pi) || (Ap[n] > 0 && !Ai)) return fail(-22, "null row-index array");
  std::lock_guard<std::mutex> lock(ctx->q_mu);
  // the bounds of every problem are checked on every call; the analysis is looked up by
  // pattern + row classes (bandqp_analyse validates the pattern on a miss)
  std::vector<int> cls;
  std::string err = bandqp_classify(m, batch, l, u, cls);
  if (!err.empty()) return fail(-22, err);
  const bool lds_ok = batch <= ctx->cus;   // bandqp_analyse's factor-in-LDS rule depends on this only
  std::vector<int32_t> key;
  key.reserve(6 + 2 * (size_t)n + Pp[n] + Ap[n] + m);
  key.insert(key.end(), {n, m, max_iter, lds_ok ? 1 : 0, Pp[n], Ap[n]});
  key.insert(key.end(), Pp, Pp + n + 1);
  key.insert(key.end(), Ap, Ap + n + 1);
  if (Pp[n] > 0) key.insert(key.end(), Pi, Pi + Pp[n]);
  if (Ap[n] > 0) key.insert(key.end(), Ai, Ai + Ap[n]);
  key.insert(key.end(), cls.begin(), cls.end());
  QPCacheEntry* ent = nullptr;
  for (auto& c : ctx->qcache)
    if (c->eps == eps && c->key == key) ent = c.get();
  HIPCHECK(hipSetDevice(ctx->device));
  if (!ent) {
    auto fresh = std::make_unique<QPCacheEntry>();
    err = bandqp_analyse(n, m, Pp, Pi, Ap, Ai, batch, l, u, max_iter, eps, fresh->h, ctx->cus, ctx->lds_per_cu);
    if (!err.empty()) return fail(-22, err);
    fresh->key.swap(key);
    fresh->eps = eps;
    HIPCHECK(fresh->tab.reserve(fresh->h.blob.size() * sizeof(int32_t)));
    HIPCHECK(hipMemcpy(fresh->tab.p, fresh->h.blob.data(), fresh->h.blob.size() * sizeof(int32_t),
                       hipMemcpyHostToDevice));
    if ((int)ctx->qcache.size() >= bmpc_ctx::kQPCache) {   // evict the least recently used
      auto lru = std::min_element(ctx->qcache.begin(), ctx->qcache.end(),
                                  [](const auto& a, const auto& b) { return a->used < b->used; });
      ctx->qcache.erase(lru);
    }
    ent = fresh.get();
    ctx->qcache.push_back(std::move(fresh));
  }
  ent->used = ++ctx->qclock;
  const HostBandQP& h = ent->h;
  const int nnzP = Pp[n], nnzA = Ap[n];
  if ((nnzP && !Px) || (nnzA && !Ax)) return fail(-22, "null value array");
  if (info) {
    info[0] = h.d.nk;
    info[1] = h.d.bw;
    info[2] = h.d.n_in;
    info[3] = h.d.nscat;
  }
  if (!ctx->qstream) HIPCHECK(hipStreamCreateWithFlags(&ctx->qstream, hipStreamNonBlocking));
  hipStream_t st = ctx->qstream;
  const size_t B = (size_t)batch;
  // host values in the kernel's per-problem order: [Px; Ax] then [q; l; u], one upload
  const size_t nv = std::max<size_t>(B * h.d.nvals, 1), nc = B * h.d.ncvals;
  std::vector<double>& hv = ctx->q_host;
  hv.resize(nv + nc);
  for (size_t b = 0; b < B; ++b) {
    double* v = hv.data() + b * h.d.nvals;
    if (nnzP) memcpy(v, Px + b * nnzP, nnzP * sizeof(double));
    if (nnzA) memcpy(v + nnzP, Ax + b * nnzA, nnzA * sizeof(double));
    double* c = hv.data() + nv + b * h.d.ncvals;
    memcpy(c, q + b * n, n * sizeof(double));
    if (m) {
      memcpy(c + n, l + b * m, m * sizeof(double));
      memcpy(c + n + m, u + b * m, m * sizeof(double));
    }
  }
  HIPCHECK(ctx->q_in.reserve(hv.size() * sizeof(double)));
  HIPCHECK(ctx->q_ws.reserve(B * h.d.stride * sizeof(double)));
  const size_t nout = B * (n + m) * sizeof(double) + 2 * B * sizeof(int32_t);
  HIPCHECK(ctx->q_out.reserve(nout));
  HIPCHECK(hipMemcpyAsync(ctx->q_in.p, hv.data(), hv.size() * sizeof(double), hipMemcpyHostToDevice, st));
  double* dx = ctx->q_out.as<double>();
  double* dy = dx + B * n;
  int32_t* dst = reinterpret_cast<int32_t*>(dy + B * m);
  int32_t* dit = dst + B;
  BandQPDesc d = h.d;
  const int32_t* base = ent->tab.as<int32_t>();
  d.kind = base;
  d.scat = d.kind + h.kind.size();
  d.cscat = d.scat + h.scat.size();
  d.xmap = d.cscat + h.cscat.size();
  d.ymap = d.xmap + h.xmap.size();
  const size_t lds = bandqp_lds_doubles(d.nk, d.W, d.lb_lds) * sizeof(double);
  HIPCHECK(optin_lds((const void*)k_bandqp, lds));
  hipLaunchKernelGGL(k_bandqp, dim3(batch), dim3(64), lds, st, d, ctx->q_in.as<double>(), ctx->q_in.as<double>() + nv,
                     ctx->q_ws.as<double>(), dx, dy, dst, dit, batch);
  HIPCHECK(hipGetLastError());
  // one read-back of x | y | status | iters
  std::vector<char> ho(nout);
  HIPCHECK(hipMemcpyAsync(ho.data(), dx, nout, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  memcpy(x, ho.data(), B * n * sizeof(double));
  if (y && m) memcpy(y, ho.data() + B * n * sizeof(double), B * m * sizeof(double));
  memcpy(status, ho.data() + B * (n + m) * sizeof(double), B * sizeof(int32_t));
  if (iters) memcpy(iters, ho.data() + B * (n + m) * sizeof(double) + B * sizeof(int32_t), B * sizeof(int32_t));
  return 0;
}

}  // extern "C"
