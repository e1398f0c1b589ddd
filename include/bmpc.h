/*
 * bmpc.h -- C ABI of the MI355X batched branch-MPC library (libbmpc.so).
 *
 * Drop-in boundary for the reference's controller / predictive-model surface
 * (Gavinli-lgf/belief-planning).  Every entry point replaces a reference interface:
 *
 *   bmpc_plan_create   <- BranchMPC_CVaR.__init__      MPC_branch.py:1601-1669
 *                         BranchMPCProx.__init__        MPC_branch.py:84-128
 *                         Init_MPC.initBranchMPC/initquadBranchMPC  Init_MPC.py:40-94
 *                         PredictiveModel.__init__      highway_branch_dyn.py:264-281,
 *                                                       quadruped_branch_dyn.py:155-173
 *   bmpc_set_policies  <- PredictiveModel.update_backup highway_branch_dyn.py:331-334
 *                         (the backup lambdas, traced to descriptors)
 *   bmpc_reset         <- "self.BT is None" first-solve path (inittree) MPC_branch.py:2062-2064
 *   bmpc_solve         <- BranchMPC_CVaR.solve           MPC_branch.py:2043-2092
 *                         BranchMPCProx.solve             MPC_branch.py:384-423
 *                         BranchMPC.solve                 MPC_branch.py:1171-1210
 *                         (BMPC_CTRL_PROX: OSQP QP, status 1 = solved / -2 = not)
 *                         (tree update, linearisation, assembly, ecos.solve / OSQP, unpack)
 *   bmpc_get_tree      <- BranchTree fields + BT2array    MPC_branch.py:65-78,2108-2122
 *   bmpc_get_branch_dp <- BranchTree.dp                    MPC_branch.py:1711,1842
 *   bmpc_set_transform <- solve(..., S, bx) arguments      MPC_branch.py:2043-2057
 *   bmpc_set_fx        <- solve(..., Fx) argument          MPC_branch.py:2055-2056
 *   bmpc_model_eval    <- PredictiveModel.dyn_linearization / branch_eval / zpred_eval /
 *                         col_eval                         highway_branch_dyn.py:284-325
 *   bmpc_model_eval_ref<- the same of PredictiveModel_merge with psiref backups
 *                                                          highway_branch_dyn.py:54-130,400-502
 *   bmpc_set_lane_ref  <- PredictiveModel_merge(..., merge_ref) / the refpsi interpolant of
 *                         the psiref backups              main_branch.py:78-85
 *   bmpc_env_step      <- Highway_env.step + Highway_sim collision rule
 *                                                          Highway_env_branch.py:83-184,421-429
 *   bmpc_merge_env_step<- Highway_env_merge.step + the same collision rule
 *                                                          Highway_env_branch.py:317-380,421-429
 *   bmpc_quad_env_step <- Quad_env.step                    quadruped_env.py:67-130
 *   bmpc_set_obstacle_sampling   (an extension: the scenes' obstacle draws its backup policy from
 *                         branch_eval's distribution instead of the reference's argmax rules)
 *   bmpc_set_obstacle_proposal   (an extension: the draw tilted per policy, or a prescribed choice
 *                         per ego and epoch, with a running log-weight in the scene row)
 *   bmpc_set_disturbance         (an extension: an actuation disturbance on both vehicles' inputs
 *                         in the scenes' Euler steps, drawn per step)
 *   bmpc_set_observation         (an extension: observation noise on the ego and obstacle states the
 *                         scenes hand to the next solve, drawn per step; the scenes keep the truth)
 *   bmpc_population_ancestors / bmpc_gather_egos / bmpc_resample_device   (an extension: resampling a
 *                         weighted population between loop segments, on the device)
 *
 * Conventions: all host buffers are caller-owned, C-contiguous, ego-major, float64
 * (int32 for status/iteration counts).  Return codes are 0 on success and a negative
 * errno-style code on failure; bmpc_last_error() gives a thread-local message.  A plan
 * owns its device buffers and the per-ego persistent warm-start state; calls are
 * synchronous on the plan's HIP stream unless the *_device variant is used.
 * Per-ego status follows ECOS exit codes for the CVaR controller (>= 0 means
 * "feasible", MPC_branch.py:2141) and OSQP status_val for the QP controllers
 * (1 means "feasible", MPC_branch.py:482).  CVaR status -9 is not an ECOS code: the
 * kernel's internal consistency guard on its best-iterate state tripped (never expected).
 */
#ifndef BMPC_H
#define BMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_ABI_VERSION 2

#define BMPC_MAX_N 8      /* state dimension            */
#define BMPC_MAX_D 4      /* input dimension            */
#define BMPC_MAX_FX 8     /* rows of Fx                 */
#define BMPC_MAX_FU 8     /* rows of Fu                 */
#define BMPC_MAX_M 4      /* backup policies per branch */

/* controller kinds */
enum {
  BMPC_CTRL_CVAR = 0, /* BranchMPC_CVaR  (ECOS SOCP)   MPC_branch.py:1598 */
  BMPC_CTRL_PROX = 1, /* BranchMPCProx   (OSQP QP)     MPC_branch.py:82   */
  BMPC_CTRL_QP = 2,   /* BranchMPC, active definition (OSQP QP) MPC_branch.py:881 */
  BMPC_CTRL_ROBUST = 3 /* robustMPC: one input sequence against every obstacle prediction
                          of the tree (OSQP QP) MPC_branch.py:1275.  T = N*NB+2 states,
                          U = N*NB+1 inputs, no branch weights; status 1 = solved, the
                          solution is taken whatever the status (:1459) */
};

/* predictive models */
enum {
  BMPC_MODEL_HIGHWAY = 0,       /* highway_branch_dyn.PredictiveModel   */
  BMPC_MODEL_QUADRUPED = 1,     /* quadruped_branch_dyn.PredictiveModel */
  BMPC_MODEL_HIGHWAY_MERGE = 2  /* highway_branch_dyn.PredictiveModel_merge (:400-502) without
                                   psiref policies: BF_traj = softmin_5 of veh_col(obs, ego,
                                   [L+1, W+0.2]) only (:463-467); plans of this model accept a
                                   per-ego state transformation S and state bound bx
                                   (bmpc_set_transform) -- the merge scene's controller */
};

/* backup-policy kinds (what the traced lambdas lower to) */
enum {
  BMPC_POL_MAINTAIN = 0,        /* backup_maintain(x,cons)          p = {Kpsi}          */
  BMPC_POL_BRAKE = 1,           /* backup_brake(x,cons)             p = {Kpsi}          */
  BMPC_POL_LC = 2,              /* backup_lc(x,x0)                  p = x0[0..3]        */
  BMPC_POL_MAINTAIN_TRACKV = 3, /* backup_maintain_trackV(x,cons,v0) p = {Kpsi, v0}     */
  BMPC_POL_FORWARD = 4,         /* quadruped backup_forward(x,v0)   p = {v0}            */
  BMPC_POL_STOP = 5,            /* quadruped backup_stop(x)                             */
  /* the merge ramp's lane-reference tracking backups: the same policies with the psiref
   * argument, psiref(X) = the plan's lane reference (bmpc_set_lane_ref; bmpc_model_eval_ref),
   * a 1-D linear interpolant (casadi.interpolant 'linear', main_branch.py:78-82);
   * highway_branch_dyn.py:54-130 MX branches.  HIGHWAY_MERGE plans only.                 */
  BMPC_POL_MAINTAIN_PSIREF = 6,        /* u = [0, psiref(X) - Kpsi psi]            p = {Kpsi}     */
  BMPC_POL_MAINTAIN_TRACKV_PSIREF = 7, /* u = [0.5 (v0 - v), psiref(X) - Kpsi psi] p = {Kpsi, v0} */
  BMPC_POL_BRAKE_PSIREF = 8            /* u = [softmax([-5, -v], 3), psiref(X) - Kpsi psi]  p = {Kpsi} */
};

/* largest lane reference (grid points) a plan or bmpc_model_eval_ref takes */
#define BMPC_MAX_LANE_REF 4096

typedef struct {
  int32_t kind;
  int32_t reserved;
  double p[4];
} bmpc_policy;

/* POD description of one controller + predictive model (one plan = one batch of egos
 * that share it).  Matrices are row-major with the leading dimension equal to their
 * logical size (Q is n*n, Fx is nFx*n, Fu is nFu*d, ...). */
typedef struct {
  int32_t controller;   /* BMPC_CTRL_*                                   */
  int32_t model;        /* BMPC_MODEL_*                                  */
  int32_t n, d;         /* state / input dimension                      */
  int32_t N, NB, m;     /* steps per branch, branching depth, policies  */
  int32_t nFx, nFu;     /* rows of Fx, Fu                                */
  int32_t maxit;        /* IPM iterations (ECOS default 100)            */
  double dt;
  double ralpha;        /* CVaR alpha (BranchMPC_CVaR ralpha)            */
  double Q[BMPC_MAX_N * BMPC_MAX_N];
  double R[BMPC_MAX_D * BMPC_MAX_D];
  double Qf[BMPC_MAX_N * BMPC_MAX_N];
  double dR[BMPC_MAX_D];
  double Fx[BMPC_MAX_FX * BMPC_MAX_N];
  double bx[BMPC_MAX_FX];
  double Fu[BMPC_MAX_FU * BMPC_MAX_D];
  double bu[BMPC_MAX_FU];
  double Qslack[2];
  /* model constants:
   *   highway   {L, W, s1, N_lane}          (Branch_constants + PredictiveModel ctor)
   *   quadruped {L1, W1, L2, W2, col_tol, s1} (Quad_constants)                       */
  double mc[8];
  double feastol, abstol, reltol; /* ECOS tolerances (defaults 1e-8)              */
  int32_t flags;        /* BMPC_PLAN_* (ABI 2)                            */
  int32_t reserved_flags;
} bmpc_plan_desc;

/* plan flags */
enum {
  BMPC_PLAN_TRANSFORM = 1  /* CVaR plans of the HIGHWAY model that accept the per-solve S / Fx / bx
                              arguments of BranchMPC_CVaR.solve (bmpc_set_transform, bmpc_set_fx);
                              HIGHWAY_MERGE plans always do */
};

typedef struct bmpc_ctx bmpc_ctx;
typedef struct bmpc_plan bmpc_plan;

/* plan geometry returned by bmpc_plan_info (all int32) */
enum {
  BMPC_INFO_T = 0,      /* totalx  (state nodes)                 */
  BMPC_INFO_U,          /* totalu  (input nodes)                 */
  BMPC_INFO_BDIM,       /* non-leaf branches                     */
  BMPC_INFO_NBRANCH,    /* branches incl. root                   */
  BMPC_INFO_NV,         /* primal variables of the solver vector */
  BMPC_INFO_NEQ,        /* equality rows                         */
  BMPC_INFO_NROWS,      /* conic rows (LP + SOC)                 */
  BMPC_INFO_NCONES,     /* second-order cones                    */
  BMPC_INFO_LP,         /* LP rows (dims['l'])                   */
  BMPC_INFO_BATCH,
  BMPC_INFO_WS_DOUBLES, /* per-ego HBM workspace slab (doubles)  */
  BMPC_INFO_SOLVER,     /* solver kernel of the plan's last solve (BMPC_KERNEL_*)      */
  BMPC_INFO_COUNT
};

/* solver kernels (BMPC_INFO_SOLVER): which launch path the last solve took */
enum {
  BMPC_KERNEL_NONE = 0,      /* no solve yet                                              */
  BMPC_KERNEL_IPM_RICH = 1,  /* k_ipm, one wave per ego, topology + coupling system in LDS */
  BMPC_KERNEL_IPM_LEAN = 2,  /* k_ipm, one wave per ego, coupling system in the slab       */
  BMPC_KERNEL_IPM_BLK4 = 3,  /* k_solve_blk, one ego per 4-wave workgroup (small batches)  */
  BMPC_KERNEL_IPM_BLK8 = 4,  /* k_solve_blk, one ego per 8-wave workgroup (small batches)  */
  BMPC_KERNEL_QP_RICH = 5,   /* k_qp (OSQP-class controllers), LDS-rich                    */
  BMPC_KERNEL_QP_LEAN = 6,   /* k_qp, lean                                                 */
  BMPC_KERNEL_LOOP_RICH = 7, /* k_loop (bmpc_*loop_device): env + tree + IPM / QP steps per ego --
                                the CVaR IPM, or the QP solver for the quadruped scene's plans and the
                                overtake scene's BranchMPC (and, on request, robust) plans */
  BMPC_KERNEL_LOOP_LEAN = 8  /* k_loop, lean                                                 */
};

const char* bmpc_last_error(void);
int bmpc_abi_version(void);

int bmpc_open(int hip_device, bmpc_ctx** out);
int bmpc_close(bmpc_ctx* ctx);

int bmpc_plan_create(bmpc_ctx* ctx, const bmpc_plan_desc* desc, int batch, bmpc_plan** out);
int bmpc_plan_destroy(bmpc_plan* plan);
int bmpc_plan_info(const bmpc_plan* plan, int32_t* info /* [BMPC_INFO_COUNT] */);
/* 1 if the solver kernel of the plan's last solve read A of the linearisation from its LDS cache
 * (the CVaR IPM's one-wave kernels of the highway models, batches beyond 8 egos per compute unit
 * on plans with room for it), else 0 */
int bmpc_last_lin_cache(const bmpc_plan* plan);

/* update_backup: policies[batch][m]; mask[batch] (NULL = all egos) */
int bmpc_set_policies(bmpc_plan* plan, const bmpc_policy* policies, const uint8_t* mask);
/* the policies in force [batch][m], including the device-side lane-change re-targets of
 * bmpc_env_step (update_backup, Highway_env_branch.py:117-118) */
int bmpc_get_policies(bmpc_plan* plan, bmpc_policy* policies);
/* forget the warm start (next solve runs inittree); mask NULL = all egos */
int bmpc_reset(bmpc_plan* plan, const uint8_t* mask);

/* One controller solve for every ego of the plan (host buffers).
 *   x, z, xref : [batch][n]
 *   upred      : [batch][U][d]     xpred : [batch][T][n]
 *   branch_w   : [batch][nbranch-1] (BFS order of BT2array)
 *   J          : [batch]            objective (CVaR: the J variable; QP: cost)
 *   status     : [batch]            ECOS exitFlag / OSQP status_val
 *   iters      : [batch]
 * Any output pointer may be NULL. */
int bmpc_solve(bmpc_plan* plan, const double* x, const double* z, const double* xref,
               double* upred, double* xpred, double* branch_w, double* J,
               int32_t* status, int32_t* iters);

/* Same with device pointers, enqueued on `stream` (hipStream_t, NULL = plan stream),
 * no host synchronisation. */
int bmpc_solve_device(bmpc_plan* plan, const double* d_x, const double* d_z,
                      const double* d_xref, double* d_upred, double* d_xpred,
                      double* d_branch_w, double* d_J, int32_t* d_status,
                      int32_t* d_iters, void* stream);

/* Checkpoint / resume of the per-ego warm start: the state the reference keeps
 * in the controller object between solves -- uLin [batch][U+1][d] (shifted by updatetree,
 * MPC_branch.py:1813-1823), the previous branch probabilities p [batch][bdim][m] (argmax
 * child, :1818), the frozen Jcons [batch] (CVaR, :1939) and OldInput [batch][d] (the rate
 * cost of BranchMPCProx, :311,:421).  set marks the egos as initialised (the next solve runs
 * updatetree, not inittree); NULL p / jcons / old_input keep the current values; mask NULL
 * = all egos. */
int bmpc_get_warm_start(bmpc_plan* plan, double* uLin, double* p, double* jcons, double* old_input);
/* robustMPC's warm start: the linearisation trajectory xLin [batch][T][n] and uLin
 * [batch][U][d] (the previous prediction shifted by one step, MPC_branch.py:1429-1431) and
 * OldInput [batch][d]; set marks the egos initialised; get/set NULL pointers skip. */
int bmpc_get_robust_warm_start(bmpc_plan* plan, double* xLin, double* uLin, double* old_input);
int bmpc_set_robust_warm_start(bmpc_plan* plan, const double* xLin, const double* uLin,
                               const double* old_input, const uint8_t* mask);
int bmpc_set_warm_start(bmpc_plan* plan, const double* uLin, const double* p,
                        const double* jcons, const double* old_input, const uint8_t* mask);

/* Per-ego state transformation S and state bound bx of the next solves: the S / bx arguments
 * of BranchMPC_CVaR.solve(x, z, xRef, S, Fx, bx) (MPC_branch.py:2043-2057), used by the merge
 * scene (Highway_env_branch.py:358-367).  HIGHWAY_MERGE plans and HIGHWAY CVaR plans created
 * with BMPC_PLAN_TRANSFORM.
 *   S    [batch][n][n] row-major, or NULL = S is None for every ego (the reference resets
 *        self.S on every solve, so pass it before each solve);
 *   s_on [batch] (NULL = 1 for all egos when S is given): 0 marks "S is None" for that ego;
 *   bx   [batch][nFx], or NULL = keep the current bound (the reference keeps self.bx).
 * The state rows follow the reference's build / update split exactly: the first solve
 * (buildIneqConstr :1894-1901) writes Fx S x <= bx (Fx x <= bx without S) from the current
 * Fx and bx; a later solve rewrites them only when S is on (updateIneqConstr :2025-2036), and
 * then also pushes the collision row's dh[0] to sign(dh0) max(0.1, |dh0|) while its rhs keeps
 * the unclipped h0; with S off the rows and their bound keep their last values (:2016-2024
 * patch the collision row alone).  The cones' middle rows use W1 S (W1 without S) on every
 * solve (:1935-1937, :1995-1998).  mask NULL = all egos. */
int bmpc_set_transform(bmpc_plan* plan, const double* S, const uint8_t* s_on, const double* bx,
                       const uint8_t* mask);
/* Per-ego state-constraint matrix Fx [batch][nFx][n] of the next solves: the Fx argument of
 * BranchMPC_CVaR.solve (self.Fx = Fx, kept until the next one, MPC_branch.py:2055-2056).  It
 * enters the state rows under the rule of bmpc_set_transform (first solve, or S on).  Same
 * plans as bmpc_set_transform; the row count must stay nFx.  mask NULL = all egos. */
int bmpc_set_fx(bmpc_plan* plan, const double* Fx, const uint8_t* mask);
/* The transform in force (host copies; NULL skips): S [batch][n][n], bx [batch][nFx] and
 * flags [batch][2] = {S is on, bx was set} -- what bmpc_set_transform or the device merge scene
 * (bmpc_merge_env_step) last wrote.  Same plans as bmpc_set_transform. */
int bmpc_get_transform(bmpc_plan* plan, double* S, double* bx, double* flags);

/* Tree of the last solve (host copies; NULL skips):
 *   xbar,zbar [batch][T][n]  ubar [batch][U][d]  w [batch][nbranch]
 *   p [batch][bdim][m]       sol [batch][nv]   (full primal vector, reference layout) */
int bmpc_get_tree(bmpc_plan* plan, double* xbar, double* ubar, double* zbar, double* w,
                  double* p, double* sol);
/* dp = d p / d x of every non-leaf branch of the last solve, [batch][bdim][m][n]: the
 * BranchTree.dp that inittree / updatetree set from branch_eval (MPC_branch.py:1711,1842). */
int bmpc_get_branch_dp(bmpc_plan* plan, double* dp);

/* Average device time per call of each kernel over the solves since the last call
 * (HIP events on the launch stream); ms[0] = tree/linearisation kernel, ms[1] = IPM
 * kernel, count = number of solves timed.  Timing must be enabled first.  Timed solves do
 * not synchronise the host: events are read back every 32 solves and by bmpc_timing. */
int bmpc_enable_timing(bmpc_plan* plan, int on);
int bmpc_timing(bmpc_plan* plan, double* ms /* [2] */, int32_t* count);

/* Per-ego phase cycle counters [batch][24] (s_memtime cycles accumulated since plan
 * creation: tree, residuals, scaling, factor, coupling, kkt, tree-solve, refine, -, init,
 * total, kkt-solve count).  All zero unless the library was built with -DBMPC_PROFILE. */
int bmpc_get_counters(bmpc_plan* plan, double* out);

/* Batched model evaluation at B independent points (parity entry for the model
 * functions).  policies [B][m].  Outputs (NULL skips):
 *   A [B][n][n], Bm [B][n][d], C [B][n], xp [B][n]    at (x, u)
 *   p [B][m], dp [B][m][n]                            branch_eval(x, z)
 *   zpred [B][N][m*n]                                 zpred_eval(z)
 *   h0 [B], dh [B][n]                                 col_eval(x, z) */
int bmpc_model_eval(bmpc_ctx* ctx, const bmpc_plan_desc* desc, const bmpc_policy* policies,
                    int B, const double* x, const double* u, const double* z,
                    double* A, double* Bm, double* C, double* xp, double* p, double* dp,
                    double* zpred, double* h0, double* dh);

/* bmpc_model_eval for models whose policies track a lane reference (BMPC_POL_*_PSIREF):
 * the reference psiref(X) is the linear interpolant of values [nref] over the increasing grid
 * [nref] (2 <= nref <= BMPC_MAX_LANE_REF; outside the grid the end cells extend linearly, as
 * casadi.interpolant 'linear' does).  Replaces PredictiveModel_merge's MX graphs with psiref
 * backups (highway_branch_dyn.py:400-502; the merge scene's pred_model[1], main_branch.py:85,
 * whose zpred_eval the scene calls, Highway_env_branch.py:331).  nref = 0: no reference (then
 * no policy may be a *_PSIREF kind). */
int bmpc_model_eval_ref(bmpc_ctx* ctx, const bmpc_plan_desc* desc, const bmpc_policy* policies,
                        int nref, const double* grid, const double* values,
                        int B, const double* x, const double* u, const double* z,
                        double* A, double* Bm, double* C, double* xp, double* p, double* dp,
                        double* zpred, double* h0, double* dh);

/* The lane reference of a HIGHWAY_MERGE plan's *_PSIREF policies (same form as
 * bmpc_model_eval_ref): shared by every ego of the plan, kept until the next call. */
int bmpc_set_lane_ref(bmpc_plan* plan, int nref, const double* grid, const double* values);

/* Closed-loop sim_overtake scene on the device, one scene per ego of a highway plan:
 * replaces Highway_env_branch.Highway_env.step (Highway_env_branch.py:83-184) around the
 * solve and the collision rule of Highway_sim (:421-429).  */
#define BMPC_ENV_STRIDE 16  /* doubles of per-ego scene state  */
#define BMPC_ENV_NSTAT 8    /* doubles of per-ego statistics   */
typedef struct {
  int32_t n_lane;     /* lanes of the env (LB = [W/2, n_lane*3.6 - W/2], :64); 4 in sim_overtake */
  int32_t reserved;
  double L, W, Kpsi;  /* Branch_constants (main_branch.py:37)                        */
  double v0;          /* 20 (Highway_env_branch.py:22)                               */
  double vlen, vwid;  /* vehicle() size 4 x 2.4 (:29), used by the collision test    */
  double target[4];   /* lane-change target of the env's construction-time backup list */
} bmpc_env_desc;

/* One closed-loop step t of every ego (device pointers, enqueued on `stream`):
 *   scene  [batch][BMPC_ENV_STRIDE]  state: ego x[0..3], obstacle z[4..7], the rest zero at
 *                                    t = 0 (the caller writes the initial states);
 *   upred  [batch][U][d]             the last solve's uPred (ignored at t = 0);
 *   J, status, iters [batch]         the last solve's outputs for the statistics (NULL skips);
 *   x, z, xref [batch][4]            out: the next solve's inputs;
 *   stats  [batch][BMPC_ENV_NSTAT]   accumulated {sum J, sum J^2, infeasible, iterations,
 *                                    solves, steps in collision, collided} (NULL skips).
 * The plan's lane-change policies are re-targeted on the device (update_backup, :118). */
int bmpc_env_step(bmpc_plan* plan, const bmpc_env_desc* env, int t, double* d_scene,
                  const double* d_upred, const double* d_J, const int32_t* d_status,
                  const int32_t* d_iters, double* d_x, double* d_z, double* d_xref,
                  double* d_stats, void* stream);

/* nsteps closed-loop steps t0 .. t0+nsteps-1 of every ego, each bmpc_env_step(t) followed by
 * bmpc_solve_device -- the loop main_branch.sim_overtake runs per ego (Highway_sim,
 * Highway_env_branch.py:408-436: env.step -> controller solve, repeated) -- with the same
 * arguments and the same per-ego results, bit for bit.  The egos' loops are independent, so a
 * CVaR plan whose batch takes the one-wave IPM runs them in ONE launch (k_loop: each wave
 * steps its ego through all nsteps without a device-wide boundary between steps, so no step
 * waits for the slowest ego of the previous one); other CVaR batches run the two launches per
 * step.  A BranchMPC plan (BMPC_CTRL_QP) runs ONE launch too, at any batch -- k_loop with the QP
 * solver, BMPC_KERNEL_LOOP_RICH / _LEAN --; a robustMPC plan keeps its launches per step
 * (BMPC_KERNEL_QP_RICH / _LEAN) unless BMPC_LOOP_FUSED=2 asks for that kernel.  BMPC_LOOP_FUSED
 * (read on every call): 0 never fuses; unset or 1 the defaults above; 2 fuses every plan that
 * has a k_loop, robust overtake plans included.
 * d_upred / d_J / d_status / d_iters hold the last solve's outputs on return (the next call's
 * t0 > 0 reads them); d_x / d_z / d_xref the last step's solve inputs.  Highway CVaR, BranchMPC
 * (BMPC_CTRL_QP) and robust plans without transform (the scene's model); -22 otherwise
 * (BMPC_CTRL_PROX: the reference never pairs it with this scene).  An extension of the drop-in ABI
 * for Monte-Carlo closed-loop batches (BASELINE config 5); the reference has no batched loop. */
int bmpc_loop_device(bmpc_plan* plan, const bmpc_env_desc* env, int t0, int nsteps, double* d_scene,
                     double* d_upred, double* d_x, double* d_z, double* d_xref, double* d_J,
                     int32_t* d_status, int32_t* d_iters, double* d_stats, void* stream);

/* Closed-loop sim_merge scene on the device, one scene per ego of a HIGHWAY_MERGE plan: replaces
 * Highway_env_branch.Highway_env_merge.step (Highway_env_branch.py:317-380) around the solve and
 * the collision rule of Highway_sim (:421-429).  The ego starts on the ramp, the obstacle on the
 * main road and keeps backup 0 of the main-road list (maintain_trackV(v0), :345-347). */
typedef struct {
  int32_t n_lane;      /* lanes of the main road (x_ref after the merge: (n_lane - 0.5) 3.6)  */
  int32_t merge_lane;  /* lanes the ramp spans (the ramp's upper bound, :361)                  */
  double merge_s;      /* a vehicle with X > merge_s + 8 has left the ramp (:328-329)         */
  double W, Kpsi;      /* Branch_constants                                                   */
  double v0;           /* 20 (Highway_env_branch.py:19)                                       */
  double psimax;       /* BranchMPC_CVaR.psimax (0.25): the ramp's heading bound around psi0  */
  double vlen, vwid;   /* vehicle() size 4 x 2.4 (:29), used by the collision test            */
} bmpc_merge_env_desc;

/* The merge scene of a plan: its constants and the ramp's lane references refY(X), refpsi(X),
 * linear interpolants of refY [nref] / refpsi [nref] over one increasing grid [nref]
 * (2 <= nref <= BMPC_MAX_LANE_REF; :308-309), copied to the device and kept with the plan.
 * HIGHWAY_MERGE CVaR plans with n = 4, d = 2 and nFx = 4; -22 otherwise.  Independent of
 * bmpc_set_lane_ref: the scene's controller uses the main-road model (no psiref policies). */
int bmpc_set_merge_scene(bmpc_plan* plan, const bmpc_merge_env_desc* desc, int nref, const double* grid,
                         const double* refY, const double* refpsi);

/* One closed-loop merge step t of every ego: bmpc_env_step's arguments without the env (the
 * plan's merge scene; -22 when none was set).  scene [batch][BMPC_ENV_STRIDE]: ego x[0..3],
 * obstacle z[4..7], slot 10 = "the ego has merged" (0 on the ramp), the rest as bmpc_env_step's;
 * all zero but x, z at t = 0.  Besides x, z and xref it writes the solve's S (on), and bx into
 * the egos' transform slots: the next bmpc_solve_device needs no bmpc_set_transform. */
int bmpc_merge_env_step(bmpc_plan* plan, int t, double* d_scene, const double* d_upred, const double* d_J,
                        const int32_t* d_status, const int32_t* d_iters, double* d_x, double* d_z,
                        double* d_xref, double* d_stats, void* stream);

/* nsteps closed-loop merge steps: bmpc_loop_device's arguments without the env, the same
 * contract (bmpc_merge_env_step(t) then bmpc_solve_device per step, bit for bit; ONE k_loop
 * launch when the batch takes the one-wave IPM, BMPC_KERNEL_LOOP_RICH / _LEAN). */
int bmpc_merge_loop_device(bmpc_plan* plan, int t0, int nsteps, double* d_scene, double* d_upred,
                           double* d_x, double* d_z, double* d_xref, double* d_J, int32_t* d_status,
                           int32_t* d_iters, double* d_stats, void* stream);

/* Closed-loop main_quadruped scene on the device, one scene per ego of a QUADRUPED plan with an
 * OSQP-class controller: replaces quadruped_env.Quad_env.step (quadruped_env.py:67-130) around the
 * solve.  The robots' lengths and col_tol come from the plan's model constants (mc). */
typedef struct {
  double switch_clearance; /* the obstacle keeps backup 0 while its clearance exceeds this: 0.5 (:98) */
  double lookahead;        /* x_ref lies at most this far towards x_des: 5 m (:108)                     */
  double near;             /* within this distance of x_des the heading reference is the ego's own: 0.1 (:110) */
} bmpc_quad_env_desc;

/* One closed-loop quadruped step t of every ego: bmpc_env_step's arguments with x, z, xref
 * [batch][3].  scene [batch][BMPC_ENV_STRIDE]: ego x[0..2], obstacle z[3..5], the obstacle's input
 * [6..8], the ego's goal x_des[9..11] (written by the caller with x and z; the scene never changes
 * it), slots 12-14 as bmpc_env_step's -- the reference has no collision rule for this scene, so
 * slot 12 and the statistics' collision columns stay 0 --, the rest zero at t = 0.  QUADRUPED plans
 * with n = d = 3 and an OSQP-class controller (not CVaR); -22 otherwise. */
int bmpc_quad_env_step(bmpc_plan* plan, const bmpc_quad_env_desc* env, int t, double* d_scene,
                       const double* d_upred, const double* d_J, const int32_t* d_status,
                       const int32_t* d_iters, double* d_x, double* d_z, double* d_xref, double* d_stats,
                       void* stream);

/* nsteps closed-loop quadruped steps: bmpc_loop_device's arguments and contract
 * (bmpc_quad_env_step(t) then bmpc_solve_device per step, bit for bit) -- ONE k_loop launch running
 * the QP solver per step (BMPC_KERNEL_LOOP_RICH / _LEAN) unless BMPC_LOOP_FUSED=0 asks for the
 * launches per step (BMPC_KERNEL_QP_RICH / _LEAN).  The same plans as bmpc_quad_env_step. */
int bmpc_quad_loop_device(bmpc_plan* plan, const bmpc_quad_env_desc* env, int t0, int nsteps,
                          double* d_scene, double* d_upred, double* d_x, double* d_z, double* d_xref,
                          double* d_J, int32_t* d_status, int32_t* d_iters, double* d_stats, void* stream);

/* The closed loops' per-step recorder: what the reference's own loops keep of an episode --
 * Highway_sim's state_rec / input_rec / backup_choice_rec / xPred_rec / zPred_rec / branch_w_rec
 * (Highway_env_branch.py:393-444) and quadruped_env.sim's -- written on the device by every step of
 * bmpc_loop_device, bmpc_merge_loop_device and bmpc_quad_loop_device, on whichever launch path the
 * plan takes (one fused k_loop launch or the launches per step).
 *
 * A row is in the device scene's own convention, state and inputs OF step t: the scene row holds
 * the ego x and obstacle z that step t's solve was given, the obstacle's backup choice and input of
 * step t, the collision flag and the step count t + 1; u is the input that solve returned, which
 * the Euler step of t + 1 applies.  Highway_sim records after the step: its state_rec[t] is row
 * t + 1's x (and z), its input_rec[t] is row t's u, its backup_choice_rec[t], xPred_rec[t],
 * zPred_rec[t] and branch_w_rec[t] are row t's.  The state after the last recorded input is not in
 * the record (no step computed it); it is the first row of the loop's continuation. */
typedef struct {
  int32_t capacity;   /* rows per ego, >= 1 */
  int32_t t_base;     /* row r of an ego holds closed-loop step t_base + r; a step outside
                         [t_base, t_base + capacity) is not recorded and touches nothing */
  /* core columns, all required (device pointers, caller-owned, ego-major) */
  double*  scene;     /* [batch][capacity][BMPC_ENV_STRIDE]  the ego's scene row as step t's solve saw it
                         (after the scene step of t, before the Euler step of t+1) */
  double*  xref;      /* [batch][capacity][n]   the solve's x_ref (x and z are in the scene row) */
  double*  u;         /* [batch][capacity][d]   uPred[0] of step t's solve: the input applied next */
  double*  J;         /* [batch][capacity] */
  int32_t* status;    /* [batch][capacity] */
  int32_t* iters;     /* [batch][capacity] */
  /* optional columns, NULL skips */
  double*  upred;     /* [batch][capacity][U][d] */
  double*  xpred;     /* [batch][capacity][T][n] */
  double*  zpred;     /* [batch][capacity][T][n]  the tree's obstacle predictions (zbar of bmpc_get_tree) */
  double*  branch_w;  /* [batch][capacity][nbranch-1] */
} bmpc_loop_record;

/* Attach (copy of *rec kept with the plan) or detach (rec == NULL) the recorder of the plan's
 * closed loops.  Host state only: nothing is enqueued or waited for, and the struct travels to the
 * kernels by value, so a loop already enqueued keeps the recorder it was launched with.  While
 * attached, every step run by the three loop entry points writes its row; a loop continued over
 * several calls fills consecutive rows (rows are addressed by t, not by call).  The single-step
 * entry points (bmpc_env_step, bmpc_solve_device, ...) do not record.  The loops' other results --
 * scene, outputs, statistics, warm start -- are the same bits with and without a recorder.  The
 * columns must stay allocated until the last loop launched with them has finished.  -22 with a
 * message for capacity < 1, a NULL core column, or zpred on a BMPC_CTRL_ROBUST plan (its tree
 * keeps no obstacle prediction per state node). */
int bmpc_set_loop_record(bmpc_plan* plan, const bmpc_loop_record* rec);

/* The obstacle's backup choice in the device closed loops.  The reference's scenes are
 * deterministic: the overtake obstacle takes the first argmax of a safety value
 * (Highway_env_branch.py:137-149), the quadruped obstacle keeps backup 0 while it is clear, else
 * the argmax (quadruped_env.py:92-101) -- BMPC_OBS_ARGMAX, what every plan does until a sampler is
 * attached.  BMPC_OBS_SAMPLE_MODEL draws the choice from the distribution the controllers plan
 * against, branch_eval's p_j(x, z) = prob_weight(bf_traj_j) / sum (highway_branch_dyn.py:298-301,
 * :355-359) at the step's pre-step state with the policies in force before the step's lane-change
 * re-targeting, so that a Monte-Carlo population shows a controller the less likely branches too.
 * An extension: the reference has no sampled obstacle.
 *
 * One draw per (ego, epoch), addressed and never consumed: Philox4x32-10 (csrc/bmpc_rng.h) at
 *   counter = {lo32(g), hi32(g), epoch, purpose},  key = {lo32(seed), hi32(seed)},
 * g = ego_base + e the ego's global index, epoch = t / hold, purpose 0 = the obstacle's policy
 * (other values reserved), u = ((o0 >> 5) 2^26 + (o1 >> 6)) / 2^53 in [0, 1).  The choice is the
 * smallest j with u < p_0 + ... + p_j (m - 1 if none), taken at t % hold == 0 and kept, in the scene
 * row's slot 13, for the epoch's other steps.  The launch path, the split of a loop over calls and
 * the shard an ego lives in (ego_base = the shard's first global ego) cannot change a draw;
 * bmpc/rng.py restates it in NumPy. */
enum { BMPC_OBS_ARGMAX = 0, BMPC_OBS_SAMPLE_MODEL = 1 };
typedef struct {
  int32_t  mode;      /* BMPC_OBS_*                                           */
  int32_t  hold;      /* >= 1: closed-loop steps a sampled choice is kept     */
  uint64_t seed;
  int64_t  ego_base;  /* >= 0: global index of the plan's ego 0 (its shard's lo) */
} bmpc_obstacle_sampling;
#ifdef __cplusplus
static_assert(sizeof(bmpc_obstacle_sampling) == 24,
              "bmpc_obstacle_sampling is 24 bytes: mode 0, hold 4, seed 8, ego_base 16");
#endif

/* Attach (copy of *s kept with the plan) or detach (s == NULL: BMPC_OBS_ARGMAX) the obstacle
 * sampler of the plan's overtake or quadruped scene.  Host state only, like bmpc_set_loop_record:
 * nothing is enqueued, and a loop already launched keeps the sampler it was launched with.  While
 * attached, bmpc_loop_device / bmpc_quad_loop_device on either launch path and the single-step
 * bmpc_env_step / bmpc_quad_env_step all obey it (unlike the recorder it changes what a step
 * computes, so a manual loop gets the same bits).  A sampler attached mid-episode, at a t with
 * t % hold != 0, keeps the scene row's last choice until the next epoch boundary.  With mode
 * BMPC_OBS_ARGMAX or nothing attached every path computes the bits it computed without this entry.
 * -22 with a message for an unknown mode, hold < 1, ego_base < 0, a HIGHWAY_MERGE plan (the merge
 * scene's obstacle never chooses), a plan with BMPC_PLAN_TRANSFORM, or a CVaR quadruped plan.  The
 * modes BMPC_OBS_SAMPLE_TILTED and BMPC_OBS_SCRIPT (below) need bmpc_set_obstacle_proposal first. */
int bmpc_set_obstacle_sampling(bmpc_plan* plan, const bmpc_obstacle_sampling* s);

/* Weighted obstacle scenarios: two more values of bmpc_obstacle_sampling.mode, both chosen by a
 * proposal attached to the plan beforehand, and a running log-weight per ego in the overtake and
 * quadruped scene rows' slot BMPC_ENV_LOGW (free in both layouts; the merge scene never writes it):
 *
 *   scene [batch][BMPC_ENV_STRIDE], slot 15 = BMPC_ENV_LOGW: accumulated onto whatever the row
 *   holds -- the caller zeroes it to start an estimate -- at the epoch starts (t % hold == 0) of
 *   modes 2 and 3 only; modes 0 and 1 and a plan without a sampler never write it.
 *
 * BMPC_OBS_SAMPLE_TILTED (importance sampling): at an epoch start the scene forms mode 1's weights
 * w_j (the same state, the same policies before the step's re-targeting) and draws, by the same
 * inverse CDF at the same draw (purpose 0 at (seed, ego_base + e, t / hold)), from w_j b_j instead
 * of w_j, b = tilt; it adds log((sum_k w_k b_k) / (b_j sum_k w_k)) = log(p_j / q_j) for the chosen j
 * to BMPC_ENV_LOGW, both sums in the order k = 0, 1, ...  With b == 1 it computes mode 1's bits and
 * adds exactly 0.  exp(BMPC_ENV_LOGW) is the likelihood ratio of the episode's choice sequence.
 *
 * BMPC_OBS_SCRIPT (prescribed choices): at an epoch start the choice of ego e is
 * script[e][t / hold - epoch0], clamped to [0, m - 1]; no draw is made and the seed is ignored.  It
 * adds log(w_j / sum_k w_k) = log p_j, the model's probability of the prescribed choice: over a full
 * enumeration of the choice sequences from one state the weights sum to one.
 *
 * Inside an epoch both keep the row's last choice and leave BMPC_ENV_LOGW alone, as mode 1 does. */
#define BMPC_ENV_LOGW 15
enum { BMPC_OBS_SAMPLE_TILTED = 2, BMPC_OBS_SCRIPT = 3 };
typedef struct {
  double tilt[BMPC_MAX_M];  /* b_j, finite and > 0 for j < m (mode BMPC_OBS_SAMPLE_TILTED)               */
  const int32_t* script;    /* device table [batch][script_epochs], caller-owned (mode BMPC_OBS_SCRIPT)  */
  int32_t script_epochs;    /* >= 0; 0: no script                                                        */
  int32_t epoch0;           /* >= 0: the epoch of the table's column 0                                   */
} bmpc_obstacle_proposal;
#ifdef __cplusplus
static_assert(sizeof(bmpc_obstacle_proposal) == 8 * BMPC_MAX_M + 16 && offsetof(bmpc_obstacle_proposal, tilt) == 0 &&
                  offsetof(bmpc_obstacle_proposal, script) == 8 * BMPC_MAX_M &&
                  offsetof(bmpc_obstacle_proposal, script_epochs) == 8 * BMPC_MAX_M + 8 &&
                  offsetof(bmpc_obstacle_proposal, epoch0) == 8 * BMPC_MAX_M + 12,
              "bmpc_obstacle_proposal is 48 bytes: tilt 0, script 32, script_epochs 40, epoch0 44");
#endif

/* Attach (a copy of *q: the plan keeps one on the host and one on the device, which the scene
 * kernels read through one pointer) or detach (q == NULL) the plan's obstacle proposal.  The script
 * table itself stays the caller's and must outlive its use.  Re-attaching waits for the plan's
 * streams before the device copy is overwritten, so a loop already launched keeps what it was
 * launched with.  While the sampler's mode is BMPC_OBS_SCRIPT every entry that steps a scene --
 * bmpc_env_step, bmpc_quad_env_step, bmpc_loop_device, bmpc_quad_loop_device -- checks on the host,
 * before anything is enqueued, that the epochs of its steps lie in [epoch0, epoch0 + script_epochs),
 * and returns -22 otherwise.  -22 with a message for a tilt entry (j < m) that is not finite and
 * > 0, script_epochs < 0 or epoch0 < 0, script_epochs > 0 with a null table, detaching (or dropping
 * the script) while the sampler's mode needs it, and the plans bmpc_set_obstacle_sampling refuses;
 * bmpc_set_obstacle_sampling in turn refuses modes 2 and 3 without a proposal and mode 3 without
 * a script. */
int bmpc_set_obstacle_proposal(bmpc_plan* plan, const bmpc_obstacle_proposal* q);

/* Process noise in the device closed loops: an actuation disturbance on the ego and on the obstacle,
 * drawn per step.  Without it both vehicles execute their inputs exactly, so a controller is only
 * ever tested against the model it plans with.  An extension: the reference's scenes have no noise.
 *
 * The law BMPC_DISTURB_IH4 is a unit-variance, bounded, near-Gaussian variate made of integers
 * (csrc/bmpc_rng.h; bmpc/rng.py restates it), the same double on host, device and in NumPy:
 *   o[0..3] = Philox4x32-10(counter {lo32(g), hi32(g), t, purpose}, key {lo32(seed), hi32(seed)})
 *   s  = (int64)o0 + o1 + o2 + o3 - 2 (2^32 - 1)         exact, |s| < 2^34
 *   xi = (double)s * 0x1.bb67ae8584caap-32               sqrt(3) / 2^32: one rounding
 * (Irwin-Hall with four terms: mean 0, variance 1 - 2^-64, kurtosis 2.7, |xi| <= 2 sqrt(3)), with
 * g = ego_base + e the ego's global index, t the closed-loop step whose input is disturbed and
 * purpose = 8 + c for component c of the obstacle's input, 12 + c for the ego's (c < BMPC_MAX_D).
 *
 * It acts only in the Euler step post(t-1) of the three scenes: the ego moves with
 * uPred[0][c] + sigma_ego[c] * xi(g, t-1, 12 + c), the obstacle with its chosen input
 * + sigma_obs[c] * xi(g, t-1, 8 + c), the product rounded before it is added.  A component with
 * sigma == 0 makes no draw.  The scene row's obstacle-input slot and the recorder's u column keep the
 * nominal inputs; the collision rule, the obstacle's choice, the x_ref rules and BMPC_ENV_LOGW are
 * untouched (the noise has the same law under the model and under a proposal), and nothing is
 * clipped to the actuator bounds.  A draw is addressed by slot, so clones made by bmpc_gather_egos
 * diverge by themselves. */
enum { BMPC_DISTURB_NONE = 0, BMPC_DISTURB_IH4 = 1 };
typedef struct {
  int32_t  law, reserved;          /* BMPC_DISTURB_*; reserved is ignored                 */
  uint64_t seed;
  int64_t  ego_base;               /* >= 0, as in bmpc_obstacle_sampling                  */
  double   sigma_ego[BMPC_MAX_D];  /* >= 0 and finite; 0 at the components >= d           */
  double   sigma_obs[BMPC_MAX_D];
} bmpc_disturbance;
#ifdef __cplusplus
static_assert(sizeof(bmpc_disturbance) == 24 + 16 * BMPC_MAX_D && offsetof(bmpc_disturbance, law) == 0 &&
                  offsetof(bmpc_disturbance, seed) == 8 && offsetof(bmpc_disturbance, ego_base) == 16 &&
                  offsetof(bmpc_disturbance, sigma_ego) == 24 &&
                  offsetof(bmpc_disturbance, sigma_obs) == 24 + 8 * BMPC_MAX_D,
              "bmpc_disturbance is 88 bytes: law 0, seed 8, ego_base 16, sigma_ego 24, sigma_obs 56");
#endif

/* Attach (a copy of *d: the plan keeps one on the host and one on the device, behind the proposal's,
 * which the scene kernels read through the same pointer) or detach (d == NULL) the plan's
 * disturbance.  Re-attaching waits for the plan's streams before the device copy is overwritten, so
 * a loop already launched keeps what it was launched with; detaching leaves the device copy
 * allocated (and, where an attached proposal keeps the pointer in use, clears its law the same
 * way).  Obeyed by bmpc_loop_device, bmpc_merge_loop_device and bmpc_quad_loop_device on either
 * launch path and by the single-step bmpc_env_step, bmpc_merge_env_step and bmpc_quad_env_step, so
 * a manual loop gets the same bits.  With law BMPC_DISTURB_NONE, all sigmas
 * zero or nothing attached every path computes the bits it computed without this entry.  -22 with a
 * message for an unknown law, ego_base < 0, a negative or non-finite sigma, a non-zero sigma at a
 * component >= d, and a plan that none of the three scene entries accepts. */
int bmpc_set_disturbance(bmpc_plan* plan, const bmpc_disturbance* d);

/* Observation noise in the device closed loops: a perception model between the scene and the
 * controller.  Without it every scene step hands the solve the true ego state x and the true obstacle
 * state z, from which the tree derives the branch probabilities, the obstacle rollouts and the
 * collision rows.  An extension: the reference's controllers see the scene exactly.
 *
 * The law BMPC_OBSERVE_IH4 is the disturbance's variate xi (above; csrc/bmpc_rng.h rng_ih4, restated
 * by bmpc/rng.py) at the counter {lo32(g), hi32(g), t, purpose} with key = seed, g = ego_base + e the
 * ego's global index, t the closed-loop step whose solve sees the observation, and
 * purpose = 16 + c for component c of the obstacle's state, 24 + c for the ego's (c < BMPC_MAX_N).
 *
 * While it is attached each of the three scene steps changes only its last two outputs, the vectors
 * the next solve reads:
 *   x_out[c] = x[c] + sigma_x[c] * xi(g, t, 24 + c)        c < n
 *   z_out[c] = z[c] + sigma_z[c] * xi(g, t, 16 + c)
 * the product rounded before it is added; a component with sigma == 0 makes no draw and passes
 * through to the bit.  Everything else in the step stays on the truth: the Euler steps and the
 * collision rule, the merged flag, the lane bookkeeping and the lane-change re-targeting, the
 * obstacle's choice in every sampler mode with its input and BMPC_ENV_LOGW, the statistics, x_ref and
 * the merge scene's S and bx.  The scene row and the recorder keep the true states; what the solve saw
 * is row + sigma * xi, reproducible on the host.  The loop entries' d_x / d_z hold the observed
 * vectors.  There is no per-ego state: a draw is addressed by slot, so clones made by
 * bmpc_gather_egos diverge by themselves. */
enum { BMPC_OBSERVE_NONE = 0, BMPC_OBSERVE_IH4 = 1 };
typedef struct {
  int32_t  law, reserved;          /* BMPC_OBSERVE_*; reserved is ignored                 */
  uint64_t seed;
  int64_t  ego_base;               /* >= 0, as in bmpc_obstacle_sampling                  */
  double   sigma_x[BMPC_MAX_N];    /* the ego's own state: >= 0 and finite; 0 at the components >= n */
  double   sigma_z[BMPC_MAX_N];    /* the obstacle's state                                */
} bmpc_observation;
#ifdef __cplusplus
static_assert(sizeof(bmpc_observation) == 24 + 16 * BMPC_MAX_N && offsetof(bmpc_observation, law) == 0 &&
                  offsetof(bmpc_observation, seed) == 8 && offsetof(bmpc_observation, ego_base) == 16 &&
                  offsetof(bmpc_observation, sigma_x) == 24 &&
                  offsetof(bmpc_observation, sigma_z) == 24 + 8 * BMPC_MAX_N,
              "bmpc_observation is 152 bytes: law 0, seed 8, ego_base 16, sigma_x 24, sigma_z 88");
#endif

/* Attach (a copy of *o: one on the host and one on the device, behind the proposal's and the
 * disturbance's in the block the scene kernels read through one pointer) or detach (o == NULL) the
 * plan's observation model; bmpc_set_disturbance's contract.  Re-attaching waits for the plan's
 * streams before the device copy is overwritten; detaching leaves the device copy allocated (and,
 * where an attached proposal or disturbance keeps the pointer in use, clears its law the same way).
 * Obeyed by bmpc_loop_device, bmpc_merge_loop_device and bmpc_quad_loop_device on either launch path
 * and by the single-step bmpc_env_step, bmpc_merge_env_step and bmpc_quad_env_step, so a manual loop
 * gets the same bits.  With law BMPC_OBSERVE_NONE, all sigmas zero or nothing attached every path
 * computes the bits it computed without this entry.  -22 with a message for an unknown law,
 * ego_base < 0, a negative or non-finite sigma, a non-zero sigma at a component >= n, and a plan that
 * none of the three scene entries accepts. */
int bmpc_set_observation(bmpc_plan* plan, const bmpc_observation* o);

/* Resampling a weighted population between loop segments (sequential Monte Carlo / particle
 * splitting): egos of large weight are cloned into the slots of egos of negligible weight and every
 * ego continues with the population's mean weight, so that montecarlo.estimate's plain estimate stays
 * unbiased while the solves go where the probability mass is.  An extension: the reference has no
 * populations.
 *
 * The ancestor rule is exact integer arithmetic (csrc/bmpc_resample.h; bmpc/resample.py restates it):
 *   M = max logw (M = -inf: nothing is resampled);  k_i = floor(exp(logw_i - M) 2^40) as uint64;
 *   C the inclusive prefix sums of k, S = C_{B-1}, Q = sum k_i^2 exactly in 128 bits;
 *   ess = (double)S (double)S / (double)Q, conversions rounded to nearest; resample iff
 *   ess < ess_fraction * batch in double (any ess_fraction > 1 always resamples);
 *   one draw per resampling: Philox4x32-10 (csrc/bmpc_rng.h) at counter {lo32(ego_base),
 *   hi32(ego_base), round, purpose 1}, key = seed; u53 its 53-bit integer ((o0 >> 5) 2^26 + (o1 >> 6)),
 *   U0 = (u53 S) >> 53;
 *   systematic resampling: child j's raw ancestor is the smallest i with C_i B > U0 + j S; n_i children
 *   have raw ancestor i;
 *   arrangement: a slot with n_i >= 1 keeps ancestor[i] = i; the dead slots (n_i = 0), in increasing
 *   order, receive the surplus list (each i repeated n_i - 1 times, in increasing i) -- sources are never
 *   destinations, most egos do not move and a surviving slot's recorder rows stay one trajectory;
 *   when resampled, every ego's new log-weight is M + log S - log batch - 40 log 2 (the log of the mean
 *   weight).  A NaN or +inf log-weight refuses the resampling.  When nothing is resampled the ancestors
 *   are the identity and no byte of any ego changes. */
enum { BMPC_RESAMPLE_SYSTEMATIC = 0 };
typedef struct {
  int32_t  scheme;        /* BMPC_RESAMPLE_SYSTEMATIC (other values reserved: -22)              */
  uint32_t round;         /* addresses the draw: e.g. the step t at which the population is resampled */
  double   ess_fraction;  /* resample iff ess < ess_fraction * batch; finite and >= 0              */
  uint64_t seed;
  int64_t  ego_base;      /* >= 0, as in bmpc_obstacle_sampling                                   */
} bmpc_resample_desc;
#ifdef __cplusplus
static_assert(sizeof(bmpc_resample_desc) == 32 && offsetof(bmpc_resample_desc, scheme) == 0 &&
                  offsetof(bmpc_resample_desc, round) == 4 && offsetof(bmpc_resample_desc, ess_fraction) == 8 &&
                  offsetof(bmpc_resample_desc, seed) == 16 && offsetof(bmpc_resample_desc, ego_base) == 24,
              "bmpc_resample_desc is 32 bytes: scheme 0, round 4, ess_fraction 8, seed 16, ego_base 24");
#endif

/* info [BMPC_RESAMPLE_NINFO] doubles: {resampled (0 / 1), ess, M, the new log-weight (log of the mean
 * weight), (double)S, survivors (slots with n_i >= 1; batch when not resampled), NaN / +inf log-weights
 * seen, 0}.  With a NaN / +inf log-weight or M = -inf nothing is quantised: ess, the new log-weight and
 * S are 0 and the weights written are 0. */
#define BMPC_RESAMPLE_NINFO 8
#define BMPC_RESAMPLE_MAX_BATCH (1 << 20)

/* The ancestors of a population of `batch` egos from their log-weights d_logw[e * stride] (device
 * pointers; stride in doubles): d_ancestor [batch] int32, d_weight [batch] uint64 the k_i used (NULL
 * skips), d_info as above.  A pure function of its inputs that needs no plan.  Enqueued on `stream`
 * (NULL: a stream of the context's), no host synchronisation; its scratch is kept with the context
 * and calls on one context are ordered with each other on the device.  -22 with a message for
 * batch < 1 or > BMPC_RESAMPLE_MAX_BATCH, stride < 1, an unknown scheme, a negative or non-finite
 * ess_fraction, ego_base < 0 and null required pointers. */
int bmpc_population_ancestors(bmpc_ctx* ctx, const bmpc_resample_desc* desc, int batch, const double* d_logw,
                              int stride, int32_t* d_ancestor, uint64_t* d_weight, double* d_info, void* stream);

/* The loop entries' per-ego device buffers with their shapes: scene [batch][BMPC_ENV_STRIDE], upred
 * [batch][U][d], x / z / xref [batch][n], J / status / iters [batch], stats [batch][BMPC_ENV_NSTAT].
 * NULL skips a buffer. */
typedef struct {
  double *scene, *upred, *x, *z, *xref, *J;
  int32_t *status, *iters;
  double* stats;
} bmpc_ego_buffers;

/* For every j with a[j] != j, ego j becomes a copy of ego a[j] as it was before the call -- for any
 * map a (a permutation and a broadcast both work: the copies are staged through the plan's scratch);
 * entries of a are clamped to [0, batch).  What moves: the ego's rows of the given buffers (NULL
 * bufs: none), its policy row, and the spans of its workspace slab that a later solve or scene step
 * reads before writing them (csrc/bmpc_resample.h, ego_state_spans: the warm start uLin, the previous
 * branch probabilities, Jcons / OldInput / the other misc slots, the last predictions and solution,
 * robustMPC's xLin, the transform slots of transform and merge plans).  Every plan kind; enqueued on
 * `stream` (NULL: the plan's), no host synchronisation.  The recorder is not touched: rows stay
 * addressed by slot, and a is the genealogy. */
int bmpc_gather_egos(bmpc_plan* plan, const int32_t* d_ancestor, const bmpc_ego_buffers* bufs, void* stream);

/* bmpc_population_ancestors from the scene's slot BMPC_ENV_LOGW, then bmpc_gather_egos, then the new
 * log-weight into slot BMPC_ENV_LOGW of every ego -- all under the device-side "resampled" decision
 * (the gather kernels read info[0] and do nothing when it is 0), no host synchronisation between the
 * stages.  bufs->scene, d_ancestor [batch] and d_info [BMPC_RESAMPLE_NINFO] are required.  The plans
 * bmpc_set_obstacle_sampling accepts; -22 otherwise with the same messages, and for what
 * bmpc_population_ancestors refuses. */
int bmpc_resample_device(bmpc_plan* plan, const bmpc_resample_desc* desc, const bmpc_ego_buffers* bufs,
                         int32_t* d_ancestor, double* d_info, void* stream);

/* HMM belief-augmented linearisation, batched over B points: replaces
 * HMM_backup_dyn.PredictiveModel.regressionAndLinearization (HMM_backup_dyn.py:216-237) of
 * the graph of calc_xp_expr (:238-276).  M agents (1..4), m backups (1..4), nb = 4 + M*m.
 *   hc      [8]           {dt, L, W, ylb, yub, col_alpha, s1, tran_diag} (Branch_constants)
 *   xb      [B][nb]       [x; b stacked column-major] (CasADi reshape, :244)
 *   u       [B][2]        xbackup [B][M*m][4] (row m*i+j: agent i under backup j)
 * Outputs (NULL skips): xbp [B][nb], A [B][nb][nb], Bm [B][nb][2], C [B][nb],
 *   h0 [B][M][m], Jh [B][M][m][nb]   (h0_i = h_i - Jh_i xb, :226-229) */
int bmpc_hmm_eval(bmpc_ctx* ctx, int M, int m, const double* hc, int B, const double* xb, const double* u,
                  const double* xbackup, double* xbp, double* A, double* Bm, double* C, double* h0,
                  double* Jh);

/* Batched convex QP in OSQP's problem form (the solver behind the belief LTV-MPC,
 * PredictiveControllers.MPC.osqp_solve_qp, PredictiveControllers.py:310-340, which the
 * reference hands to OSQP(...).setup(P, q, A, l, u, polish=True).solve()):
 *     minimise 1/2 x'Px + q'x  subject to  l <= A x <= u
 * by a Mehrotra interior-point method on the quasidefinite KKT matrix, band-factored after a
 * reverse Cuthill-McKee ordering, one wave per problem (csrc/bmpc_bandqp.h).  The problems of
 * a batch share one sparsity pattern:
 *   Pp [n+1], Pi [nnzP]      upper triangle of P, CSC (OSQP keeps only the upper triangle)
 *   Ap [n+1], Ai [nnzA]      A (m x n), CSC; row indices increasing within a column
 *   Px [batch][nnzP], Ax [batch][nnzA], q [batch][n], l, u [batch][m]
 * |bound| >= 1e20 is infinite; a row with l == u is an equality; every problem must classify
 * every row alike.  Outputs: x [batch][n]; y [batch][m] (OSQP's dual, P x + q + A'y = 0;
 * NULL skips); status [batch] (1 solved to eps, -2 max_iter reached, -8 numerical failure);
 * iters [batch] (NULL skips); info [4] = {KKT dimension, bandwidth, inequality rows, band
 * entries} (NULL skips).  -22 when the KKT band does not fit the 160 KB LDS window. */
int bmpc_qp_solve(bmpc_ctx* ctx, int n, int m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                  const int32_t* Ai, int batch, const double* Px, const double* q, const double* Ax, const double* l,
                  const double* u, int max_iter, double eps, double* x, double* y, int32_t* status, int32_t* iters,
                  int32_t* info);

#ifdef __cplusplus
}
#endif
#endif /* BMPC_H */
