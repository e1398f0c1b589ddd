"""ctypes mirror of ``include/bmpc.h`` (the C ABI of libbmpc.so)."""
from __future__ import annotations

import ctypes as C

import numpy as np

MAX_N, MAX_D, MAX_FX, MAX_FU, MAX_M = 8, 4, 8, 8, 4

CTRL_CVAR, CTRL_PROX, CTRL_QP, CTRL_ROBUST = 0, 1, 2, 3
MODEL_HIGHWAY, MODEL_QUADRUPED, MODEL_HIGHWAY_MERGE = 0, 1, 2
PLAN_TRANSFORM = 1      # bmpc_plan_desc.flags: solve's S / Fx / bx on a HIGHWAY CVaR plan
POL_MAINTAIN, POL_BRAKE, POL_LC, POL_MAINTAIN_TRACKV, POL_FORWARD, POL_STOP = range(6)
# the merge ramp's lane-reference (psiref) tracking backups (include/bmpc.h)
POL_MAINTAIN_PSIREF, POL_MAINTAIN_TRACKV_PSIREF, POL_BRAKE_PSIREF = 6, 7, 8
MAX_LANE_REF = 4096

(INFO_T, INFO_U, INFO_BDIM, INFO_NBRANCH, INFO_NV, INFO_NEQ, INFO_NROWS, INFO_NCONES,
 INFO_LP, INFO_BATCH, INFO_WS_DOUBLES, INFO_SOLVER, INFO_COUNT) = range(13)
# solver kernels reported in INFO_SOLVER (include/bmpc.h BMPC_KERNEL_*)
(KERNEL_NONE, KERNEL_IPM_RICH, KERNEL_IPM_LEAN, KERNEL_IPM_BLK4, KERNEL_IPM_BLK8, KERNEL_QP_RICH,
 KERNEL_QP_LEAN, KERNEL_LOOP_RICH, KERNEL_LOOP_LEAN) = range(9)


class Policy(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 4)]


class PlanDesc(C.Structure):
    _fields_ = [
        ("controller", C.c_int32), ("model", C.c_int32),
        ("n", C.c_int32), ("d", C.c_int32),
        ("N", C.c_int32), ("NB", C.c_int32), ("m", C.c_int32),
        ("nFx", C.c_int32), ("nFu", C.c_int32),
        ("maxit", C.c_int32),
        ("dt", C.c_double), ("ralpha", C.c_double),
        ("Q", C.c_double * (MAX_N * MAX_N)),
        ("R", C.c_double * (MAX_D * MAX_D)),
        ("Qf", C.c_double * (MAX_N * MAX_N)),
        ("dR", C.c_double * MAX_D),
        ("Fx", C.c_double * (MAX_FX * MAX_N)),
        ("bx", C.c_double * MAX_FX),
        ("Fu", C.c_double * (MAX_FU * MAX_D)),
        ("bu", C.c_double * MAX_FU),
        ("Qslack", C.c_double * 2),
        ("mc", C.c_double * 8),
        ("feastol", C.c_double), ("abstol", C.c_double), ("reltol", C.c_double),
        ("flags", C.c_int32), ("reserved_flags", C.c_int32),
    ]


ENV_STRIDE, ENV_NSTAT = 16, 8
# scene state / statistics slots (bmpc_env.h)
ENV_X, ENV_Z, ENV_UOBS, ENV_LANE0, ENV_LANE1, ENV_COLL, ENV_OBSPOL, ENV_STEPS = 0, 4, 8, 10, 11, 12, 13, 14
ENV_LOGW = 15   # overtake and quadruped scenes: the running log-weight of OBS_SAMPLE_TILTED / OBS_SCRIPT (BMPC_ENV_LOGW)
ENVS_J, ENVS_J2, ENVS_INFEAS, ENVS_ITERS, ENVS_SOLVES, ENVS_COLL_STEPS, ENVS_COLLIDED = range(7)


class EnvDesc(C.Structure):
    """bmpc_env_desc: the sim_overtake scene (Highway_env_branch.py:46-72)."""
    _fields_ = [("n_lane", C.c_int32), ("reserved", C.c_int32), ("L", C.c_double), ("W", C.c_double),
                ("Kpsi", C.c_double), ("v0", C.c_double), ("vlen", C.c_double), ("vwid", C.c_double),
                ("target", C.c_double * 4)]


def make_env(n_lane=4, L=4.0, W=2.5, Kpsi=0.1, v0=20.0, target=(0.5, 1.8, 15.0, 0.0), vlen=4.0, vwid=2.4):
    """Scene constants of main_branch.sim_overtake: Branch_constants (main_branch.py:37), the
    construction-time lane-change target xRef (:39), vehicle() size (Highway_env_branch.py:29)."""
    E = EnvDesc()
    E.n_lane, E.L, E.W, E.Kpsi, E.v0, E.vlen, E.vwid = int(n_lane), L, W, Kpsi, v0, vlen, vwid
    _fill(E.target, target)
    return E


ENV_MERGED = ENV_LANE0   # merge scene: "the ego has merged" (0 on the ramp)


class MergeEnvDesc(C.Structure):
    """bmpc_merge_env_desc: the sim_merge scene (Highway_env_branch.py:275-380)."""
    _fields_ = [("n_lane", C.c_int32), ("merge_lane", C.c_int32), ("merge_s", C.c_double), ("W", C.c_double),
                ("Kpsi", C.c_double), ("v0", C.c_double), ("psimax", C.c_double), ("vlen", C.c_double),
                ("vwid", C.c_double)]


def make_merge_env(n_lane=2, merge_lane=1, merge_s=50.0, W=2.5, Kpsi=0.1, v0=20.0, psimax=0.25, vlen=4.0, vwid=2.4):
    """Scene constants of main_branch.sim_merge (main_branch.py:53-88): Branch_constants, the ramp
    of merge_geometry(N_lane, 1, 50, 300), BranchMPC_CVaR.psimax, vehicle() size."""
    E = MergeEnvDesc()
    E.n_lane, E.merge_lane = int(n_lane), int(merge_lane)
    E.merge_s, E.W, E.Kpsi, E.v0, E.psimax, E.vlen, E.vwid = merge_s, W, Kpsi, v0, psimax, vlen, vwid
    return E


# quadruped scene: three-component states in the slots before ENV_COLL (bmpc_env_quad.h)
QENV_X, QENV_Z, QENV_UOBS, QENV_XDES = 0, 3, 6, 9


class QuadEnvDesc(C.Structure):
    """bmpc_quad_env_desc: the main_quadruped scene's literals (quadruped_env.py:98-110)."""
    _fields_ = [("switch_clearance", C.c_double), ("lookahead", C.c_double), ("near", C.c_double)]


def make_quad_env(switch_clearance=0.5, lookahead=5.0, near=0.1):
    """Scene constants of quadruped_env.Quad_env.step: the obstacle keeps backup 0 above 0.5 m of
    clearance (:98), x_ref lies 5 m ahead (:108), the ego's own heading within 0.1 m of x_des (:110)."""
    E = QuadEnvDesc()
    E.switch_clearance, E.lookahead, E.near = switch_clearance, lookahead, near
    return E


class LoopRecord(C.Structure):
    """bmpc_loop_record: the closed loops' per-step recorder (device pointers, ego-major; row r of
    an ego holds closed-loop step t_base + r).  The last four columns are optional (NULL skips)."""
    _fields_ = [("capacity", C.c_int32), ("t_base", C.c_int32),
                ("scene", C.c_void_p), ("xref", C.c_void_p), ("u", C.c_void_p), ("J", C.c_void_p),
                ("status", C.c_void_p), ("iters", C.c_void_p),
                ("upred", C.c_void_p), ("xpred", C.c_void_p), ("zpred", C.c_void_p), ("branch_w", C.c_void_p)]


OBS_ARGMAX, OBS_SAMPLE_MODEL = 0, 1   # bmpc_obstacle_sampling.mode (include/bmpc.h BMPC_OBS_*)
OBS_SAMPLE_TILTED, OBS_SCRIPT = 2, 3   # ... the two modes that need a proposal (bmpc_set_obstacle_proposal)
OBS_MODES = {"argmax": OBS_ARGMAX, "model": OBS_SAMPLE_MODEL, "tilted": OBS_SAMPLE_TILTED, "script": OBS_SCRIPT}


class ObstacleSampling(C.Structure):
    """bmpc_obstacle_sampling: how the overtake / quadruped scene's obstacle chooses its backup
    policy (bmpc_set_obstacle_sampling; the draws are bmpc.rng's)."""
    _fields_ = [("mode", C.c_int32), ("hold", C.c_int32), ("seed", C.c_uint64), ("ego_base", C.c_int64)]


def make_obstacle_sampling(mode="model", seed=0, hold=1, ego_base=0):
    """Validated bmpc_obstacle_sampling: mode "argmax" / "model" / "tilted" / "script" (or abi.OBS_*;
    the last two need a proposal on the plan, make_obstacle_proposal), a seed of 64 bits,
    hold >= 1 closed-loop steps per sampled choice, ego_base >= 0 the global index of the plan's
    ego 0 (a shard's first ego)."""
    if isinstance(mode, str):
        if mode not in OBS_MODES:
            raise ValueError(f"obstacle sampling mode {mode!r}: one of {sorted(OBS_MODES)}")
        mode = OBS_MODES[mode]
    if int(mode) not in OBS_MODES.values():
        raise ValueError(f"obstacle sampling mode {mode!r}: one of abi.OBS_ARGMAX, OBS_SAMPLE_MODEL, OBS_SAMPLE_TILTED, "
                         "OBS_SCRIPT")
    if int(hold) != hold or not 1 <= int(hold) < 2 ** 31:
        raise ValueError("hold must be an integer of at least 1")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if int(ego_base) != ego_base or not 0 <= int(ego_base) < 2 ** 63:
        raise ValueError("ego_base must be an integer of at least 0")
    S = ObstacleSampling()
    S.mode, S.hold, S.seed, S.ego_base = int(mode), int(hold), int(seed), int(ego_base)
    return S


class ObstacleProposal(C.Structure):
    """bmpc_obstacle_proposal: what modes OBS_SAMPLE_TILTED and OBS_SCRIPT choose by
    (bmpc_set_obstacle_proposal) -- a positive tilt per policy and a device table of prescribed choices
    int32 [batch][script_epochs] whose column 0 is epoch `epoch0`."""
    _fields_ = [("tilt", C.c_double * MAX_M), ("script", C.c_void_p), ("script_epochs", C.c_int32),
                ("epoch0", C.c_int32)]


def make_obstacle_proposal(tilt=None, script=None, epoch0=0, m=None):
    """Validated bmpc_obstacle_proposal.  tilt: m positive finite numbers b_j (None: all 1), the
    tilted mode draws policy j with probability p_j b_j / sum_k p_k b_k; m: the plan's policy count
    (default len(tilt), MAX_M without a tilt) -- entries beyond it are 1.  script: None, or
    (device pointer, epochs) of a C-contiguous int32 table [batch][epochs] the caller keeps alive
    (BatchPlan.set_obstacle_proposal uploads one from an array); epoch0 >= 0: the epoch of its
    column 0."""
    P = ObstacleProposal()
    if tilt is None:
        b = np.ones(MAX_M if m is None else int(m))
    else:
        b = np.asarray(tilt, dtype=np.float64)
    if b.ndim != 1 or not 1 <= b.size <= MAX_M or (m is not None and b.size != int(m)):
        raise ValueError(f"tilt must hold one entry per policy ({'1..%d' % MAX_M if m is None else int(m)}), "
                         f"got shape {b.shape}")
    if not (np.all(np.isfinite(b)) and np.all(b > 0)):
        raise ValueError("every tilt entry must be finite and > 0")
    for j in range(MAX_M):
        P.tilt[j] = float(b[j]) if j < b.size else 1.0
    if int(epoch0) != epoch0 or not 0 <= int(epoch0) < 2 ** 31:
        raise ValueError("epoch0 must be an integer of at least 0")
    P.epoch0 = int(epoch0)
    if script is not None:
        ptr, epochs = script
        if int(epochs) != epochs or not 1 <= int(epochs) < 2 ** 31:
            raise ValueError("a script needs at least one epoch (column)")
        if not ptr:
            raise ValueError("a script needs a device table")
        P.script, P.script_epochs = int(ptr), int(epochs)
    return P


DISTURB_NONE, DISTURB_IH4 = 0, 1   # bmpc_disturbance.law (include/bmpc.h BMPC_DISTURB_*)


class Disturbance(C.Structure):
    """bmpc_disturbance: the actuation disturbance of the closed loops' Euler steps
    (bmpc_set_disturbance; the draws are bmpc.rng.disturbance's).  88 bytes."""
    _fields_ = [("law", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("ego_base", C.c_int64),
                ("sigma_ego", C.c_double * MAX_D), ("sigma_obs", C.c_double * MAX_D)]


def make_disturbance(sigma_ego=None, sigma_obs=None, seed=0, ego_base=0, law=DISTURB_IH4, d=None):
    """Validated bmpc_disturbance.  sigma_ego / sigma_obs: the standard deviation per input component
    of the ego / the obstacle (None: zeros; finite and >= 0, at most MAX_D entries -- d when the
    plan's input dimension is given), a seed of 64 bits, ego_base >= 0 the global index of the plan's
    ego 0, law abi.DISTURB_IH4 or abi.DISTURB_NONE."""
    if int(law) not in (DISTURB_NONE, DISTURB_IH4):
        raise ValueError("law: abi.DISTURB_NONE or abi.DISTURB_IH4")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if int(ego_base) != ego_base or not 0 <= int(ego_base) < 2 ** 63:
        raise ValueError("ego_base must be an integer of at least 0")
    D = Disturbance()
    D.law, D.seed, D.ego_base = int(law), int(seed), int(ego_base)
    lim = MAX_D if d is None else int(d)
    for name, sig in (("sigma_ego", sigma_ego), ("sigma_obs", sigma_obs)):
        s = np.zeros(0) if sig is None else np.atleast_1d(np.asarray(sig, dtype=np.float64))
        if s.ndim != 1 or s.size > lim:
            raise ValueError(f"{name} must hold at most {lim} entries (one per input component), got shape {s.shape}")
        if not (np.all(np.isfinite(s)) and np.all(s >= 0)):
            raise ValueError(f"every {name} entry must be finite and >= 0")
        _fill(getattr(D, name), s)
    return D


OBSERVE_NONE, OBSERVE_IH4 = 0, 1   # bmpc_observation.law (include/bmpc.h BMPC_OBSERVE_*)


class Observation(C.Structure):
    """bmpc_observation: the observation noise on the states the closed loops' scene steps hand to the
    next solve (bmpc_set_observation; the draws are bmpc.rng.observation's).  152 bytes."""
    _fields_ = [("law", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("ego_base", C.c_int64),
                ("sigma_x", C.c_double * MAX_N), ("sigma_z", C.c_double * MAX_N)]


def make_observation(sigma_x=None, sigma_z=None, seed=0, ego_base=0, law=OBSERVE_IH4, n=None):
    """Validated bmpc_observation.  sigma_x / sigma_z: the standard deviation per state component of
    the observed ego / obstacle state (None: zeros; finite and >= 0, at most MAX_N entries -- n when
    the plan's state dimension is given), a seed of 64 bits, ego_base >= 0 the global index of the
    plan's ego 0, law abi.OBSERVE_IH4 or abi.OBSERVE_NONE."""
    if int(law) not in (OBSERVE_NONE, OBSERVE_IH4):
        raise ValueError("law: abi.OBSERVE_NONE or abi.OBSERVE_IH4")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if int(ego_base) != ego_base or not 0 <= int(ego_base) < 2 ** 63:
        raise ValueError("ego_base must be an integer of at least 0")
    O = Observation()
    O.law, O.seed, O.ego_base = int(law), int(seed), int(ego_base)
    lim = MAX_N if n is None else int(n)
    for name, sig in (("sigma_x", sigma_x), ("sigma_z", sigma_z)):
        s = np.zeros(0) if sig is None else np.atleast_1d(np.asarray(sig, dtype=np.float64))
        if s.ndim != 1 or s.size > lim:
            raise ValueError(f"{name} must hold at most {lim} entries (one per state component), got shape {s.shape}")
        if not (np.all(np.isfinite(s)) and np.all(s >= 0)):
            raise ValueError(f"every {name} entry must be finite and >= 0")
        _fill(getattr(O, name), s)
    return O


RESAMPLE_SYSTEMATIC = 0        # bmpc_resample_desc.scheme (include/bmpc.h BMPC_RESAMPLE_*)
RESAMPLE_NINFO = 8             # doubles of the info vector (R_* slots)
RESAMPLE_MAX_BATCH = 1 << 20
R_RESAMPLED, R_ESS, R_MAX, R_NEW_LOGW, R_SUM, R_SURVIVORS, R_NONFINITE = range(7)


class ResampleDesc(C.Structure):
    """bmpc_resample_desc: one resampling of a weighted population (bmpc_population_ancestors,
    bmpc_resample_device; bmpc.resample restates the rule)."""
    _fields_ = [("scheme", C.c_int32), ("round", C.c_uint32), ("ess_fraction", C.c_double), ("seed", C.c_uint64),
                ("ego_base", C.c_int64)]


def make_resample_desc(round, seed=0, ess_fraction=0.5, ego_base=0, scheme=RESAMPLE_SYSTEMATIC):
    """Validated bmpc_resample_desc: round in [0, 2^32) addresses the draw (e.g. the step at which the
    population is resampled), a seed of 64 bits, ess_fraction finite and >= 0 (resample iff
    ess < ess_fraction * batch: 0 never does, anything above 1 always), ego_base >= 0."""
    if int(scheme) != RESAMPLE_SYSTEMATIC:
        raise ValueError("scheme: abi.RESAMPLE_SYSTEMATIC")
    if int(round) != round or not 0 <= int(round) < 2 ** 32:
        raise ValueError("round must be an integer in [0, 2^32)")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if not (np.isfinite(ess_fraction) and ess_fraction >= 0):
        raise ValueError("ess_fraction must be finite and >= 0")
    if int(ego_base) != ego_base or not 0 <= int(ego_base) < 2 ** 63:
        raise ValueError("ego_base must be an integer of at least 0")
    D = ResampleDesc()
    D.scheme, D.round, D.ess_fraction, D.seed, D.ego_base = int(scheme), int(round), float(ess_fraction), int(seed), \
        int(ego_base)
    return D


class EgoBuffers(C.Structure):
    """bmpc_ego_buffers: the loop entries' per-ego device buffers (None skips one)."""
    _fields_ = [(k, C.c_void_p) for k in ("scene", "upred", "x", "z", "xref", "J", "status", "iters", "stats")]


def make_ego_buffers(buffers=None, **named):
    """bmpc_ego_buffers from a mapping (or keywords) name -> device pointer or torch tensor; the names
    are EgoBuffers' fields."""
    E = EgoBuffers()
    items = dict(buffers or {}, **named)
    unknown = set(items) - {k for k, _ in EgoBuffers._fields_}
    if unknown:
        raise ValueError(f"unknown ego buffers {sorted(unknown)}")
    for k, v in items.items():
        setattr(E, k, None if v is None else int(v.data_ptr()) if hasattr(v, "data_ptr") else int(v))
    return E


def _fill(arr, values):
    v = np.asarray(values, dtype=np.float64).ravel()
    for i, x in enumerate(v):
        arr[i] = float(x)


def make_desc(controller, model, n, d, N, NB, m, dt, Q, R, Fx, bx, Fu, bu, Qslack,
              mc, ralpha=0.9, Qf=None, dR=None, maxit=100,
              feastol=1e-8, abstol=1e-8, reltol=1e-8, flags=0) -> PlanDesc:
    """Pack a plan description (all matrices row-major at their logical size)."""
    Fx = np.asarray(Fx, float).reshape(-1, n)
    Fu = np.asarray(Fu, float).reshape(-1, d)
    if n > MAX_N or d > MAX_D or Fx.shape[0] > MAX_FX or Fu.shape[0] > MAX_FU or m > MAX_M:
        raise ValueError("problem dimensions exceed the C ABI limits")
    D = PlanDesc()
    D.controller, D.model = int(controller), int(model)
    D.n, D.d, D.N, D.NB, D.m = int(n), int(d), int(N), int(NB), int(m)
    D.nFx, D.nFu = int(Fx.shape[0]), int(Fu.shape[0])
    D.maxit = int(maxit)
    D.dt, D.ralpha = float(dt), float(ralpha)
    _fill(D.Q, np.asarray(Q, float).reshape(n, n))
    _fill(D.R, np.asarray(R, float).reshape(d, d))
    _fill(D.Qf, np.asarray(Q if Qf is None else Qf, float).reshape(n, n))
    _fill(D.dR, np.zeros(d) if dR is None else dR)
    _fill(D.Fx, Fx)
    _fill(D.bx, np.asarray(bx, float).ravel())
    _fill(D.Fu, Fu)
    _fill(D.bu, np.asarray(bu, float).ravel())
    _fill(D.Qslack, Qslack)
    _fill(D.mc, mc)
    D.feastol, D.abstol, D.reltol = feastol, abstol, reltol
    D.flags = int(flags)
    return D


def policy_array(rows):
    """rows: iterable (per ego) of iterables of (kind, params) -> ctypes array."""
    rows = [list(r) for r in rows]
    flat = [pp for r in rows for pp in r]
    arr = (Policy * len(flat))()
    for i, (kind, params) in enumerate(flat):
        arr[i].kind = int(kind)
        for j, v in enumerate(params):
            arr[i].p[j] = float(v)
    return arr
