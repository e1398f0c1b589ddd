"""Python handle over a libbmpc plan: one batch of egos sharing one controller/model."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import abi
from ._lib import check, lib

_CTX = {}


def context(device: int = 0):
    """One bmpc_ctx per HIP device per process."""
    if device not in _CTX:
        h = C.c_void_p()
        check(lib().bmpc_open(device, C.byref(h)), "bmpc_open")
        _CTX[device] = h
    return _CTX[device]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _vp(*ptrs):
    """Device pointers and stream handles (integers; None or 0: absent) as a C entry point's arguments."""
    return [C.c_void_p(p) if p else None for p in ptrs]


SCENE_KINDS = {abi.MODEL_HIGHWAY: "overtake", abi.MODEL_HIGHWAY_MERGE: "merge", abi.MODEL_QUADRUPED: "quadruped"}


class LoopRecording:
    """The per-step record of a plan's closed loops (bmpc_loop_record): its columns and the struct
    that points at them.

    ``cols`` maps the column names of the struct -- scene [B, capacity, ENV_STRIDE], xref
    [B, capacity, n], u [B, capacity, d], J / status / iters [B, capacity] and, with predictions,
    upred [B, capacity, U, d], xpred / zpred [B, capacity, T, n], branch_w [B, capacity,
    nbranch-1] -- to torch tensors on the plan's device (BatchPlan.new_loop_record) or NumPy
    arrays.  Row r of an ego holds closed-loop step ``t_base + r`` in the device scene's own
    convention: the scene row as step t's solve saw it (state and inputs OF step t) and that
    solve's outputs; ``u[:, r]`` is the input the ego applies next.  Highway_sim's post-step
    ``state_rec[t]`` is therefore ``x[:, t + 1]``; no final post-step row exists.

    ``col(name)`` is the column on the host (a copy when it lives on the device); the properties
    below are NumPy views of the scene column by scene kind ("overtake", "merge", "quadruped"),
    through the abi.ENV_* / abi.QENV_* slots.  ``host()`` snapshots every column once.

    Memory: a row is 16 + n + d + 2 doubles (0.2 KB; 8-byte J, 4-byte status and iters), and with
    predictions U d + 2 T n + nbranch - 1 doubles more: about 5 KB per ego-step at N = 20, NB = 1
    (T = 64, U = 61: 637 doubles), so 4,096 egos x 20 steps take 0.4 GB with predictions and 16 MB without."""

    CORE = ("scene", "xref", "u", "J", "status", "iters")
    OPTIONAL = ("upred", "xpred", "zpred", "branch_w")

    def __init__(self, kind, capacity, t_base, cols):
        if kind not in SCENE_KINDS.values():
            raise ValueError(f"scene kind {kind!r}: one of {sorted(SCENE_KINDS.values())}")
        missing = [k for k in self.CORE if cols.get(k) is None]
        if missing:
            raise ValueError(f"core columns missing: {missing}")
        self.kind, self.capacity, self.t_base = kind, int(capacity), int(t_base)
        self.cols = {k: cols[k] for k in self.CORE + self.OPTIONAL if cols.get(k) is not None}
        self.struct = None
        if all(hasattr(v, "data_ptr") for v in self.cols.values()):
            self.struct = abi.LoopRecord(capacity=self.capacity, t_base=self.t_base,
                                         **{k: v.data_ptr() for k, v in self.cols.items()})

    @property
    def nbytes(self):
        return sum(int(np.prod(v.shape)) * (4 if k in ("status", "iters") else 8) for k, v in self.cols.items())

    def col(self, name):
        v = self.cols[name]
        return v if isinstance(v, np.ndarray) else v.cpu().numpy()

    def host(self):
        """A snapshot with every column on the host (wait for the loop's stream first)."""
        return LoopRecording(self.kind, self.capacity, self.t_base, {k: self.col(k) for k in self.cols})

    def _scene(self, lo, width=None, kinds=None):
        if kinds is not None and self.kind not in kinds:
            raise AttributeError(f"the {self.kind} scene has no such column")
        s = self.col("scene")
        return s[..., lo] if width is None else s[..., lo:lo + width]

    @property
    def _quad(self):
        return self.kind == "quadruped"

    @property
    def x(self):
        """Ego state of each recorded step [B, capacity, n]."""
        return self._scene(abi.QENV_X, 3) if self._quad else self._scene(abi.ENV_X, 4)

    @property
    def z(self):
        """Obstacle state [B, capacity, n]."""
        return self._scene(abi.QENV_Z, 3) if self._quad else self._scene(abi.ENV_Z, 4)

    @property
    def u_obs(self):
        """The obstacle's input chosen at the step (applied by the next step's Euler step)."""
        return self._scene(abi.QENV_UOBS, 3) if self._quad else self._scene(abi.ENV_UOBS, 2)

    @property
    def obs_policy(self):
        """The obstacle's backup choice (Highway_sim's backup_choice_rec)."""
        return self._scene(abi.ENV_OBSPOL)

    @property
    def logw(self):
        """The running log-weight after each step (modes "tilted" and "script"; 0 or the caller's
        value otherwise)."""
        return self._scene(abi.ENV_LOGW, kinds=("overtake", "quadruped"))

    @property
    def collided(self):
        return self._scene(abi.ENV_COLL)

    @property
    def steps(self):
        """Control steps taken, t + 1 in the row of step t."""
        return self._scene(abi.ENV_STEPS)

    @property
    def merged(self):
        """Merge scene: the ego has left the ramp."""
        return self._scene(abi.ENV_MERGED, kinds=("merge",))

    @property
    def x_des(self):
        """Quadruped scene: the ego's goal."""
        return self._scene(abi.QENV_XDES, 3, kinds=("quadruped",))


class BatchPlan:
    """A batch of ``batch`` independent egos, each with its own scenario tree, warm start
    and policy set, solved together by one kernel launch per phase."""

    def __init__(self, desc: abi.PlanDesc, batch: int, device: int = 0):
        self.desc = desc
        self.batch = int(batch)
        self.device = device
        self._ctx = context(device)
        h = C.c_void_p()
        check(lib().bmpc_plan_create(self._ctx, C.byref(desc), self.batch, C.byref(h)), "bmpc_plan_create")
        self._h = h
        self._loop_record = None   # the attached LoopRecording (set_loop_record)
        info = np.zeros(abi.INFO_COUNT, np.int32)
        check(lib().bmpc_plan_info(h, _p(info)), "bmpc_plan_info")
        self.info = info
        self.T, self.U = int(info[abi.INFO_T]), int(info[abi.INFO_U])
        self.bdim, self.nbranch = int(info[abi.INFO_BDIM]), int(info[abi.INFO_NBRANCH])
        self.nv, self.neq = int(info[abi.INFO_NV]), int(info[abi.INFO_NEQ])
        self.nrows, self.ncones = int(info[abi.INFO_NROWS]), int(info[abi.INFO_NCONES])

    def close(self):
        if getattr(self, "_h", None):
            lib().bmpc_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----------------------------------------------------------------------------
    def set_policies(self, rows, mask=None):
        """rows: per ego, m (kind, params) tuples (``update_backup``)."""
        arr = abi.policy_array(rows)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(lib().bmpc_set_policies(self._h, arr, _p(m)), "bmpc_set_policies")

    def get_policies(self):
        """The policies in force, per ego m (kind, params) tuples -- including the device-side
        lane-change re-targets of env_step_device."""
        arr = (abi.Policy * (self.batch * self.desc.m))()
        check(lib().bmpc_get_policies(self._h, arr), "bmpc_get_policies")
        m = self.desc.m
        return [[(int(arr[e * m + i].kind), tuple(arr[e * m + i].p)) for i in range(m)] for e in range(self.batch)]

    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(lib().bmpc_reset(self._h, _p(m)), "bmpc_reset")

    # ---- solves ---------------------------------------------------------------------------
    def solve(self, x, z, xref):
        B, n, d = self.batch, self.desc.n, self.desc.d
        x, z, xref = (np.ascontiguousarray(np.asarray(v, np.float64).reshape(B, n)) for v in (x, z, xref))
        out = dict(upred=np.zeros((B, self.U, d)), xpred=np.zeros((B, self.T, n)),
                   branch_w=np.zeros((B, self.nbranch - 1)), J=np.zeros(B),
                   status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))
        check(lib().bmpc_solve(self._h, _p(x), _p(z), _p(xref), *(_p(out[k]) for k in
                               ("upred", "xpred", "branch_w", "J", "status", "iters"))), "bmpc_solve")
        return out

    def solve_device(self, x_ptr, z_ptr, xref_ptr, upred_ptr=None, xpred_ptr=None, bw_ptr=None,
                     J_ptr=None, status_ptr=None, iters_ptr=None, stream=None):
        """Device-pointer variant (e.g. torch tensors' data_ptr()), asynchronous, enqueued on
        `stream` (a hipStream_t handle; None = the plan's own non-blocking stream, which is
        NOT ordered with the legacy default stream -- pass the caller's stream)."""
        vp = _vp(x_ptr, z_ptr, xref_ptr, upred_ptr, xpred_ptr, bw_ptr, J_ptr, status_ptr, iters_ptr, stream)
        check(lib().bmpc_solve_device(self._h, *vp), "bmpc_solve_device")

    def env_step_device(self, env: abi.EnvDesc, t: int, scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr,
                        J_ptr=None, status_ptr=None, iters_ptr=None, stats_ptr=None, stream=None):
        """One closed-loop sim_overtake step of every ego on the device (bmpc_env_step):
        Euler step with the last uPred[0], collision flag, obstacle backup choice, lane /
        lane-change-target bookkeeping and x_ref -> the next solve's x, z, xref.  Async."""
        vp = _vp(scene_ptr, upred_ptr, J_ptr, status_ptr, iters_ptr, x_ptr, z_ptr, xref_ptr, stats_ptr, stream)
        check(lib().bmpc_env_step(self._h, C.byref(env), int(t), *vp), "bmpc_env_step")

    def loop_device(self, env: abi.EnvDesc, t0: int, nsteps: int, scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr,
                    J_ptr, status_ptr, iters_ptr, stats_ptr=None, stream=None):
        """nsteps closed-loop steps of every ego (bmpc_loop_device): env_step_device(t) then
        solve_device for t = t0 .. t0+nsteps-1, the same results; one fused launch (k_loop) when
        a CVaR batch takes the one-wave IPM and for BranchMPC (CTRL_QP) plans at any batch; robust
        plans keep their launches per step unless BMPC_LOOP_FUSED=2.  Async on `stream`."""
        vp = _vp(scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr, J_ptr, status_ptr, iters_ptr, stats_ptr, stream)
        check(lib().bmpc_loop_device(self._h, C.byref(env), int(t0), int(nsteps), *vp), "bmpc_loop_device")

    def set_merge_scene(self, env: abi.MergeEnvDesc, grid, refY, refpsi):
        """The plan's sim_merge scene (bmpc_set_merge_scene): its constants and the ramp's lane
        references refY(X), refpsi(X) over one grid.  HIGHWAY_MERGE CVaR plans."""
        g, y, p = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)) for a in (grid, refY, refpsi))
        if not (g.size == y.size == p.size):
            raise ValueError("grid, refY and refpsi must have one length")
        check(lib().bmpc_set_merge_scene(self._h, C.byref(env), g.size, _p(g), _p(y), _p(p)), "bmpc_set_merge_scene")

    def merge_env_step_device(self, t: int, scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr, J_ptr=None,
                              status_ptr=None, iters_ptr=None, stats_ptr=None, stream=None):
        """One closed-loop sim_merge step of every ego on the device (bmpc_merge_env_step): Euler
        steps, collision flag, lane flag, obstacle input -> the next solve's x, z, xref, and its S /
        bx in the plan's transform slots (no set_transform before solve_device).  Async."""
        vp = _vp(scene_ptr, upred_ptr, J_ptr, status_ptr, iters_ptr, x_ptr, z_ptr, xref_ptr, stats_ptr, stream)
        check(lib().bmpc_merge_env_step(self._h, int(t), *vp), "bmpc_merge_env_step")

    def merge_loop_device(self, t0: int, nsteps: int, scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr, J_ptr,
                          status_ptr, iters_ptr, stats_ptr=None, stream=None):
        """nsteps closed-loop sim_merge steps of every ego (bmpc_merge_loop_device):
        merge_env_step_device(t) then solve_device per step, the same results; one fused launch
        (k_loop) when the batch takes the one-wave IPM.  Async on `stream`."""
        vp = _vp(scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr, J_ptr, status_ptr, iters_ptr, stats_ptr, stream)
        check(lib().bmpc_merge_loop_device(self._h, int(t0), int(nsteps), *vp), "bmpc_merge_loop_device")

    def quad_env_step_device(self, env: abi.QuadEnvDesc, t: int, scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr,
                             J_ptr=None, status_ptr=None, iters_ptr=None, stats_ptr=None, stream=None):
        """One closed-loop main_quadruped step of every ego on the device (bmpc_quad_env_step): Euler
        steps of both robots, the obstacle's backup choice from the clearance along the ego's
        predicted path, x_ref towards the scene's per-ego x_des -> the next solve's x, z, xref
        [batch][3].  QUADRUPED plans with an OSQP-class controller.  Async."""
        vp = _vp(scene_ptr, upred_ptr, J_ptr, status_ptr, iters_ptr, x_ptr, z_ptr, xref_ptr, stats_ptr, stream)
        check(lib().bmpc_quad_env_step(self._h, C.byref(env), int(t), *vp), "bmpc_quad_env_step")

    def quad_loop_device(self, env: abi.QuadEnvDesc, t0: int, nsteps: int, scene_ptr, upred_ptr, x_ptr, z_ptr,
                         xref_ptr, J_ptr, status_ptr, iters_ptr, stats_ptr=None, stream=None):
        """nsteps closed-loop main_quadruped steps of every ego (bmpc_quad_loop_device):
        quad_env_step_device(t) then solve_device per step, the same results; one fused launch
        (k_loop with the QP solver) unless BMPC_LOOP_FUSED=0.  Async on `stream`."""
        vp = _vp(scene_ptr, upred_ptr, x_ptr, z_ptr, xref_ptr, J_ptr, status_ptr, iters_ptr, stats_ptr, stream)
        check(lib().bmpc_quad_loop_device(self._h, C.byref(env), int(t0), int(nsteps), *vp), "bmpc_quad_loop_device")

    def _scene_loop(self):
        """This plan's closed-loop entry for its model as f(t0, nsteps, *pointers): quad_loop_device
        or loop_device with the scene's default constants, or merge_loop_device (set_merge_scene's)."""
        if self.desc.model == abi.MODEL_QUADRUPED:
            return functools.partial(self.quad_loop_device, abi.make_quad_env())
        if self.desc.model == abi.MODEL_HIGHWAY_MERGE:
            return self.merge_loop_device
        return functools.partial(self.loop_device, abi.make_env())

    # ---- the closed loops' recorder ---------------------------------------------------------
    def set_loop_record(self, rec):
        """Attach a LoopRecording (or a raw abi.LoopRecord) to the plan's closed loops, or detach
        with None (bmpc_set_loop_record).  While attached, every step of loop_device /
        merge_loop_device / quad_loop_device writes its row; the single-step entry points do not
        record.  The plan keeps a reference to the attached object, so its tensors stay alive."""
        struct = getattr(rec, "struct", rec)
        if rec is not None and struct is None:
            raise ValueError("the recording's columns are not on a device (a host snapshot?)")
        check(lib().bmpc_set_loop_record(self._h, None if struct is None else C.byref(struct)), "bmpc_set_loop_record")
        self._loop_record = rec

    # ---- the scenes' obstacle sampler --------------------------------------------------------
    def set_obstacle_sampling(self, mode="model", seed=0, hold=1, ego_base=0):
        """How the obstacle of the plan's overtake or quadruped scene chooses its backup policy
        (bmpc_set_obstacle_sampling).  mode "model": at every closed-loop step t with t % hold == 0
        the obstacle draws its policy from the model's own branch distribution p_j(x, z) at the
        step's state -- the smallest j with u < p_0 + ... + p_j for
        u = bmpc.rng.obstacle_uniform(seed, ego_base + e, t // hold) -- and keeps it for `hold`
        steps; a sampler attached mid-episode keeps the scene row's last choice until the next
        such step.  mode None or "argmax" detaches: the reference's deterministic rule.  A plan
        holding egos lo..hi-1 of a sharded population passes ego_base=lo (distributed.shard): every
        ego then gets the trajectory it has in the unsharded run.  Host state only; loop_device /
        quad_loop_device on either launch path and the single-step env_step_device /
        quad_env_step_device obey it.  Also takes an abi.ObstacleSampling."""
        if mode is None:
            struct = None
        elif isinstance(mode, abi.ObstacleSampling):
            struct = mode
        else:
            struct = abi.make_obstacle_sampling(mode, seed, hold, ego_base)
        check(lib().bmpc_set_obstacle_sampling(self._h, None if struct is None else C.byref(struct)),
              "bmpc_set_obstacle_sampling")
        self.obstacle_sampling = struct

    def set_obstacle_proposal(self, tilt=None, script=None, epoch0=0):
        """What set_obstacle_sampling's modes "tilted" and "script" choose by
        (bmpc_set_obstacle_proposal); attach it before selecting either mode.

        tilt: one positive finite b_j per policy (None: all 1).  Mode "tilted" draws, at the draw and
        the epochs of mode "model", policy j with probability q_j = p_j b_j / sum_k p_k b_k and adds
        log(p_j / q_j) to the scene row's slot abi.ENV_LOGW: exp of it is the episode's likelihood
        ratio (montecarlo.estimate).  script: an integer array [batch, E] (NumPy or torch) of
        prescribed choices in [0, m), row e for the plan's ego e, column c for epoch epoch0 + c;
        it is checked here, uploaded as int32 and kept alive by the plan.  Mode "script" takes the
        choice of epoch t // hold from it, makes no draw, and adds log p_j -- the model's own
        probability of the prescribed choice -- to abi.ENV_LOGW.  Every entry point that steps a
        scene refuses steps whose epochs the script does not cover.  The caller zeroes the slot to
        start an estimate.  tilt=None, script=None detaches (refused while the sampler's mode is
        "tilted" or "script").  Also takes an abi.ObstacleProposal as `tilt`."""
        keep = None
        if isinstance(tilt, abi.ObstacleProposal):
            struct = tilt
        elif tilt is None and script is None:
            struct = None
        else:
            m = int(self.desc.m)
            table = None
            if script is not None:
                host = script.detach().cpu().numpy() if hasattr(script, "detach") else np.asarray(script)
                if host.dtype.kind not in "iu":
                    raise ValueError("the script must hold integers")
                if host.ndim != 2 or host.shape[0] != self.batch or host.shape[1] < 1:
                    raise ValueError(f"the script must have shape [batch = {self.batch}, epochs >= 1], got {host.shape}")
                if host.min() < 0 or host.max() >= m:
                    raise ValueError(f"script entries must lie in [0, {m})")
                table = (np.ascontiguousarray(host, np.int32), host.shape[1])
            struct = abi.make_obstacle_proposal(tilt, None, epoch0, m=m)
            if table is not None:
                import torch
                keep = torch.tensor(table[0], dtype=torch.int32, device=torch.device("cuda", self.device))
                torch.cuda.synchronize(keep.device)
                struct.script, struct.script_epochs = keep.data_ptr(), table[1]
        check(lib().bmpc_set_obstacle_proposal(self._h, None if struct is None else C.byref(struct)),
              "bmpc_set_obstacle_proposal")
        self.obstacle_proposal, self._script = struct, keep

    # ---- the scenes' actuation disturbance ----------------------------------------------------
    def set_disturbance(self, sigma_ego=None, sigma_obs=None, seed=0, ego_base=0):
        """Process noise in the plan's closed loops (bmpc_set_disturbance): in the Euler step that
        follows closed-loop step t the ego of row e moves with
        ``uPred[0] + sigma_ego * bmpc.rng.disturbance(seed, ego_base + e, t, "ego", d)`` and the
        obstacle with its chosen input ``+ sigma_obs * bmpc.rng.disturbance(seed, ego_base + e, t,
        "obstacle", d)`` -- a unit-variance, bounded, near-Gaussian variate per component, the product
        rounded before it is added.  sigma_ego / sigma_obs: up to d standard deviations >= 0 (None:
        zeros; a zero component makes no draw).  The scene row's obstacle-input slot and the
        recorder's u column keep the nominal inputs; nothing is clipped.  All three scenes, both
        launch paths and the single-step entries obey it; a shard passes ego_base=lo.
        sigma_ego=None, sigma_obs=None detaches.  Also takes an abi.Disturbance as `sigma_ego`."""
        if isinstance(sigma_ego, abi.Disturbance):
            struct = sigma_ego
        elif sigma_ego is None and sigma_obs is None:
            struct = None
        else:
            struct = abi.make_disturbance(sigma_ego, sigma_obs, seed, ego_base, d=int(self.desc.d))
        check(lib().bmpc_set_disturbance(self._h, None if struct is None else C.byref(struct)), "bmpc_set_disturbance")
        self.disturbance = struct

    # ---- the scenes' observation noise ---------------------------------------------------------
    def set_observation(self, sigma_x=None, sigma_z=None, seed=0, ego_base=0):
        """Observation noise in the plan's closed loops (bmpc_set_observation): the solve of
        closed-loop step t of row e is handed
        ``x + sigma_x * bmpc.rng.observation(seed, ego_base + e, t, "ego", n)`` and
        ``z + sigma_z * bmpc.rng.observation(seed, ego_base + e, t, "obstacle", n)`` instead of the
        scene's true states x, z -- the disturbance's unit-variance bounded variate per component, the
        product rounded before it is added.  sigma_x / sigma_z: up to n standard deviations >= 0 (None:
        zeros; a zero component makes no draw and passes through).  Only the solve's two inputs change
        (the loop entries' x / z buffers hold the observed vectors): the scene row, the recorder, the
        collision rule, the obstacle's choice, the statistics, x_ref and the merge scene's S / bx stay
        on the truth.  All three scenes, both launch paths and the single-step entries obey it; a shard
        passes ego_base=lo.  sigma_x=None, sigma_z=None detaches.  Also takes an abi.Observation as
        `sigma_x`."""
        if isinstance(sigma_x, abi.Observation):
            struct = sigma_x
        elif sigma_x is None and sigma_z is None:
            struct = None
        else:
            struct = abi.make_observation(sigma_x, sigma_z, seed, ego_base, n=int(self.desc.n))
        check(lib().bmpc_set_observation(self._h, None if struct is None else C.byref(struct)), "bmpc_set_observation")
        self.observation = struct

    # ---- resampling a weighted population ------------------------------------------------------
    def _ego_buffers(self, buffers):
        return buffers if isinstance(buffers, abi.EgoBuffers) else abi.make_ego_buffers(buffers)

    def resample(self, buffers, round, seed=0, ess_fraction=0.5, ego_base=0, stream=None):
        """Resample the plan's weighted population between two loop calls (bmpc_resample_device):
        ancestors from the scene's abi.ENV_LOGW column by the rule of bmpc.resample (systematic, at the
        draw bmpc.resample.offset(seed, ego_base, round), iff ess < ess_fraction * batch), then every
        ego j with ancestor[j] != j becomes a copy of ego ancestor[j] -- its rows of `buffers`, its
        policies and its warm start -- and every ego's log-weight becomes the log of the mean weight.
        buffers: a mapping from abi.EgoBuffers' names (scene, upred, x, z, xref, J, status, iters,
        stats) to the loop's torch tensors or device pointers ("scene" is required), or an
        abi.EgoBuffers.  Asynchronous on `stream`, like loop_device.  Returns (ancestor [batch] int32,
        info [abi.RESAMPLE_NINFO] float64) as torch tensors on the plan's device (abi.R_* slots;
        info[abi.R_RESAMPLED] says whether anything moved).  The recorder is not touched: rows stay
        addressed by slot, and the ancestors are the genealogy (montecarlo.lineage)."""
        import torch
        dev = torch.device("cuda", self.device)
        desc = abi.make_resample_desc(round, seed, ess_fraction, ego_base)
        bufs = self._ego_buffers(buffers)
        anc = torch.empty(self.batch, dtype=torch.int32, device=dev)
        info = torch.empty(abi.RESAMPLE_NINFO, dtype=torch.float64, device=dev)
        check(lib().bmpc_resample_device(self._h, C.byref(desc), C.byref(bufs), C.c_void_p(anc.data_ptr()),
                                         C.c_void_p(info.data_ptr()), C.c_void_p(stream) if stream else None),
              "bmpc_resample_device")
        return anc, info

    def gather_egos(self, ancestor, buffers=None, stream=None):
        """Ego j continues as a copy of ego ancestor[j], for every j, as the egos were before the call
        (bmpc_gather_egos): any map -- a permutation, a broadcast -- of int32 entries clamped to the
        batch.  ancestor: a torch int32 tensor [batch] on the plan's device, or a device pointer;
        buffers as in resample (None: only the plan's own state moves).  Asynchronous on `stream`."""
        ptr = ancestor.data_ptr() if hasattr(ancestor, "data_ptr") else int(ancestor)
        if hasattr(ancestor, "dtype"):
            import torch
            if ancestor.dtype != torch.int32 or ancestor.numel() != self.batch or not ancestor.is_contiguous():
                raise ValueError(f"ancestor must be a contiguous int32 tensor of {self.batch} entries")
        bufs = None if buffers is None else self._ego_buffers(buffers)
        check(lib().bmpc_gather_egos(self._h, C.c_void_p(ptr), None if bufs is None else C.byref(bufs),
                                     C.c_void_p(stream) if stream else None), "bmpc_gather_egos")

    def new_loop_record(self, capacity, t_base=0, predictions=False, device=None):
        """A LoopRecording of `capacity` rows per ego from closed-loop step `t_base` on, in fresh
        zeroed torch tensors on `device` (default: the plan's); predictions adds the optional
        upred / xpred / zpred / branch_w columns (no zpred on robust plans, whose tree keeps no
        obstacle predictions per node).  Not attached yet: pass it to set_loop_record."""
        import torch
        dev = torch.device("cuda", self.device) if device is None else torch.device(device)
        B, c, n, d = self.batch, int(capacity), self.desc.n, self.desc.d
        if c < 1:
            raise ValueError("capacity must be at least 1")
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        cols = dict(scene=torch.zeros((B, c, abi.ENV_STRIDE), **f64), xref=torch.zeros((B, c, n), **f64),
                    u=torch.zeros((B, c, d), **f64), J=torch.zeros((B, c), **f64),
                    status=torch.zeros((B, c), **i32), iters=torch.zeros((B, c), **i32))
        if predictions:
            cols.update(upred=torch.zeros((B, c, self.U, d), **f64), xpred=torch.zeros((B, c, self.T, n), **f64),
                        branch_w=torch.zeros((B, c, self.nbranch - 1), **f64))
            if self.desc.controller != abi.CTRL_ROBUST:
                cols["zpred"] = torch.zeros((B, c, self.T, n), **f64)
        torch.cuda.synchronize(dev)   # the zero fills are done before a loop's own stream writes rows
        return LoopRecording(SCENE_KINDS[self.desc.model], c, t_base, cols)

    def get_transform(self):
        """The S [B,n,n], bx [B,nFx] and (S on, bx set) flags [B,2] in the egos' transform slots."""
        B, n, nF = self.batch, self.desc.n, self.desc.nFx
        S, bx, fl = np.zeros((B, n, n)), np.zeros((B, nF)), np.zeros((B, 2))
        check(lib().bmpc_get_transform(self._h, _p(S), _p(bx), _p(fl)), "bmpc_get_transform")
        return dict(S=S, bx=bx, s_on=fl[:, 0] != 0, bx_set=fl[:, 1] != 0)

    def get_warm_start(self):
        """Checkpoint of the per-ego warm start (uLin, p, Jcons, OldInput)."""
        B, d = self.batch, self.desc.d
        uLin = np.zeros((B, self.U + 1, d))
        p = np.zeros((B, self.bdim, self.desc.m))
        jc = np.zeros(B)
        old = np.zeros((B, d))
        check(lib().bmpc_get_warm_start(self._h, _p(uLin), _p(p), _p(jc), _p(old)), "bmpc_get_warm_start")
        return dict(uLin=uLin, p=p, jcons=jc, old_input=old)

    def set_warm_start(self, uLin, p=None, jcons=None, old_input=None, mask=None):
        """Resume from a checkpoint (the next solve runs updatetree); None keeps a part."""
        B, d = self.batch, self.desc.d
        uLin = np.ascontiguousarray(np.asarray(uLin, np.float64).reshape(B, self.U + 1, d))
        p = None if p is None else np.ascontiguousarray(np.asarray(p, np.float64).reshape(B, self.bdim, self.desc.m))
        jc = None if jcons is None else np.ascontiguousarray(np.asarray(jcons, np.float64).reshape(B))
        old = None if old_input is None else np.ascontiguousarray(np.asarray(old_input, np.float64).reshape(B, d))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(lib().bmpc_set_warm_start(self._h, _p(uLin), _p(p), _p(jc), _p(old), _p(m)), "bmpc_set_warm_start")

    def set_transform(self, S=None, bx=None, s_on=None, mask=None):
        """Per-ego state transformation S [B,n,n] (None = "S is None" for every ego) and
        state bound bx [B,nFx] (None = keep) of the next solves -- the S / bx arguments of
        BranchMPC_CVaR.solve (MPC_branch.py:2043-2057); HIGHWAY_MERGE plans and HIGHWAY CVaR
        plans created with abi.PLAN_TRANSFORM."""
        B, n = self.batch, self.desc.n
        S = None if S is None else np.ascontiguousarray(np.asarray(S, np.float64).reshape(B, n, n))
        bx = None if bx is None else np.ascontiguousarray(np.asarray(bx, np.float64).reshape(B, self.desc.nFx))
        on = None if s_on is None else np.ascontiguousarray(s_on, np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(lib().bmpc_set_transform(self._h, _p(S), _p(on), _p(bx), _p(m)), "bmpc_set_transform")

    def set_fx(self, Fx, mask=None):
        """Per-ego state-constraint matrix Fx [B,nFx,n] of the next solves -- the Fx argument of
        BranchMPC_CVaR.solve (MPC_branch.py:2055-2056), kept until the next one; transform
        plans only (bmpc_set_fx)."""
        Fx = np.ascontiguousarray(np.asarray(Fx, np.float64).reshape(self.batch, self.desc.nFx, self.desc.n))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(lib().bmpc_set_fx(self._h, _p(Fx), _p(m)), "bmpc_set_fx")

    def branch_dp(self):
        """BranchTree.dp (d p / d x) of every non-leaf branch of the last solve [B,bdim,m,n]."""
        out = np.zeros((self.batch, self.bdim, self.desc.m, self.desc.n))
        check(lib().bmpc_get_branch_dp(self._h, _p(out)), "bmpc_get_branch_dp")
        return out

    def get_robust_warm_start(self):
        """robustMPC's warm start: xLin [B,T,n], uLin [B,U,d], OldInput [B,d]."""
        B, n, d = self.batch, self.desc.n, self.desc.d
        xl, ul, old = np.zeros((B, self.T, n)), np.zeros((B, self.U, d)), np.zeros((B, d))
        check(lib().bmpc_get_robust_warm_start(self._h, _p(xl), _p(ul), _p(old)), "bmpc_get_robust_warm_start")
        return dict(xLin=xl, uLin=ul, old_input=old)

    def set_robust_warm_start(self, xLin, uLin, old_input=None, mask=None):
        """robustMPC resume: the shifted prediction (MPC_branch.py:1429-1431) and OldInput."""
        B, n, d = self.batch, self.desc.n, self.desc.d
        xl = np.ascontiguousarray(np.asarray(xLin, np.float64).reshape(B, self.T, n))
        ul = np.ascontiguousarray(np.asarray(uLin, np.float64).reshape(B, self.U, d))
        old = None if old_input is None else np.ascontiguousarray(np.asarray(old_input, np.float64).reshape(B, d))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        check(lib().bmpc_set_robust_warm_start(self._h, _p(xl), _p(ul), _p(old), _p(m)),
              "bmpc_set_robust_warm_start")

    def tree(self):
        B, n, d = self.batch, self.desc.n, self.desc.d
        out = dict(xbar=np.zeros((B, self.T, n)), ubar=np.zeros((B, self.U, d)),
                   zbar=np.zeros((B, self.T, n)), w=np.zeros((B, self.nbranch)),
                   p=np.zeros((B, self.bdim, self.desc.m)), sol=np.zeros((B, self.nv)))
        check(lib().bmpc_get_tree(self._h, *(_p(out[k]) for k in ("xbar", "ubar", "zbar", "w", "p", "sol"))),
              "bmpc_get_tree")
        return out

    def set_lane_ref(self, grid, values):
        """The lane reference psiref(X) of the plan's *_PSIREF policies (bmpc_set_lane_ref)."""
        g, v = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)) for a in (grid, values))
        check(lib().bmpc_set_lane_ref(self._h, g.size, _p(g), _p(v)), "bmpc_set_lane_ref")

    def last_lin_cache(self):
        """Whether the solver kernel of the plan's last solve read A of the linearisation from its LDS
        cache (bmpc_last_lin_cache)."""
        return bool(lib().bmpc_last_lin_cache(self._h))

    def last_kernel(self):
        """The solver kernel the plan's last solve launched (abi.KERNEL_*, BMPC_INFO_SOLVER)."""
        info = np.zeros(abi.INFO_COUNT, np.int32)
        check(lib().bmpc_plan_info(self._h, _p(info)), "bmpc_plan_info")
        return int(info[abi.INFO_SOLVER])

    # ---- timing ---------------------------------------------------------------------------
    PHASES = ("tree", "resid", "scaling", "factor", "coupling", "kkt", "treesolve", "refine", "-",
              "init", "total", "nsolve", "applyW", "applyG", "applyGT", "ntree", "G_lp", "G_cone", "napplyG",
              "ts_pre", "ts_bw", "ts_fw", "ts_post", "riccati", "coup_ts", "coup_dot", "coup_lu", "lu_solve",
              "kkt_back", "ric_load", "ric_a", "ric_b")

    def counters(self, width=24):
        """Per-ego phase cycle counters (non-zero only for a -DBMPC_PROFILE build, whose counter
        block is 32 wide: pass width=32 for it)."""
        out = np.zeros((self.batch, width))
        check(lib().bmpc_get_counters(self._h, _p(out)), "bmpc_get_counters")
        return out

    def enable_timing(self, on=True):
        check(lib().bmpc_enable_timing(self._h, 1 if on else 0), "bmpc_enable_timing")

    def timing(self):
        ms = np.zeros(2)
        cnt = C.c_int32()
        check(lib().bmpc_timing(self._h, _p(ms), C.byref(cnt)), "bmpc_timing")
        return dict(tree_ms=float(ms[0]), ipm_ms=float(ms[1]), count=int(cnt.value))


def population_ancestors(logw, round, seed=0, ess_fraction=0.5, ego_base=0, stride=1, batch=None, weights=True,
                         device: int = 0, stream=None):
    """The resampling rule alone, on the GPU (bmpc_population_ancestors): a pure function of the
    log-weights that needs no plan.  logw: a float64 torch tensor on the device (entry e at
    logw.flatten()[e * stride]; batch defaults to numel // stride -- a scene tensor's ENV_LOGW
    column is ``scene[:, abi.ENV_LOGW:]`` flattened, stride abi.ENV_STRIDE) or any host array, which
    is uploaded.  Returns torch tensors on the device: (ancestor [batch] int32, k [batch] int64 --
    the integer weights used, bit patterns of the C side's uint64, or None with weights=False --,
    info [abi.RESAMPLE_NINFO]).  Asynchronous on `stream` (None: the context's own stream, which is
    not ordered with torch's: synchronise the device before reading)."""
    import torch
    dev = torch.device("cuda", device)
    if not hasattr(logw, "data_ptr"):
        logw = torch.tensor(np.ascontiguousarray(np.asarray(logw, np.float64)), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
    if logw.dtype != torch.float64 or not logw.is_contiguous():
        raise ValueError("logw must be a contiguous float64 tensor")
    B = (logw.numel() + int(stride) - 1) // int(stride) if batch is None else int(batch)
    if int(stride) >= 1 and B >= 1 and (B - 1) * int(stride) >= logw.numel():
        raise ValueError(f"{B} entries at stride {stride} do not fit a tensor of {logw.numel()}")
    desc = abi.make_resample_desc(round, seed, ess_fraction, ego_base)
    anc = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    k = torch.empty(max(B, 1), dtype=torch.int64, device=dev) if weights else None
    info = torch.empty(abi.RESAMPLE_NINFO, dtype=torch.float64, device=dev)
    check(lib().bmpc_population_ancestors(context(device), C.byref(desc), B, C.c_void_p(logw.data_ptr()), int(stride),
                                          C.c_void_p(anc.data_ptr()), C.c_void_p(k.data_ptr()) if weights else None,
                                          C.c_void_p(info.data_ptr()), C.c_void_p(stream) if stream else None),
          "bmpc_population_ancestors")
    return anc, k, info


def model_eval(desc: abi.PlanDesc, pol_rows, x, u, z, device: int = 0, lane_ref=None):
    """Batched PredictiveModel evaluation on the GPU (parity entry); lane_ref = (grid, values)
    of the psiref policies' lane reference (bmpc_model_eval_ref)."""
    x, u, z = (np.ascontiguousarray(np.atleast_2d(np.asarray(v, np.float64))) for v in (x, u, z))
    B, n, d, m, N = x.shape[0], desc.n, desc.d, desc.m, desc.N
    out = dict(A=np.zeros((B, n, n)), B=np.zeros((B, n, d)), C=np.zeros((B, n)), xp=np.zeros((B, n)),
               p=np.zeros((B, m)), dp=np.zeros((B, m, n)), zpred=np.zeros((B, N, m * n)),
               h0=np.zeros(B), dh=np.zeros((B, n)))
    arr = abi.policy_array(pol_rows)
    g, v = (None, None) if lane_ref is None else (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))
                                                  for a in lane_ref)
    check(lib().bmpc_model_eval_ref(context(device), C.byref(desc), arr, 0 if g is None else g.size, _p(g), _p(v),
                                    B, _p(x), _p(u), _p(z),
                                    *(_p(out[k]) for k in ("A", "B", "C", "xp", "p", "dp", "zpred", "h0", "dh"))),
          "bmpc_model_eval_ref")
    return out


def hmm_eval(M, m, consts, xb, u, xbackup, device: int = 0):
    """Batched HMM belief-model linearisation on the GPU (HMM_backup_dyn.py:216-276).
    consts = (dt, L, W, ylb, yub, col_alpha, s1, tran_diag)."""
    xb = np.ascontiguousarray(np.atleast_2d(np.asarray(xb, np.float64)))
    B, nb = xb.shape[0], 4 + M * m
    u = np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(u, np.float64)), (B, 2)))
    xbk = np.ascontiguousarray(np.broadcast_to(np.asarray(xbackup, np.float64).reshape(-1, M * m, 4), (B, M * m, 4)))
    hc = np.ascontiguousarray(np.asarray(consts, np.float64).reshape(8))
    out = dict(xbp=np.zeros((B, nb)), A=np.zeros((B, nb, nb)), B=np.zeros((B, nb, 2)), C=np.zeros((B, nb)),
               h0=np.zeros((B, M, m)), Jh=np.zeros((B, M, m, nb)))
    check(lib().bmpc_hmm_eval(context(device), M, m, _p(hc), B, _p(xb), _p(u), _p(xbk),
                              *(_p(out[k]) for k in ("xbp", "A", "B", "C", "h0", "Jh"))), "bmpc_hmm_eval")
    return out


def qp_arrays(P, q, A, l, u):
    """CSC arrays of one QP -- or of a batch sharing one pattern -- in bmpc_qp_solve's layout.

    ``P`` / ``A`` are scipy sparse or dense matrices (or equal-length sequences of them); only
    the upper triangle of P is kept (OSQP's interface does the same, PredictiveControllers.py:
    325).  A batch's pattern is the union of its members' patterns."""
    import scipy.sparse as sp
    many = isinstance(P, (list, tuple))
    B = len(P) if many else 1
    same = many and all(p is P[0] for p in P) and all(a is A[0] for a in A)   # one matrix pair, B right sides
    Ps = [sp.triu(sp.csc_matrix(p), format="csc") for p in ([P[0]] if same else P if many else [P])]
    As = [sp.csc_matrix(a) for a in ([A[0]] if same else A if many else [A])]
    n = Ps[0].shape[1]
    m = As[0].shape[0]

    def pattern(ms):
        pat = sp.csc_matrix(ms[0].shape)
        for mat in ms:
            pat = pat + sp.csc_matrix((np.ones(mat.nnz), mat.indices, mat.indptr), shape=mat.shape)
        pat = sp.csc_matrix(pat)
        pat.sort_indices()
        rows = pat.indices.astype(np.int64)
        cols = np.repeat(np.arange(pat.shape[1]), np.diff(pat.indptr))
        vals = np.stack([np.asarray(sp.csr_matrix(mat)[rows, cols]).reshape(-1) for mat in ms]) if len(rows) else \
            np.zeros((len(ms), 0))
        return pat.indptr.astype(np.int32), pat.indices.astype(np.int32), vals

    Pp, Pi, Px = pattern(Ps)
    Ap, Ai, Ax = pattern(As) if m else (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros((len(As), 0)))
    if same:
        Px, Ax = np.repeat(Px, B, axis=0), np.repeat(Ax, B, axis=0)
    def f2(a, k):
        a = np.asarray(a, np.float64)
        return np.ascontiguousarray(np.broadcast_to(a.reshape(-1, k) if k else np.zeros((B, 0)), (B, k)))
    return dict(n=n, m=m, Pp=Pp, Pi=Pi, Ap=Ap, Ai=Ai, Px=np.ascontiguousarray(Px), q=f2(q, n),
                Ax=np.ascontiguousarray(Ax), l=f2(l, m), u=f2(u, m))


def qp_solve(P, q, A, l, u, max_iter: int = 100, eps: float = 1e-10, device: int = 0):
    """OSQP-form QP(s)  min 1/2 x'Px + q'x  s.t. l <= Ax <= u  on the GPU (bmpc_qp_solve:
    interior point on the band-ordered KKT matrix, one wave per problem).  Returns
    dict(x [B][n], y [B][m], status [B] (1 solved, -2 max_iter, -8 numerics), iters [B],
    info = (KKT dimension, bandwidth, inequality rows, band entries))."""
    a = qp_arrays(P, q, A, l, u)
    B, n, m = a["q"].shape[0], a["n"], a["m"]
    x, y = np.zeros((B, n)), np.zeros((B, max(m, 1)))
    st, it, info = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(4, np.int32)
    check(lib().bmpc_qp_solve(context(device), n, m, _p(a["Pp"]), _p(a["Pi"]), _p(a["Ap"]), _p(a["Ai"]), B,
                              _p(a["Px"]), _p(a["q"]), _p(a["Ax"]), _p(a["l"]), _p(a["u"]), int(max_iter),
                              float(eps), _p(x), _p(y), _p(st), _p(it), _p(info)), "bmpc_qp_solve")
    return dict(x=x, y=y[:, :m], status=st, iters=it, info=info)
