"""Synthetic workloads of the headline benchmark and the plan descriptions
of the reference's scenes (Init_MPC.initBranchMPC + Branch_constants, main_branch.py:37)."""
from __future__ import annotations

import numpy as np

from . import abi


# the overtake scene's three controllers (main_branch.py): BranchMPC_CVaR, BranchMPC (the expected-cost
# branch MPC, MPC_branch.py:881) and robustMPC
HIGHWAY_CONTROLLERS = {"cvar": abi.CTRL_CVAR, "branch": abi.CTRL_QP, "robust": abi.CTRL_ROBUST}


def highway_desc(N=20, NB=1, N_lane=4, am=6.0, rm=0.3, L=4.0, W=2.5, s1=2.0, model_lanes=3, controller="cvar"):
    """initBranchMPC(n=4,d=2,N,NB,...) + Branch_constants of main_branch.py:37.  controller: "cvar"
    (BranchMPC_CVaR), "branch" (BranchMPC) or "robust" (robustMPC) -- HIGHWAY_CONTROLLERS."""
    if controller not in HIGHWAY_CONTROLLERS:
        raise ValueError(f"controller={controller!r}: one of {sorted(HIGHWAY_CONTROLLERS)}")
    Fx = np.array([[0., 1, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1], [0, 0, 0, -1]])
    bx = np.array([N_lane * 3.6 - W / 2, -W / 2, 0.25, 0.25])
    Fu = np.kron(np.eye(2), np.array([1, -1])).T
    bu = np.array([am, am, rm, rm])
    return abi.make_desc(HIGHWAY_CONTROLLERS[controller], abi.MODEL_HIGHWAY, 4, 2, N, NB, 3, 0.1,
                         np.diag([0., 3, 3, 10]), np.diag([1., 100]), Fx, bx, Fu, bu, [0., 300.],
                         [L, W, s1, float(model_lanes)], ralpha=0.9)


def highway_desc_from_golden(g, controller="cvar"):
    return highway_desc(N=int(g["N"]), NB=int(g["NB"]), N_lane=int(g["N_lane"]), am=float(g["am"]),
                        rm=float(g["rm"]), L=float(g["L"]), W=float(g["W"]), s1=float(g["s1"]),
                        controller=controller)


def highway_policy_rows(targets, Kpsi=0.1):
    return [[(abi.POL_MAINTAIN, (Kpsi,)), (abi.POL_BRAKE, (Kpsi,)), (abi.POL_LC, tuple(map(float, t)))]
            for t in np.atleast_2d(targets)]


LANES = np.array([1.8, 5.4, 9.0, 12.6])


def seeded_batch(B, seed=0):
    """SURVEY §8(d) synthetic inputs; row 0 is the sim_overtake initial state."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 4))
    z = np.zeros((B, 4))
    li = rng.integers(0, 4, B)
    x[:, 0] = rng.uniform(-5, 5, B)
    x[:, 1] = LANES[li] + rng.normal(0, 0.1, B)
    x[:, 2] = rng.uniform(15, 25, B)
    x[:, 3] = np.clip(rng.normal(0, 0.02, B), -0.2, 0.2)
    lo = (li + rng.integers(1, 4, B)) % 4
    z[:, 0] = x[:, 0] + rng.uniform(-10, 30, B)
    z[:, 1] = LANES[lo]
    z[:, 2] = rng.uniform(15, 25, B)
    x[0] = [0, 1.8, 20, 0]
    z[0] = [5, 5.4, 20, 0]
    xref, tgt = xref_rule(x, z)
    return x, z, xref, tgt


def xref_rule(x, z, v0=20.0):
    """x_ref of Highway_env.step (Highway_env_branch.py:153-167) and the lane-change target
    of update_backup (:103-116), vectorised over egos (first step, t == 0)."""
    B = x.shape[0]
    l0 = np.array([round((v - 1.8) / 3.6) for v in x[:, 1]])
    l1 = np.array([round((v - 1.8) / 3.6) for v in z[:, 1]])
    tgt = np.zeros((B, 4))
    tgt[:, 2] = v0
    for i in range(B):
        if l0[i] < l1[i]:
            tgt[i, 1] = 1.8 + 3.6 * (l1[i] - 1)
        elif l0[i] > l1[i]:
            tgt[i, 1] = 1.8 + 3.6 * (l1[i] + 1)
        elif l1[i] > 0:
            tgt[i, 1] = 1.8 + 3.6 * (l1[i] - 1)
        else:
            tgt[i, 1] = 1.8 + 3.6 * (l1[i] + 1)
    Ydes = np.where(x[:, 0] < z[:, 0], 1.8 + l0 * 3.6, z[:, 1])
    vdes = np.where((np.abs(x[:, 1] - Ydes) < 1) & (x[:, 0] > z[:, 0] + 3), v0,
                    z[:, 2] + 1 * (z[:, 0] + 1.5 - x[:, 0]))
    xref = np.stack([np.zeros(B), Ydes, vdes, np.zeros(B)], axis=1)
    return xref, tgt


def _attach_record(pl, steps, record):
    """The recorder of a *_population call: None, or a LoopRecording of `steps` rows per ego attached
    to the plan -- record=True the core columns, record="predictions" also uPred / xPred / zPred /
    branch_w (BatchPlan.new_loop_record)."""
    if not record:
        return None
    rec = pl.new_loop_record(steps, 0, predictions=(record == "predictions"))
    pl.set_loop_record(rec)
    return rec


def _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base):
    """The obstacle sampler of a sampled_*_population call: obstacle=None leaves the plan on the
    reference's deterministic rule, "model" attaches BatchPlan.set_obstacle_sampling("model", ...)."""
    if obstacle is None:
        return None
    if obstacle != "model":
        raise ValueError(f"obstacle={obstacle!r}: None (the reference's rule) or 'model'")
    pl.set_obstacle_sampling("model", seed=obstacle_seed, hold=hold, ego_base=ego_base)
    return pl.obstacle_sampling


def _shard_rows(B, ego_base, population):
    """Rows [ego_base, ego_base + B) of a population of `population` egos (default: ends with them)."""
    lo = int(ego_base)
    total = lo + B if population is None else int(population)
    if lo < 0 or B < 1 or lo + B > total:
        raise ValueError(f"egos {lo}..{lo + B - 1} do not lie in a population of {total}")
    return total, slice(lo, lo + B)


def overtake_population(B, steps, seed=0, device=0, record=False):
    """`steps` closed-loop overtake steps of B seeded episodes (seeded_batch: row 0 is
    sim_overtake's initial state), resident on the GPU (BatchPlan.loop_device).  Returns the per-ego
    statistics rows [B, ENV_NSTAT] (the form distributed.episode_stats takes; a step's solve is
    booked by the next step, so they cover steps - 1 solves) and the final scene [B, ENV_STRIDE];
    with `record` also the per-step record on the host (plan.LoopRecording: row t holds step t,
    the last row's scene is the returned one).  The obstacle follows the reference's deterministic
    rule; sampled_overtake_population draws its policy from the model's branch distribution (and
    takes a plan description: desc=highway_desc(controller="branch") runs BranchMPC)."""
    return sampled_overtake_population(B, steps, seed, device, record, obstacle=None)


def sampled_overtake_population(B, steps, seed=0, device=0, record=False, obstacle="model", obstacle_seed=0, hold=1,
                                ego_base=0, population=None, desc=None):
    """overtake_population with an obstacle that draws its backup policy from the model's own branch
    distribution (obstacle="model": BatchPlan.set_obstacle_sampling with seed `obstacle_seed`, a
    choice kept for `hold` steps; obstacle=None is overtake_population itself).  The B egos are rows
    ego_base .. ego_base + B - 1 of seeded_batch(population, seed) (population defaults to
    ego_base + B) and draw as those global egos: a sharded run passes
    ego_base = distributed.shard(population, rank, world)[0] and B = hi - lo on every rank, and each
    ego then has the trajectory it has in the unsharded run.  desc: another highway plan description
    than highway_desc() -- highway_desc(controller="branch" | "robust") runs the scene's other two
    controllers, BranchMPC and robustMPC.  Any draw can be audited on the host with bmpc.rng.obstacle_uniform(
    obstacle_seed, global ego, t // hold)."""
    pl, scene0 = _seeded_plan("overtake", B, seed, device, ego_base, population, desc)
    _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def _overtake_scene(x, z):
    """The overtake and merge scenes' initial state rows [B, ENV_STRIDE] (csrc/bmpc_env.h)."""
    x = np.atleast_2d(np.asarray(x, float))
    scene = np.zeros((x.shape[0], abi.ENV_STRIDE))
    scene[:, abi.ENV_X:abi.ENV_X + 4] = x
    scene[:, abi.ENV_Z:abi.ENV_Z + 4] = np.atleast_2d(np.asarray(z, float))
    return scene


def _scene_desc(kind, desc=None):
    """desc, or the description of scene `kind` ("overtake", "merge", "quadruped") with its defaults."""
    if desc is not None:
        return desc
    return {"overtake": highway_desc, "merge": merge_desc, "quadruped": quadruped_desc}[kind]()


def _scene_plan(kind, x, z, x_des=None, desc=None, device=0):
    """The plan of scene `kind` ("overtake", "merge", "quadruped") for the egos of states x, z [B, n]
    (quadruped: goals x_des) -- its description (desc=None: the scene's own), policies and, for the
    merge, scene constants -- and the egos' initial scene rows [B, ENV_STRIDE]."""
    from . import plan
    B = len(x)
    if kind == "overtake":
        rows, scene0 = highway_policy_rows(xref_rule(x, z)[1]), _overtake_scene(x, z)
    elif kind == "merge":
        rows, scene0 = merge_policy_rows(B), _overtake_scene(x, z)
    else:
        rows, scene0 = quadruped_policy_rows(B), quad_scene(x, z, x_des)
    pl = plan.BatchPlan(_scene_desc(kind, desc), B, device)
    pl.set_policies(rows)
    if kind == "merge":
        pl.set_merge_scene(abi.make_merge_env(), *merge_lane_ref())
    return pl, scene0


def _seeded_plan(kind, B, seed, device, ego_base=0, population=None, desc=None):
    """_scene_plan for rows [ego_base, ego_base + B) of the scene's seeded population: seeded_batch,
    seeded_merge_batch, or seeded_quadruped_batch with seeded_quadruped_goals."""
    total, rows = _shard_rows(B, ego_base, population)
    x_des = None
    if kind == "overtake":
        x, z = seeded_batch(total, seed)[:2]
    elif kind == "merge":
        x, z = seeded_merge_batch(total, seed)
    else:
        x, z = seeded_quadruped_batch(total, seed)[:2]
        x_des = seeded_quadruped_goals(total, seed)[rows]
    return _scene_plan(kind, x[rows], z[rows], x_des, desc, device)


_LOOP_BUFFERS = ("scene", "upred", "x", "z", "xref", "J", "status", "iters", "stats")   # the loop entries' order


def _closed_loop(pl, scene0, steps, record, device, every=None, resample=None):
    """`steps` closed-loop steps from t = 0 of the plan `pl` (policies, scene and options set) from the
    scene rows scene0 [B, ENV_STRIDE], on one stream without a host synchronisation: the population
    entries' results (stats, scene[, record]); closes the plan.  every: loop calls of `every` steps
    with BatchPlan.resample(buffers, round = the step the next call starts at, **resample) between
    them; then also the list of (ancestor, info) per resampling."""
    import torch
    B, n, d = pl.batch, pl.desc.n, pl.desc.d
    steps = int(steps)
    every = steps if every is None else int(every)
    dev = torch.device("cuda", device)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    b = dict(scene=torch.tensor(scene0, **f64), upred=torch.zeros((B, pl.U, d), **f64), x=torch.zeros((B, n), **f64),
             z=torch.zeros((B, n), **f64), xref=torch.zeros((B, n), **f64), J=torch.zeros(B, **f64),
             status=torch.zeros(B, **i32), iters=torch.zeros(B, **i32), stats=torch.zeros((B, abi.ENV_NSTAT), **f64))
    rec = _attach_record(pl, steps, record)
    torch.cuda.synchronize(dev)          # the buffers are written before the loop's stream starts
    stream = torch.cuda.Stream(dev)
    loop = pl._scene_loop()
    rounds = []
    for t in ((0,) if resample is None else range(0, steps, every)):
        if t > 0:
            rounds.append(pl.resample(b, t, stream=stream.cuda_stream, **resample))
        loop(t, min(every, steps - t), *(b[k].data_ptr() for k in _LOOP_BUFFERS), stream.cuda_stream)
    stream.synchronize()
    out = b["stats"].cpu().numpy(), b["scene"].cpu().numpy()
    if rec is not None:
        out += (rec.host(),)
    pl.close()
    if resample is None:
        return out
    return out, [(a.cpu().numpy(), i.cpu().numpy()) for a, i in rounds]


def merge_desc(N=40, NB=1, N_lane=2, am=7.0, rm=0.3, L=4.0, W=2.5, s1=2.0, ralpha=0.1):
    """main_branch.sim_merge (:53-88): initBranchMPC(4, 2, 40, 1, ..., N_lane=2) driving
    BranchMPC_CVaR(ralpha=0.1) over PredictiveModel_merge's main-road model (pred_model[0])."""
    Fx = np.array([[0., 1, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1], [0, 0, 0, -1]])
    bx = np.array([N_lane * 3.6 - W / 2, -W / 2, 0.25, 0.25])
    Fu = np.kron(np.eye(2), np.array([1, -1])).T
    bu = np.array([am, am, rm, rm])
    return abi.make_desc(abi.CTRL_CVAR, abi.MODEL_HIGHWAY_MERGE, 4, 2, N, NB, 2, 0.1,
                         np.diag([0., 3, 3, 10]), np.diag([1., 100]), Fx, bx, Fu, bu, [0., 300.],
                         [L, W, s1, float(N_lane)], ralpha=ralpha)


def merge_policy_rows(B, Kpsi=0.1, v0=20.0):
    """backupcons_normal of sim_merge (:83): maintain_trackV(v0), brake."""
    return [[(abi.POL_MAINTAIN_TRACKV, (Kpsi, v0)), (abi.POL_BRAKE, (Kpsi,))] for _ in range(B)]


def merge_lane_ref(N_lane=2, merge_lane=1, merge_s=50, merge_R=300, merge_side=0):
    """The ramp's lane references (grid X, refY, refpsi) of sim_merge (:74-79), from the drop-in
    module's merge_geometry."""
    from Highway_env_branch import merge_geometry
    X1, X2, Y1, Y2, p1, p2 = merge_geometry(N_lane, merge_lane, merge_s, merge_R, merge_side)
    return np.append(X1, X2), np.append(Y1, Y2), np.append(p1, p2)


MERGE_X0 = np.array([24., 13, 20, -0.2])   # Highway_env_merge's initial states (:312)
MERGE_Z0 = np.array([15., 5.4, 20, 0])


def seeded_merge_batch(B, seed=0):
    """A Monte-Carlo population of merge episodes: row 0 is sim_merge's initial state, the others
    start around it (ego +-2 m along / +-0.2 m across the ramp, +-1 m/s, +-0.02 rad; obstacle
    +-3 m along its lane, +-1 m/s)."""
    rng = np.random.default_rng(seed)
    x = np.repeat(MERGE_X0[None], B, 0)
    z = np.repeat(MERGE_Z0[None], B, 0)
    x[1:] += rng.uniform(-1, 1, (B - 1, 4)) * [2, 0.2, 1, 0.02]
    z[1:] += rng.uniform(-1, 1, (B - 1, 4)) * [3, 0, 1, 0]
    return x, z


def merge_population(B, steps, seed=0, device=0, record=False):
    """`steps` closed-loop merge steps of B seeded episodes, resident on the GPU
    (BatchPlan.merge_loop_device).  Returns the per-ego statistics rows [B, ENV_NSTAT] (the form
    distributed.episode_stats takes; a step's solve is booked by the next step, so they cover
    steps - 1 solves) and the final scene [B, ENV_STRIDE]; with `record` (overtake_population's)
    also the per-step record on the host."""
    pl, scene0 = _seeded_plan("merge", B, seed, device)
    return _closed_loop(pl, scene0, steps, record, device)


def quadruped_desc(N=25, NB=2, vxm=0.2, vym=0.1, rm=0.5, dt=0.2, L1=0.5, W1=0.3, L2=1.0, W2=0.6,
                   col_tol=0.2, s1=2.0):
    """initquadBranchMPC(3,3,N,NB,...) + the main_quadruped.py:15-30 constants
    (BranchMPCProx controller, 2 policies)."""
    Fu = np.kron(np.eye(3), np.array([1, -1])).T
    bu = np.array([vxm, 0.0, vym, vym, rm, rm])
    return abi.make_desc(abi.CTRL_PROX, abi.MODEL_QUADRUPED, 3, 3, N, NB, 2, dt, np.eye(3),
                         np.diag([1., 100., 1.]), np.zeros((0, 3)), [], Fu, bu, [0., 300.],
                         [L1, W1, L2, W2, col_tol, s1], dR=[0.9, 5.0, 1.0])


def quadruped_policy_rows(B, v0=0.2):
    return [[(abi.POL_FORWARD, (v0,)), (abi.POL_STOP, ())] for _ in range(B)]


def seeded_quadruped_batch(B, seed=1):
    """Synthetic quadruped egos (BASELINE config 4): ego in a 6 m x 6 m yard heading anywhere,
    obstacle 1-4 m away walking at any heading; goal x_des = (5, -3, 0) as in the recorded
    loop.  Row 0 is main_quadruped's state (ego (0, 1.8, 0), obstacle (2.5, 2.5, -pi/2))."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-1, 1, B), rng.uniform(0, 3, B), rng.uniform(-np.pi, np.pi, B)], 1)
    r, a = rng.uniform(1, 4, B), rng.uniform(-np.pi, np.pi, B)
    z = np.stack([x[:, 0] + r * np.cos(a), x[:, 1] + r * np.sin(a), rng.uniform(-np.pi, np.pi, B)], 1)
    x[0] = [0, 1.8, 0]
    z[0] = [2.5, 2.5, -np.pi / 2]
    return x, z, quadruped_xref(x)


QUAD_X_DES = np.array([5.0, -3.0, 0.0])   # quadruped_env.sim's goal (:327)


def seeded_quadruped_goals(B, seed=1):
    """Per-ego goals of a quadruped population: row 0 is sim's x_des, the others lie 2 m around it
    with any heading."""
    rng = np.random.default_rng([seed, 1])
    g = QUAD_X_DES + np.stack([rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(-np.pi, np.pi, B)], 1)
    g[0] = QUAD_X_DES
    return g


def quad_scene(x, z, x_des):
    """The quadruped scene's initial state rows [B, ENV_STRIDE] (csrc/bmpc_env_quad.h)."""
    x = np.atleast_2d(np.asarray(x, float))
    scene = np.zeros((x.shape[0], abi.ENV_STRIDE))
    scene[:, abi.QENV_X:abi.QENV_X + 3] = x
    scene[:, abi.QENV_Z:abi.QENV_Z + 3] = np.atleast_2d(np.asarray(z, float))
    scene[:, abi.QENV_XDES:abi.QENV_XDES + 3] = np.asarray(x_des, float)
    return scene


def quadruped_population(B, steps, seed=0, device=0, record=False):
    """`steps` closed-loop main_quadruped steps of B seeded episodes (seeded_quadruped_batch, each
    ego walking to a goal of its own), resident on the GPU (BatchPlan.quad_loop_device).  Returns
    the per-ego statistics rows [B, ENV_NSTAT] (the form distributed.episode_stats takes; a step's
    solve is booked by the next step, so they cover steps - 1 solves) and the final scene
    [B, ENV_STRIDE]; with `record` (overtake_population's) also the per-step record on the host.
    The obstacle follows the reference's deterministic rule; sampled_quadruped_population draws its
    policy from the model's branch distribution."""
    return sampled_quadruped_population(B, steps, seed, device, record, obstacle=None)


def sampled_quadruped_population(B, steps, seed=0, device=0, record=False, obstacle="model", obstacle_seed=0, hold=1,
                                 ego_base=0, population=None, desc=None):
    """quadruped_population with the sampled obstacle: sampled_overtake_population's arguments and
    sharding rule (rows ego_base .. ego_base + B - 1 of seeded_quadruped_batch(population, seed) and
    of seeded_quadruped_goals; a sharded run passes ego_base = distributed.shard(...)[0])."""
    pl, scene0 = _seeded_plan("quadruped", B, seed, device, ego_base, population, desc)
    _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def _attach_tilt(pl, tilt, obstacle_seed, hold, ego_base):
    """The tilted obstacle of a weighted_*_population call: the proposal, then the mode that needs it."""
    pl.set_obstacle_proposal(tilt=tilt)
    pl.set_obstacle_sampling("tilted", seed=obstacle_seed, hold=hold, ego_base=ego_base)


def _attach_script(pl, m, epochs, hold):
    """The full enumeration of an enumerated_*_population call: ego e follows row e of
    montecarlo.enumerate_scripts(m, epochs), one choice per `hold` steps."""
    from . import montecarlo
    if pl.batch != m ** epochs:
        raise ValueError(f"the plan must hold {m} ** {epochs} egos, one per path")
    script = montecarlo.enumerate_scripts(m, epochs)
    pl.set_obstacle_proposal(script=script)
    pl.set_obstacle_sampling("script", hold=hold)
    return script


def _with_logw(out):
    """(stats, scene[, record]) -> (stats, scene, logw[, record]): the scenes' ENV_LOGW column."""
    return out[:2] + (out[1][:, abi.ENV_LOGW].copy(),) + out[2:]


def weighted_overtake_population(B, steps, seed=0, device=0, record=False, obstacle_seed=0, hold=1, ego_base=0,
                                 population=None, desc=None, tilt=None):
    """sampled_overtake_population under importance sampling: the obstacle draws from the model's
    branch distribution tilted by `tilt` (one positive b_j per policy, None: all 1 -- the sampled
    population itself; BatchPlan.set_obstacle_proposal, mode "tilted"), at the same draws and with the
    same sharding rule (ego_base = distributed.shard(...)[0]).  Returns the statistics rows, the final
    scene and the per-ego log-weight logw [B] = log of the likelihood ratio p / q of each ego's
    realised choice sequence (the scene's abi.ENV_LOGW column, which starts at 0); with `record` also
    the record, whose `logw` column holds the weight's history.  montecarlo.estimate(f, logw) is the
    estimate of E_p[f] with its standard error."""
    pl, scene0 = _seeded_plan("overtake", B, seed, device, ego_base, population, desc)
    _attach_tilt(pl, tilt, obstacle_seed, hold, ego_base)
    return _with_logw(_closed_loop(pl, scene0, steps, record, device))


def weighted_quadruped_population(B, steps, seed=0, device=0, record=False, obstacle_seed=0, hold=1, ego_base=0,
                                  population=None, desc=None, tilt=None):
    """sampled_quadruped_population under importance sampling: weighted_overtake_population's
    arguments and results (sharding by ego_base = distributed.shard(...)[0])."""
    pl, scene0 = _seeded_plan("quadruped", B, seed, device, ego_base, population, desc)
    _attach_tilt(pl, tilt, obstacle_seed, hold, ego_base)
    return _with_logw(_closed_loop(pl, scene0, steps, record, device))


def _resampled(kind, B, steps, resample_every, ess_fraction, resample_seed, tilt, seed, device, record, obstacle_seed,
               hold, ego_base, population, desc):
    """The resampled_*_population entries: the weighted population of scene `kind` in loop calls of
    `resample_every` steps with BatchPlan.resample between them."""
    if int(resample_every) < 1 or int(resample_every) % int(hold):
        raise ValueError(f"resample_every must be a positive multiple of hold = {hold}")
    pl, scene0 = _seeded_plan(kind, B, seed, device, ego_base, population, desc)
    _attach_tilt(pl, tilt, obstacle_seed, hold, ego_base)
    out, rounds = _closed_loop(pl, scene0, steps, record, device, every=resample_every,
                               resample=dict(seed=resample_seed, ess_fraction=ess_fraction, ego_base=ego_base))
    return _with_logw(out) + (rounds,)


def resampled_overtake_population(B, steps, resample_every, ess_fraction=0.5, resample_seed=0, tilt=None, seed=0,
                                  device=0, record=False, obstacle_seed=0, hold=1, ego_base=0, population=None,
                                  desc=None):
    """weighted_overtake_population with the population resampled between loop segments: loop calls
    of `resample_every` steps (a multiple of `hold`) with BatchPlan.resample between them, at round =
    the step the next call starts at and the draw bmpc.resample.offset(resample_seed, ego_base, round),
    whenever the effective sample size is below ess_fraction * B.  Egos of large weight are cloned
    into the slots of egos of negligible weight and all continue with the mean weight, so
    montecarlo.estimate(f, logw) stays the unbiased plain estimate while the solves go where the
    probability mass is.  Returns weighted_overtake_population's tuple plus the list of
    (ancestor [B], info [abi.RESAMPLE_NINFO]) per resampling; with `record` the record's rows stay
    addressed by slot and montecarlo.lineage(ancestors) tells which slot a final ego lived in.  A
    sharded run (ego_base = distributed.shard(...)[0]) resamples every shard by itself: a shard's mean
    weight carries its mass, and montecarlo.reduce_terms over the shards stays the plain estimate."""
    return _resampled("overtake", B, steps, resample_every, ess_fraction, resample_seed, tilt, seed, device, record,
                      obstacle_seed, hold, ego_base, population, desc)


def resampled_quadruped_population(B, steps, resample_every, ess_fraction=0.5, resample_seed=0, tilt=None, seed=0,
                                   device=0, record=False, obstacle_seed=0, hold=1, ego_base=0, population=None,
                                   desc=None):
    """weighted_quadruped_population with the population resampled between loop segments:
    resampled_overtake_population's arguments and results (a sharded run, ego_base =
    distributed.shard(...)[0], resamples every shard by itself)."""
    return _resampled("quadruped", B, steps, resample_every, ess_fraction, resample_seed, tilt, seed, device, record,
                      obstacle_seed, hold, ego_base, population, desc)


def enumerated_overtake_population(x0, z0, epochs, hold, device=0, record=False, desc=None):
    """One initial state (x0, z0) against every obstacle choice sequence of `epochs` epochs of `hold`
    steps: m ** epochs egos, ego e following row e of montecarlo.enumerate_scripts(m, epochs)
    (BatchPlan.set_obstacle_proposal, mode "script"), for epochs * hold closed-loop steps.  Returns
    the statistics rows, the final scene, the path log-probabilities logp [m ** epochs] under the
    model's branch distribution (they sum to one: montecarlo.exact_expectation gives exact closed-loop
    expectations over the scenario tree) and the script; with `record` also the record."""
    return _enumerated("overtake", x0, z0, None, epochs, hold, device, record, desc)


def enumerated_quadruped_population(x0, z0, x_des, epochs, hold, device=0, record=False, desc=None):
    """enumerated_overtake_population for the quadruped scene: one initial state (x0, z0 [3]) and goal
    x_des [3] against all m ** epochs choice sequences."""
    return _enumerated("quadruped", x0, z0, x_des, epochs, hold, device, record, desc)


def _enumerated(kind, x0, z0, x_des, epochs, hold, device, record, desc):
    """The enumerated_*_population entries: m ** epochs copies of one state of scene `kind`, one per
    obstacle choice sequence."""
    desc = _scene_desc(kind, desc)
    m, epochs, n = int(desc.m), int(epochs), int(desc.n)
    x, z = (np.tile(np.asarray(a, float).reshape(1, n), (m ** epochs, 1)) for a in (x0, z0))
    x_des = None if x_des is None else np.asarray(x_des, float).reshape(1, n)
    pl, scene0 = _scene_plan(kind, x, z, x_des, desc, device)
    script = _attach_script(pl, m, epochs, hold)
    out = _with_logw(_closed_loop(pl, scene0, epochs * int(hold), record, device))
    return out[:3] + (script,) + out[3:]


def quadruped_xref(x, x_des=(5.0, -3.0, 0.0)):
    """Reference of the recorded quadruped loop (tools/gen_golden.py, after quadruped_env.py):
    a point at most 5 m towards x_des, heading along the way."""
    x = np.atleast_2d(x)
    xd = np.asarray(x_des, float)
    dx = xd[None, 0:2] - x[:, 0:2]
    nrm = np.linalg.norm(dx, axis=1)
    dx = dx / np.maximum(nrm, 1e-300)[:, None] * np.minimum(nrm, 5.0)[:, None]
    psi = np.arctan2(dx[:, 1], dx[:, 0])
    psi = np.where(np.linalg.norm(dx, axis=1) > 0.1, psi, x[:, 2])
    psi = psi - 2 * np.pi * np.round((psi - xd[2]) / (2 * np.pi))
    xr = x.copy()
    xr[:, 0:2] += dx
    xr[:, 2] = psi
    return xr


def _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base):
    """The actuation disturbance of a disturbed_*_population call (BatchPlan.set_disturbance); both
    sigmas None leaves the plan undisturbed."""
    if sigma_ego is None and sigma_obs is None:
        return None
    pl.set_disturbance(sigma_ego, sigma_obs, seed=disturbance_seed, ego_base=ego_base)
    return pl.disturbance


def disturbed_overtake_population(B, steps, sigma_ego=None, sigma_obs=None, disturbance_seed=0, seed=0, device=0,
                                  record=False, obstacle=None, obstacle_seed=0, hold=1, ego_base=0, population=None,
                                  desc=None):
    """sampled_overtake_population under process noise: in every Euler step the ego applies
    uPred[0] + sigma_ego * xi and the obstacle its chosen input + sigma_obs * xi, xi =
    bmpc.rng.disturbance(disturbance_seed, global ego, t, vehicle, 2) a unit-variance bounded variate per
    component (BatchPlan.set_disturbance).  sigma_ego / sigma_obs: standard deviations of
    (acceleration, yaw rate), None: zeros.  obstacle=None keeps the reference's deterministic choice,
    "model" also samples it (obstacle_seed, hold).  The sharding rule is sampled_overtake_population's
    (ego_base = distributed.shard(...)[0]): each ego has the trajectory it has in the unsharded run.
    The record's u and the scene's obstacle input are the nominal inputs; the applied ones are
    nominal + sigma * bmpc.rng.disturbance(...)."""
    pl, scene0 = _seeded_plan("overtake", B, seed, device, ego_base, population, desc)
    _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base)
    _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def disturbed_merge_population(B, steps, sigma_ego=None, sigma_obs=None, disturbance_seed=0, seed=0, device=0,
                               record=False, ego_base=0, population=None):
    """merge_population under process noise (disturbed_overtake_population's disturbance arguments):
    the merge scene's first source of randomness beyond its initial states.  The B egos are rows
    ego_base .. ego_base + B - 1 of seeded_merge_batch(population, seed) and draw as those global
    egos."""
    pl, scene0 = _seeded_plan("merge", B, seed, device, ego_base, population)
    _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def disturbed_quadruped_population(B, steps, sigma_ego=None, sigma_obs=None, disturbance_seed=0, seed=0, device=0,
                                   record=False, obstacle=None, obstacle_seed=0, hold=1, ego_base=0, population=None,
                                   desc=None):
    """sampled_quadruped_population under process noise: disturbed_overtake_population's arguments,
    the sigmas those of (vx, vy, yaw rate)."""
    pl, scene0 = _seeded_plan("quadruped", B, seed, device, ego_base, population, desc)
    _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base)
    _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def _attach_observation(pl, sigma_x, sigma_z, observation_seed, ego_base):
    """The observation noise of an observed_*_population call (BatchPlan.set_observation); both sigmas
    None leaves the controller on the true states."""
    if sigma_x is None and sigma_z is None:
        return None
    pl.set_observation(sigma_x, sigma_z, seed=observation_seed, ego_base=ego_base)
    return pl.observation


def observed_overtake_population(B, steps, sigma_x=None, sigma_z=None, observation_seed=0, sigma_ego=None,
                                 sigma_obs=None, disturbance_seed=0, seed=0, device=0, record=False, obstacle=None,
                                 obstacle_seed=0, hold=1, ego_base=0, population=None, desc=None):
    """disturbed_overtake_population with a controller that only measures the scene: the solve of step t
    is handed x + sigma_x * xi and z + sigma_z * xi, xi = bmpc.rng.observation(observation_seed, global
    ego, t, vehicle, 4) a unit-variance bounded variate per component (BatchPlan.set_observation).
    sigma_x / sigma_z: standard deviations of the observed (X, Y, v, psi) of the ego / the obstacle,
    None: zeros; the suggested use is sigma_x=None, a localised ego that perceives others with noise.
    The scene, its statistics, x_ref and the record keep the true states; what a solve saw is
    row + sigma * bmpc.rng.observation(...).  The other arguments are disturbed_overtake_population's,
    so the sampler, the disturbance and the observation combine; with all four sigmas None it is that
    entry."""
    pl, scene0 = _seeded_plan("overtake", B, seed, device, ego_base, population, desc)
    _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base)
    _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base)
    _attach_observation(pl, sigma_x, sigma_z, observation_seed, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def observed_merge_population(B, steps, sigma_x=None, sigma_z=None, observation_seed=0, sigma_ego=None, sigma_obs=None,
                              disturbance_seed=0, seed=0, device=0, record=False, ego_base=0, population=None):
    """disturbed_merge_population under observation noise (observed_overtake_population's observation
    arguments); S and bx stay those of the ego's true state."""
    pl, scene0 = _seeded_plan("merge", B, seed, device, ego_base, population)
    _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base)
    _attach_observation(pl, sigma_x, sigma_z, observation_seed, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def observed_quadruped_population(B, steps, sigma_x=None, sigma_z=None, observation_seed=0, sigma_ego=None,
                                  sigma_obs=None, disturbance_seed=0, seed=0, device=0, record=False, obstacle=None,
                                  obstacle_seed=0, hold=1, ego_base=0, population=None, desc=None):
    """disturbed_quadruped_population under observation noise: observed_overtake_population's
    arguments, the sigmas those of the observed (x, y, psi)."""
    pl, scene0 = _seeded_plan("quadruped", B, seed, device, ego_base, population, desc)
    _attach_obstacle(pl, obstacle, obstacle_seed, hold, ego_base)
    _attach_disturbance(pl, sigma_ego, sigma_obs, disturbance_seed, ego_base)
    _attach_observation(pl, sigma_x, sigma_z, observation_seed, ego_base)
    return _closed_loop(pl, scene0, steps, record, device)


def controller_comparison(B, steps, controllers=("cvar", "branch", "robust"), seed=0, device=0, record=False,
                          obstacle=None, obstacle_seed=0, hold=1, sigma_x=None, sigma_z=None, observation_seed=0,
                          sigma_ego=None, sigma_obs=None, disturbance_seed=0):
    """The overtake scene's controllers on one population of episodes: observed_overtake_population
    once per entry of `controllers` (highway_desc's keywords, each run with
    desc=highway_desc(controller=c)) with the same seeded initial states and
    the same obstacle, disturbance and observation seeds -- common random numbers: every draw is
    addressed by (seed, ego, step), so ego e of one run and ego e of another meet the same noise and,
    while their states agree, the same obstacle choices, and the episodes are paired across controllers.
    Returns a dict with
      "runs":  per controller dict(stats [B, ENV_NSTAT], scene [B, ENV_STRIDE][, record]);
      "pairs": per pair (a, b) in the order of `controllers`, dict(collided=, cost=) of
               montecarlo.paired_difference (mean of a - b, its standard error, the correlation) of the
               egos' collided flags (ENVS_COLLIDED) and mean solve costs (ENVS_J / ENVS_SOLVES).
    The runs are unweighted (obstacle None or "model"): a tilted run's log-weights depend on the
    states, hence on the controller, and do not pair (montecarlo.paired_difference)."""
    from . import montecarlo
    controllers = tuple(controllers)
    for c in controllers:
        if c not in HIGHWAY_CONTROLLERS:
            raise ValueError(f"controller={c!r}: one of {sorted(HIGHWAY_CONTROLLERS)}")
    if len(set(controllers)) != len(controllers) or not controllers:
        raise ValueError("controllers: at least one, each once")
    runs = {}
    for c in controllers:
        out = observed_overtake_population(B, steps, sigma_x, sigma_z, observation_seed, sigma_ego, sigma_obs,
                                           disturbance_seed, seed, device, record, obstacle, obstacle_seed, hold,
                                           desc=highway_desc(controller=c))
        runs[c] = dict(zip(("stats", "scene", "record"), out))
    collided = {c: r["stats"][:, abi.ENVS_COLLIDED] for c, r in runs.items()}
    cost = {c: r["stats"][:, abi.ENVS_J] / np.maximum(r["stats"][:, abi.ENVS_SOLVES], 1.0) for c, r in runs.items()}
    pairs = {(a, b): dict(collided=montecarlo.paired_difference(collided[a], collided[b]),
                          cost=montecarlo.paired_difference(cost[a], cost[b]))
             for i, a in enumerate(controllers) for b in controllers[i + 1:]}
    return dict(runs=runs, pairs=pairs)
