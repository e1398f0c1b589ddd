"""The weighted obstacle modes of the device closed loops (bmpc_set_obstacle_proposal) on the GPU.

Shapes: overtake N = 6, NB = 1, m = 3 at 27 egos -- the full enumeration of 3 epochs of 2 steps from one
state, 6 steps -- and quadruped N = 6, NB = 2, m = 2 at 16 egos -- 4 epochs of 2 steps, 8 steps; the
launch paths are selected as tests/loop_common.py does (BMPC_BLOCK_EGOS=0 / BMPC_LDS_RICH for
the one-wave kernels and the fused k_loop, the defaults for the small-batch kernel).  The state is row 0
of the batches whose loops the existing GPU tests hold to solving; every case asserts the kernel the
plan reports and that every solve succeeded.

Yardsticks: bit-for-bit equality between manual stepping, one loop call, a split loop and
BMPC_LOOP_FUSED=0 on the same solver kernels; bmpc/rng.py's inverse CDF and NumPy's logarithms over
bmpc_model_eval's p at the recorded state (tests/obstacle_proposal_common.py, 1e-9 on ENV_LOGW); the sum
of a full enumeration's path probabilities, which is one."""
import numpy as np
import pytest

import obstacle_proposal_common as P
import scene_common as SC
from bmpc import abi, montecarlo
from bmpc.scenarios import highway_desc, merge_desc, quadruped_desc
from loop_common import (PATHS, Loop, assert_all_solved, assert_same_finals, gpu, manual, model_p,  # noqa: F401
                         overtake_case, quad_case, recorded, set_path)

pytestmark = pytest.mark.gpu

SEED, HOLD = 7, 2
EPOCHS = {"overtake": 3, "quadruped": 4}
MODES = ("tilted", "script")
CASES = [("overtake", "blk"), ("overtake", "wave"), ("overtake", "lean"), ("quadruped", "wave"), ("quadruped", "lean")]


def one_state_case(kind, robust=False):
    """m ** epochs egos, all at row 0 of the kind's test batch; their script rows; the step count."""
    m = 3 if kind == "overtake" else 2
    paths = montecarlo.enumerate_scripts(m, EPOCHS[kind])
    B = len(paths)
    case = overtake_case(6, 1, B, robust) if kind == "overtake" else quad_case(B)
    case = dict(case, scene=np.tile(case["scene"][:1], (B, 1)), policies=[case["policies"][0]] * B)
    return case, paths, EPOCHS[kind] * HOLD


def attach(pl, kind, mode, paths, hold=HOLD, ego_base=0, tilt=None):
    """The proposal (the kind's tilt and the enumeration's script), then the sampler in `mode`."""
    pl.set_obstacle_proposal(tilt=P.TILTS[kind] if tilt is None else tilt, script=paths)
    pl.set_obstacle_sampling(mode, seed=SEED, hold=hold, ego_base=ego_base)
    return pl.obstacle_sampling


def run_manual(plan, case, setup, steps):
    """*_env_step_device + solve_device with a host copy per step, setup(plan) before the first: finals,
    scene rows and statuses [B, steps, ...], the kernels taken."""
    cols, kernels, fin = manual(plan, case, steps, setup=lambda d: setup(d.pl))
    return fin, cols["scene"], cols["status"], kernels


def run_loop(plan, case, setup, chunks, record=True):
    """The closed loop in `chunks` calls: finals, the record on the host (or None), the kernels."""
    rec, kernels, fin = recorded(plan, case, chunks, predictions=False, attach=record, setup=lambda d: setup(d.pl))
    return fin, rec, kernels


_MANUAL = {}


def manual_reference(plan, monkeypatch, kind, path, mode, robust=False):
    """Manual stepping of the enumeration case on one launch path, computed once and shared (never
    modified): (finals, scenes, statuses, kernels, case, paths, steps)."""
    key = (kind, path, mode, robust)
    if key not in _MANUAL:
        case, paths, steps = one_state_case(kind, robust)
        if robust:
            set_path(monkeypatch)
        else:
            set_path(monkeypatch, *PATHS[kind, path][:2])
        fin, scenes, sts, km = run_manual(plan, case, lambda pl: attach(pl, kind, mode, paths), steps)
        assert_all_solved(case["desc"], sts)
        assert np.all(scenes[:, -1, abi.ENV_STEPS] == steps)
        _MANUAL[key] = (fin, scenes, sts, km, case, paths, steps)
    return _MANUAL[key]


# ---- 1: every launch path, bit for bit ---------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,path", CASES, ids=[f"{k}-{p}" for k, p in CASES])
def test_paths_agree(gpu, monkeypatch, kind, path, mode):
    """Manual stepping (bmpc_env_step / bmpc_quad_env_step + solve), one loop call, a loop split inside
    an epoch and BMPC_LOOP_FUSED=0 agree bit for bit in scene rows (ENV_LOGW among them), outputs,
    statistics and warm start; the record's scene column is the manual path's."""
    egos, rich, k_step, k_loop = PATHS[kind, path]
    fin, scenes, sts, km, case, paths, steps = manual_reference(gpu, monkeypatch, kind, path, mode)
    assert km <= set(k_step), km
    setup = lambda pl: attach(pl, kind, mode, paths)   # noqa: E731
    set_path(monkeypatch, egos, rich)
    f1, rec, k1 = run_loop(gpu, case, setup, [steps])
    assert set(k1) <= set(k_loop), k1
    assert_same_finals(fin, f1)
    assert np.array_equal(rec.col("scene"), scenes) and np.array_equal(rec.col("status"), sts)
    assert np.array_equal(rec.logw, scenes[:, :, abi.ENV_LOGW]) and np.any(rec.logw != 0.0)
    f2, _, k2 = run_loop(gpu, case, setup, [3, steps - 3], record=False)   # (3: the second call starts inside an epoch)
    assert set(k2) <= set(k_loop) and len(k2) == 2, k2
    assert_same_finals(fin, f2)
    set_path(monkeypatch, egos, rich, fused=0)
    f3, rec3, k3 = run_loop(gpu, case, setup, [steps])
    assert set(k3) <= set(k_step), k3
    assert_same_finals(fin, f3)
    assert np.array_equal(rec3.col("scene"), scenes)


@pytest.mark.parametrize("mode", MODES)
def test_robust_plan_on_its_per_step_path(gpu, monkeypatch, mode):
    """A robustMPC overtake plan (never fused): manual stepping equals bmpc_loop_device bit for bit, and the
    choices and weights follow the model."""
    fin, scenes, sts, km, case, paths, steps = manual_reference(gpu, monkeypatch, "overtake", "robust", mode, robust=True)
    assert km <= {abi.KERNEL_QP_RICH, abi.KERNEL_QP_LEAN}, km
    set_path(monkeypatch)
    f1, rec, k1 = run_loop(gpu, case, lambda pl: attach(pl, "overtake", mode, paths), [steps])
    assert set(k1) == km, k1
    assert_same_finals(fin, f1)
    assert np.array_equal(rec.col("scene"), scenes)
    check_against_model(gpu, "overtake", mode, case, paths, scenes)


# ---- 2: against the model; 3: the enumeration on real solves -------------------------------------------

def check_against_model(plan, kind, mode, case, paths, scenes, ego_base=0, tilt=None):
    """Every epoch's choice and ENV_LOGW increment of recorded rows [B, T, 16] from step 0 follow
    bmpc_model_eval's p at the row's (x, z) -- the state the step's solve saw, the choice's pre-step
    state -- by obstacle_proposal_common.check_weighted (margin 1e-9, at most 1 % left out, 1e-9 on
    ENV_LOGW)."""
    sc = SC.Scene(kind, len(scenes), case=case)
    n = sc.n
    tg = sc.lc_targets(scenes) if kind == "overtake" else None
    smp = abi.make_obstacle_sampling(mode, seed=SEED, hold=HOLD, ego_base=ego_base)
    p_at = lambda r: model_p(plan, sc, None if tg is None else tg[:, r], scenes[:, r, 0:n], scenes[:, r, n:2 * n])  # noqa: E731
    if mode == "script":
        return P.check_weighted(smp, sc.m, scenes, p_at, script=paths)
    return P.check_weighted(smp, sc.m, scenes, p_at, tilt=P.TILTS[kind] if tilt is None else tilt, ego_base=ego_base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_choices_and_weights_follow_the_model(gpu, monkeypatch, kind, mode):
    fin, scenes, sts, km, case, paths, steps = manual_reference(gpu, monkeypatch, kind, "wave", mode)
    compared, logw = check_against_model(gpu, kind, mode, case, paths, scenes)
    print(kind, mode, "compared", compared, "logw", logw.min(), logw.max())
    assert np.abs(logw).max() > 0.1
    if mode == "tilted":
        assert compared >= 0.99 * len(scenes) * EPOCHS[kind]


@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_enumeration_sums_to_one_on_real_solves(gpu, monkeypatch, kind):
    """Script mode over all 27 (16) paths from one state, every step a real solve on the fused rich k_loop:
    the path probabilities exp(ENV_LOGW) sum to 1 within 1e-10, the egos follow their script rows, and the
    record's scene[..., 15] column -- the weight's history, a sum of log-probabilities -- never increases
    and drops at every epoch start."""
    egos, rich, _, k_loop = PATHS[kind, "wave"]
    fin, scenes, sts, km, case, paths, steps = manual_reference(gpu, monkeypatch, kind, "wave", "script")
    set_path(monkeypatch, egos, rich)
    f1, rec, k1 = run_loop(gpu, case, lambda pl: attach(pl, kind, "script", paths), [steps])
    assert set(k1) <= set(k_loop)
    logp = f1["scene"][:, abi.ENV_LOGW]
    total = float(np.exp(logp).sum())
    print(kind, "paths", len(paths), "sum of path probabilities - 1 =", total - 1.0)
    assert abs(total - 1.0) <= 1e-10
    assert np.array_equal(rec.obs_policy[:, ::HOLD], paths)
    hist = rec.col("scene")[..., 15]
    assert np.array_equal(hist, rec.logw) and np.array_equal(hist[:, -1], logp)
    assert np.all(np.diff(hist, axis=1) <= 0.0)
    assert np.all(hist[:, 0] < 0.0) and np.all(np.diff(hist, axis=1)[:, HOLD - 1::HOLD] < 0.0)
    assert np.all(np.diff(hist, axis=1)[:, 0::HOLD] == 0.0)
    # an exact closed-loop expectation over the tree: the collision probability is a probability
    value, mass = montecarlo.exact_expectation(f1["scene"][:, abi.ENV_COLL], logp)
    assert 0.0 <= value <= 1.0 and mass == pytest.approx(1.0, abs=1e-10)


# ---- 4: a tilt of ones; a proposal that is attached but not used --------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_tilt_of_ones_and_unused_proposal(gpu, monkeypatch, kind):
    """Rich k_loop, 27 (16) distinct egos: mode 2 with b == 1 equals mode 1 bit for bit with ENV_LOGW all
    zero; modes 0 and 1 (and no sampler) on a plan with a proposal attached equal the same plan without
    one -- ENV_LOGW, seeded with a sentinel, is never written."""
    egos, rich, _, k_loop = PATHS[kind, "wave"]
    set_path(monkeypatch, egos, rich)
    _, paths, steps = one_state_case(kind)
    B = len(paths)
    case = overtake_case(6, 1, B) if kind == "overtake" else quad_case(B)
    m = 3 if kind == "overtake" else 2

    def model(pl):
        pl.set_obstacle_sampling("model", seed=SEED, hold=HOLD)

    def ones(pl):
        pl.set_obstacle_proposal(tilt=np.ones(m))
        pl.set_obstacle_sampling("tilted", seed=SEED, hold=HOLD)

    ref, rrec, k = run_loop(gpu, case, model, [steps])
    assert set(k) <= set(k_loop)
    assert_all_solved(case["desc"], rrec.col("status"))
    got, grec, _ = run_loop(gpu, case, ones, [steps])
    assert_same_finals(ref, got)
    assert np.array_equal(grec.col("scene"), rrec.col("scene")) and np.all(grec.logw == 0.0)
    assert not np.signbit(grec.logw).any()
    marked = dict(case, scene=case["scene"].copy())
    marked["scene"][:, abi.ENV_LOGW] = -7777.25
    for mode in (None, "argmax", "model"):
        def plain(pl, mode=mode):
            if mode:
                pl.set_obstacle_sampling(mode, seed=SEED, hold=HOLD)

        def unused(pl, mode=mode):
            pl.set_obstacle_proposal(tilt=P.TILTS[kind], script=paths)
            plain(pl)

        a, _, _ = run_loop(gpu, marked, plain, [steps], record=False)
        b, _, _ = run_loop(gpu, marked, unused, [steps], record=False)
        assert_same_finals(a, b)
        assert np.all(b["scene"][:, abi.ENV_LOGW] == -7777.25)
        if mode == "model":
            keep = np.arange(abi.ENV_STRIDE) != abi.ENV_LOGW
            assert np.array_equal(a["scene"][:, keep], ref["scene"][:, keep])


# ---- 5: shard invariance -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_tilted_shard_gets_the_unsharded_rows(gpu, monkeypatch, kind):
    """Mode 2: a 5-ego plan holding egos 3..7 of 8 with ego_base = 3 computes those egos' rows of the
    8-ego plan bit for bit, ENV_LOGW included; the weights follow the model with the global draws."""
    egos, rich, _, k_loop = PATHS[kind, "wave"]
    set_path(monkeypatch, egos, rich)
    case = overtake_case(6, 1, 8) if kind == "overtake" else quad_case(8)

    def tilted(ego_base):
        def setup(pl):
            pl.set_obstacle_proposal(tilt=P.TILTS[kind])
            pl.set_obstacle_sampling("tilted", seed=SEED, hold=HOLD, ego_base=ego_base)
        return setup

    whole, rec, k = run_loop(gpu, case, tilted(0), [6])
    part_case = dict(case, scene=case["scene"][3:8].copy(), policies=case["policies"][3:8])
    part, prec, kp = run_loop(gpu, part_case, tilted(3), [6])
    assert set(k) | set(kp) <= set(k_loop)
    for key in whole:
        if key == "ws":
            for kk in whole[key]:
                assert np.array_equal(whole[key][kk][3:8], part[key][kk]), ("warm start", kk)
        else:
            assert np.array_equal(whole[key][3:8], part[key]), key
    assert np.array_equal(rec.col("scene")[3:8], prec.col("scene")) and np.any(prec.logw != 0.0)
    check_against_model(gpu, kind, "tilted", part_case, None, prec.col("scene"), ego_base=3)


# ---- 6: refusals -------------------------------------------------------------------------------------

def raw_proposal(m, script=None, epochs=0, epoch0=0):
    q = abi.make_obstacle_proposal(m=m)
    q.script, q.script_epochs, q.epoch0 = script, epochs, epoch0
    return q


def test_refusals(gpu):
    import torch
    pl = gpu.BatchPlan(highway_desc(N=6, NB=1), 2)
    refused = lambda msg: pytest.raises(RuntimeError, match=rf"\(-22\).*{msg}")   # noqa: E731
    table = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    # no proposal: modes 2 and 3 are refused, 0 and 1 are not
    for mode in ("tilted", "script"):
        with refused("need a proposal"):
            pl.set_obstacle_sampling(mode)
    pl.set_obstacle_sampling("model")
    # a proposal's own fields
    for j, v in ((0, 0.0), (1, -1.0), (2, float("inf")), (2, float("nan"))):
        q = raw_proposal(3)
        q.tilt[j] = v
        with refused(rf"tilt\[{j}\]"):
            pl.set_obstacle_proposal(q)
    q = raw_proposal(3)
    q.tilt[3] = -1.0                      # (beyond m: not a policy's)
    pl.set_obstacle_proposal(q)
    with refused("script_epochs must not be negative"):
        pl.set_obstacle_proposal(raw_proposal(3, table.data_ptr(), -1))
    with refused("null script"):
        pl.set_obstacle_proposal(raw_proposal(3, None, 2))
    with refused("epoch0"):
        pl.set_obstacle_proposal(raw_proposal(3, table.data_ptr(), 2, -1))
    # a proposal without a script: mode 2 is accepted, mode 3 is not
    pl.set_obstacle_proposal(tilt=(1, 2, 3))
    pl.set_obstacle_sampling("tilted")
    with refused("needs a proposal with a script"):
        pl.set_obstacle_sampling("script")
    with refused("sampler's mode needs the proposal"):
        pl.set_obstacle_proposal(None)
    pl.set_obstacle_proposal(raw_proposal(3, table.data_ptr(), 2))
    pl.set_obstacle_sampling("script", hold=2)
    with refused("sampler's mode needs the proposal"):
        pl.set_obstacle_proposal(None)
    with refused("needs a proposal with a script"):
        pl.set_obstacle_proposal(raw_proposal(3))
    for field, value, msg in (("mode", 7, "mode"), ("mode", -1, "mode"), ("mode", 4, "mode")):
        s = abi.make_obstacle_sampling("script")
        setattr(s, field, value)
        with refused(msg):
            pl.set_obstacle_sampling(s)
    pl.set_obstacle_sampling(None)
    pl.set_obstacle_proposal(None)         # detaching is allowed once no mode needs it
    # the plan kinds mode 1 refuses
    merge = gpu.BatchPlan(merge_desc(N=6), 2)
    with refused("merge"):
        merge.set_obstacle_proposal(raw_proposal(2))
    merge.set_obstacle_proposal(None)
    xf = highway_desc(N=6, NB=1)
    xf.flags = abi.PLAN_TRANSFORM
    with refused("TRANSFORM"):
        gpu.BatchPlan(xf, 2).set_obstacle_proposal(raw_proposal(3))
    cvar_quad = quadruped_desc(N=6, NB=1)
    cvar_quad.controller = abi.CTRL_CVAR
    with refused("OSQP-class"):
        gpu.BatchPlan(cvar_quad, 2).set_obstacle_proposal(raw_proposal(2))


@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_script_too_short_is_refused_on_the_host(gpu, monkeypatch, kind):
    """Script columns 0..1 are epochs 1..2 of hold 2, steps 2..5: a loop or a single step that needs
    another epoch returns -22 before anything is enqueued -- scene, statistics and outputs keep their
    bits -- and the covered steps run."""
    set_path(monkeypatch)
    case = overtake_case(6, 1, 3) if kind == "overtake" else quad_case(3)
    d = Loop(gpu, case)
    d.pl.set_obstacle_proposal(script=np.zeros((3, 2), np.int64), epoch0=1)
    d.pl.set_obstacle_sampling("script", hold=2)
    before = d.finals()
    entry = "bmpc_loop_device" if kind == "overtake" else "bmpc_quad_loop_device"
    step = "bmpc_env_step" if kind == "overtake" else "bmpc_quad_env_step"
    for t, n in ((0, 1), (1, 2), (2, 5), (5, 2), (6, 1)):
        d.t = t
        with pytest.raises(RuntimeError, match=rf"{entry} failed \(-22\).*script covers epochs 1\.\.2"):
            d.loop(n)
    for t in (0, 1, 6, 40):
        d.t = t
        with pytest.raises(RuntimeError, match=rf"{step} failed \(-22\).*script covers epochs 1\.\.2"):
            d.env_step()
    assert_same_finals(before, d.finals())
    d.pl.set_obstacle_sampling("model")          # (steps 0 and 1 under another mode)
    d.t = 0
    d.loop(2)
    d.pl.set_obstacle_sampling("script", hold=2)
    d.loop(4)
    after = d.finals()
    assert np.all(after["scene"][:, abi.ENV_STEPS] == 6) and np.all(after["scene"][:, abi.ENV_LOGW] < 0.0)
    assert np.all(after["scene"][:, abi.ENV_OBSPOL] == 0)


# ---- the population entries ----------------------------------------------------------------------------

def test_weighted_and_enumerated_populations(gpu, monkeypatch):
    from bmpc import scenarios
    set_path(monkeypatch)
    descs = {"overtake": highway_desc(N=6, NB=1), "quadruped": quadruped_desc(N=6, NB=2)}
    for kind, fn in (("overtake", scenarios.weighted_overtake_population),
                     ("quadruped", scenarios.weighted_quadruped_population)):
        stats, scene, logw, rec = fn(8, 4, record=True, obstacle_seed=SEED, hold=2, desc=descs[kind], tilt=P.TILTS[kind])
        assert np.array_equal(logw, scene[:, abi.ENV_LOGW]) and np.array_equal(rec.logw[:, -1], logw)
        assert np.any(logw != 0.0) and np.all(stats[:, abi.ENVS_SOLVES] == 3)
        # two shards of the population: their rows, and the estimate from their reduced terms
        parts = [fn(hi - lo, 4, obstacle_seed=SEED, hold=2, desc=descs[kind], tilt=P.TILTS[kind], ego_base=lo,
                    population=8) for lo, hi in ((0, 3), (3, 8))]
        assert np.array_equal(np.concatenate([p[1] for p in parts]), scene)
        f = scene[:, abi.ENV_OBSPOL]
        terms = sum(montecarlo.reduce_terms(p[1][:, abi.ENV_OBSPOL], p[2]) for p in parts)
        np.testing.assert_allclose(montecarlo.estimate_from_terms(terms), montecarlo.estimate(f, logw), rtol=1e-12)
    x0, z0 = [0, 1.8, 20, 0], [5, 5.4, 20, 0]
    stats, scene, logp, script, rec = scenarios.enumerated_overtake_population(x0, z0, 2, 2, record=True,
                                                                               desc=descs["overtake"])
    assert script.shape == (9, 2) and np.array_equal(rec.obs_policy[:, ::2], script)
    assert abs(np.exp(logp).sum() - 1.0) <= 1e-10 and np.array_equal(logp, scene[:, abi.ENV_LOGW])
    stats, scene, logp, script = scenarios.enumerated_quadruped_population([0, 1.8, 0], [2.5, 2.5, -np.pi / 2],
                                                                           [5, -3, 0], 3, 1, desc=descs["quadruped"])
    assert script.shape == (8, 3) and abs(np.exp(logp).sum() - 1.0) <= 1e-10
