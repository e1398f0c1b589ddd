"""The actuation disturbance of the device closed loops (bmpc_set_disturbance) on the GPU.

Two yardsticks, both bit for bit.  The launch paths against each other: manual stepping, one loop
call, a loop split over two calls and the per-step path of a loop call.  And NumPy: an undisturbed
"twin" plan stepped by hand whose uPred[0] and obstacle-input slot are overwritten, before every scene
step, with nominal + sigma * bmpc.rng.disturbance(...) -- the scene step is the only reader of uPred
between two solves, and it rewrites the slot, so the twin computes the disturbed plan's bits if and
only if the device applies exactly NumPy's numbers.

Every case asserts that all its solves succeeded (CVaR: 0 or 10, OSQP-class: 1) with the issue's
suggested sigmas, highway (0.3, 0.01) / (0.5, 0.02), quadruped (0.02, 0.01, 0.05) for both vehicles.
The scenes, plans and helpers are those of tests/loop_common.py; 6 steps everywhere."""
import numpy as np
import pytest

import disturbance_common as D
import scene_common as SC
from bmpc import abi
from bmpc.scenarios import highway_desc, merge_desc, quadruped_desc
from loop_common import (BLK, COLUMNS, Loop, assert_record_equals, assert_same_finals, gpu, merge_case,  # noqa: F401
                         overtake_case, quad_case, recorded, set_path)

pytestmark = pytest.mark.gpu

STEPS = 6
# name: (scene, egos, BMPC_BLOCK_EGOS, BMPC_LDS_RICH, the per-step solver kernels, the loop's kernels)
PATHS = {
    "overtake_wave": ("overtake", 65, 0, 1, (abi.KERNEL_IPM_RICH,), (abi.KERNEL_LOOP_RICH,)),
    "overtake_lean": ("overtake", 65, 0, 0, (abi.KERNEL_IPM_LEAN,), (abi.KERNEL_LOOP_LEAN,)),
    "overtake_blk": ("overtake", 3, None, None, BLK, BLK),
    "merge_rich": ("merge", 65, 0, 1, (abi.KERNEL_IPM_RICH,), (abi.KERNEL_LOOP_RICH,)),
    "merge_lean": ("merge", 65, 0, 0, (abi.KERNEL_IPM_LEAN,), (abi.KERNEL_LOOP_LEAN,)),
    "quadruped_rich": ("quadruped", 65, None, 1, (abi.KERNEL_QP_RICH,), (abi.KERNEL_LOOP_RICH,)),
    "quadruped_lean": ("quadruped", 65, None, 0, (abi.KERNEL_QP_LEAN,), (abi.KERNEL_LOOP_LEAN,)),
    "quadruped_one": ("quadruped", 1, None, 1, (abi.KERNEL_QP_RICH,), (abi.KERNEL_LOOP_RICH,)),
}
FUSED = {"overtake": "overtake_wave", "merge": "merge_rich", "quadruped": "quadruped_rich"}
TILT = dict(tilt=(1.0, 4.0, 0.25), seed=5, hold=2)


def case_of(kind, B):
    return overtake_case(6, 1, B) if kind == "overtake" else merge_case(B) if kind == "merge" else quad_case(B)


def rows_of(case, rows):
    return dict(case, scene=case["scene"][rows], policies=case["policies"][rows])


def attach(d, dist=None, tilt=None):
    if tilt is not None:
        d.pl.set_obstacle_proposal(tilt=tilt["tilt"])
        d.pl.set_obstacle_sampling("tilted", seed=tilt["seed"], hold=tilt["hold"])
    if dist is not None:
        d.pl.set_disturbance(dist)
    return d


def perturb_on_device(d, dist):
    """The twin's inputs of the next scene step (t = d.t >= 1): uPred[0] and the obstacle-input slot
    become what the disturbed plan applies, formed on the host in NumPy and copied back unchanged."""
    torch = d.torch
    lo, w = D.slot(d.kind)
    up, scene = d.host("up", "scene")
    u, uo = D.perturbed(d.kind, dist, d.t - 1, up[:, 0], scene[:, lo:lo + w], np.arange(d.B))
    d.up[:, 0] = torch.tensor(u, dtype=torch.float64, device=d.up.device)
    d.scene[:, lo:lo + w] = torch.tensor(uo, dtype=torch.float64, device=d.up.device)
    torch.cuda.synchronize()


def manual(plan, case, dist=None, twin=None, tilt=None, steps=STEPS):
    """loop_common.manual with a disturbance attached (`dist`) or applied from outside to an
    undisturbed plan (`twin`): the columns a record must hold, the kernels taken, the final state."""
    d = attach(Loop(plan, case), dist, tilt)
    rows = {k: [] for k in COLUMNS}
    kernels = set()
    for t in range(steps):
        if twin is not None and t > 0:
            perturb_on_device(d, twin)
        d.env_step()
        d.solve()
        scene, xref, up, J, st, it, xpred, bw = d.host("scene", "xref", "up", "J", "st", "it", "xpred", "bw")
        kernels.add(d.pl.last_kernel())
        for k, v in zip(COLUMNS, (scene, xref, up[:, 0], J, st, it, up, xpred, d.pl.tree()["zbar"],
                                  bw[:, :d.pl.nbranch - 1])):
            rows[k].append(v)
    return {k: np.stack(v, axis=1) for k, v in rows.items()}, kernels, d.finals()


def looped(plan, case, chunks, dist=None, tilt=None, detach=False):
    """The loop in `chunks` calls with a recorder: the record, the kernels reported, the final state."""
    def setup(d):
        attach(d, dist, tilt)
        if detach:
            d.pl.set_disturbance(None)
    return recorded(plan, case, chunks, setup=setup)


def assert_all_solved(case, cols):
    st = cols["status"]
    print(f"{case['kind']} B {st.shape[0]}: statuses {np.unique(st, return_counts=True)}, iterations "
          f"{cols['iters'].min()}-{cols['iters'].max()}")
    if case["desc"].controller == abi.CTRL_CVAR:
        assert np.all((st == 0) | (st == 10)), np.unique(st, return_counts=True)
    else:
        assert np.all(st == 1), np.unique(st, return_counts=True)
    assert np.all(np.isfinite(cols["J"])) and np.all(np.isfinite(cols["xpred"]))


def assert_same_cols(a, b):
    for k in COLUMNS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, np.argwhere(a[k] != b[k])[:4])


_REF = {}


def reference(plan, monkeypatch, name):
    """The disturbed manual path of a PATHS entry, computed once and shared (never modified)."""
    kind, B, egos, rich, k_step, _ = PATHS[name]
    set_path(monkeypatch, egos, rich)
    if name not in _REF:
        case = case_of(kind, B)
        _REF[name] = (case,) + manual(plan, case, dist=D.make(kind))
        assert_all_solved(case, _REF[name][1])
        assert _REF[name][2] <= set(k_step), _REF[name][2]
    return _REF[name]


# ---- 1: the scene kernels ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_scene_kernels_equal_perturbed_inputs(gpu, kind):
    """k_env / k_env_merge / k_env_quad teacher-forced over 6 steps at 65 egos: the disturbed plan
    equals an undisturbed plan whose upred[:, 0] and obstacle-input slots are perturbed with NumPy's
    numbers before each step, bit for bit (merge: the transform slots too)."""
    import torch
    case, dist = case_of(kind, 65), D.make(kind)
    script = SC.Scene(kind, 65).script
    a, b, c = attach(Loop(gpu, case), dist), Loop(gpu, case), Loop(gpu, case)
    moved = False
    for t in range(STEPS):
        for d in (a, b, c):
            if t > 0:
                d.up[:, 0] = torch.tensor(script(t), dtype=torch.float64, device=d.up.device)
                torch.cuda.synchronize()
        if t > 0:
            perturb_on_device(b, dist)
        for d in (a, b, c):
            d.env_step()
        got, want, plain = (d.host("scene", "x", "z", "xref") for d in (a, b, c))
        for k, g, w in zip(("scene", "x", "z", "xref"), got, want):
            assert np.array_equal(g, w), (t, k, np.argwhere(g != w)[:4])
        if kind == "merge":
            ta, tb = a.pl.get_transform(), b.pl.get_transform()
            for k in ta:
                assert np.array_equal(ta[k], tb[k]), (t, k)
        moved = moved or not np.array_equal(got[1], plain[1])
        assert t > 0 or np.array_equal(got[0], plain[0])
    assert moved
    lo, w = D.slot(kind)
    assert np.array_equal(got[0][:, abi.ENV_STEPS], np.full(65, float(STEPS))) and np.any(got[0][:, lo:lo + w] != 0)


# ---- 2: the launch paths -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PATHS))
def test_launch_paths_agree_and_equal_the_twin(gpu, monkeypatch, name):
    """Manual stepping, one loop call, a loop split 3 + 3 and BMPC_LOOP_FUSED=0 agree in scene, outputs,
    statistics, warm start and record, on the kernels the case names; and equal a manual loop on an
    undisturbed twin plan fed NumPy-perturbed inputs."""
    kind, B, egos, rich, k_step, k_loop = PATHS[name]
    case, ref, _, fin = reference(gpu, monkeypatch, name)
    dist = D.make(kind)
    rec, k1, f1 = looped(gpu, case, [STEPS], dist)
    assert set(k1) <= set(k_loop), k1
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    rec, k2, f2 = looped(gpu, case, [3, 3], dist)
    assert set(k2) <= set(k_loop) and len(k2) == 2, k2
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f2)
    set_path(monkeypatch, egos, rich, fused=0)
    rec, k3, f3 = looped(gpu, case, [STEPS], dist)
    assert set(k3) <= set(k_step), k3
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f3)
    set_path(monkeypatch, egos, rich)
    twin, kt, ft = manual(gpu, case, twin=dist)
    assert kt <= set(k_step), kt
    assert_same_cols(ref, twin)
    assert_same_finals(fin, ft)
    # the record's u column and the scene's obstacle-input slot keep the nominal inputs
    assert np.array_equal(rec.col("u"), rec.col("upred")[:, :, 0])


def test_tilted_sampler_rides_along(gpu, monkeypatch):
    """Overtake, 65 egos, the tilted sampler (hold 2) attached beside the disturbance: the paths agree,
    and the twin -- the same sampler, NumPy-perturbed inputs -- has the same choices and ENV_LOGW."""
    kind, B, egos, rich, k_step, k_loop = PATHS["overtake_wave"]
    set_path(monkeypatch, egos, rich)
    case, dist = case_of(kind, B), D.make(kind)
    ref, kr, fin = manual(gpu, case, dist=dist, tilt=TILT)
    assert_all_solved(case, ref)
    assert kr <= set(k_step)
    rec, k1, f1 = looped(gpu, case, [3, 3], dist, tilt=TILT)
    assert set(k1) <= set(k_loop)
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    twin, _, ft = manual(gpu, case, twin=dist, tilt=TILT)
    assert_same_cols(ref, twin)
    assert_same_finals(fin, ft)
    logw = ref["scene"][:, :, abi.ENV_LOGW]
    assert np.array_equal(logw, twin["scene"][:, :, abi.ENV_LOGW]) and np.any(logw[:, -1] != 0)
    assert len(np.unique(ref["scene"][:, :, abi.ENV_OBSPOL])) > 1


# ---- 3: off is the parent ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_off_computes_the_undisturbed_bits(gpu, monkeypatch, kind):
    """Sigma = 0, law NONE with non-zero sigmas, and attach-then-detach (with and, on the overtake
    scene, beside an unused proposal that keeps the options block alive) give the bits of a plan that
    never had a disturbance, fused and per step; a non-zero sigma does not."""
    _, B, egos, rich, k_step, k_loop = PATHS[FUSED[kind]]
    case = case_of(kind, B)
    zero = (0.0,) * D.slot(kind)[1]
    for fused in (None, 0):
        set_path(monkeypatch, egos, rich, fused)
        plain, k0, f0 = looped(gpu, case, [STEPS])
        assert set(k0) <= set(k_loop if fused is None else k_step), k0
        variants = [dict(dist=D.make(kind, sigma_ego=zero, sigma_obs=zero)),
                    dict(dist=D.make(kind, law=abi.DISTURB_NONE, seed=99, ego_base=5)),
                    dict(dist=D.make(kind), detach=True)]
        for v in variants if fused is None else variants[1:2]:
            rec, _, f = looped(gpu, case, [STEPS], **v)
            assert_same_finals(f0, f)
            for k in COLUMNS:
                assert np.array_equal(rec.col(k), plain.col(k)), k
    d = Loop(gpu, case)   # ... and with a proposal attached, which keeps the block's pointer in use
    if kind == "overtake":
        d.pl.set_obstacle_proposal(tilt=TILT["tilt"])
        d.pl.set_disturbance(D.make(kind))
        d.pl.set_disturbance(None)
        d.loop(STEPS)
        assert np.array_equal(d.host("scene")[0], f0["scene"])
    rec, _, f = looped(gpu, case, [STEPS], D.make(kind))
    assert not np.array_equal(f["x"], f0["x"]) and not np.array_equal(f["z"], f0["z"])


# ---- 4: channel separation ---------------------------------------------------------------------------

def test_merge_channels_are_separate(gpu, monkeypatch):
    """The merge scene with sigma_ego only: the obstacle's trajectory is the undisturbed run's bit for
    bit (it never reacts to the ego), the ego's is not; and the other way round with sigma_obs only."""
    _, B, egos, rich, _, _ = PATHS["merge_rich"]
    set_path(monkeypatch, egos, rich)
    case = case_of("merge", B)
    plain, _, _ = looped(gpu, case, [STEPS])
    ego_only, _, _ = looped(gpu, case, [STEPS], D.make("merge", sigma_obs=(0.0, 0.0)))
    assert np.array_equal(ego_only.z, plain.z) and not np.array_equal(ego_only.x, plain.x)
    assert np.array_equal(ego_only.x[:, 0], plain.x[:, 0])      # (step 0 has no Euler step)
    assert not np.array_equal(ego_only.x[:, 1], plain.x[:, 1])
    obs_only, _, _ = looped(gpu, case, [STEPS], D.make("merge", sigma_ego=(0.0, 0.0)))
    assert not np.array_equal(obs_only.z, plain.z) and np.array_equal(obs_only.z[:, 0], plain.z[:, 0])


# ---- 5, 6: shards and seeds ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_shard_and_seed(gpu, monkeypatch, kind):
    """Egos 40..59 in a plan of their own with ego_base = 40 take the rows they have in the 65-ego run;
    with ego_base = 0 they do not.  The same seed twice is identical (the launch-path test ran it
    several times); another seed differs."""
    name = FUSED[kind]
    _, B, egos, rich, _, k_loop = PATHS[name]
    case, ref, _, fin = reference(gpu, monkeypatch, name)
    part = rows_of(case, slice(40, 60))
    rec, k, f = looped(gpu, part, [STEPS], D.make(kind, ego_base=40))
    assert set(k) <= set(k_loop)
    for c in COLUMNS:
        assert np.array_equal(rec.col(c), ref[c][40:60]), c
    for c in ("scene", "up", "J", "st", "it", "stats", "x", "z", "xref"):
        assert np.array_equal(f[c], fin[c][40:60]), c
    _, _, f0 = looped(gpu, part, [STEPS], D.make(kind))
    assert not np.array_equal(f0["x"], fin["x"][40:60])
    _, _, f7 = looped(gpu, case, [STEPS], D.make(kind, seed=D.SEED))
    assert_same_finals(fin, f7)
    _, _, f8 = looped(gpu, case, [STEPS], D.make(kind, seed=D.SEED + 1))
    assert not np.array_equal(f8["x"], fin["x"]) and not np.array_equal(f8["z"], fin["z"])


# ---- 7: clones ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_clones_diverge_by_themselves(gpu, monkeypatch, kind):
    """3 steps, then every ego becomes a copy of ego 0 (gather_egos with a broadcast), then 2 more
    steps: with sigma > 0 the clones leave their ancestor -- a draw is addressed by slot --, with
    sigma = 0 they stay its copies."""
    import torch
    _, B, egos, rich, _, _ = PATHS[FUSED[kind]]
    set_path(monkeypatch, egos, rich)
    case = rows_of(case_of(kind, B), slice(0, 8))
    zero = (0.0,) * D.slot(kind)[1]
    n = case["desc"].n
    for dist, diverge in ((D.make(kind), True), (D.make(kind, sigma_ego=zero, sigma_obs=zero), False)):
        d = attach(Loop(gpu, case), dist)
        d.loop(3)
        anc = torch.zeros(8, dtype=torch.int32, device=d.up.device)
        torch.cuda.synchronize()
        d.pl.gather_egos(anc, dict(scene=d.scene, upred=d.up, x=d.x, z=d.z, xref=d.xref, J=d.J, status=d.st, iters=d.it,
                                   stats=d.stats), d.stream.cuda_stream)
        scene = d.host("scene")[0]
        assert np.array_equal(scene, np.tile(scene[:1], (8, 1)))
        d.loop(2)
        scene, st = d.host("scene", "st")
        same = [np.array_equal(scene[j], scene[0]) for j in range(1, 8)]
        assert (not any(same)) if diverge else all(same), same
        if diverge:
            assert len(np.unique(scene[:, :n], axis=0)) == 8 and len(np.unique(scene[:, n:2 * n], axis=0)) == 8
        assert np.all(st >= 0) if case["desc"].controller == abi.CTRL_CVAR else np.all(st == 1)


# ---- 8: refusals and the population entries -------------------------------------------------------------

def test_refusals(gpu):
    pl = gpu.BatchPlan(highway_desc(N=6, NB=1), 2)
    pl.set_disturbance((0.3, 0.01), (0.5, 0.02), seed=2 ** 64 - 1, ego_base=2 ** 40)
    pl.set_disturbance(None)
    pl.set_disturbance(None)                      # detaching is always allowed

    def struct(**fields):
        s = abi.make_disturbance((0.3, 0.01), (0.5, 0.02))
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    for fields, msg in ((dict(law=2), "law"), (dict(law=-1), "law"), (dict(ego_base=-1), "ego_base"),
                        (dict(sigma_ego=(0, -0.1)), r"sigma_ego\[0\]"), (dict(sigma_obs=(1, float("nan"))), r"sigma_obs\[1\]"),
                        (dict(sigma_obs=(0, float("inf"))), r"sigma_obs\[0\]"),
                        (dict(sigma_ego=(2, 0.1)), r"sigma_ego\[2\].*2 components"),
                        (dict(sigma_obs=(3, 0.1)), r"sigma_obs\[3\]")):
        with pytest.raises(RuntimeError, match=rf"\(-22\).*{msg}"):
            pl.set_disturbance(struct(**fields))
    q = quadruped_desc(N=6)
    assert gpu.BatchPlan(q, 2).set_disturbance((0.02, 0.01, 0.05)) is None      # three components there
    q.controller = abi.CTRL_CVAR
    with pytest.raises(RuntimeError, match=r"\(-22\).*quadruped scene"):
        gpu.BatchPlan(q, 2).set_disturbance((0.02,))
    m = merge_desc(N=6)
    assert gpu.BatchPlan(m, 2).set_disturbance((0.3,)) is None
    xf = highway_desc(N=6, NB=1)
    xf.flags = abi.PLAN_TRANSFORM
    assert gpu.BatchPlan(xf, 2).set_disturbance((0.3,)) is None    # bmpc_env_step takes such a plan


def test_population_entries(gpu, monkeypatch):
    """The three disturbed_*_population entries: without sigmas they are the undisturbed entries, with
    them they differ and are reproducible, and a shard of a population takes its rows."""
    from bmpc import scenarios as sc
    set_path(monkeypatch)
    small = dict(overtake=highway_desc(N=6, NB=1), quadruped=quadruped_desc(N=6))
    for kind, fn, base in (("overtake", sc.disturbed_overtake_population, sc.sampled_overtake_population),
                           ("quadruped", sc.disturbed_quadruped_population, sc.sampled_quadruped_population)):
        se, so = D.SIGMAS[kind]
        plain = base(6, 4, obstacle=None, desc=small[kind])
        off = fn(6, 4, desc=small[kind])
        assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
        stats, scene, rec = fn(6, 4, se, so, disturbance_seed=3, record=True, obstacle="model", obstacle_seed=2, hold=2,
                               desc=small[kind])
        assert stats.shape == (6, abi.ENV_NSTAT) and not np.array_equal(scene, plain[1])
        assert np.array_equal(rec.col("scene")[:, -1], scene) and np.all(stats[:, abi.ENVS_SOLVES] == 3)
        again = fn(6, 4, se, so, disturbance_seed=3, obstacle="model", obstacle_seed=2, hold=2, desc=small[kind])
        assert np.array_equal(again[1], scene)
        shard = fn(3, 4, se, so, disturbance_seed=3, obstacle="model", obstacle_seed=2, hold=2, ego_base=2, population=6,
                   desc=small[kind])
        assert np.array_equal(shard[1], scene[2:5]) and np.array_equal(shard[0], stats[2:5])
    se, so = D.SIGMAS["merge"]
    plain = sc.merge_population(4, 3)
    off = sc.disturbed_merge_population(4, 3)
    assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
    stats, scene = sc.disturbed_merge_population(4, 3, se, so, disturbance_seed=3)
    assert not np.array_equal(scene, plain[1]) and np.all(stats[:, abi.ENVS_SOLVES] == 2)
    shard = sc.disturbed_merge_population(2, 3, se, so, disturbance_seed=3, ego_base=1, population=4)
    assert np.array_equal(shard[1], scene[1:3]) and np.array_equal(shard[0], stats[1:3])
