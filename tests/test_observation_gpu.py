"""The observation noise of the device closed loops (bmpc_set_observation) on the GPU.

Two yardsticks, both bit for bit.  The launch paths against each other: manual stepping, one loop
call, a loop split over two calls and the per-step path of a loop call.  And NumPy: an unobserved
"twin" plan stepped by hand whose d_x / d_z are overwritten, between every scene step and its solve,
with the scene row's true states + sigma * bmpc.rng.observation(...) -- the solve is the only reader of
d_x / d_z and the next scene step rewrites them from the row, so the twin computes the observed plan's
bits if and only if the device applies exactly NumPy's numbers.

Every case asserts that all its solves succeeded (CVaR: 0 or 10, OSQP-class: 1) with the issue's
suggested sigmas (tests/observation_common.py SIGMAS).  The scenes, plans and helpers are those of
tests/loop_common.py at tests/test_disturbance_gpu.py's shapes; 6 steps everywhere."""
import numpy as np
import pytest

import disturbance_common as D
import loop_common as LC
import observation_common as O
import scene_common as SC
from bmpc import abi
from bmpc.scenarios import highway_desc, merge_desc, quadruped_desc
from loop_common import (BLK, COLUMNS, Loop, assert_record_equals, assert_same_finals, gpu, merge_case,  # noqa: F401
                         overtake_case, quad_case, recorded, set_path)

pytestmark = pytest.mark.gpu

STEPS = 6
QP = (abi.KERNEL_QP_RICH, abi.KERNEL_QP_LEAN)
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
    "overtake_robust": ("overtake", 65, None, None, QP, QP),          # a robustMPC plan is never fused
}
FUSED = {"overtake": "overtake_wave", "merge": "merge_rich", "quadruped": "quadruped_rich"}
TILT = dict(tilt=(1.0, 4.0, 0.25), seed=5, hold=2)


def case_of(kind, B, robust=False):
    if kind == "overtake":
        return overtake_case(6, 1, B, robust=robust)
    return merge_case(B) if kind == "merge" else quad_case(B)


def rows_of(case, rows):
    return dict(case, scene=case["scene"][rows], policies=case["policies"][rows])


def attach(d, obs=None, tilt=None, dist=None):
    if tilt is not None:
        d.pl.set_obstacle_proposal(tilt=tilt["tilt"])
        d.pl.set_obstacle_sampling("tilted", seed=tilt["seed"], hold=tilt["hold"])
    if dist is not None:
        d.pl.set_disturbance(dist)
    if obs is not None:
        d.pl.set_observation(obs)
    return d


def observe_on_device(d, obs):
    """The twin's solve inputs after the scene step of t = d.t - 1: d_x / d_z become what the observed
    plan's scene step wrote, formed on the host in NumPy from the scene row and copied back unchanged."""
    torch = d.torch
    scene = d.host("scene")[0]
    x, z = O.observed_rows(d.kind, obs, d.t - 1, scene)
    d.x[:] = torch.tensor(x, dtype=torch.float64, device=d.x.device)
    d.z[:] = torch.tensor(z, dtype=torch.float64, device=d.x.device)
    torch.cuda.synchronize()


def manual(plan, case, obs=None, twin=None, tilt=None, dist=None, steps=STEPS):
    """loop_common.manual with an observation model attached (`obs`) or applied from outside to an
    unobserved plan (`twin`, between the scene step and the solve): the columns a record must hold, the
    kernels taken, the final state."""
    def setup(d):
        attach(d, obs, tilt, dist)
        if twin is not None:
            solve = d.solve
            d.solve = lambda: (observe_on_device(d, twin), solve())
    return LC.manual(plan, case, steps, setup=setup)


def looped(plan, case, chunks, obs=None, tilt=None, dist=None, detach=False):
    """The loop in `chunks` calls with a recorder: the record, the kernels reported, the final state."""
    def setup(d):
        attach(d, obs, tilt, dist)
        if detach:
            d.pl.set_observation(None)
    return recorded(plan, case, chunks, setup=setup)


def assert_all_solved(case, status, what=""):
    st = np.asarray(status)
    print(f"{case['kind']} B {len(case['scene'])} {what}: statuses {np.unique(st, return_counts=True)}")
    LC.assert_all_solved(case["desc"], st)


def assert_same_cols(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, np.argwhere(a[k] != b[k])[:4])


_REF = {}


def reference(plan, monkeypatch, name):
    """The observed manual path of a PATHS entry, computed once and shared (never modified)."""
    kind, B, egos, rich, k_step, _ = PATHS[name]
    set_path(monkeypatch, egos, rich)
    if name not in _REF:
        case = case_of(kind, B, robust=name.endswith("robust"))
        _REF[name] = (case,) + manual(plan, case, obs=O.make(kind))
        assert_all_solved(case, _REF[name][1]["status"], name)
        assert np.all(np.isfinite(_REF[name][1]["J"])) and np.all(np.isfinite(_REF[name][1]["xpred"]))
        assert _REF[name][2] <= set(k_step), _REF[name][2]
    return _REF[name]


# ---- 1: the scene kernels ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_scene_kernels_equal_plain_plus_numpy_noise(gpu, kind):
    """k_env / k_env_merge / k_env_quad teacher-forced over 6 steps at 65 egos: the observed plan's d_x /
    d_z equal a plain plan's plus NumPy's noise bit for bit; the scene, x_ref and, on the merge, the
    transform slots equal the plain plan's."""
    import torch
    case, obs = case_of(kind, 65), O.make(kind)
    script = SC.Scene(kind, 65).script
    a, c = attach(Loop(gpu, case), obs), Loop(gpu, case)
    for t in range(STEPS):
        for d in (a, c):
            if t > 0:
                d.up[:, 0] = torch.tensor(script(t), dtype=torch.float64, device=d.up.device)
                torch.cuda.synchronize()
            d.env_step()
        got, plain = (dict(zip(("scene", "x", "z", "xref"), d.host("scene", "x", "z", "xref"))) for d in (a, c))
        assert np.array_equal(got["scene"], plain["scene"]) and np.array_equal(got["xref"], plain["xref"]), t
        x, z = O.observed(kind, obs, t, plain["x"], plain["z"], np.arange(65))
        assert np.array_equal(got["x"], x), (t, np.argwhere(got["x"] != x)[:4])
        assert np.array_equal(got["z"], z), (t, np.argwhere(got["z"] != z)[:4])
        assert np.all(got["x"] != plain["x"]) and np.all(got["z"] != plain["z"])
        xr, zr = O.observed_rows(kind, obs, t, got["scene"])      # reproducible from the row
        assert np.array_equal(got["x"], xr) and np.array_equal(got["z"], zr)
        if kind == "merge":
            ta, tc = a.pl.get_transform(), c.pl.get_transform()
            for k in ta:
                assert np.array_equal(ta[k], tc[k]), (t, k)
    assert np.array_equal(got["scene"][:, abi.ENV_STEPS], np.full(65, float(STEPS)))


# ---- 2: the launch paths -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PATHS))
def test_launch_paths_agree_and_equal_the_twin(gpu, monkeypatch, name):
    """Manual stepping, one loop call, a loop split 3 + 3 and BMPC_LOOP_FUSED=0 agree in scene, outputs,
    statistics, warm start and record, on the kernels the case names; and equal a manual loop on an
    unobserved twin plan whose d_x / d_z get NumPy's numbers between the scene step and the solve."""
    kind, B, egos, rich, k_step, k_loop = PATHS[name]
    case, ref, _, fin = reference(gpu, monkeypatch, name)
    obs = O.make(kind)
    rec, k1, f1 = looped(gpu, case, [STEPS], obs)
    assert set(k1) <= set(k_loop), k1
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    rec, k2, f2 = looped(gpu, case, [3, 3], obs)
    assert set(k2) <= set(k_loop) and len(k2) == 2, k2
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f2)
    set_path(monkeypatch, egos, rich, fused=0)
    rec, k3, f3 = looped(gpu, case, [STEPS], obs)
    assert set(k3) <= set(k_step), k3
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f3)
    set_path(monkeypatch, egos, rich)
    twin, kt, ft = manual(gpu, case, twin=obs)
    assert kt <= set(k_step), kt
    assert_same_cols(ref, twin)
    assert_same_finals(fin, ft)
    # the loop's d_x / d_z hold the observed vectors of the last step; the record keeps the truth
    x, z = O.observed_rows(kind, obs, STEPS - 1, fin["scene"])
    assert np.array_equal(fin["x"], x) and np.array_equal(fin["z"], z)
    assert np.array_equal(rec.col("scene")[:, -1], fin["scene"])
    plain, _, f0 = looped(gpu, case, [STEPS])
    assert not np.array_equal(f0["scene"], fin["scene"]) and not np.array_equal(f0["up"], fin["up"])


# ---- 3: the three options at once ----------------------------------------------------------------------

def test_sampler_and_disturbance_ride_along(gpu, monkeypatch):
    """Overtake, 65 egos, the tilted sampler (hold 2), the disturbance and the observation model
    together: the paths agree, and the twin -- the same sampler and disturbance, the observation from
    NumPy -- has the same choices and the same ENV_LOGW."""
    kind, B, egos, rich, k_step, k_loop = PATHS["overtake_wave"]
    set_path(monkeypatch, egos, rich)
    case, obs, dist = case_of(kind, B), O.make(kind), D.make(kind)
    ref, kr, fin = manual(gpu, case, obs=obs, tilt=TILT, dist=dist)
    assert_all_solved(case, ref["status"], "three options")
    assert kr <= set(k_step)
    rec, k1, f1 = looped(gpu, case, [3, 3], obs, tilt=TILT, dist=dist)
    assert set(k1) <= set(k_loop)
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    set_path(monkeypatch, egos, rich, fused=0)
    rec, k2, f2 = looped(gpu, case, [STEPS], obs, tilt=TILT, dist=dist)
    assert set(k2) <= set(k_step)
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f2)
    set_path(monkeypatch, egos, rich)
    twin, _, ft = manual(gpu, case, twin=obs, tilt=TILT, dist=dist)
    assert_same_cols(ref, twin)
    assert_same_finals(fin, ft)
    logw = ref["scene"][:, :, abi.ENV_LOGW]
    assert np.array_equal(logw, twin["scene"][:, :, abi.ENV_LOGW]) and np.any(logw[:, -1] != 0)
    assert np.array_equal(ref["scene"][:, :, abi.ENV_OBSPOL], twin["scene"][:, :, abi.ENV_OBSPOL])
    assert len(np.unique(ref["scene"][:, :, abi.ENV_OBSPOL])) > 1
    unobserved, _, _ = manual(gpu, case, tilt=TILT, dist=dist)
    assert not np.array_equal(unobserved["scene"], ref["scene"])


# ---- 4: off is the parent ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_off_computes_the_unobserved_bits(gpu, monkeypatch, kind):
    """Sigma = 0, law NONE with non-zero sigmas, and attach-then-detach (alone and beside a disturbance
    with zero sigmas that keeps the options block alive) give the bits of a plan that never saw the
    entry, fused and per step; a non-zero sigma does not."""
    _, B, egos, rich, k_step, k_loop = PATHS[FUSED[kind]]
    case = case_of(kind, B)
    zero = (0.0,) * O.width(kind)
    for fused in (None, 0):
        set_path(monkeypatch, egos, rich, fused)
        plain, k0, f0 = looped(gpu, case, [STEPS])
        assert set(k0) <= set(k_loop if fused is None else k_step), k0
        assert_all_solved(case, plain.col("status"), "plain")
        variants = [dict(obs=O.make(kind, sigma_x=zero, sigma_z=zero)),
                    dict(obs=O.make(kind, law=abi.OBSERVE_NONE, seed=99, ego_base=5)),
                    dict(obs=O.make(kind), detach=True),
                    dict(obs=O.make(kind), detach=True, dist=D.make(kind, law=abi.DISTURB_NONE))]
        for v in variants:
            rec, _, f = looped(gpu, case, [STEPS], **v)
            assert_same_finals(f0, f)
            for k in COLUMNS:
                assert np.array_equal(rec.col(k), plain.col(k)), k
    _, _, f = looped(gpu, case, [STEPS], O.make(kind))
    assert not np.array_equal(f["x"], f0["x"]) and not np.array_equal(f["z"], f0["z"])
    assert not np.array_equal(f["scene"], f0["scene"])


# ---- 5: channels -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_channels_are_separate(gpu, monkeypatch, kind):
    """With sigma_z only, d_x equals the scene row's x exactly and d_z does not equal its z; with
    sigma_x only the other way round."""
    _, B, egos, rich, _, _ = PATHS[FUSED[kind]]
    set_path(monkeypatch, egos, rich)
    case = case_of(kind, B)
    n = O.width(kind)
    lo_x, lo_z = O.rows(kind)
    zero = (0.0,) * n
    rec, _, f = looped(gpu, case, [STEPS], O.make(kind, sigma_x=zero))
    assert_all_solved(case, rec.col("status"), "sigma_z only")
    assert np.array_equal(f["x"], f["scene"][:, lo_x:lo_x + n]) and np.all(f["z"] != f["scene"][:, lo_z:lo_z + n])
    rec, _, f = looped(gpu, case, [STEPS], O.make(kind, sigma_z=zero))
    assert_all_solved(case, rec.col("status"), "sigma_x only")
    assert np.array_equal(f["z"], f["scene"][:, lo_z:lo_z + n]) and np.all(f["x"] != f["scene"][:, lo_x:lo_x + n])


# ---- 6: shards and seeds -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_shard_and_seed(gpu, monkeypatch, kind):
    """Egos 40..59 in a plan of their own with ego_base = 40 take the rows they have in the 65-ego run;
    with ego_base = 0 they do not.  The same seed again is identical; another seed differs."""
    name = FUSED[kind]
    _, B, egos, rich, _, k_loop = PATHS[name]
    case, ref, _, fin = reference(gpu, monkeypatch, name)
    part = rows_of(case, slice(40, 60))
    rec, k, f = looped(gpu, part, [STEPS], O.make(kind, ego_base=40))
    assert set(k) <= set(k_loop)
    for c in COLUMNS:
        assert np.array_equal(rec.col(c), ref[c][40:60]), c
    for c in ("scene", "up", "J", "st", "it", "stats", "x", "z", "xref"):
        assert np.array_equal(f[c], fin[c][40:60]), c
    _, _, f0 = looped(gpu, part, [STEPS], O.make(kind))
    assert not np.array_equal(f0["z"], fin["z"][40:60]) and not np.array_equal(f0["up"], fin["up"][40:60])
    _, _, f7 = looped(gpu, case, [STEPS], O.make(kind, seed=O.SEED))
    assert_same_finals(fin, f7)
    _, _, f8 = looped(gpu, case, [STEPS], O.make(kind, seed=O.SEED + 1))
    assert not np.array_equal(f8["x"], fin["x"]) and not np.array_equal(f8["z"], fin["z"])
    assert not np.array_equal(f8["scene"], fin["scene"])


# ---- 7: clones ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
def test_clones_see_their_own_observations(gpu, monkeypatch, kind):
    """3 steps, then every ego becomes a copy of ego 0 (gather_egos with a broadcast), then one more
    step: the clones and their ancestor have equal scene rows -- the truth has no noise of its own --
    and differing d_z (and d_x), because a draw is addressed by slot; one step later their solves have
    taken them apart.  With sigma = 0 they stay copies."""
    import torch
    _, B, egos, rich, _, _ = PATHS[FUSED[kind]]
    set_path(monkeypatch, egos, rich)
    case = rows_of(case_of(kind, B), slice(0, 8))
    zero = (0.0,) * O.width(kind)
    for obs, diverge in ((O.make(kind), True), (O.make(kind, sigma_x=zero, sigma_z=zero), False)):
        d = attach(Loop(gpu, case), obs)
        d.loop(3)
        anc = torch.zeros(8, dtype=torch.int32, device=d.up.device)
        torch.cuda.synchronize()
        d.pl.gather_egos(anc, dict(scene=d.scene, upred=d.up, x=d.x, z=d.z, xref=d.xref, J=d.J, status=d.st, iters=d.it,
                                   stats=d.stats), d.stream.cuda_stream)
        scene, z = d.host("scene", "z")
        assert np.array_equal(scene, np.tile(scene[:1], (8, 1))) and np.array_equal(z, np.tile(z[:1], (8, 1)))
        d.loop(1)
        scene, x, z, st = d.host("scene", "x", "z", "st")
        assert np.array_equal(scene, np.tile(scene[:1], (8, 1)))
        if diverge:
            assert len(np.unique(z, axis=0)) == 8 and len(np.unique(x, axis=0)) == 8
            xo, zo = O.observed_rows(kind, obs, 3, scene)
            assert np.array_equal(x, xo) and np.array_equal(z, zo)
        else:
            assert np.array_equal(z, np.tile(z[:1], (8, 1))) and np.array_equal(x, np.tile(x[:1], (8, 1)))
        LC.assert_all_solved(case["desc"], st)
        d.loop(1)
        scene, st = d.host("scene", "st")
        same = [np.array_equal(scene[j], scene[0]) for j in range(1, 8)]
        assert (not any(same)) if diverge else all(same), same
        LC.assert_all_solved(case["desc"], st)


# ---- 8: refusals -------------------------------------------------------------------------------------

def test_refusals(gpu):
    pl = gpu.BatchPlan(highway_desc(N=6, NB=1), 2)
    pl.set_observation((0.05, 0.02, 0.05, 0.002), (0.2, 0.1, 0.2, 0.01), seed=2 ** 64 - 1, ego_base=2 ** 40)
    pl.set_observation(None)
    pl.set_observation(None)                      # detaching is always allowed

    def struct(**fields):
        s = abi.make_observation((0.05, 0.02), (0.2, 0.1))
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    for fields, msg in ((dict(law=2), "law"), (dict(law=-1), "law"), (dict(ego_base=-1), "ego_base"),
                        (dict(sigma_x=(0, -0.1)), r"sigma_x\[0\]"), (dict(sigma_z=(1, float("nan"))), r"sigma_z\[1\]"),
                        (dict(sigma_z=(0, float("inf"))), r"sigma_z\[0\]"),
                        (dict(sigma_x=(4, 0.1)), r"sigma_x\[4\].*4 components"),
                        (dict(sigma_z=(7, 0.1)), r"sigma_z\[7\]")):
        with pytest.raises(RuntimeError, match=rf"bmpc_set_observation.*\(-22\).*{msg}"):
            pl.set_observation(struct(**fields))
    q = quadruped_desc(N=6)
    assert gpu.BatchPlan(q, 2).set_observation((0.005,) * 3, (0.02,) * 3) is None      # three components there
    with pytest.raises(RuntimeError, match=r"\(-22\).*sigma_z\[3\].*3 components"):
        gpu.BatchPlan(q, 2).set_observation(struct(sigma_z=(3, 0.1)))
    q.controller = abi.CTRL_CVAR
    with pytest.raises(RuntimeError, match=r"\(-22\).*quadruped scene"):
        gpu.BatchPlan(q, 2).set_observation((0.005,))
    m = merge_desc(N=6)
    assert gpu.BatchPlan(m, 2).set_observation((0.05,)) is None
    xf = highway_desc(N=6, NB=1)
    xf.flags = abi.PLAN_TRANSFORM
    assert gpu.BatchPlan(xf, 2).set_observation(None, (0.2,)) is None    # bmpc_env_step takes such a plan


# ---- 9: the population entries -----------------------------------------------------------------------

def test_population_entries(gpu, monkeypatch):
    """The three observed_*_population entries on both launch paths: with all sigmas None they return
    disturbed_*_population's bits, with sigmas they differ and are reproducible, and a shard of a
    population takes its rows."""
    from bmpc import scenarios as sc
    small = dict(overtake=highway_desc(N=6, NB=1), quadruped=quadruped_desc(N=6))
    for fused in (None, 0):
        set_path(monkeypatch, fused=fused)
        for kind in ("overtake", "quadruped"):
            fn, base = getattr(sc, f"observed_{kind}_population"), getattr(sc, f"disturbed_{kind}_population")
            sx, sz = O.SIGMAS[kind]
            se, so = D.SIGMAS[kind]
            kw = dict(sigma_ego=se, sigma_obs=so, disturbance_seed=3, obstacle="model", obstacle_seed=2, hold=2,
                      desc=small[kind])
            plain = base(6, 4, **kw)
            off = fn(6, 4, **kw)
            assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
            stats, scene, rec = fn(6, 4, sx, sz, observation_seed=4, record=True, **kw)
            assert stats.shape == (6, abi.ENV_NSTAT) and not np.array_equal(scene, plain[1])
            assert np.array_equal(rec.col("scene")[:, -1], scene) and np.all(stats[:, abi.ENVS_SOLVES] == 3)
            assert np.all(stats[:, abi.ENVS_INFEAS] == 0)
            shard = fn(3, 4, sx, sz, observation_seed=4, ego_base=2, population=6, **kw)
            assert np.array_equal(shard[1], scene[2:5]) and np.array_equal(shard[0], stats[2:5])
            _REF[("population", kind, fused)] = (stats, scene)
        sx, sz = O.SIGMAS["merge"]
        plain = sc.disturbed_merge_population(4, 3)
        off = sc.observed_merge_population(4, 3)
        assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
        stats, scene = sc.observed_merge_population(4, 3, sx, sz, observation_seed=4)
        assert not np.array_equal(scene, plain[1]) and np.all(stats[:, abi.ENVS_SOLVES] == 2)
        assert np.all(stats[:, abi.ENVS_INFEAS] == 0)
        shard = sc.observed_merge_population(2, 3, sx, sz, observation_seed=4, ego_base=1, population=4)
        assert np.array_equal(shard[1], scene[1:3]) and np.array_equal(shard[0], stats[1:3])
        _REF[("population", "merge", fused)] = (stats, scene)
    for kind in ("overtake", "quadruped", "merge"):      # the two launch paths give the same population
        a, b = _REF[("population", kind, None)], _REF[("population", kind, 0)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), kind
