"""The sampled obstacle of the device closed loops (bmpc_set_obstacle_sampling) on the GPU.

Shapes: overtake N = 6, NB = 1, m = 3 at 65 egos (one past a wave: the one-wave kernels and the fused
k_loop, selected with BMPC_BLOCK_EGOS=0 / BMPC_LDS_RICH as tests/loop_common.py does) and at
3 egos (the small-batch k_solve_blk path); quadruped N = 6, NB = 2 at 65 egos and at 1.  6 steps with
hold = 2 (3 for the teacher-forced scene kernels).  The egos are the first rows of the batches whose
loops the existing GPU tests hold to solving (seeded_batch(300, seed=5), test_quad_loop.loop_batch).

Yardsticks: the host build of the scene functions (tests/hostsim/scene_host.cpp, held to
oracle.model and bmpc/rng.py by tests/test_obstacle_sampling.py) for the scene kernels; bit-for-bit
equality between the launch paths; bmpc/rng.py's inverse CDF of bmpc_model_eval's p at the recorded
state for the closed loops' choices.  Every case asserts the kernel the plan reports and that every
solve succeeded (CVaR 0 or 10, OSQP-class 1)."""
import numpy as np
import pytest

import obstacle_sampling_common as S
import scene_common as SC
from bmpc import abi, rng
from bmpc.scenarios import highway_desc, merge_desc
from loop_common import (PATHS, Loop, assert_all_solved, assert_same_finals, gpu, manual, model_p,  # noqa: F401
                         overtake_case, quad_case, recorded, set_path)

pytestmark = pytest.mark.gpu

STEPS, HOLD, SEED = 6, 2, 7
CASES = [("overtake", "wave", 65), ("overtake", "lean", 65), ("overtake", "blk", 3), ("quadruped", "wave", 65),
         ("quadruped", "lean", 65), ("quadruped", "wave", 1)]


def scene_of(kind, B, robust=False):
    case = overtake_case(6, 1, B, robust) if kind == "overtake" else quad_case(B)
    return SC.Scene(kind, B, case=case), case


def sampler(seed=SEED, hold=HOLD, ego_base=0):
    return abi.make_obstacle_sampling("model", seed=seed, hold=hold, ego_base=ego_base)


def attached(smp):
    """The setup callback that attaches the sampler (None: none)."""
    return None if smp is None else lambda d: d.pl.set_obstacle_sampling(smp)


def run_loop(plan, case, smp, chunks, record=True):
    """The closed loop in `chunks` calls with the sampler attached: finals, the record on the host, kernels."""
    rec, kernels, fin = recorded(plan, case, chunks, predictions=False, attach=record, setup=attached(smp))
    return fin, rec, kernels


def run_manual(plan, case, smp, steps):
    """The same loop as *_env_step_device + solve_device with a host copy per step: finals, the scene
    rows and statuses [B, steps, ...], kernels."""
    cols, kernels, fin = manual(plan, case, steps, setup=attached(smp))
    return fin, cols["scene"], cols["status"], kernels


def check_recorded_choices(plan, sc, smp, scenes, ego_base=0):
    """Every choice of recorded scene rows [B, T, 16] from step 0: epoch starts are the inverse CDF of
    bmpc_model_eval's p at the row's (x, z) -- the state the step's solve saw, which is the choice's
    pre-step state -- under bmpc/rng.py's u, the margin rule of tests/test_obstacle_sampling.py."""
    B, T = scenes.shape[:2]
    n = sc.n
    tg = sc.lc_targets(scenes) if sc.kind == "overtake" else None
    choices = scenes[:, :, abi.ENV_OBSPOL].astype(int)
    left_out = draws = 0
    for t in range(T):
        if t % smp.hold:
            np.testing.assert_array_equal(choices[:, t], choices[:, t - t % smp.hold])
            continue
        p = model_p(plan, sc, None if tg is None else tg[:, t], scenes[:, t, 0:n], scenes[:, t, n:2 * n])
        want, sure = S.expected_choice(p, rng.obstacle_uniform(smp.seed, ego_base + np.arange(B), t // smp.hold))
        draws += B
        left_out += int((~sure).sum())
        np.testing.assert_array_equal(choices[sure, t], want[sure], err_msg=f"epoch start {t}")
    print(f"{sc.kind} B {B}: {draws - left_out} of {draws} draws compared, counts",
          np.bincount(choices[:, ::smp.hold].ravel()))
    assert left_out <= S.MAX_LEFT_OUT * draws, (left_out, draws)


# ---- 1: the scene kernels against the host scene function ------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_scene_kernel_equals_host_function(gpu, monkeypatch, kind):
    """k_env / k_env_quad with the sampler, 65 egos, 12 teacher-forced steps, hold 3: x / z / x_ref to
    1e-9 and equal choices against the host build.  An epoch start whose u lies within 1e-9 of a
    partial sum (oracle.model's p at the host's state) is left out with the rest of that ego's
    episode; at most 1 % of the decisions may be."""
    import torch
    set_path(monkeypatch)
    sc, case = scene_of(kind, 65)
    smp = sampler(hold=3)
    steps = 12
    host = SC.host_run(sc, steps, smp)[0]
    d = Loop(gpu, case)
    d.pl.set_obstacle_sampling(smp)
    valid = np.ones(65, bool)
    left_out = 0
    for t in range(steps):
        if t > 0:
            up = np.zeros((65, d.pl.U, sc.desc.d))
            up[:, 0] = sc.script(t)
            d.up.copy_(torch.tensor(up, dtype=torch.float64))
            torch.cuda.synchronize()
        d.env_step()
        scene, x, z, xr = d.host("scene", "x", "z", "xref")
        h = host[t]
        if t % 3 == 0:
            p = np.stack([sc.oracle_p(h["pol"], e, h["x"][e], h["z"][e]) for e in range(65)])
            _, sure = S.expected_choice(p, rng.obstacle_uniform(SEED, np.arange(65), t // 3))
            left_out += int((valid & ~sure).sum())
            valid &= sure
        np.testing.assert_array_equal(scene[valid, abi.ENV_OBSPOL], h["scene"][valid, abi.ENV_OBSPOL],
                                      err_msg=f"step {t}")
        for got, key in ((x, "x"), (z, "z"), (xr, "xref")):
            np.testing.assert_allclose(got[valid], h[key][valid], rtol=0, atol=1e-9, err_msg=f"{key} step {t}")
        np.testing.assert_allclose(scene[valid], h["scene"][valid], rtol=0, atol=1e-9)
    assert left_out <= S.MAX_LEFT_OUT * 65 * (steps // 3), left_out
    assert len(np.unique(host[0]["scene"][:, abi.ENV_OBSPOL])) == sc.m       # every policy is drawn


# ---- 2: every launch path, bit for bit; 4: the record and the rule ---------------------------------

@pytest.mark.parametrize("kind,path,B", CASES, ids=[f"{k}-{p}-{b}" for k, p, b in CASES])
def test_paths_agree_and_choices_follow_the_model(gpu, monkeypatch, kind, path, B):
    """With the sampler on, one loop call, a loop split over two calls, BMPC_LOOP_FUSED=0 and manual
    stepping agree bit for bit in scene, outputs, statistics and warm start; the recorded obs_policy
    column is the scene's, and follows the draws' inverse CDF of bmpc_model_eval's p."""
    egos, rich, k_step, k_loop = PATHS[kind, path]
    sc, case = scene_of(kind, B)
    smp = sampler()
    set_path(monkeypatch, egos, rich)
    fin, scenes, sts, km = run_manual(gpu, case, smp, STEPS)
    assert km <= set(k_step), km
    assert_all_solved(sc.desc, sts)
    assert np.all(scenes[:, -1, abi.ENV_STEPS] == STEPS)
    f1, rec, k1 = run_loop(gpu, case, smp, [STEPS])
    assert set(k1) <= set(k_loop), k1
    assert_same_finals(fin, f1)
    assert np.array_equal(rec.col("scene"), scenes) and np.array_equal(rec.col("status"), sts)
    assert np.array_equal(rec.obs_policy, scenes[:, :, abi.ENV_OBSPOL])
    f2, _, k2 = run_loop(gpu, case, smp, [3, STEPS - 3], record=False)     # (3: the second call starts inside an epoch)
    assert set(k2) <= set(k_loop) and len(k2) == 2, k2
    assert_same_finals(fin, f2)
    set_path(monkeypatch, egos, rich, fused=0)
    f3, rec3, k3 = run_loop(gpu, case, smp, [STEPS])
    assert set(k3) <= set(k_step), k3
    assert_same_finals(fin, f3)
    assert np.array_equal(rec3.col("scene"), scenes)
    check_recorded_choices(gpu, sc, smp, scenes)


def test_robust_plan_samples_on_its_per_step_path(gpu, monkeypatch):
    sc, case = scene_of("overtake", 3, robust=True)
    smp = sampler()
    set_path(monkeypatch)
    fin, scenes, sts, km = run_manual(gpu, case, smp, STEPS)
    assert km <= {abi.KERNEL_QP_RICH, abi.KERNEL_QP_LEAN}, km
    assert_all_solved(sc.desc, sts)
    f1, rec, k1 = run_loop(gpu, case, smp, [STEPS])
    assert set(k1) == km, k1
    assert_same_finals(fin, f1)
    assert np.array_equal(rec.col("scene"), scenes)
    check_recorded_choices(gpu, sc, smp, scenes)


# ---- 3: shard invariance ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_shard_gets_the_unsharded_rows(gpu, monkeypatch, kind):
    """A 20-ego plan holding egos 40..59 of the 65 with ego_base = 40 computes those egos' rows of the
    65-ego plan bit for bit (fused loop, LDS-rich)."""
    egos, rich, _, k_loop = PATHS[kind, "wave"]
    set_path(monkeypatch, egos, rich)
    _, case = scene_of(kind, 65)
    whole, rec, k = run_loop(gpu, case, sampler(), [STEPS])
    part_case = dict(case, scene=case["scene"][40:60].copy(), policies=case["policies"][40:60])
    part, prec, kp = run_loop(gpu, part_case, sampler(ego_base=40), [STEPS])
    assert set(k) | set(kp) <= set(k_loop)
    for key in whole:
        if key == "ws":
            for kk in whole[key]:
                assert np.array_equal(whole[key][kk][40:60], part[key][kk]), ("warm start", kk)
        else:
            assert np.array_equal(whole[key][40:60], part[key]), key
    for c in rec.cols:
        assert np.array_equal(rec.col(c)[40:60], prec.col(c)), c
    # ... and without ego_base the shard draws as egos 0..19: other choices somewhere
    _, other, _ = run_loop(gpu, part_case, sampler(), [STEPS])
    assert (other.obs_policy != prec.obs_policy).any()


# ---- 4, 5: seeds; attach and detach ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_seeds_and_detach(gpu, monkeypatch, kind):
    """The same seed twice gives identical results, another seed other choices somewhere; mode argmax,
    and attach then detach, give the bits of a plan that never had a sampler -- which differ from the
    sampled ones."""
    egos, rich, _, k_loop = PATHS[kind, "wave"]
    set_path(monkeypatch, egos, rich)
    sc, case = scene_of(kind, 65)
    a, ra, _ = run_loop(gpu, case, sampler(), [STEPS])
    b, rb, _ = run_loop(gpu, case, sampler(), [STEPS])
    assert_same_finals(a, b)
    assert all(np.array_equal(ra.col(c), rb.col(c)) for c in ra.cols)
    _, rc, _ = run_loop(gpu, case, sampler(seed=SEED + 1), [STEPS])
    assert (rc.obs_policy != ra.obs_policy).any()
    plain, rp, kp = run_loop(gpu, case, None, [STEPS])
    assert set(kp) <= set(k_loop)
    assert_all_solved(sc.desc, rp.col("status"))
    assert (rp.obs_policy != ra.obs_policy).any()
    off, _, _ = run_loop(gpu, case, abi.make_obstacle_sampling("argmax", seed=99, hold=5, ego_base=3), [STEPS])
    assert_same_finals(plain, off)
    d = Loop(gpu, case)
    d.pl.set_obstacle_sampling(sampler())
    d.pl.set_obstacle_sampling(None)
    d.loop(STEPS)
    assert_same_finals(plain, d.finals())


def test_sampler_attached_mid_episode_waits_for_the_epoch(gpu, monkeypatch):
    """Attached after step 0 of a hold-2 episode, the sampler keeps the argmax choice of step 0 at step 1
    and draws at step 2."""
    set_path(monkeypatch, 0, 1)
    sc, case = scene_of("overtake", 65)
    d = Loop(gpu, case)
    rec = d.pl.new_loop_record(3, 0)
    d.pl.set_loop_record(rec)
    d.loop(1)
    d.stream.synchronize()
    d.pl.set_obstacle_sampling(sampler())
    d.loop(2)
    d.stream.synchronize()
    c = rec.host().obs_policy
    np.testing.assert_array_equal(c[:, 1], c[:, 0])
    assert (c[:, 2] != c[:, 1]).any()


# ---- 6: refusals -----------------------------------------------------------------------------------

def test_refusals(gpu):
    pl = gpu.BatchPlan(highway_desc(N=6, NB=1), 2)
    pl.set_obstacle_sampling("model", seed=2 ** 64 - 1, hold=4, ego_base=2 ** 40)
    pl.set_obstacle_sampling(None)
    for field, value, msg in (("hold", 0, "hold"), ("hold", -3, "hold"), ("mode", 7, "mode"), ("mode", -1, "mode"),
                              ("ego_base", -1, "ego_base")):
        s = sampler()
        setattr(s, field, value)
        with pytest.raises(RuntimeError, match=rf"\(-22\).*{msg}"):
            pl.set_obstacle_sampling(s)
    merge = gpu.BatchPlan(merge_desc(N=6), 2)
    with pytest.raises(RuntimeError, match=r"\(-22\).*merge"):
        merge.set_obstacle_sampling("model")
    merge.set_obstacle_sampling(None)            # detaching is always allowed
    xf = highway_desc(N=6, NB=1)
    xf.flags = abi.PLAN_TRANSFORM
    with pytest.raises(RuntimeError, match=r"\(-22\).*TRANSFORM"):
        gpu.BatchPlan(xf, 2).set_obstacle_sampling("model")


# ---- 7: the population entries ---------------------------------------------------------------------

def test_sampled_populations(gpu, monkeypatch):
    from bmpc import scenarios
    set_path(monkeypatch)
    for fn, kind in ((scenarios.sampled_overtake_population, "overtake"),
                     (scenarios.sampled_quadruped_population, "quadruped")):
        stats, scene, rec = fn(8, 3, obstacle="model", record=True, obstacle_seed=SEED)
        assert rec.kind == kind and np.array_equal(rec.col("scene")[:, -1], scene)
        assert np.all(stats[:, abi.ENVS_SOLVES] == 2)
        sc = SC.Scene(kind, 8, N=20 if kind == "overtake" else 25)      # the entries' own batches and plans
        if kind == "quadruped":
            sc = SC.Scene(kind, 8, case=dict(desc=scenarios.quadruped_desc(), env=abi.make_quad_env(),
                                            scene=rec.col("scene")[:, 0], policies=scenarios.quadruped_policy_rows(8)))
        assert_all_solved(sc.desc, rec.col("status"))
        check_recorded_choices(gpu, sc, sampler(hold=1), rec.col("scene"))
        # a shard of the population: egos 3..7 of the 8 with ego_base = 3
        _, pscene, prec = fn(5, 3, obstacle="model", record=True, obstacle_seed=SEED, ego_base=3, population=8)
        assert np.array_equal(prec.col("scene"), rec.col("scene")[3:]) and np.array_equal(pscene, scene[3:])
