"""The overtake closed loop under BranchMPC (BMPC_CTRL_QP) and robustMPC on the GPU: bmpc_loop_device
accepts BranchMPC plans and fuses them into one k_loop launch (OvertakeQpScene, the QP solver);
robust plans keep their launches per step unless BMPC_LOOP_FUSED=2 asks for the same kernel.

Shapes: N = 8, NB = 2 (T = 106: the recording's shape, and the one where the lean path moves the
coupling system to the slab) at 1, 3 and 65 egos -- 65 gives k_env its second workgroup on the
per-step path --, 6 steps, and the recording's 30.

Yardsticks: the reference's own BranchMPC closed loop (tests/golden/highway_qp_n8_nb2.npz), which the
host build follows free-running to 7.5e-14 in x and 1.7e-13 in u (tests/test_overtake_qp_loop.py), at
the project's 1e-6 for this controller on the GPU (test_gpu_parity.test_branch_mpc_qp_replay_gpu) and
1e-9 for the obstacle, whose inputs are discrete choices (tests/test_env_gpu.py); bit-for-bit
equality between the launch paths.  Where the fused path is meant the tests set BMPC_LOOP_FUSED=2, so
they do not depend on the shipped default, which one assertion pins
(test_default_launch_of_each_controller).

Measured on the MI355X against the recording over the 30 steps (the same on every path, rich and
lean): 1.9e-13 in x, 7.1e-13 in u, 6.4e-14 in x_ref, z exact."""
import numpy as np
import pytest

from bmpc import abi, scenarios
from bmpc.scenarios import highway_desc, highway_desc_from_golden, highway_policy_rows
from common import golden
from loop_common import (Loop, assert_all_solved, assert_record_equals, assert_same_finals, gpu, manual,  # noqa: F401
                         overtake_case, recorded, set_path)

pytestmark = pytest.mark.gpu

N, NB, STEPS = 8, 2, 6
K_STEP = {1: abi.KERNEL_QP_RICH, 0: abi.KERNEL_QP_LEAN}
K_LOOP = {1: abi.KERNEL_LOOP_RICH, 0: abi.KERNEL_LOOP_LEAN}
FUSED, PER_STEP = 2, 0
BUFFERS = dict(scene="scene", upred="up", x="x", z="z", xref="xref", J="J", status="st", iters="it", stats="stats")


def case_of(B, controller):
    case = overtake_case(N, NB, B)
    case["desc"].controller = controller
    return case


def assert_same_record(a, b):
    assert sorted(a.cols) == sorted(b.cols)
    for k in a.cols:
        assert np.array_equal(a.col(k), b.col(k)), (k, np.argwhere(a.col(k) != b.col(k))[:4])


# ---- 1: the loop entry follows the reference's recording ---------------------------------------------

def recording_case(g, B=2):
    return dict(kind="overtake", desc=highway_desc_from_golden(g, controller="branch"),
                scene=scenarios._overtake_scene(np.repeat(np.asarray(g["traj_x"][0], float)[None], B, 0),
                                                np.repeat(np.asarray(g["traj_z"][0], float)[None], B, 0)),
                policies=highway_policy_rows(np.repeat(np.asarray(g["xRef0"], float)[None], B, 0), float(g["Kpsi"])),
                env=abi.make_env(n_lane=int(g["N_lane"]), L=float(g["L"]), W=float(g["W"]), Kpsi=float(g["Kpsi"]),
                                 target=np.asarray(g["xRef0"], float)))


@pytest.mark.parametrize("fused", [FUSED, PER_STEP], ids=["fused", "per_step"])
@pytest.mark.parametrize("rich", [1, 0], ids=["rich", "lean"])
def test_loop_follows_the_reference_recording(gpu, monkeypatch, rich, fused):
    """30 steps of the reference's BranchMPC closed loop through loop_device in chunks [1, 14, 15] with a
    recorder, two identical egos: x, u and x_ref to 1e-6, z to 1e-9, every status 1, 29 solves booked,
    none infeasible, the recording's collision flag."""
    g = golden("highway_qp_n8_nb2")
    T = len(g["traj_x"])
    assert T == 30
    set_path(monkeypatch, None, rich, fused)
    rec, kernels, fin = recorded(gpu, recording_case(g), [1, 14, 15], predictions=False)
    assert set(kernels) == {(K_LOOP if fused else K_STEP)[rich]}, kernels
    dev = {k: float(np.abs(got - np.asarray(g[key], float)[None]).max())
           for k, got, key in (("x", rec.x, "traj_x"), ("z", rec.z, "traj_z"), ("u", rec.col("u"), "traj_u"),
                               ("xref", rec.col("xref"), "traj_xRef"))}
    print("rich" if rich else "lean", "fused" if fused else "per step", "max deviation from the recording:", dev,
          "iterations", rec.col("iters").min(), "-", rec.col("iters").max())
    assert dev["x"] <= 1e-6 and dev["u"] <= 1e-6 and dev["xref"] <= 1e-6 and dev["z"] <= 1e-9, dev
    assert np.all(rec.col("status") == 1), rec.col("status")
    assert np.array_equal(rec.col("status")[0], np.asarray(g["traj_status"]))
    assert np.array_equal(rec.col("scene")[0], rec.col("scene")[1])        # identical scenes: the egos agree
    st = fin["stats"]
    assert np.all(st[:, abi.ENVS_SOLVES] == T - 1) and np.all(st[:, abi.ENVS_INFEAS] == 0)
    assert np.all(st[:, abi.ENVS_COLLIDED] == float(g["traj_collision"][-1]))


# ---- 2: every launch path, bit for bit ---------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("rich", [1, 0], ids=["rich", "lean"])
def test_every_launch_path_bit_for_bit(gpu, monkeypatch, rich, B):
    """Manual stepping, one loop call, a loop split [3, 3], a loop continued after one manual step and
    BMPC_LOOP_FUSED=0 agree bit for bit in every final buffer, in the warm start (uLin, p, OldInput) and
    in the record; manual and =0 run k_qp, the fused calls k_loop; every solve returns status 1."""
    case = case_of(B, abi.CTRL_QP)
    set_path(monkeypatch, None, rich, FUSED)
    cols, km, fin = manual(gpu, case, STEPS)
    assert km == {K_STEP[rich]}, km
    assert_all_solved(case["desc"], cols["status"])
    assert np.all(fin["stats"][:, abi.ENVS_SOLVES] == STEPS - 1) and np.all(fin["stats"][:, abi.ENVS_INFEAS] == 0)
    assert {"uLin", "p", "old_input"} <= set(fin["ws"]) and fin["ws"]["uLin"].any() and fin["ws"]["p"].any()
    print("B", B, "rich" if rich else "lean", "iterations", cols["iters"].min(), "-", cols["iters"].max())

    rec, k1, f1 = recorded(gpu, case, [STEPS])
    assert k1 == [K_LOOP[rich]], k1
    assert_same_finals(fin, f1)
    assert_record_equals(rec, cols)

    rec, k2, f2 = recorded(gpu, case, [3, 3])
    assert k2 == [K_LOOP[rich]] * 2, k2
    assert_same_finals(fin, f2)
    assert_record_equals(rec, cols)

    d = Loop(gpu, case)                       # one manual step, then the loop from t = 1
    d.env_step()
    d.solve()
    d.stream.synchronize()
    assert d.pl.last_kernel() == K_STEP[rich]
    rec = d.pl.new_loop_record(STEPS - 1, 1, predictions=True)
    d.pl.set_loop_record(rec)
    d.loop(STEPS - 1)
    d.stream.synchronize()
    assert d.pl.last_kernel() == K_LOOP[rich]
    assert_same_finals(fin, d.finals())
    assert_record_equals(rec.host(), cols, slice(1, None))

    set_path(monkeypatch, None, rich, PER_STEP)
    rec, k3, f3 = recorded(gpu, case, [STEPS])
    assert k3 == [K_STEP[rich]], k3
    assert_same_finals(fin, f3)
    assert_record_equals(rec, cols)


def test_default_launch_of_each_controller(gpu, monkeypatch):
    """The documented defaults (BMPC_LOOP_FUSED unset, and 1): BranchMPC plans fuse at any batch, robust
    plans keep their launches per step."""
    for value in (None, 1):
        set_path(monkeypatch, None, 1, value)
        for controller, want in ((abi.CTRL_QP, abi.KERNEL_LOOP_RICH), (abi.CTRL_ROBUST, abi.KERNEL_QP_RICH)):
            for B in (1, 3):
                _, kernels, _ = recorded(gpu, case_of(B, controller), [2], attach=False)
                assert kernels == [want], (value, controller, B, kernels)


# ---- 3: the options compose --------------------------------------------------------------------------

def test_sampler_disturbance_and_observation_compose(gpu, monkeypatch):
    """65 egos with the sampled obstacle (hold 2), a disturbance and an observation model attached
    together: the fused launch and BMPC_LOOP_FUSED=0 agree bit for bit in the finals and the record."""
    case = case_of(65, abi.CTRL_QP)

    def setup(d):
        d.pl.set_obstacle_sampling("model", seed=7, hold=2)
        d.pl.set_disturbance((0.3, 0.01), (0.5, 0.02), seed=7)
        d.pl.set_observation((0.05, 0.02, 0.05, 0.002), (0.2, 0.1, 0.2, 0.01), seed=11)

    set_path(monkeypatch, None, None, FUSED)
    ra, ka, fa = recorded(gpu, case, [STEPS], setup=setup)
    assert set(ka) <= set(K_LOOP.values()), ka
    set_path(monkeypatch, None, None, PER_STEP)
    rb, kb, fb = recorded(gpu, case, [STEPS], setup=setup)
    assert set(kb) <= set(K_STEP.values()), kb
    assert_same_finals(fa, fb)
    assert_same_record(ra, rb)
    # the options were in force: the plain loop differs in the choices, the states and what the solves saw
    set_path(monkeypatch, None, None, FUSED)
    rp, _, fp = recorded(gpu, case, [STEPS])
    assert (rp.obs_policy != ra.obs_policy).any() and not np.array_equal(rp.x, ra.x)
    assert np.array_equal(fp["x"], fp["scene"][:, abi.ENV_X:abi.ENV_X + 4])
    assert not np.array_equal(fa["x"], fa["scene"][:, abi.ENV_X:abi.ENV_X + 4])    # observed, not true, states


def test_tilted_resampled_population_composes(gpu, monkeypatch):
    """Tilted sampling with one BatchPlan.resample (ess_fraction 2: always) between two 3-step segments:
    fused and BMPC_LOOP_FUSED=0 agree bit for bit, ENV_LOGW and the ancestors included."""
    case = case_of(65, abi.CTRL_QP)

    def run(fused):
        set_path(monkeypatch, None, None, fused)
        d = Loop(gpu, case)
        d.pl.set_obstacle_proposal(tilt=(1.0, 4.0, 0.25))
        d.pl.set_obstacle_sampling("tilted", seed=7, hold=1)
        rec = d.pl.new_loop_record(STEPS, 0, predictions=True)
        d.pl.set_loop_record(rec)
        d.loop(3)
        anc, info = d.pl.resample({k: getattr(d, v) for k, v in BUFFERS.items()}, 3, seed=11, ess_fraction=2.0,
                                  stream=d.stream.cuda_stream)
        d.loop(3)
        d.stream.synchronize()
        return d.finals(), rec.host(), anc.cpu().numpy(), info.cpu().numpy(), d.pl.last_kernel()

    fa, ra, anc_a, info_a, ka = run(FUSED)
    fb, rb, anc_b, info_b, kb = run(PER_STEP)
    assert ka in K_LOOP.values() and kb in K_STEP.values(), (ka, kb)
    assert info_a[abi.R_RESAMPLED] == 1.0 and (anc_a != np.arange(65)).any()
    assert np.array_equal(anc_a, anc_b) and np.array_equal(info_a, info_b)
    assert_same_finals(fa, fb)
    assert np.array_equal(fa["scene"][:, abi.ENV_LOGW], fb["scene"][:, abi.ENV_LOGW])
    assert np.all(np.isfinite(fa["scene"][:, abi.ENV_LOGW])) and (ra.logw[:, 2] != 0.0).any()
    assert_same_record(ra, rb)


# ---- 4: robust plans, opt-in -------------------------------------------------------------------------

@pytest.mark.parametrize("B", [3, 65])
def test_robust_plans_fuse_on_request(gpu, monkeypatch, B):
    """A robustMPC plan under BMPC_LOOP_FUSED=2 runs k_loop and equals, bit for bit, the unset run on
    its per-step kernels: finals, the warm start (xLin, uLin, OldInput) and the record (no zpred)."""
    case = case_of(B, abi.CTRL_ROBUST)
    set_path(monkeypatch)
    ra, ka, fa = recorded(gpu, case, [STEPS])
    assert set(ka) <= set(K_STEP.values()), ka
    assert_all_solved(case["desc"], ra.col("status"))
    rich = 1 if ka[0] == abi.KERNEL_QP_RICH else 0
    set_path(monkeypatch, None, None, FUSED)
    rb, kb, fb = recorded(gpu, case, [STEPS])
    assert kb == [K_LOOP[rich]], (ka, kb)
    assert "zpred" not in rb.cols and "xpred" in rb.cols
    assert sorted(fa["ws"]) == ["old_input", "uLin", "xLin"] and fa["ws"]["xLin"].any()
    assert_same_finals(fa, fb)
    assert_same_record(ra, rb)
    rc, kc, fc = recorded(gpu, case, [3, 3])
    assert kc == [K_LOOP[rich]] * 2
    assert_same_finals(fa, fc)
    assert_same_record(ra, rc)


# ---- 5: refusals -------------------------------------------------------------------------------------

def test_refusals(gpu, monkeypatch):
    set_path(monkeypatch)
    prox = Loop(gpu, case_of(2, abi.CTRL_PROX))
    with pytest.raises(RuntimeError, match=r"\(-22\).*bmpc_loop_device.*CVaR.*BranchMPC.*robust"):
        prox.loop(2)
    d = Loop(gpu, case_of(2, abi.CTRL_QP))
    for n in (0, -1):
        with pytest.raises(RuntimeError, match=r"\(-22\).*nsteps"):
            d.loop(n)
        d.t = 0
    script = np.zeros((2, 2), np.int32)
    d.pl.set_obstacle_proposal(script=script)
    d.pl.set_obstacle_sampling("script", hold=1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*bmpc_loop_device"):
        d.loop(3)                              # the script covers steps 0 and 1 only
    d.t = 0
    d.loop(2)
    d.stream.synchronize()
    assert np.all(d.host("scene")[0][:, abi.ENV_STEPS] == 2)


# ---- 6: the population entries -----------------------------------------------------------------------

def test_scenarios(gpu, monkeypatch):
    """A BranchMPC population (the population entries keep their parameter lists, which existing tests
    pin, so the controller travels in desc=highway_desc(controller=...)), and controller_comparison."""
    from bmpc import montecarlo
    set_path(monkeypatch)
    stats, scene = scenarios.sampled_overtake_population(8, 4, obstacle=None, desc=highway_desc(controller="branch"))
    assert stats.shape == (8, abi.ENV_NSTAT) and np.all(stats[:, abi.ENVS_SOLVES] == 3)
    assert np.all(scene[:, abi.ENV_STEPS] == 4)
    out = scenarios.controller_comparison(8, 4)
    assert list(out["runs"]) == ["cvar", "branch", "robust"]
    for c, run in out["runs"].items():
        assert run["stats"].shape == (8, abi.ENV_NSTAT) and run["scene"].shape == (8, abi.ENV_STRIDE), c
        assert np.all(run["stats"][:, abi.ENVS_SOLVES] == 3), c
    assert np.array_equal(out["runs"]["branch"]["stats"], stats) and np.array_equal(out["runs"]["branch"]["scene"], scene)
    plain_stats, plain_scene = scenarios.overtake_population(8, 4)
    assert np.array_equal(out["runs"]["cvar"]["stats"], plain_stats)
    assert np.array_equal(out["runs"]["cvar"]["scene"], plain_scene)
    assert sorted(out["pairs"]) == [("branch", "robust"), ("cvar", "branch"), ("cvar", "robust")]
    for pair, d in out["pairs"].items():
        for key in ("collided", "cost"):
            mean, se, corr = d[key]
            assert np.isfinite(mean) and np.isfinite(se) and se >= 0.0, (pair, key, d[key])
        a, b = (out["runs"][c]["stats"] for c in pair)
        cost = [s[:, abi.ENVS_J] / s[:, abi.ENVS_SOLVES] for s in (a, b)]
        assert d["cost"] == montecarlo.paired_difference(*cost)
        assert np.isfinite(d["cost"][2])
    with pytest.raises(ValueError):
        scenarios.controller_comparison(8, 4, controllers=("cvar", "prox"))
