"""The overtake scene under BranchMPC and robustMPC, on the CPU: the reference the GPU tests of
tests/test_overtake_qp_loop_gpu.py lean on, and the Python surface around the loop.

* The host build of the kernels, free-running (the scene step feeds the solve, the solve's uPred[0]
  feeds the next scene step, nothing teacher-forced), follows the reference's own closed loops of
  BranchMPC (tests/golden/highway_qp_n8_nb2.npz, 30 steps) and robustMPC (highway_robust_n8_nb2.npz,
  20 steps) to the project's scene-replay bar of 1e-9 in x, z and uPred[0], every status 1.
  Measured: 7.5e-14 in x and 1.7e-13 in u (BranchMPC), 5.5e-12 and 2.7e-11 (robustMPC), z exact.
* scenarios.highway_desc(controller=...) and montecarlo.paired_difference."""
import ctypes as C

import numpy as np
import pytest

from bmpc import abi, montecarlo
from bmpc.scenarios import highway_desc, highway_desc_from_golden, highway_policy_rows
from common import golden


def _env(g):
    return abi.make_env(n_lane=int(g["N_lane"]), L=float(g["L"]), W=float(g["W"]), Kpsi=float(g["Kpsi"]),
                        target=np.asarray(g["xRef0"], float))


@pytest.mark.parametrize("name,controller,steps", [("highway_qp_n8_nb2", "branch", 30),
                                                  ("highway_robust_n8_nb2", "robust", 20)])
def test_host_closed_loop_follows_the_recording(name, controller, steps):
    import hostsim_lib as H
    g = golden(name)
    assert len(g["traj_x"]) == steps
    B = 2                                   # identical scenes: both egos must agree
    hs = H.HostSim(highway_desc_from_golden(g, controller=controller), B)
    hs.set_policies(highway_policy_rows(np.repeat(np.asarray(g["xRef0"], float)[None], B, 0), float(g["Kpsi"])))
    env = _env(g)
    scene = np.zeros((B, abi.ENV_STRIDE))
    scene[:, abi.ENV_X:abi.ENV_X + 4] = g["traj_x"][0]
    scene[:, abi.ENV_Z:abi.ENV_Z + 4] = g["traj_z"][0]
    stats = np.zeros((B, abi.ENV_NSTAT))
    up = J = st = it = None
    worst = dict(x=0.0, z=0.0, u=0.0)
    for t in range(steps):
        x, z, xr = hs.env_step(env, t, scene, up, J, st, it, stats)
        r = hs.solve(x, z, xr)
        up, J, st, it = r["upred"], r["J"], r["status"], r["iters"]
        for k, got, want in (("x", x, g["traj_x"][t]), ("z", z, g["traj_z"][t]), ("u", up[:, 0], g["traj_u"][t])):
            worst[k] = max(worst[k], float(np.abs(got - np.asarray(want)[None]).max()))
        np.testing.assert_allclose(xr, np.repeat(np.asarray(g["traj_xRef"][t])[None], B, 0), rtol=0, atol=1e-9)
        assert np.all(st == 1), (t, st, it)
    print(name, "max deviation from the recording:", worst)
    assert worst["x"] <= 1e-9 and worst["z"] <= 1e-9 and worst["u"] <= 1e-9, worst
    assert np.all(stats[:, abi.ENVS_SOLVES] == steps - 1) and np.all(stats[:, abi.ENVS_INFEAS] == 0)
    assert np.all(scene[:, abi.ENV_COLL] == float(g["traj_collision"][-1]))


def test_highway_desc_controller_keyword():
    raw = lambda d: bytes((C.c_char * C.sizeof(d)).from_buffer_copy(d))
    base = highway_desc(N=8, NB=2)
    assert base.controller == abi.CTRL_CVAR
    assert raw(highway_desc(N=8, NB=2, controller="cvar")) == raw(base)
    for key, val in (("cvar", abi.CTRL_CVAR), ("branch", abi.CTRL_QP), ("robust", abi.CTRL_ROBUST)):
        d = highway_desc(N=8, NB=2, controller=key)
        assert d.controller == val
        d.controller = abi.CTRL_CVAR            # nothing else depends on the keyword
        assert raw(d) == raw(base)
    g = golden("highway_qp_n8_nb2")
    assert raw(highway_desc_from_golden(g)) == raw(highway_desc_from_golden(g, controller="cvar"))
    assert highway_desc_from_golden(g, controller="branch").controller == abi.CTRL_QP
    for bad in ("prox", "CVAR", None, abi.CTRL_QP):
        with pytest.raises(ValueError):
            highway_desc(controller=bad)


def test_paired_difference():
    rng = np.random.default_rng(3)
    a = rng.normal(2.0, 1.0, 257)
    b = 0.8 * a + rng.normal(0.0, 0.3, 257)
    mean, se, corr = montecarlo.paired_difference(a, b)
    d = a - b
    assert mean == pytest.approx(d.mean(), rel=1e-14)
    assert se == pytest.approx(np.std(d, ddof=1) / np.sqrt(d.size), rel=1e-13)
    assert corr == pytest.approx(np.corrcoef(a, b)[0, 1], rel=1e-12)
    # pairing pays: the error is below that of two independent samples
    assert se < np.sqrt(a.var(ddof=1) / a.size + b.var(ddof=1) / b.size)
    # 0/1 flags, lists, a constant side, one ego
    m, s, c = montecarlo.paired_difference([1, 0, 1, 1], [0, 0, 1, 0])
    assert (m, s) == (0.5, pytest.approx(np.std([1, 0, 0, 1], ddof=1) / 2.0))
    assert c == pytest.approx(np.corrcoef([1, 0, 1, 1], [0, 0, 1, 0])[0, 1])
    m, s, c = montecarlo.paired_difference([1.0, 2.0, 3.0], [0.0, 0.0, 0.0])
    assert m == 2.0 and s == pytest.approx(1.0 / np.sqrt(3.0)) and np.isnan(c)
    m, s, c = montecarlo.paired_difference([4.0], [1.0])
    assert (m, s) == (3.0, 0.0) and np.isnan(c)
    for bad in (([1.0, 2.0], [1.0]), ([], []), (np.zeros((2, 2)), np.zeros(3))):
        with pytest.raises(ValueError):
            montecarlo.paired_difference(*bad)
