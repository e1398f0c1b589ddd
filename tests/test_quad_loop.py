"""The quadruped scene's closed loop (csrc/bmpc_env_quad.h; bmpc_quad_env_step, bmpc_quad_loop_device)
against the reference's own scene code, ``tests/golden/quadruped_scene.npz``.

The fixture (tools/gen_golden_quad_scene.py) is the reference's unmodified Quad_env.step driven by a
scripted stand-in for the controller: 6 scenes of 30 steps -- per step the ego, the obstacle, xRef
and the obstacle's backup choice -- that together reach every branch of the rules (backup 0 kept,
the argmax picking 1 and picking 0, a return to 0, x_ref clipped at 5 m and not, the ego's own
heading within 0.1 m of the goal, each of the two heading wraps), every decision at least 1e-6 from
its boundary.  No MPC solve is involved; quadruped_n25_nb2.npz pins the controller.

Host (not gpu): the scene function itself, compiled with g++ (tests/hostsim/scene_host.cpp), and
the package's quadruped_env.Quad_env.step, both fed the fixture's scripted inputs: x / z / xRef to
1e-9 on every step of every scene (the bar of tests/test_env_host.py: cos / sin / atan2 of a
different libm), every backup choice equal.

GPU: the same drive through k_env_quad in a batch of 65; one ego in lockstep with the host Quad_env
around real BranchMPCProx solves; the fused k_loop (scene + tree + QP per step) against the
per-step launches bit for bit, LDS-rich and lean; the refusals; bmpc.scenarios.quadruped_population.
"""
import ctypes as C
import types

import numpy as np
import pytest

import hostbuild
import scene_common as SC
from bmpc import abi
from bmpc.scenarios import (quad_scene, quadruped_desc, quadruped_policy_rows, seeded_quadruped_batch,
                            seeded_quadruped_goals)
from common import golden

NAME = "quadruped_scene"


def fixture_desc(g, N=None, NB=2):
    return quadruped_desc(N=int(g["N"]) if N is None else N, NB=NB, dt=float(g["dt"]), L1=float(g["L1"]),
                          W1=float(g["W1"]), L2=float(g["L2"]), W2=float(g["W2"]), col_tol=float(g["col_tol"]))


def scene_env(g):
    return abi.make_quad_env(float(g["switch_clearance"]), float(g["lookahead"]), float(g["near"]))


def host_env_step(g, t, scene, upred=None, J=None, status=None, iters=None, stats=None):
    """k_env_quad on the host: advances `scene` [B][16] in place; returns x, z, xref."""
    desc = fixture_desc(g)
    sc = types.SimpleNamespace(kind="quadruped", n=3, env=scene_env(g), desc=desc, mc=np.array(desc.mc[:8], float))
    pol = abi.policy_array(quadruped_policy_rows(scene.shape[0], float(g["v0"])))
    return SC.host_step(sc, t, scene, pol, upred, solve=(J, status, iters, stats))


def check_scene_step(g, t, scene, x, z, xref):
    """One teacher-forced step of the fixture's scenes (the first rows of the batch) against it."""
    S = len(g["x"])
    for got, key in ((x, "x"), (z, "z"), (xref, "xRef")):
        np.testing.assert_allclose(got[:S], g[key][:, t], rtol=0, atol=1e-9, err_msg=f"{key} step {t}")
    np.testing.assert_array_equal(scene[:S, abi.ENV_OBSPOL], g["choice"][:, t], err_msg=f"backup choice step {t}")
    # the stored input is the chosen backup's: forward(v0) or stop
    np.testing.assert_array_equal(scene[:S, abi.QENV_UOBS:abi.QENV_UOBS + 3],
                                  np.where(g["choice"][:, t, None] == 0, [float(g["v0"]), 0, 0], 0.0))
    np.testing.assert_array_equal(scene[:S, abi.QENV_XDES:abi.QENV_XDES + 3], g["x_des"])
    assert np.all(scene[:, abi.ENV_COLL] == 0.0) and np.all(scene[:, abi.ENV_STEPS] == t + 1), t


def forced_inputs(g, t, B):
    """uPred[0] rows of the batch before step t: the scripts for the fixture's scenes, rest for padding."""
    if t == 0:
        return None
    up = np.zeros((B, 3))
    up[:len(g["x"])] = g["script"][:, t - 1]
    return up


def test_fixture_reaches_every_rule():
    g = golden(NAME)
    S, T = g["choice"].shape
    assert (S, T) == (6, 30) and g["x"].shape == g["z"].shape == g["xRef"].shape == (S, T, 3)
    c, hi = g["choice"], g["hi"]
    keep0 = hi[:, :, 0] > 0.5
    assert np.array_equal(c, np.where(keep0, 0, np.argmax(hi, axis=2)))
    assert (c[keep0] == 0).any() and (c[~keep0] == 1).any() and (c[~keep0] == 0).any()
    assert any(((c[s, :-1] == 1) & (c[s, 1:] == 0)).any() for s in range(S))      # a return to 0
    full = np.linalg.norm(g["x_des"][:, None, 0:2] - g["x"][:, :, 0:2], axis=2)
    ahead = np.linalg.norm(g["xRef"][:, :, 0:2] - g["x"][:, :, 0:2], axis=2)
    assert (full > 5).any() and (full < 5).any() and np.all(ahead <= 5 + 1e-12)
    own = ahead <= 0.1
    assert own.any() and np.array_equal(g["xRef"][:, :, 2][own], g["x"][:, :, 2][own])
    raw = np.arctan2(*(g["xRef"][:, :, k] - g["x"][:, :, k] for k in (1, 0))) - g["x_des"][:, None, 2]
    assert (raw[~own] > np.pi).any() and (raw[~own] < -np.pi).any() and (np.abs(raw[~own]) < np.pi).any()
    assert np.all(np.abs(g["xRef"][:, :, 2] - g["x_des"][:, None, 2])[~own] <= np.pi)


def test_quad_env_desc_layout_matches_header(tmp_path):
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("%zu %zu %zu\\n", sizeof(bmpc_quad_env_desc), offsetof(bmpc_quad_env_desc, lookahead),'
            ' offsetof(bmpc_quad_env_desc, near));return 0;}\n')
    size, a, b = hostbuild.header_program(tmp_path, code)
    D = abi.QuadEnvDesc
    assert (size, a, b) == (C.sizeof(D), D.lookahead.offset, D.near.offset)


def test_host_scene_replays_fixture():
    g = golden(NAME)
    scene = quad_scene(g["x"][:, 0], g["z"][:, 0], g["x_des"])
    for t in range(g["x"].shape[1]):
        out = host_env_step(g, t, scene, forced_inputs(g, t, len(scene)))
        check_scene_step(g, t, scene, *out)


def test_host_scene_statistics():
    """The statistics read an OSQP-class status: 1 is solved, anything else is booked infeasible."""
    g = golden(NAME)
    B = 3
    scene = quad_scene(g["x"][:B, 0], g["z"][:B, 0], g["x_des"][:B])
    stats = np.zeros((B, abi.ENV_NSTAT))
    J = np.array([1.0, 2.0, 3.0])
    st = np.array([1, -2, 0], np.int32)
    it = np.array([20, 21, 22], np.int32)
    host_env_step(g, 0, scene, None, J, st, it, stats)
    assert not stats.any()                      # t = 0: no solve yet
    host_env_step(g, 1, scene, np.zeros((B, 3)), J, st, it, stats)
    np.testing.assert_array_equal(stats[:, abi.ENVS_J], J)
    np.testing.assert_array_equal(stats[:, abi.ENVS_J2], J * J)
    np.testing.assert_array_equal(stats[:, abi.ENVS_INFEAS], [0, 1, 1])
    np.testing.assert_array_equal(stats[:, abi.ENVS_ITERS], it)
    np.testing.assert_array_equal(stats[:, abi.ENVS_SOLVES], 1)
    assert not stats[:, abi.ENVS_COLL_STEPS:].any()    # the scene has no collision rule


class OracleRollouts:
    """What quadruped_env.Quad_env touches of a predictive model, with the rollouts of the CPU oracle
    (oracle.model.QuadrupedModel, pinned to the reference's model by tests/test_oracle_model.py) in
    place of the package's GPU zpred_eval."""

    def __init__(self, g):
        from oracle.model import QuadrupedModel, quadruped_policies
        from quadruped_branch_dyn import backup_forward, backup_stop
        v0 = float(g["v0"])
        self.n, self.dt, self.N = 3, float(g["dt"]), int(g["N"])
        self.cons = types.SimpleNamespace(**{k: float(g[k]) for k in ("L1", "W1", "L2", "W2", "col_tol")})
        self.backupcons = [lambda x: backup_forward(x, v0), lambda x: backup_stop(x)]
        self._m = QuadrupedModel(self.N, self.dt, quadruped_policies(v0), self.cons.L1, self.cons.W1, self.cons.L2,
                                 self.cons.W2, self.cons.col_tol)

    def zpred_eval(self, z):
        return np.stack([self._m.zpred_eval(row) for row in np.atleast_2d(z)])


class ScriptedMPC:
    """The controller Quad_env.step sees: solve records its arguments and answers with `next_u`."""

    def __init__(self, model):
        self.predictiveModel, self.N = model, model.N
        self.calls, self.uPred, self.next_u = [], None, np.zeros(3)

    def solve(self, x, z, xRef):
        self.calls.append([np.array(v, float).copy() for v in (x, z, xRef)])
        self.uPred = np.array([self.next_u], float)

    def BT2array(self):
        return None, None, None, None


def compat_env(g, x, z, x_des):
    import quadruped_env
    env = quadruped_env.Quad_env(NR=2, mpc=ScriptedMPC(OracleRollouts(g)), x_des=np.array(x_des, float))
    env.robot_set[0].state = np.array(x, float)
    env.robot_set[1].state = np.array(z, float)
    return env


def test_compat_scene_replays_fixture():
    """The package's quadruped_env.Quad_env.step (the host restatement the drop-in main runs) on the
    same data: x / z / xRef as handed to the controller, and the obstacle's backup index."""
    g = golden(NAME)
    for s in range(len(g["x"])):
        env = compat_env(g, g["x"][s, 0], g["z"][s, 0], g["x_des"][s])
        for t in range(g["x"].shape[1]):
            env.mpc.next_u = g["script"][s, t]
            env.step(t)
            for got, key in zip(env.mpc.calls[-1], ("x", "z", "xRef")):
                np.testing.assert_allclose(got, g[key][s, t], rtol=0, atol=1e-9, err_msg=f"{key} scene {s} step {t}")
            assert env.robot_set[1].backupidx == g["choice"][s, t], (s, t)


# ---- GPU ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from bmpc import plan
    plan.context(0)
    return plan


class DeviceLoop:
    """A quadruped plan with the device buffers of the closed loop."""

    def __init__(self, plan, g, desc, x, z, x_des):
        import torch
        self.torch = torch
        B = self.B = len(x)
        self.env = scene_env(g)
        self.pl = pl = plan.BatchPlan(desc, B)
        pl.set_policies(quadruped_policy_rows(B, float(g["v0"])))
        dev = torch.device("cuda", 0)
        f64 = dict(dtype=torch.float64, device=dev)
        self.scene = torch.tensor(quad_scene(x, z, x_des), **f64)
        self.up = torch.zeros((B, pl.U, 3), **f64)
        self.J = torch.zeros(B, **f64)
        self.st = torch.zeros(B, dtype=torch.int32, device=dev)
        self.it = torch.zeros(B, dtype=torch.int32, device=dev)
        self.stats = torch.zeros((B, abi.ENV_NSTAT), **f64)
        self.x, self.z, self.xref = (torch.zeros((B, 3), **f64) for _ in range(3))
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream(dev)
        self.t = 0

    def _ptrs(self, *names):
        return [getattr(self, n).data_ptr() for n in names]

    def env_step(self):
        self.pl.quad_env_step_device(self.env, self.t,
                                     *self._ptrs("scene", "up", "x", "z", "xref", "J", "st", "it", "stats"),
                                     stream=self.stream.cuda_stream)
        self.t += 1

    def solve(self):
        self.pl.solve_device(*self._ptrs("x", "z", "xref", "up"), None, None, *self._ptrs("J", "st", "it"),
                             self.stream.cuda_stream)

    def loop(self, n):
        self.pl.quad_loop_device(self.env, self.t, n,
                                 *self._ptrs("scene", "up", "x", "z", "xref", "J", "st", "it", "stats"),
                                 self.stream.cuda_stream)
        self.t += n

    def sync(self):
        self.stream.synchronize()

    def host(self, *names):
        self.sync()
        out = [getattr(self, n).cpu().numpy().copy() for n in names]
        return out[0] if len(out) == 1 else out


@pytest.mark.gpu
def test_gpu_scene_replays_fixture(gpu):
    """k_env_quad, teacher-forced with the scripts: the 6 scenes and 59 seeded egos at rest, a batch
    of 65 (two thread blocks, the second with one ego)."""
    g = golden(NAME)
    S, B = len(g["x"]), 65
    px, pz, _ = seeded_quadruped_batch(B - S, seed=3)
    d = DeviceLoop(gpu, g, fixture_desc(g), np.concatenate([g["x"][:, 0], px]), np.concatenate([g["z"][:, 0], pz]),
                   np.concatenate([g["x_des"], seeded_quadruped_goals(B - S, seed=3)]))
    for t in range(g["x"].shape[1]):
        if t > 0:
            d.up[:, 0] = d.torch.tensor(forced_inputs(g, t, B), device=d.up.device)
            d.torch.cuda.synchronize()
        d.env_step()
        scene, x, z, xref = d.host("scene", "x", "z", "xref")
        check_scene_step(g, t, scene, x, z, xref)
        assert np.all(np.isfinite(scene)) and np.all(np.isfinite(xref))
        np.testing.assert_array_equal(x[S:], px)          # the padding egos rest; their obstacles may walk
        np.testing.assert_array_equal(x, scene[:, abi.QENV_X:abi.QENV_X + 3])
        np.testing.assert_array_equal(z, scene[:, abi.QENV_Z:abi.QENV_Z + 3])


@pytest.mark.gpu
def test_gpu_lockstep_closed_loop(gpu):
    """main_quadruped's ego, N=25, NB=2, BranchMPCProx, 10 steps: the device scene step feeds
    solve_device; the host Quad_env, advanced with the device's u, sees the same x / z / xRef (1e-9)
    and makes the same choice.  While the rule keeps the obstacle on backup 0 the loop is the one
    quadruped_n25_nb2 recorded (its obstacle walks forward on every step): uPred[0] to 1e-6, the bar
    of tests/test_compat_quad_gpu.py."""
    from common import quadruped_desc_from_golden
    g, rec = golden(NAME), golden("quadruped_n25_nb2")
    x0, z0, x_des = rec["traj_x"][0], rec["traj_z"][0], [5., -3., 0.]
    d = DeviceLoop(gpu, g, quadruped_desc_from_golden(rec), x0[None], z0[None], [x_des])
    env = compat_env(g, x0, z0, x_des)
    choices, us = [], []
    for t in range(10):
        d.env_step()
        d.solve()
        scene, x, z, xref, up, st = d.host("scene", "x", "z", "xref", "up", "st")
        assert st[0] == 1, (t, st)
        env.mpc.next_u = up[0, 0]
        env.step(t)
        for got, want, key in zip((x, z, xref), env.mpc.calls[-1], ("x", "z", "xRef")):
            np.testing.assert_allclose(got[0], want, rtol=0, atol=1e-9, err_msg=f"{key} step {t}")
        assert scene[0, abi.ENV_OBSPOL] == env.robot_set[1].backupidx, t
        choices.append(int(scene[0, abi.ENV_OBSPOL])), us.append(up[0, 0])
    on_record = choices.index(1) if 1 in choices else len(choices)   # steps whose inputs are the recording's
    print("backup choices", choices, "|du| vs the recording",
          np.abs(np.array(us) - rec["traj_u"][:10]).max(axis=1)[:on_record + 1])
    assert on_record >= 2, choices
    np.testing.assert_allclose(np.array(us)[:on_record], rec["traj_u"][:on_record], rtol=0, atol=1e-6)


def loop_batch(B, seed=4):
    x, z, _ = seeded_quadruped_batch(B, seed)
    return x, z, seeded_quadruped_goals(B, seed)


def _run(gpu, g, chunks, monkeypatch, rich, fused_env=None, B=300, N=None):
    """rich: BMPC_LDS_RICH for the run (None: unset, the executor chooses)."""
    for k in ("BMPC_BLOCK_EGOS", "BMPC_LDS_RICH", "BMPC_LOOP_FUSED"):
        monkeypatch.delenv(k, raising=False)
    if rich is not None:
        monkeypatch.setenv("BMPC_LDS_RICH", "1" if rich else "0")
    if fused_env is not None:
        monkeypatch.setenv("BMPC_LOOP_FUSED", fused_env)
    d = DeviceLoop(gpu, g, fixture_desc(g, N), *loop_batch(B))
    kernels, per_step = [], []
    for c in chunks:
        if c == "step":   # one step as its launches
            d.env_step()
            d.solve()
            per_step.append(d.host("st", "J"))
        else:
            d.loop(c)
        d.sync()
        kernels.append(d.pl.last_kernel())
    keys = ("scene", "up", "J", "st", "it", "stats", "x", "z", "xref")
    out = dict(zip(keys, d.host(*keys)))
    out["ws"] = d.pl.get_warm_start()
    return out, kernels, per_step


def _same(a, b):
    for k in a:
        if k == "ws":
            for kk in a[k]:
                assert np.array_equal(a[k][kk], b[k][kk]), ("warm start", kk)
        else:
            assert np.array_equal(a[k], b[k]), k


def _not_between_failures(ref, steps):
    """Equality is not equality between failures: every solve solved, every step booked."""
    for t, (st, J) in enumerate(steps):
        assert np.all(st >= 0), (t, np.unique(st, return_counts=True))
        assert np.all(np.isfinite(J)), t
    assert np.all(ref["st"] >= 0) and np.all(ref["stats"][:, abi.ENVS_SOLVES] == 4)
    assert np.all(ref["scene"][:, abi.ENV_STEPS] == 5) and np.all(np.isfinite(ref["up"]))


@pytest.mark.gpu
@pytest.mark.parametrize("rich", [True, False], ids=["rich", "lean"])
def test_fused_quad_loop_equals_per_step_launches(gpu, monkeypatch, rich):
    """5 steps of 300 egos at N=25, NB=2: one k_loop launch, a loop split over calls, a loop after a
    per-step start and the per-step path of the same call all give the bits of 5 rounds of k_env_quad
    + k_tree + k_qp."""
    g = golden(NAME)
    k_qp, k_loop = (abi.KERNEL_QP_RICH, abi.KERNEL_LOOP_RICH) if rich else (abi.KERNEL_QP_LEAN, abi.KERNEL_LOOP_LEAN)
    ref, kr, steps = _run(gpu, g, ["step"] * 5, monkeypatch, rich)
    assert set(kr) == {k_qp}, kr
    _not_between_failures(ref, steps)
    print(f"obstacles stopped {int(ref['scene'][:, abi.ENV_OBSPOL].sum())} of 300, iterations "
          f"{ref['it'].min()}-{ref['it'].max()}")
    fused, kf, _ = _run(gpu, g, [5], monkeypatch, rich)
    assert kf == [k_loop], kf
    _same(ref, fused)
    split, ks, _ = _run(gpu, g, [2, 3], monkeypatch, rich)          # a loop continued over calls
    assert ks == [k_loop] * 2, ks
    _same(ref, split)
    mixed, km, _ = _run(gpu, g, ["step", 4], monkeypatch, rich)       # t0 > 0 after a per-step start
    assert km == [k_qp, k_loop], km
    _same(ref, mixed)
    per, kp, _ = _run(gpu, g, [5], monkeypatch, rich, fused_env="0")   # the per-step path of the same call
    assert kp == [k_qp], kp
    _same(ref, per)


@pytest.mark.gpu
def test_fused_quad_loop_one_ego_short_tree(gpu, monkeypatch):
    """Batch 1, N=6, NB=2, the executor's own LDS choice (rich): OSQP-class plans have no small-batch
    kernel, so one ego fuses too."""
    g = golden(NAME)
    ref, kr, steps = _run(gpu, g, ["step"] * 5, monkeypatch, None, B=1, N=6)
    assert set(kr) == {abi.KERNEL_QP_RICH}, kr
    _not_between_failures(ref, steps)
    fused, kf, _ = _run(gpu, g, [5], monkeypatch, None, B=1, N=6)
    assert kf == [abi.KERNEL_LOOP_RICH], kf
    _same(ref, fused)


@pytest.mark.gpu
def test_quad_scene_refusals(gpu):
    from bmpc.scenarios import highway_desc
    env = abi.make_quad_env()
    cvar = quadruped_desc(N=6, NB=1)
    cvar.controller = abi.CTRL_CVAR
    for desc in (highway_desc(N=8, NB=1), cvar):
        pl = gpu.BatchPlan(desc, 2)
        with pytest.raises(RuntimeError, match=r"\(-22\).*quadruped scene needs a QUADRUPED plan"):
            pl.quad_env_step_device(env, 0, 1, 1, 1, 1, 1)
        with pytest.raises(RuntimeError, match=r"\(-22\).*quadruped scene needs a QUADRUPED plan"):
            pl.quad_loop_device(env, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    pl = gpu.BatchPlan(quadruped_desc(N=6, NB=1), 2)
    with pytest.raises(RuntimeError, match=r"\(-22\).*t >= 0"):
        pl.quad_env_step_device(env, -1, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*needs the last uPred"):
        pl.quad_env_step_device(env, 1, 1, None, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*nsteps >= 1"):
        pl.quad_loop_device(env, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*t0 >= 0"):
        pl.quad_loop_device(env, -1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*overtake scene"):   # the overtake loop still refuses it
        pl.loop_device(abi.make_env(), 0, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*no merge scene"):   # ... and the merge loop
        pl.merge_loop_device(0, 1, 1, 1, 1, 1, 1, 1, 1, 1)


@pytest.mark.gpu
def test_quadruped_population_runs_on_device(gpu):
    from bmpc.scenarios import quadruped_population
    stats, scene = quadruped_population(64, 4)
    assert stats.shape == (64, abi.ENV_NSTAT) and scene.shape == (64, abi.ENV_STRIDE)
    assert np.all(np.isfinite(stats)) and np.all(np.isfinite(scene))
    assert np.all(stats[:, abi.ENVS_SOLVES] == 3) and np.all(scene[:, abi.ENV_STEPS] == 4)
    np.testing.assert_array_equal(scene[:, abi.QENV_XDES:abi.QENV_XDES + 3], seeded_quadruped_goals(64, 0))
