"""The merge scene's closed loop (csrc/bmpc_env_merge.h; bmpc_merge_env_step, bmpc_merge_loop_device)
against the reference's own recording of main_branch.sim_merge, ``tests/golden/merge_n40_nb1.npz``.

The recording is exactly self-consistent with the scene's rules (Highway_env_branch.py:317-380):
traj_x[t+1] from traj_x[t] and traj_u[t], traj_z from traj_obs_u, traj_obs_u from the main-road
backup 0, traj_S / traj_xRef / traj_bx from refX / refY / refpsi.  The ego leaves the ramp at step 19.

Host build (not gpu): the scene function itself, compiled with g++ (tests/hostsim/scene_host.cpp),
driven through all 60 recorded steps with the recorded inputs; bar 1e-9 as tests/test_env_host.py
(tan / cos / sin of a different libm), the obstacle's input 1e-12.

GPU: the same drive through k_env_merge with the transform slots read back; one solve per recorded
step fed by the device scene alone (no set_transform) under test_merge.check_merge_replay; the fused
k_loop against the per-step launches bit for bit, LDS-rich and lean; a free run against the recording;
the refusals.
"""
import ctypes as C
import types

import numpy as np
import pytest

import hostbuild
import scene_common as SC
from bmpc import abi
from bmpc.scenarios import _overtake_scene as new_scene
from bmpc.scenarios import merge_desc, merge_lane_ref, merge_policy_rows
from common import golden
from test_merge import NAME, check_merge_replay, replay_inputs
from test_merge import merge_desc as golden_merge_desc


def scene_env(g):
    return abi.make_merge_env(n_lane=int(g["N_lane"]), merge_lane=1, merge_s=50.0, W=float(g["W"]),
                              Kpsi=float(g["Kpsi"]), v0=float(g["v0"]), psimax=float(g["bx"][2]))


def host_env_step(g, t, scene, upred=None, J=None, status=None, iters=None, stats=None, dt=0.1):
    """k_env_merge on the host: advances `scene` [B][16] in place; returns x, z, xref, S, bx."""
    ref = np.ascontiguousarray(np.concatenate([g["refX"], g["refY"], g["refpsi"]]).astype(float))
    sc = types.SimpleNamespace(kind="merge", n=4, env=scene_env(g), desc=types.SimpleNamespace(dt=dt), ref=ref,
                               bx=np.ascontiguousarray(np.asarray(g["bx"], float)))
    return SC.host_step(sc, t, scene, None, upred, solve=(J, status, iters, stats))


def check_scene_step(g, t, scene, x, z, xref, S, bx):
    """One teacher-forced step against the recording (the bars of the module docstring)."""
    for got, key in ((x, "traj_x"), (z, "traj_z"), (xref, "traj_xRef"), (S, "traj_S"), (bx, "traj_bx")):
        np.testing.assert_allclose(got[0], g[key][t], rtol=0, atol=1e-9, err_msg=f"{key} step {t}")
    np.testing.assert_allclose(scene[0, abi.ENV_UOBS:abi.ENV_UOBS + 2], g["traj_obs_u"][t], rtol=0, atol=1e-12,
                               err_msg=f"obstacle input step {t}")
    assert scene[0, abi.ENV_MERGED] == 1 - int(g["traj_laneID"][t]), t
    assert scene[0, abi.ENV_COLL] == 0.0, t
    assert scene[0, abi.ENV_STEPS] == t + 1 and scene[0, abi.ENV_OBSPOL] == 0.0


def test_scenario_matches_recording():
    """bmpc.scenarios' sim_merge set-up is the recorded one: plan description, policies, ramp."""
    g = golden(NAME)
    assert bytes(merge_desc()) == bytes(golden_merge_desc(g))
    assert merge_policy_rows(1) == [[(abi.POL_MAINTAIN_TRACKV, (float(g["Kpsi"]), float(g["v0"]))),
                                     (abi.POL_BRAKE, (float(g["Kpsi"]),))]]
    for got, key in zip(merge_lane_ref(), ("refX", "refY", "refpsi")):
        np.testing.assert_allclose(got, g[key], rtol=0, atol=1e-12)
    assert bytes(abi.make_merge_env()) == bytes(scene_env(g))


def test_merge_env_desc_layout_matches_header(tmp_path):
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("%zu %zu %zu %zu\\n", sizeof(bmpc_merge_env_desc), offsetof(bmpc_merge_env_desc, merge_s),'
            ' offsetof(bmpc_merge_env_desc, psimax), offsetof(bmpc_merge_env_desc, vwid));return 0;}\n')
    size, a, b, c = hostbuild.header_program(tmp_path, code)
    D = abi.MergeEnvDesc
    assert (size, a, b, c) == (C.sizeof(D), D.merge_s.offset, D.psimax.offset, D.vwid.offset)


def test_host_scene_replays_recording():
    g = golden(NAME)
    T = len(g["traj_x"])
    assert T == 60 and list(g["traj_laneID"]).index(0) == 19
    scene = new_scene(g["traj_x"][0], g["traj_z"][0])
    for t in range(T):
        up = None if t == 0 else np.asarray(g["traj_u"][t - 1], float)[None]
        out = host_env_step(g, t, scene, up)
        check_scene_step(g, t, scene, *out)
    # the recorded minimum clearance is +1.21 m: far from the flag's threshold
    clear = np.maximum(np.abs(g["traj_x"][:, 0] - g["traj_z"][:, 0]) - 4.0, np.abs(g["traj_x"][:, 1] - g["traj_z"][:, 1]) - 2.4)
    assert abs(clear.min() - 1.21) < 0.01


def test_host_scene_collision_flag_is_sticky():
    g = golden(NAME)
    scene = new_scene([[30, 5.4, 20, 0], [30, 5.4, 20, 0]], [[32, 5.4, 20, 0], [40, 5.4, 20, 0]])
    host_env_step(g, 0, scene)
    assert list(scene[:, abi.ENV_COLL]) == [1.0, 0.0]
    scene[0, abi.ENV_Z] = 80.0          # apart again: the flag stays
    host_env_step(g, 1, scene, np.zeros((2, 2)))
    assert list(scene[:, abi.ENV_COLL]) == [1.0, 0.0]


def test_host_scene_statistics():
    g = golden(NAME)
    B = 3
    scene = new_scene(np.repeat(g["traj_x"][:1], B, 0), np.repeat(g["traj_z"][:1], B, 0))
    stats = np.zeros((B, abi.ENV_NSTAT))
    J = np.array([1.0, 2.0, 3.0])
    st = np.array([0, -1, 10], np.int32)
    it = np.array([20, 21, 22], np.int32)
    host_env_step(g, 0, scene, None, J, st, it, stats)
    assert not stats.any()                      # t = 0: no solve yet
    host_env_step(g, 1, scene, np.zeros((B, 2)), J, st, it, stats)
    np.testing.assert_array_equal(stats[:, abi.ENVS_J], J)
    np.testing.assert_array_equal(stats[:, abi.ENVS_J2], J * J)
    np.testing.assert_array_equal(stats[:, abi.ENVS_INFEAS], [0, 1, 0])   # ECOS: exitFlag >= 0 feasible
    np.testing.assert_array_equal(stats[:, abi.ENVS_ITERS], it)
    np.testing.assert_array_equal(stats[:, abi.ENVS_SOLVES], 1)


def host_loop(g, x, z, steps):
    """The closed loop on the host build: scene step -> transform slots -> solve, per step.
    Returns per-step uPred[0], status, iters, J and the final scene."""
    import hostsim_lib as H
    B = len(x)
    hs = H.HostSim(golden_merge_desc(g), B)
    hs.set_policies(merge_policy_rows(B, float(g["Kpsi"]), float(g["v0"])))
    scene = new_scene(x, z)
    rec = dict(u=[], status=[], iters=[], J=[])
    r = None
    for t in range(steps):
        xs, zs, xr, S, bx = host_env_step(g, t, scene, None if r is None else r["upred"][:, 0])
        hs.set_transform(S, bx)
        r = hs.solve(xs, zs, xr)
        for k, v in (("u", r["upred"][:, 0]), ("status", r["status"]), ("iters", r["iters"]), ("J", r["J"])):
            rec[k].append(v.copy())
    return {k: np.array(v) for k, v in rec.items()}, scene


def test_host_free_run_follows_recording():
    """Three closed-loop steps of the recorded ego on the host build: the scene feeds the solver
    the recorded problem at step 0 (uPred[0] to the replay bar 1e-5; the host build's 1e-6 of
    tests/test_dropin_mains.py holds too) and the loop stays on the recording."""
    g = golden(NAME)
    rec, scene = host_loop(g, g["traj_x"][:1], g["traj_z"][:1], 3)
    assert np.all(rec["status"] >= 0)
    dev = np.abs(rec["u"][:, 0] - g["traj_u"][:3]).max(axis=1)
    print("host free run |du| per step:", dev)
    assert dev[0] <= 1e-6 and dev[1] <= 1e-6 and dev[2] <= 2e-2


# ---- GPU ---------------------------------------------------------------------------------------

def loop_batch(g, B=300):
    """The fused-loop batch: 236 egos around the recording's start, the rest around its steps
    14-19 (about to leave the ramp); ego 0 is the unperturbed recording."""
    rng = np.random.default_rng(7)
    src = np.array([0 if e < 236 else 14 + e % 6 for e in range(B)])
    x = np.asarray(g["traj_x"], float)[src].copy()
    z = np.asarray(g["traj_z"], float)[src].copy()
    x[1:] += rng.uniform(-1, 1, (B - 1, 4)) * [2, 0.2, 1, 0.02]
    z[1:] += rng.uniform(-1, 1, (B - 1, 4)) * [3, 0, 1, 0]
    return x, z


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from bmpc import plan
    plan.context(0)
    return plan


class DeviceLoop:
    """A merge plan with its scene and the device buffers of the closed loop."""

    def __init__(self, plan, g, x, z):
        import torch
        self.torch = torch
        B = self.B = len(x)
        self.pl = pl = plan.BatchPlan(golden_merge_desc(g), B)
        pl.set_policies(merge_policy_rows(B, float(g["Kpsi"]), float(g["v0"])))
        pl.set_merge_scene(scene_env(g), g["refX"], g["refY"], g["refpsi"])
        dev = torch.device("cuda", 0)
        f64 = dict(dtype=torch.float64, device=dev)
        self.scene = torch.tensor(new_scene(x, z), **f64)
        self.up = torch.zeros((B, pl.U, 2), **f64)
        self.J = torch.zeros(B, **f64)
        self.st = torch.zeros(B, dtype=torch.int32, device=dev)
        self.it = torch.zeros(B, dtype=torch.int32, device=dev)
        self.stats = torch.zeros((B, abi.ENV_NSTAT), **f64)
        self.x, self.z, self.xref = (torch.zeros((B, 4), **f64) for _ in range(3))
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream(dev)
        self.t = 0

    def _ptrs(self, *names):
        return [getattr(self, n).data_ptr() for n in names]

    def env_step(self):
        self.pl.merge_env_step_device(self.t, *self._ptrs("scene", "up", "x", "z", "xref", "J", "st", "it", "stats"),
                                      stream=self.stream.cuda_stream)
        self.t += 1

    def solve(self):
        self.pl.solve_device(*self._ptrs("x", "z", "xref", "up"), None, None, *self._ptrs("J", "st", "it"),
                             self.stream.cuda_stream)

    def loop(self, n):
        self.pl.merge_loop_device(self.t, n, *self._ptrs("scene", "up", "x", "z", "xref", "J", "st", "it", "stats"),
                                  self.stream.cuda_stream)
        self.t += n

    def sync(self):
        self.stream.synchronize()

    def host(self, *names):
        self.sync()
        out = [getattr(self, n).cpu().numpy().copy() for n in names]
        return out[0] if len(out) == 1 else out


@pytest.mark.gpu
def test_gpu_scene_replays_recording(gpu):
    """k_env_merge, teacher-forced with the recorded inputs; S / bx read back from the slab."""
    g = golden(NAME)
    d = DeviceLoop(gpu, g, g["traj_x"][:1], g["traj_z"][:1])
    for t in range(len(g["traj_x"])):
        if t > 0:
            d.up[0, 0] = d.torch.tensor(np.asarray(g["traj_u"][t - 1], float), device=d.up.device)
            d.torch.cuda.synchronize()
        d.env_step()
        scene, x, z, xref = d.host("scene", "x", "z", "xref")
        xf = d.pl.get_transform()
        assert xf["s_on"].all() and xf["bx_set"].all()
        check_scene_step(g, t, scene, x, z, xref, xf["S"], xf["bx"])


@pytest.mark.gpu
def test_gpu_solve_fed_by_device_scene(gpu, solver_path):
    """Every recorded step as one ego at scene time 0, with the recorded warm start: one scene
    step and one solve, no set_transform -- the S, bx and x_ref the kernel wrote reach the solver
    as the host path's do (test_merge.check_merge_replay, unchanged)."""
    from conftest import assert_solver_path
    g = golden(NAME)
    rb = replay_inputs(g)
    assert rb["T"] == 60
    d = DeviceLoop(gpu, g, rb["x"], rb["z"])
    d.pl.set_warm_start(rb["uLin"], rb["p"], rb["jcons"], mask=rb["warm"])
    d.env_step()
    d.solve()
    up, J, st = d.host("up", "J", "st")
    assert_solver_path(d.pl, solver_path)
    check_merge_replay(dict(status=st, J=J, upred=up), g, rb["T"])


def _run(gpu, g, chunks, monkeypatch, rich, fused_env=None):
    for k in ("BMPC_BLOCK_EGOS", "BMPC_LDS_RICH", "BMPC_LOOP_FUSED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BMPC_LDS_RICH", "1" if rich else "0")
    if fused_env is not None:
        monkeypatch.setenv("BMPC_LOOP_FUSED", fused_env)
    d = DeviceLoop(gpu, g, *loop_batch(g))
    kernels, per_step = [], []
    for c in chunks:
        if c == "step":   # one step as its launches
            d.env_step()
            d.solve()
            per_step.append(d.host("st", "J", "up"))
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


@pytest.mark.gpu
@pytest.mark.parametrize("rich", [True, False], ids=["rich", "lean"])
def test_fused_merge_loop_equals_per_step_launches(gpu, monkeypatch, rich):
    """5 steps of 300 egos: one k_loop launch, a loop split over calls, a loop after a per-step
    start and the per-step path of the same call all give the bits of 5 rounds of k_env_merge +
    k_tree + k_ipm.  Host build on exactly this batch: status >= 0 for 300/300 on all 5 steps, 295
    or more exit 0, 19-39 iterations, 53 egos merged after step 4, some perturbed egos collide."""
    g = golden(NAME)
    k_ipm, k_loop = (abi.KERNEL_IPM_RICH, abi.KERNEL_LOOP_RICH) if rich else (abi.KERNEL_IPM_LEAN, abi.KERNEL_LOOP_LEAN)
    ref, kr, steps = _run(gpu, g, ["step"] * 5, monkeypatch, rich)
    assert set(kr) == {k_ipm}, kr
    # guards against an empty pass
    for t, (st, J, up) in enumerate(steps):
        assert np.all(st >= 0), (t, st)
        assert np.all(np.isfinite(J)), t
    assert np.all(ref["stats"][:, abi.ENVS_SOLVES] == 4)
    merged = int(ref["scene"][:, abi.ENV_MERGED].sum())
    print(f"merged {merged}, collided {int(ref['scene'][:, abi.ENV_COLL].sum())}, iterations "
          f"{ref['it'].min()}-{ref['it'].max()}, |du0| ego 0 {np.abs(steps[0][2][0, 0] - g['traj_u'][0]).max():.2e}")
    assert merged >= 40
    np.testing.assert_allclose(steps[0][2][0, 0], g["traj_u"][0], rtol=0, atol=1e-5)
    fused, kf, _ = _run(gpu, g, [5], monkeypatch, rich)
    assert kf == [k_loop], kf
    _same(ref, fused)
    split, ks, _ = _run(gpu, g, [2, 3], monkeypatch, rich)          # a loop continued over calls
    assert ks == [k_loop] * 2, ks
    _same(ref, split)
    mixed, _, _ = _run(gpu, g, ["step", 4], monkeypatch, rich)        # t0 > 0 after a per-step start
    _same(ref, mixed)
    per, kp, _ = _run(gpu, g, [5], monkeypatch, rich, fused_env="0")   # the per-step path of the same call
    assert kp == [k_ipm], kp
    _same(ref, per)


@pytest.mark.gpu
def test_gpu_free_run_follows_recording(gpu):
    """One ego, 10 closed-loop steps from the recorded start, with the bars tests/test_dropin_mains.py
    derived for this scene (its :153-169): states 1e-2, inputs 2e-2, the obstacle 1e-9; step 0, a
    problem identical to the recording's, to the replay bar 1e-5.  Measured on an MI355X: |du| per
    step 9.2e-11, 4.2e-8, 2.0e-5, 2.8e-3, 7.0e-3, 9.4e-3, 3.4e-3, 3.5e-3, 7.8e-4, 2.5e-3; |dx| <= 2.6e-3."""
    g = golden(NAME)
    d = DeviceLoop(gpu, g, g["traj_x"][:1], g["traj_z"][:1])
    xs, zs, us = [], [], []
    for t in range(10):
        d.loop(1)
        x, z, up, st = d.host("x", "z", "up", "st")
        assert st[0] >= 0, (t, st)
        xs.append(x[0]), zs.append(z[0]), us.append(up[0, 0])
    xs, zs, us = map(np.array, (xs, zs, us))
    print("gpu free run |du| per step:", np.abs(us - g["traj_u"][:10]).max(axis=1))
    print("gpu free run |dx| per step:", np.abs(xs - g["traj_x"][:10]).max(axis=1))
    np.testing.assert_allclose(us[0], g["traj_u"][0], rtol=0, atol=1e-5)
    np.testing.assert_allclose(xs[1:], g["traj_x"][1:10], rtol=0, atol=1e-2)
    np.testing.assert_allclose(us, g["traj_u"][:10], rtol=0, atol=2e-2)
    np.testing.assert_allclose(zs, g["traj_z"][:10], rtol=0, atol=1e-9)


@pytest.mark.gpu
def test_merge_population_runs_on_device(gpu):
    from bmpc.scenarios import merge_population
    from bmpc.distributed import episode_stats, STAT_SOLVES
    stats, scene = merge_population(8, 3, seed=1)
    assert stats.shape == (8, abi.ENV_NSTAT) and scene.shape == (8, abi.ENV_STRIDE)
    assert np.all(scene[:, abi.ENV_STEPS] == 3) and np.all(stats[:, abi.ENVS_INFEAS] == 0)
    assert episode_stats(stats)[STAT_SOLVES] == 16


@pytest.mark.gpu
def test_merge_scene_refusals(gpu):
    from bmpc.scenarios import highway_desc, quadruped_desc
    g = golden(NAME)
    env, ref = scene_env(g), (g["refX"], g["refY"], g["refpsi"])
    pl = gpu.BatchPlan(golden_merge_desc(g), 2)
    with pytest.raises(RuntimeError, match=r"\(-22\).*no merge scene"):
        pl.merge_loop_device(0, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*no merge scene"):
        pl.merge_env_step_device(0, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match=r"\(-22\).*strictly increasing"):
        pl.set_merge_scene(env, ref[0][::-1], ref[1], ref[2])
    pl.set_merge_scene(env, *ref)
    with pytest.raises(RuntimeError, match=r"\(-22\).*overtake scene"):   # the overtake loop still refuses merge plans
        pl.loop_device(abi.make_env(), 0, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    for desc in (highway_desc(N=8, NB=1), quadruped_desc()):
        other = gpu.BatchPlan(desc, 2)
        with pytest.raises(RuntimeError, match=r"\(-22\).*HIGHWAY_MERGE"):
            other.set_merge_scene(env, *ref)
