"""Shared by tests/test_obstacle_proposal.py and tests/test_obstacle_proposal_gpu.py: the host build of
the weighted obstacle modes (tests/hostsim/obstacle_proposal_host.cpp), teacher-forced host runs of the
two scenes with a sampler and a proposal, and the NumPy restatement of the two rules -- the choice and
the log-weight increment of every epoch start from branch probabilities p at the recorded pre-step
state (bmpc_set_obstacle_proposal; the scenes and the margin rule are obstacle_sampling_common's)."""
import ctypes as C
import os
import subprocess

import numpy as np

import obstacle_sampling_common as S
from bmpc import abi, rng
from common import HERE, PKG, REPO

SRC = os.path.join(HERE, "hostsim", "obstacle_proposal_host.cpp")
SO = os.path.join(HERE, "hostsim", "libbmpc_hostsim_obstacle_proposal.so")
LOGW_TOL = 1e-9        # the project's host-versus-NumPy scene bar (tests/test_env_host.py)
TILTS = {"overtake": (1.0, 4.0, 0.25), "quadruped": (1.0, 5.0)}
_shim = None


def shim():
    """The shared-library build of the host file, rebuilt when a source it is compiled from is newer."""
    global _shim
    if _shim is None:
        deps = [SRC, os.path.join(REPO, "include", "bmpc.h")] + [
            os.path.join(PKG, "csrc", f) for f in ("bmpc_rng.h", "bmpc_env_quad.h", "bmpc_env.h", "bmpc_model.h",
                                                   "bmpc_core.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            tmp = SO + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", *S.INCLUDES,
                                   SRC, "-o", tmp])
            os.replace(tmp, SO)
        _shim = C.CDLL(SO)
    return _shim


def proposal(sc, tilt=None, script=None, epoch0=0):
    """(abi.ObstacleProposal, the int32 table it points at or None -- keep it alive) for a host run."""
    table = None if script is None else np.ascontiguousarray(script, np.int32)
    where = None if table is None else (table.ctypes.data, table.shape[1])
    return abi.make_obstacle_proposal(tilt, where, epoch0, m=sc.m), table


def host_step(sc, t, scene, pol, u0, smp, prop):
    """k_env / k_env_quad on the host with a sampler and a proposal: advances `scene` (and the overtake
    `pol`) in place; x, z, xref."""
    B, n = scene.shape[0], sc.n
    x, z, xref = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
    up = None if u0 is None else np.ascontiguousarray(np.asarray(u0, float).reshape(B, -1))
    fn = shim().op_env_step if sc.kind == "overtake" else shim().op_quad_env_step
    rc = fn(C.byref(sc.env), S._p(sc.mc), C.c_double(sc.desc.dt), sc.desc.N, sc.desc.m, int(t), B, S._p(scene), pol,
            S._p(up), 0 if up is None else up.shape[1], S._p(x), S._p(z), S._p(xref),
            None if smp is None else C.byref(smp), None if prop is None else C.byref(prop))
    assert rc == 0
    return x, z, xref


def host_run(sc, smp, prop, steps, t0=0, egos=None, same_input=False):
    """`steps` teacher-forced host steps t0 .. t0 + steps - 1 from the scene's initial rows (`egos`: an
    index array or slice of them; same_input: every ego gets ego 0's scripted input, so that egos
    from one state differ by the obstacle's choices alone).  Per step: the scene rows after it, the
    step's x / z outputs -- the choice's pre-step state -- and the policies in force before it."""
    sel = slice(None) if egos is None else egos
    scene = np.ascontiguousarray(sc.scene0[sel]).copy()
    ids = np.arange(sc.B)[sel]
    pol = abi.policy_array([sc.rows[i] for i in ids])
    out = []
    for t in range(t0, t0 + steps):
        before = S.copy_policies(pol)
        u0 = None if t == 0 else sc.script(t, np.zeros(len(ids)) if same_input else ids)
        x, z, _ = host_step(sc, t, scene, pol, u0, smp, prop)
        out.append(dict(scene=scene.copy(), x=x, z=z, pol=before))
    return out


def host_weights(sc, pol, x, z):
    """The model weights w [B, m] the scene rule forms at (x, z) [B, n] under the policy array `pol`."""
    B = len(x)
    w = np.zeros((B, sc.m))
    shim().op_weights(0 if sc.kind == "overtake" else 1, S._p(sc.mc), C.c_double(sc.desc.dt), sc.desc.N, sc.m, B, pol,
                      S._p(np.ascontiguousarray(x)), S._p(np.ascontiguousarray(z)), S._p(w))
    return w


def oracle_probabilities(sc, run):
    """p_at for check_weighted from a host run: oracle.model's branch_eval at every recorded pre-step
    state under the policies in force before the step."""
    return lambda r: np.stack([sc.oracle_p(run[r]["pol"], e, run[r]["x"][e], run[r]["z"][e])
                               for e in range(len(run[r]["x"]))])


def check_weighted(smp, m, scenes, p_at, tilt=None, script=None, epoch0=0, t0=0, ego_base=0, logw0=0.0):
    """The rule of every choice and log-weight of recorded scene rows [B, T, ENV_STRIDE] of steps
    t0 .. t0 + T - 1 in mode "tilted" (tilt given) or "script" (script [B, E] given), from branch
    probabilities p_at(r) [B, m] at row r's pre-step state.

    Epoch starts: the tilted choice is bmpc.rng's inverse CDF of p b / sum(p b) at the draw of
    (seed, ego_base + e, t // hold) and adds log(sum(p b) / b_j); the scripted one is the table's entry
    clamped to a policy and adds log p_j.  A tilted decision whose u lies within MARGIN of a partial sum
    is not compared -- the running sum then follows the recorded choice --, at most MAX_LEFT_OUT of them.
    ENV_LOGW after every step equals the running sum (from logw0) within LOGW_TOL; inside an epoch
    choice and weight are the previous row's.  Returns (compared decisions, the running sum [B])."""
    scenes = np.asarray(scenes)
    B, T = scenes.shape[:2]
    logw = np.full(B, float(logw0))
    rows = np.arange(B)
    left_out = draws = 0
    for r in range(T):
        t = t0 + r
        c = scenes[:, r, abi.ENV_OBSPOL].astype(int)
        assert np.all((c >= 0) & (c < m))
        if t % smp.hold:
            if r > 0:
                np.testing.assert_array_equal(c, scenes[:, r - 1, abi.ENV_OBSPOL], err_msg=f"step {t} inside an epoch")
                np.testing.assert_array_equal(scenes[:, r, abi.ENV_LOGW], scenes[:, r - 1, abi.ENV_LOGW])
            continue
        p = np.asarray(p_at(r))
        np.testing.assert_allclose(p.sum(-1), 1.0, rtol=0, atol=1e-12)
        if script is not None:
            want = np.clip(np.asarray(script)[:, t // smp.hold - epoch0], 0, m - 1)
            np.testing.assert_array_equal(c, want, err_msg=f"epoch start {t}")
            inc = np.log(p[rows, c])
        else:
            b = np.asarray(tilt, float)
            pb = p * b
            u = rng.obstacle_uniform(smp.seed, ego_base + rows, t // smp.hold)
            want, sure = S.expected_choice(pb / pb.sum(-1, keepdims=True), u)
            draws += B
            left_out += int((~sure).sum())
            np.testing.assert_array_equal(c[sure], want[sure], err_msg=f"epoch start {t}")
            inc = np.log(pb.sum(-1) / b[c])
        logw += inc
        np.testing.assert_allclose(scenes[:, r, abi.ENV_LOGW], logw, rtol=0, atol=LOGW_TOL, err_msg=f"log-weight, step {t}")
    assert left_out <= S.MAX_LEFT_OUT * max(draws, 1), (left_out, draws)
    return draws - left_out, logw


def numpy_left_out(smp, p_at, tilt, T, ego_base=0, t0=0):
    """The NumPy side alone: how many of a tilted run's decisions lie within MARGIN of a partial sum."""
    n = total = 0
    for r in range(T):
        if (t0 + r) % smp.hold:
            continue
        pb = np.asarray(p_at(r)) * np.asarray(tilt, float)
        u = rng.obstacle_uniform(smp.seed, ego_base + np.arange(len(pb)), (t0 + r) // smp.hold)
        n += int((~S.expected_choice(pb / pb.sum(-1, keepdims=True), u)[1]).sum())
        total += len(pb)
    return n, total
