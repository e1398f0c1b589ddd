"""Shared by tests/test_obstacle_proposal.py and tests/test_obstacle_proposal_gpu.py: the NumPy
restatement of the weighted obstacle modes' two rules -- the choice and the log-weight increment of every
epoch start from branch probabilities p at the recorded pre-step state (bmpc_set_obstacle_proposal; the
scenes and their host steps are tests/scene_common.py's, the margin rule obstacle_sampling_common's)."""
import ctypes as C

import numpy as np

import obstacle_sampling_common as S
import scene_common as SC
from bmpc import abi, rng

LOGW_TOL = 1e-9        # the project's host-versus-NumPy scene bar (tests/test_env_host.py)
TILTS = {"overtake": (1.0, 4.0, 0.25), "quadruped": (1.0, 5.0)}


def proposal(sc, tilt=None, script=None, epoch0=0):
    """(abi.ObstacleProposal, the int32 table it points at or None -- keep it alive) for a host run."""
    table = None if script is None else np.ascontiguousarray(script, np.int32)
    where = None if table is None else (table.ctypes.data, table.shape[1])
    return abi.make_obstacle_proposal(tilt, where, epoch0, m=sc.m), table


def host_weights(sc, pol, x, z):
    """The model weights w [B, m] the scene rule forms at (x, z) [B, n] under the policy array `pol`."""
    B = len(x)
    w = np.zeros((B, sc.m))
    SC.shim().op_weights(0 if sc.kind == "overtake" else 1, SC._p(sc.mc), C.c_double(sc.desc.dt), sc.desc.N, sc.m, B, pol,
                      SC._p(np.ascontiguousarray(x)), SC._p(np.ascontiguousarray(z)), SC._p(w))
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
