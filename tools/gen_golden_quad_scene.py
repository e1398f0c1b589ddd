"""Record the reference's quadruped SCENE rules alone (run where the reference checkout is).

``tests/golden/quadruped_n25_nb2.npz`` moves the obstacle forward on every step, so it records
neither the obstacle's backup choice nor anything but one goal.  This generator drives the
reference's unmodified ``quadruped_env.Quad_env.step`` (``quadruped_env.py:67-130``) over the
reference's own ``quadruped_branch_dyn.PredictiveModel`` (``tools/gen_golden.py``'s loader: the
CasADi stand-in, the solver-package stubs) with a stub controller of ours in place of the MPC:
its ``solve`` records the (x, z, xRef) the scene hands it and answers with the next input of a
script, its ``BT2array`` returns three values so that the reference's ``:120`` unpack succeeds.
No MPC solve is involved: the fixture pins the scene rules.

Every decision of every recorded step must clear its boundary by MARGIN (a test cannot use a
step on which a rounding error decides), and the scenes together must reach every branch of the
rules; the generator fails otherwise.  Output: ``tests/golden/quadruped_scene.npz`` (numbers only).
Usage:  python tools/gen_golden_quad_scene.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402

N, DT, V0 = 25, 0.2, 0.2
L1, W1, L2, W2, COL_TOL = 0.5, 0.3, 1.0, 0.6, 0.2
SWITCH, LOOKAHEAD, NEAR = 0.5, 5.0, 0.1     # the literals of quadruped_env.py:98, :108, :110
STEPS = 30
MARGIN = 1e-6


def scripts():
    """(name, ego, obstacle, x_des, inputs [STEPS][3]) of every scene."""
    rng = np.random.default_rng(11)
    fwd, left, still = np.array([0.2, 0, 0]), np.array([0.05, 0, 0.5]), np.zeros(3)

    def seq(*parts):
        u = np.concatenate([np.repeat(np.asarray(v, float)[None], k, 0) for v, k in parts])
        assert u.shape == (STEPS, 3), u.shape
        return u

    bound = np.array([0.2, 0.1, 0.5])
    return [
        # main_quadruped's start: walks into the obstacle's path (choice 0 -> 1), then turns away (-> 0)
        ("main", [0, 1.8, 0], [2.5, 2.5, -np.pi / 2], [5., -3., 0.], seq((fwd, 8), (left, 22))),
        # goal behind the ego with x_des[2] = 3: atan2 - x_des[2] < -pi, the second wrap loop fires
        ("wrap_up", [0, 0, 2.0], [6, 6, 0.3], [-3., -1., 3.0], seq(([0.1, 0.05, 0.3], 30))),
        # ... and x_des[2] = -3: atan2 - x_des[2] > pi, the first one
        ("wrap_down", [0, 0, -2.0], [-6, 5, 1.0], [-3., 1., -3.0], seq(([0.15, -0.05, -0.2], 30))),
        # starts 0.05 m from the goal (heading = the ego's own), rests, then walks out of the 0.1 m ball
        ("at_goal", [1.03, 1.04, 0.3], [4, -2, 2.0], [1., 1., 0.5], seq((still, 5), (fwd, 10), ([0, 0.1, -0.5], 15))),
        # back to back and close: the clearance is below 0.5 and walking on is the safer backup (argmax 0)
        ("back_to_back", [0, 0, np.pi], [1.2, 0, 0], [-4., 0.5, 3.0], seq((fwd, 30))),
        # a random walk around an obstacle that crosses its way
        ("random", [-0.5, 0.5, 0.7], [1.0, 1.5, -2.0], [4., 4., 1.0], rng.uniform(-1, 1, (STEPS, 3)) * bound),
    ]


class ScriptedMPC:
    """What Quad_env.step touches of a controller: predictiveModel, N, solve, uPred, BT2array."""

    def __init__(self, model, script):
        self.predictiveModel, self.N, self.script = model, N, script
        self.calls, self.uPred = [], None

    def solve(self, x, z, xRef):
        self.calls.append([np.array(v, float).copy() for v in (x, z, xRef)])
        self.uPred = np.array([self.script[len(self.calls) - 1]])

    def BT2array(self):
        return None, None, None


def margins(Q, model, ego, obs, x_des):
    """The decision margins of one step, from the reference's own functions (the quantities of
    :92-116 recomputed before env.step sees the same states)."""
    x1 = model.zpred_eval(ego)[:, 0:3]
    zz = model.zpred_eval(obs)
    hi = np.array([min(Q.robot_col(x1, zz[:, 3 * j:3 * j + 3], L1, W1, L2, W2, COL_TOL)) for j in range(2)])
    mg = [abs(hi[0] - SWITCH)]
    if hi[0] <= SWITCH:
        mg.append(abs(hi[0] - hi[1]))
    dx = x_des[0:2] - ego[0:2]
    full = np.linalg.norm(dx)
    dx = dx / full * min(full, LOOKAHEAD)
    mg += [abs(np.linalg.norm(dx) - NEAR), abs(full - LOOKAHEAD)]
    raw = None
    if np.linalg.norm(dx) > NEAR:
        raw = np.arctan2(dx[1], dx[0]) - x_des[2]
        mg.append(min(abs(raw - k * np.pi) for k in (-3, -1, 1, 3)))
    return hi, min(mg), full, raw


def main():
    G.install_stubs()
    model = G.ref_quadruped_model(N, DT, V0, L1, W1, L2, W2, COL_TOL)
    _, Q = G.ref_models()
    import quadruped_env as QE
    assert os.path.dirname(os.path.abspath(QE.__file__)) == G.REF, QE.__file__
    # the module takes its bare `arctan2` (:104) from `from casadi import *`, which the stand-in
    # does not export; CasADi's arctan2 of two floats is libm's atan2, as NumPy's is
    if not hasattr(QE, "arctan2"):
        QE.arctan2 = np.arctan2
    rec = {k: [] for k in ("x", "z", "xRef", "choice", "hi", "script", "x_des")}
    seen = set()
    worst = np.inf
    for name, ego0, obs0, x_des, script in scripts():
        mpc = ScriptedMPC(model, script)
        env = QE.Quad_env(NR=2, mpc=mpc, x_des=np.array(x_des, float))
        env.robot_set[0].state = np.array(ego0, float)
        env.robot_set[1].state = np.array(obs0, float)
        choice, his = [], []
        for t in range(STEPS):
            hi, mg, full, raw = margins(Q, model, env.robot_set[0].state, env.robot_set[1].state, env.desired_x[0])
            assert mg >= MARGIN, (name, t, mg)
            worst = min(worst, mg)
            with contextlib.redirect_stdout(io.StringIO()):   # the reference prints xRef (:118)
                env.step(t)
            c = int(env.robot_set[1].backupidx)
            assert c == (0 if hi[0] > SWITCH else int(np.argmax(hi))), (name, t)
            seen.add("keep0" if hi[0] > SWITCH else f"argmax{c}")
            if choice and choice[-1] != 0 and c == 0:
                seen.add("back_to_0")
            seen.add("clipped" if full > LOOKAHEAD else "unclipped")
            seen.add("own_heading" if raw is None else "wrap_down" if raw > np.pi else "wrap_up" if raw < -np.pi
                     else "no_wrap")
            choice.append(c), his.append(hi)
        x, z, xr = (np.array([c[i] for c in mpc.calls]) for i in range(3))
        assert x.shape == (STEPS, 3)
        print(f"[{name}] choices {''.join(map(str, choice))}")
        for k, v in zip(rec, (x, z, xr, choice, his, script, x_des)):
            rec[k].append(np.asarray(v))
    need = {"keep0", "argmax0", "argmax1", "back_to_0", "clipped", "unclipped", "own_heading", "wrap_down", "wrap_up",
            "no_wrap"}
    assert seen == need, sorted(need - seen)
    print(f"smallest decision margin {worst:.3e}")
    out = os.path.join(G.REPO, "tests", "golden", "quadruped_scene.npz")
    np.savez_compressed(out, **{k: np.array(v) for k, v in rec.items()}, names=np.array([s[0] for s in scripts()]),
                        N=N, dt=DT, v0=V0, L1=L1, W1=W1, L2=L2, W2=W2, col_tol=COL_TOL, switch_clearance=SWITCH,
                        lookahead=LOOKAHEAD, near=NEAR, margin=MARGIN)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
