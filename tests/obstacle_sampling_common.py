"""Shared by tests/test_obstacle_sampling.py and tests/test_obstacle_sampling_gpu.py: the host build
of the sampled scene functions (tests/hostsim/obstacle_sampling_host.cpp), the two test scenes with
their scripted controller inputs, and the yardstick of a sampled choice -- the inverse CDF of
oracle.model's branch_eval at the recorded pre-step state under bmpc.rng's draw."""
import ctypes as C
import os
import subprocess

import numpy as np

from bmpc import abi, rng
from bmpc.scenarios import (highway_desc, highway_policy_rows, quad_scene, quadruped_desc, quadruped_policy_rows,
                            seeded_batch, seeded_quadruped_batch, seeded_quadruped_goals)
from common import HERE, PKG, REPO

SRC = os.path.join(HERE, "hostsim", "obstacle_sampling_host.cpp")
SO = os.path.join(HERE, "hostsim", "libbmpc_hostsim_obstacle_sampling.so")
INCLUDES = ["-I" + os.path.join(REPO, "include"), "-I" + os.path.join(PKG, "csrc")]
MARGIN = 1e-9          # the project's host-versus-NumPy scene bar (tests/test_env_host.py)
MAX_LEFT_OUT = 0.01    # at most 1 % of the decisions may lie within MARGIN of a partial sum
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
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", *INCLUDES,
                                   SRC, "-o", tmp])
            os.replace(tmp, SO)
        _shim = C.CDLL(SO)
        _shim.os_inverse_cdf.argtypes = [C.c_void_p, C.c_int, C.c_double]
    return _shim


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Scene:
    """One of the two scenes with a choice, at the tests' small shapes: its plan description, scene
    constants, initial scene rows and policies, a scripted stand-in for the controller's uPred[0], the
    host scene step, and oracle.model's branch probabilities."""

    def __init__(self, kind, B, N=6, NB=None, case=None):
        self.kind, self.B = kind, B
        if case is not None:   # a case of tests/test_loop_record_gpu.py: kind, desc, scene, policies, env
            self.n, self.m = case["desc"].n, case["desc"].m
            self.desc, self.env, self.scene0, self.rows = case["desc"], case["env"], case["scene"], case["policies"]
        elif kind == "overtake":
            self.n, self.m = 4, 3
            self.desc = highway_desc(N=N, NB=1 if NB is None else NB)
            self.env = abi.make_env()
            x, z, _, self.tgt = seeded_batch(B, 0)
            self.scene0 = np.zeros((B, abi.ENV_STRIDE))
            self.scene0[:, abi.ENV_X:abi.ENV_X + 4] = x
            self.scene0[:, abi.ENV_Z:abi.ENV_Z + 4] = z
            self.rows = highway_policy_rows(self.tgt)
        else:
            self.n, self.m = 3, 2
            self.desc = quadruped_desc(N=N, NB=2 if NB is None else NB)
            self.env = abi.make_quad_env()
            x, z, _ = seeded_quadruped_batch(B, 1)
            self.scene0 = quad_scene(x, z, seeded_quadruped_goals(B, 1))
            self.rows = quadruped_policy_rows(B)
        self.mc = np.array(self.desc.mc[:8], float)

    def policies(self):
        return abi.policy_array(self.rows)

    def script(self, t, egos=None):
        """uPred[0] applied by the Euler step of t (t >= 1), per GLOBAL ego: smooth, within the input bounds."""
        e = np.arange(self.B, dtype=float) if egos is None else np.asarray(egos, float)
        if self.kind == "overtake":
            return np.stack([1.5 * np.sin(0.7 * t + e), 0.05 * np.cos(0.4 * t + 2 * e)], 1)
        return np.stack([0.15 + 0.05 * np.sin(0.5 * t + e), 0.05 * np.cos(0.3 * t + e),
                         0.3 * np.sin(0.9 * t + 3 * e)], 1)

    def lc_targets(self, scenes):
        """The overtake lane-change targets in force BEFORE each step of recorded scene rows
        [B, T, ENV_STRIDE] that start at step 0: update_backup re-targets when the obstacle's lane
        entry changes (and at t = 0), from the lane entries of that step (csrc/bmpc_env.h)."""
        B, T = scenes.shape[:2]
        cur = np.array([r[2][1] for r in self.rows], float)
        out = np.zeros((B, T, 4))
        for t in range(T):
            out[:, t] = cur
            l0, l1 = scenes[:, t, abi.ENV_LANE0], scenes[:, t, abi.ENV_LANE1]
            changed = np.ones(B, bool) if t == 0 else l1 != scenes[:, t - 1, abi.ENV_LANE1]
            tl = np.where(l0 < l1, l1 - 1, np.where(l0 > l1, l1 + 1, np.where(l1 > 0, l1 - 1, l1 + 1)))
            new = np.stack([np.zeros(B), 1.8 + 3.6 * tl, np.full(B, self.env.v0), np.zeros(B)], 1)
            cur = np.where(changed[:, None], new, cur)
        return out

    def host_step(self, t, scene, pol, u0=None, smp=None, legacy=False):
        """k_env / k_env_quad on the host: advances `scene` (and the overtake `pol`) in place; x, z, xref."""
        B, n = scene.shape[0], self.n
        x, z, xref = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
        up = None if u0 is None else np.ascontiguousarray(np.asarray(u0, float).reshape(B, -1))
        fn = shim().os_env_step if self.kind == "overtake" else shim().os_quad_env_step
        rc = fn(C.byref(self.env), _p(self.mc), C.c_double(self.desc.dt), self.desc.N, self.desc.m, int(t), B,
                _p(scene), pol, _p(up), 0 if up is None else up.shape[1], _p(x), _p(z), _p(xref),
                None if smp is None else C.byref(smp), 1 if legacy else 0)
        assert rc == 0
        return x, z, xref

    def oracle_p(self, pol, e, x, z):
        """oracle.model's branch_eval(x, z) under ego e's policies `pol` (a ctypes policy array)."""
        from oracle import model as M
        m = self.m
        ps = [M.Policy(int(pol[e * m + j].kind), tuple(pol[e * m + j].p)) for j in range(m)]
        if self.kind == "overtake":
            mdl = M.HighwayModel(self.desc.N, self.desc.dt, ps, L=self.mc[0], W=self.mc[1], s1=self.mc[2],
                                 N_lane=self.mc[3])
        else:
            mdl = M.QuadrupedModel(self.desc.N, self.desc.dt, ps, *self.mc[:6])
        return mdl.branch_eval(x, z)[0]


def expected_choice(p, u):
    """(choice, sure): bmpc.rng's inverse CDF of probabilities p [..., m] at u [...], and whether u
    keeps MARGIN from every partial sum that separates two policies."""
    choice, cum = rng.inverse_cdf(p, u)
    return choice, np.abs(np.asarray(u)[..., None] - cum[..., :-1]).min(-1) >= MARGIN


def copy_policies(pol):
    out = type(pol)()
    C.memmove(out, pol, C.sizeof(pol))
    return out


def check_choices(sc, smp, choices, pre, ego_base=0):
    """The rule of every sampled choice of a run.  choices [T][B]: the scene row's policy index after
    each step; pre [T]: (pol, x, z) the policies in force before the step and the step's pre-step
    state (its x / z outputs) -- needed at epoch starts only (None elsewhere).  Epoch starts equal the
    inverse CDF of the oracle's p under bmpc.rng's u unless u lies within MARGIN of a partial sum (at
    most MAX_LEFT_OUT of them may); inside an epoch the choice is the epoch's first.  Returns the
    number of compared draws."""
    T, B = np.asarray(choices).shape
    left_out = draws = 0
    for t in range(T):
        if t % smp.hold:
            np.testing.assert_array_equal(choices[t], choices[t - t % smp.hold], err_msg=f"step {t} inside an epoch")
            continue
        pol, x, z = pre[t]
        u = rng.obstacle_uniform(smp.seed, ego_base + np.arange(B), t // smp.hold)
        p = np.stack([sc.oracle_p(pol, e, x[e], z[e]) for e in range(B)])
        want, sure = expected_choice(p, u)
        draws += B
        left_out += int((~sure).sum())
        np.testing.assert_array_equal(np.asarray(choices[t])[sure], want[sure], err_msg=f"epoch start {t}")
    assert left_out <= MAX_LEFT_OUT * draws, (left_out, draws)
    return draws - left_out


def host_run(sc, smp, steps, legacy=False, egos=None):
    """`steps` teacher-forced host steps from the scene's initial rows (`egos`: a slice of them, drawing
    as plan egos 0.. with the sampler's ego_base); returns per step the scene, x, z, xref and the
    pre-step policies, plus the final policy array."""
    sel = slice(None) if egos is None else egos
    scene = np.ascontiguousarray(sc.scene0[sel]).copy()
    B = scene.shape[0]
    ids = np.arange(sc.B)[sel]
    pol = abi.policy_array([sc.rows[i] for i in ids])
    out = []
    for t in range(steps):
        before = copy_policies(pol)
        u0 = None if t == 0 else sc.script(t, ids)
        x, z, xr = sc.host_step(t, scene, pol, u0, smp, legacy)
        out.append(dict(scene=scene.copy(), x=x, z=z, xref=xr, pol=before))
    assert B == len(ids)
    return out, pol
