"""The three scene steps on the host, shared by the closed-loop feature tests (obstacle sampling,
obstacle proposal, disturbance; CPU and GPU sides) and by tests/test_merge_loop.py /
tests/test_quad_loop.py: the shared-library build of tests/hostsim/scene_host.cpp, the test scenes
with their scripted controller inputs, one scene step and a teacher-forced run."""
import ctypes as C

import numpy as np

import hostbuild
from bmpc import abi
from bmpc.scenarios import (_overtake_scene, highway_desc, highway_policy_rows, merge_desc, merge_lane_ref, quad_scene,
                            quadruped_desc, quadruped_policy_rows, seeded_batch, seeded_merge_batch,
                            seeded_quadruped_batch, seeded_quadruped_goals)

KINDS = ("overtake", "merge", "quadruped")


def shim():
    """libbmpc_hostsim_scene.so: scene_host.h's wrappers and the probes of scene_host.cpp."""
    lib = hostbuild.shared("scene", ["scene_host.cpp"])
    lib.os_inverse_cdf.argtypes = [C.c_void_p, C.c_int, C.c_double]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ref(s):
    return None if s is None else C.byref(s)


class Scene:
    """One of the three scenes at the tests' small shapes: its plan description, scene constants,
    initial scene rows and policies, a scripted stand-in for the controller's uPred[0], and
    oracle.model's branch probabilities.  merge: merge_desc(N=12) and the first rows of
    seeded_merge_batch, its ramp table `ref` and the plan's `bx`."""

    def __init__(self, kind, B, N=6, NB=None, case=None):
        self.kind, self.B = kind, B
        if case is not None:   # a case of tests/loop_common.py: kind, desc, scene, policies, env
            self.n, self.m = case["desc"].n, case["desc"].m
            self.desc, self.env, self.scene0, self.rows = case["desc"], case["env"], case["scene"], case["policies"]
        elif kind == "overtake":
            self.n, self.m = 4, 3
            self.desc = highway_desc(N=N, NB=1 if NB is None else NB)
            self.env = abi.make_env()
            x, z, _, self.tgt = seeded_batch(B, 0)
            self.scene0 = _overtake_scene(x, z)
            self.rows = highway_policy_rows(self.tgt)
        elif kind == "merge":
            self.n, self.m = 4, 2
            self.desc = merge_desc(N=12)
            self.env = abi.make_merge_env()
            self.scene0 = _overtake_scene(*seeded_merge_batch(B))
            self.rows = None
        else:
            self.n, self.m = 3, 2
            self.desc = quadruped_desc(N=N, NB=2 if NB is None else NB)
            self.env = abi.make_quad_env()
            x, z, _ = seeded_quadruped_batch(B, 1)
            self.scene0 = quad_scene(x, z, seeded_quadruped_goals(B, 1))
            self.rows = quadruped_policy_rows(B)
        self.mc = np.array(self.desc.mc[:8], float)
        if kind == "merge":
            self.ref = np.ascontiguousarray(np.concatenate([np.asarray(a, float).ravel() for a in merge_lane_ref()]))
            self.bx = np.ascontiguousarray(np.array(self.desc.bx[:4], float))

    def policies(self, ids=None):
        """The scene's policy array (rows `ids` of it); None for the merge, whose step takes none."""
        if self.kind == "merge":
            return None
        return abi.policy_array(self.rows if ids is None else [self.rows[i] for i in ids])

    def script(self, t, egos=None):
        """uPred[0] applied by the Euler step of t (t >= 1), per GLOBAL ego: smooth, within the input bounds."""
        e = np.arange(self.B, dtype=float) if egos is None else np.asarray(egos, float)
        if self.kind == "overtake":
            return np.stack([1.5 * np.sin(0.7 * t + e), 0.05 * np.cos(0.4 * t + 2 * e)], 1)
        if self.kind == "merge":
            return np.stack([1.5 * np.sin(0.7 * t + e), 0.03 * np.cos(0.4 * t + 2 * e)], 1)
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


def copy_policies(pol):
    if pol is None:
        return None
    out = type(pol)()
    C.memmove(out, pol, C.sizeof(pol))
    return out


def host_step(sc, t, scene, pol, u0=None, smp=None, prop=None, dist=None, arglist=0, solve=None):
    """k_env / k_env_merge / k_env_quad on the host with the plan's scene options (None: not attached):
    advances `scene` (and the overtake `pol`) in place; returns x, z, xref (merge: also S, bx).
    arglist: scene_host.h's selector of the scene function's argument list.  solve (merge, quadruped):
    (J, status, iters, stats) of the last solve, booked into stats before the step."""
    B, n = scene.shape[0], sc.n
    x, z, xref = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
    up = None if u0 is None else np.ascontiguousarray(np.asarray(u0, float).reshape(B, -1))
    stride = 0 if up is None else up.shape[1]
    J, status, iters, stats = (None,) * 4 if solve is None else solve
    dt = C.c_double(sc.desc.dt)
    if sc.kind == "merge":
        Sm, bx = np.zeros((B, 4, 4)), np.zeros((B, 4))
        rc = shim().sh_merge_env_step(C.byref(sc.env), len(sc.ref) // 3, _p(sc.ref), _p(sc.bx), 4, dt, int(t), B,
                                      _p(scene), _p(up), stride, _p(J), _p(status), _p(iters), _p(x), _p(z), _p(xref),
                                      _p(Sm), _p(bx), _p(stats), _ref(dist), int(arglist))
        assert rc == 0
        return x, z, xref, Sm, bx
    head = (C.byref(sc.env), _p(sc.mc), dt, sc.desc.N, sc.desc.m, int(t), B, _p(scene), pol, _p(up), stride)
    tail = (_ref(smp), _ref(prop), _ref(dist), int(arglist))
    if sc.kind == "overtake":
        assert solve is None, "the overtake statistics are hostsim_lib.HostSim.env_step's"
        rc = shim().sh_env_step(*head, _p(x), _p(z), _p(xref), *tail)
    else:
        rc = shim().sh_quad_env_step(*head, _p(J), _p(status), _p(iters), _p(x), _p(z), _p(xref), _p(stats), *tail)
    assert rc == 0
    return x, z, xref


def host_run(sc, steps, smp=None, prop=None, dist=None, arglist=0, t0=0, egos=None, same_input=False, twin=None):
    """`steps` teacher-forced host steps t0 .. t0 + steps - 1 from the scene's initial rows.  egos: an
    index array or slice of them, drawing as plan egos 0.. (with the options' ego_base); same_input:
    every ego gets ego 0's scripted input, so that egos from one state differ by the obstacle's choices
    alone; twin(step, u0, u_obs, egos) -> (u0, u_obs): a disturbance applied OUTSIDE the scene function
    -- before each step the scripted uPred[0] and the row's obstacle-input slot are replaced by its
    result, and the nominal slot the step then writes is what the next step perturbs.
    Returns per step a dict of the scene rows after it, the step's x, z, xref (merge: S, bx) -- a
    choice's pre-step state -- and `pol`, the policies in force before it; and the final policy array."""
    sel = slice(None) if egos is None else egos
    scene = np.ascontiguousarray(sc.scene0[sel]).copy()
    ids = np.arange(sc.B)[sel]
    pol = sc.policies(ids)
    lo, w = (abi.QENV_UOBS, 3) if sc.kind == "quadruped" else (abi.ENV_UOBS, 2)
    out = []
    for t in range(t0, t0 + steps):
        before = copy_policies(pol)
        u0 = None if t == 0 else sc.script(t, np.zeros(len(ids)) if same_input else ids)
        if twin is not None and t > 0:
            u0, scene[:, lo:lo + w] = twin(t - 1, u0, scene[:, lo:lo + w], np.arange(len(ids)))
        res = host_step(sc, t, scene, pol, u0, smp, prop, dist, arglist)
        out.append(dict(zip(("x", "z", "xref", "S", "bx"), res), scene=scene.copy(), pol=before))
    return out, pol
