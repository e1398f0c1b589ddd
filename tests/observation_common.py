"""Shared by tests/test_observation.py and tests/test_observation_gpu.py: the suggested observation
models, the yardstick of an observed step -- the true states plus sigma * bmpc.rng.observation formed
in NumPy -- and the host scene steps that pass the observation model
(tests/hostsim/observation_host.cpp; the scenes and the plain steps are tests/scene_common.py's)."""
import ctypes as C

import numpy as np

import hostbuild
import scene_common as SC
from bmpc import abi, rng

# the issue's suggested standard deviations (sigma_x, sigma_z): of (X, Y, v, psi) on the highway and the
# merge, of (x, y, psi) for the quadrupeds
SIGMAS = {"overtake": ((0.05, 0.02, 0.05, 0.002), (0.2, 0.1, 0.2, 0.01)),
          "merge": ((0.05, 0.02, 0.05, 0.002), (0.2, 0.1, 0.2, 0.01)),
          "quadruped": ((0.005, 0.005, 0.005), (0.02, 0.02, 0.02))}
SEED = 11


def width(kind):
    """The scene's state dimension."""
    return 3 if kind == "quadruped" else 4


def rows(kind):
    """(first slot of x, first slot of z) in a scene row."""
    return (abi.QENV_X, abi.QENV_Z) if kind == "quadruped" else (abi.ENV_X, abi.ENV_Z)


def make(kind, sigma_x=None, sigma_z=None, seed=SEED, ego_base=0, law=abi.OBSERVE_IH4):
    """The scene's suggested observation model (or the given sigmas) as an abi.Observation."""
    sx, sz = SIGMAS[kind]
    return abi.make_observation(sx if sigma_x is None else sigma_x, sz if sigma_z is None else sigma_z, seed, ego_base,
                                law, n=width(kind))


def observed(kind, obs, step, x, z, egos):
    """What the solve of closed-loop step `step` is handed, formed in NumPy: true state + sigma *
    bmpc.rng.observation(...) at the components with sigma != 0, the true state itself elsewhere.
    x, z [B, n] the true states (the scene row's), egos [B] the plan's ego indices (the model's
    ego_base is added here)."""
    n = width(kind)
    g = np.asarray(egos, np.uint64) + np.uint64(obs.ego_base)
    out = []
    for truth, sigma, vehicle in ((x, obs.sigma_x, "ego"), (z, obs.sigma_z, "obstacle")):
        sg = np.array(sigma[:n])
        xi = rng.observation(int(obs.seed), g, int(step), vehicle, n)
        truth = np.asarray(truth, float)
        out.append(np.where(sg != 0, truth + sg * xi, truth) if obs.law == abi.OBSERVE_IH4 else truth.copy())
    return out


def observed_rows(kind, obs, step, scene, egos=None):
    """observed() of the true states in the scene rows [B, ENV_STRIDE] after step `step`."""
    lo_x, lo_z = rows(kind)
    n = width(kind)
    egos = np.arange(len(scene)) if egos is None else egos
    return observed(kind, obs, step, scene[:, lo_x:lo_x + n], scene[:, lo_z:lo_z + n], egos)


def shim():
    """libbmpc_hostsim_observation.so: observation_host.cpp's wrappers."""
    return hostbuild.shared("observation", ["observation_host.cpp"])


def host_step(sc, t, scene, pol, u0=None, obs=None, smp=None, prop=None, dist=None, solve=None):
    """scene_common.host_step through the wrappers that pass the observation model `obs` (None: a null
    pointer): advances `scene` (and the overtake `pol`) in place; returns x, z, xref (merge: S, bx)."""
    p, ref = SC._p, SC._ref
    B, n = scene.shape[0], sc.n
    x, z, xref = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
    up = None if u0 is None else np.ascontiguousarray(np.asarray(u0, float).reshape(B, -1))
    stride = 0 if up is None else up.shape[1]
    J, status, iters, stats = (None,) * 4 if solve is None else solve
    dt = C.c_double(sc.desc.dt)
    if sc.kind == "merge":
        Sm, bx = np.zeros((B, 4, 4)), np.zeros((B, 4))
        rc = shim().oh_merge_env_step(C.byref(sc.env), len(sc.ref) // 3, p(sc.ref), p(sc.bx), 4, dt, int(t), B, p(scene),
                                      p(up), stride, p(J), p(status), p(iters), p(x), p(z), p(xref), p(Sm), p(bx),
                                      p(stats), ref(dist), ref(obs))
        assert rc == 0
        return x, z, xref, Sm, bx
    head = (C.byref(sc.env), p(sc.mc), dt, sc.desc.N, sc.desc.m, int(t), B, p(scene), pol, p(up), stride)
    tail = (ref(smp), ref(prop), ref(dist), ref(obs))
    if sc.kind == "overtake":
        rc = shim().oh_env_step(*head, p(x), p(z), p(xref), *tail)
    else:
        rc = shim().oh_quad_env_step(*head, p(J), p(status), p(iters), p(x), p(z), p(xref), p(stats), *tail)
    assert rc == 0
    return x, z, xref


def quad_solve(B, t):
    """A made-up last solve (J, status, iters) for the merge and quadruped steps' statistics."""
    e = np.arange(B, dtype=float)
    return (np.ascontiguousarray(10.0 + np.sin(e + t)), np.ones(B, np.int32), np.full(B, 5 + t % 3, np.int32))


def host_run(sc, steps, obs=None, plain=False, egos=None, **options):
    """`steps` teacher-forced host steps from the scene's initial rows (scene_common.Scene.script is
    the controller).  plain: through scene_common.host_step, the scene functions' argument list before
    the observation model; else through this module's host_step with `obs`.  egos: a slice of the
    scene's egos, drawing as plan egos 0.. (with the model's ego_base).  Returns per step a dict of the
    scene rows after it, x, z, xref (merge: S, bx), the statistics rows (merge and quadruped) and the
    policies after it (bytes)."""
    sel = slice(None) if egos is None else egos
    scene = np.ascontiguousarray(sc.scene0[sel]).copy()
    ids = np.arange(sc.B)[sel]
    pol = sc.policies(ids)
    stats = None if sc.kind == "overtake" else np.zeros((len(ids), abi.ENV_NSTAT))
    out = []
    for t in range(steps):
        u0 = None if t == 0 else sc.script(t, ids)
        solve = None if stats is None else quad_solve(len(ids), t) + (stats,)
        if plain:
            res = SC.host_step(sc, t, scene, pol, u0, solve=solve, **options)
        else:
            res = host_step(sc, t, scene, pol, u0, obs, solve=solve, **options)
        out.append(dict(zip(("x", "z", "xref", "S", "bx"), res), scene=scene.copy(),
                        stats=None if stats is None else stats.copy(), pol=None if pol is None else bytes(pol)))
    return out
