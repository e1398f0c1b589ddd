"""Shared by tests/test_disturbance.py and tests/test_disturbance_gpu.py: the host build of the
disturbed scene functions (tests/hostsim/disturbance_host.cpp), the three test scenes with their
scripted controller inputs, and the yardstick of a disturbed step -- an undisturbed step whose inputs
were perturbed beforehand in NumPy with bmpc.rng.disturbance."""
import ctypes as C
import os
import subprocess

import numpy as np

import obstacle_sampling_common as S
from bmpc import abi, rng
from bmpc.scenarios import merge_desc, merge_lane_ref, seeded_merge_batch
from common import HERE, PKG, REPO

SRC = os.path.join(HERE, "hostsim", "disturbance_host.cpp")
SO = os.path.join(HERE, "hostsim", "libbmpc_hostsim_disturbance.so")
INCLUDES = S.INCLUDES
KINDS = ("overtake", "merge", "quadruped")
# the issue's suggested standard deviations: (acceleration, yaw rate) on the highway, (vx, vy, yaw rate)
# for the quadrupeds
SIGMAS = {"overtake": ((0.3, 0.01), (0.5, 0.02)), "merge": ((0.3, 0.01), (0.5, 0.02)),
          "quadruped": ((0.02, 0.01, 0.05), (0.02, 0.01, 0.05))}
SEED = 7
_shim = None
_p = S._p


def shim():
    """The shared-library build of the host file, rebuilt when a source it is compiled from is newer."""
    global _shim
    if _shim is None:
        deps = [SRC, os.path.join(REPO, "include", "bmpc.h")] + [
            os.path.join(PKG, "csrc", f) for f in ("bmpc_rng.h", "bmpc_env_quad.h", "bmpc_env_merge.h", "bmpc_env.h",
                                                   "bmpc_model.h", "bmpc_core.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
            tmp = SO + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                                   "-Wno-unknown-pragmas", *INCLUDES, SRC, "-o", tmp])
            os.replace(tmp, SO)
        _shim = C.CDLL(SO)
    return _shim


def slot(kind):
    """(first slot, width) of the obstacle's input in a scene row."""
    return (abi.QENV_UOBS, 3) if kind == "quadruped" else (abi.ENV_UOBS, 2)


def make(kind, sigma_ego=None, sigma_obs=None, seed=SEED, ego_base=0, law=abi.DISTURB_IH4):
    """The scene's suggested disturbance (or the given sigmas) as an abi.Disturbance."""
    se, so = SIGMAS[kind]
    return abi.make_disturbance(se if sigma_ego is None else sigma_ego, so if sigma_obs is None else sigma_obs, seed,
                                ego_base, law, d=slot(kind)[1])


def perturbed(kind, dist, step, u, u_obs, egos):
    """What the two vehicles apply in the Euler step after closed-loop step `step`, formed in NumPy:
    nominal + sigma * bmpc.rng.disturbance(...) at the components with sigma != 0, the nominal input
    itself elsewhere.  u [B, d] the egos' uPred[0], u_obs [B, d] the obstacles' inputs, egos [B] the
    plan's ego indices (the disturbance's ego_base is added here)."""
    d = slot(kind)[1]
    g = np.asarray(egos, np.uint64) + np.uint64(dist.ego_base)
    out = []
    for nominal, sigma, vehicle in ((u, dist.sigma_ego, "ego"), (u_obs, dist.sigma_obs, "obstacle")):
        sg = np.array(sigma[:d])
        xi = rng.disturbance(int(dist.seed), g, int(step), vehicle, d)
        nominal = np.asarray(nominal, float)
        out.append(np.where(sg != 0, nominal + sg * xi, nominal) if dist.law == abi.DISTURB_IH4 else nominal.copy())
    return out


class MergeScene:
    """The merge scene at the tests' small shape (merge_desc(N=12), the first rows of seeded_merge_batch):
    the interface of obstacle_sampling_common.Scene that the disturbance tests use."""
    kind, n, m = "merge", 4, 2

    def __init__(self, B):
        self.B = B
        self.desc = merge_desc(N=12)
        self.env = abi.make_merge_env()
        x, z = seeded_merge_batch(B)
        self.scene0 = np.zeros((B, abi.ENV_STRIDE))
        self.scene0[:, abi.ENV_X:abi.ENV_X + 4], self.scene0[:, abi.ENV_Z:abi.ENV_Z + 4] = x, z
        self.ref = np.ascontiguousarray(np.concatenate([np.asarray(a, float).ravel() for a in merge_lane_ref()]))
        self.bx = np.ascontiguousarray(np.array(self.desc.bx[:4], float))

    def policies(self):
        return None

    def script(self, t, egos=None):
        e = np.arange(self.B, dtype=float) if egos is None else np.asarray(egos, float)
        return np.stack([1.5 * np.sin(0.7 * t + e), 0.03 * np.cos(0.4 * t + 2 * e)], 1)


def scene_of(kind, B):
    return MergeScene(B) if kind == "merge" else S.Scene(kind, B)


def host_step(sc, t, scene, pol, u0=None, dist=None, legacy=False):
    """k_env / k_env_merge / k_env_quad on the host with the plan's disturbance `dist` (None: none);
    advances `scene` (and the overtake `pol`) in place; returns x, z, xref (merge: also S, bx)."""
    B, n = scene.shape[0], sc.n
    x, z, xref = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
    up = None if u0 is None else np.ascontiguousarray(np.asarray(u0, float).reshape(B, -1))
    stride = 0 if up is None else up.shape[1]
    dp = None if dist is None else C.byref(dist)
    if sc.kind == "merge":
        Sm, bx = np.zeros((B, 16)), np.zeros((B, 4))
        rc = shim().dh_merge_env_step(C.byref(sc.env), len(sc.ref) // 3, _p(sc.ref), _p(sc.bx), 4,
                                      C.c_double(sc.desc.dt), int(t), B, _p(scene), _p(up), stride, _p(x), _p(z),
                                      _p(xref), _p(Sm), _p(bx), dp, 1 if legacy else 0)
        assert rc == 0
        return x, z, xref, Sm, bx
    fn = shim().dh_env_step if sc.kind == "overtake" else shim().dh_quad_env_step
    rc = fn(C.byref(sc.env), _p(sc.mc), C.c_double(sc.desc.dt), sc.desc.N, sc.desc.m, int(t), B, _p(scene), pol, _p(up),
            stride, _p(x), _p(z), _p(xref), dp, 1 if legacy else 0)
    assert rc == 0
    return x, z, xref


def host_run(sc, steps, dist=None, legacy=False, twin=None, egos=None):
    """`steps` teacher-forced host steps of the scene's rows `egos` (a slice; default all).  dist: the
    disturbance the scene function gets.  twin: a disturbance applied OUTSIDE the scene function
    instead -- before each step the scripted uPred[0] and the row's obstacle-input slot are replaced
    by `perturbed(...)`, and the nominal slot the step then writes is what the next step perturbs.
    Returns per step a dict of scene, x, z, xref (merge: S, bx) and the final policy array."""
    sel = slice(None) if egos is None else egos
    scene = np.ascontiguousarray(sc.scene0[sel]).copy()
    ids = np.arange(sc.B)[sel]
    pol = None if sc.kind == "merge" else abi.policy_array([sc.rows[i] for i in ids])
    lo, w = slot(sc.kind)
    out = []
    for t in range(steps):
        u0 = None if t == 0 else sc.script(t, ids)
        if twin is not None and t > 0:
            u0, scene[:, lo:lo + w] = perturbed(sc.kind, twin, t - 1, u0, scene[:, lo:lo + w], np.arange(len(ids)))
        res = host_step(sc, t, scene, pol, u0, dist, legacy)
        out.append(dict(zip(("x", "z", "xref", "S", "bx"), res), scene=scene.copy()))
    return out, pol


def assert_same_but_uobs(kind, a, b, keys=("scene", "x", "z", "xref", "S", "bx")):
    """Two runs' steps agree bit for bit, the scene rows everywhere; the obstacle-input slot is compared
    too (both hold the nominal input the step wrote)."""
    assert len(a) == len(b)
    for t, (ra, rb) in enumerate(zip(a, b)):
        for k in keys:
            if k in ra:
                assert np.array_equal(ra[k], rb[k]), (kind, t, k, np.argwhere(ra[k] != rb[k])[:4])
