"""Shared by tests/test_disturbance.py and tests/test_disturbance_gpu.py: the suggested disturbances
and the yardstick of a disturbed step -- an undisturbed step whose inputs were perturbed beforehand in
NumPy with bmpc.rng.disturbance.  The scenes and their host steps are tests/scene_common.py's."""
import functools

import numpy as np

from bmpc import abi, rng

# the issue's suggested standard deviations: (acceleration, yaw rate) on the highway, (vx, vy, yaw rate)
# for the quadrupeds
SIGMAS = {"overtake": ((0.3, 0.01), (0.5, 0.02)), "merge": ((0.3, 0.01), (0.5, 0.02)),
          "quadruped": ((0.02, 0.01, 0.05), (0.02, 0.01, 0.05))}
SEED = 7


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


def twin(kind, dist):
    """scene_common.host_run's `twin`: the disturbance `dist` applied outside the scene function."""
    return functools.partial(perturbed, kind, dist)


def assert_same_but_uobs(kind, a, b, keys=("scene", "x", "z", "xref", "S", "bx")):
    """Two runs' steps agree bit for bit, the scene rows everywhere; the obstacle-input slot is compared
    too (both hold the nominal input the step wrote)."""
    assert len(a) == len(b)
    for t, (ra, rb) in enumerate(zip(a, b)):
        for k in keys:
            if k in ra:
                assert np.array_equal(ra[k], rb[k]), (kind, t, k, np.argwhere(ra[k] != rb[k])[:4])
