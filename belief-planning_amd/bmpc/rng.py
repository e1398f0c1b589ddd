"""The closed loops' random draws in NumPy: Philox4x32-10 and the uniform of one obstacle-policy
draw, as ``csrc/bmpc_rng.h`` computes them on the device (``BatchPlan.set_obstacle_sampling``).

A draw is addressed by (seed, global ego, epoch), never consumed: anyone can reproduce or audit the
choice an obstacle made at closed-loop step t from ``obstacle_uniform(seed, ego_base + e, t // hold)``
and the model's branch probabilities at that step's state (``inverse_cdf``), without a GPU.  The
actuation disturbance (``BatchPlan.set_disturbance``) is addressed the same way: the inputs applied
after step t are ``nominal + sigma * disturbance(seed, ego_base + e, t, vehicle, d)``.  So is the
observation noise (``BatchPlan.set_observation``): the solve of step t sees
``true state + sigma * observation(seed, ego_base + e, t, vehicle, n)``."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
PURPOSE_OBSTACLE_POLICY = 0      # counter word 3; 1 is bmpc.resample's, 2-7 are reserved, 8-15 and 16-31 below
DISTURBANCE_PURPOSE = {"obstacle": 8, "ego": 12}   # ... + c for component c of the vehicle's input
OBSERVATION_PURPOSE = {"obstacle": 16, "ego": 24}   # ... + c for component c of the vehicle's observed state
DISTURBANCE_SCALE = float.fromhex("0x1.bb67ae8584caap-32")   # sqrt(3) / 2^32
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10.  counter [..., 4] and key [..., 2] of 32-bit words (broadcast against each
    other) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2      # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform53(o0, o1):
    """((o0 >> 5) 2^26 + (o1 >> 6)) / 2^53: a double in [0, 1), exact."""
    bits = ((np.asarray(o0, np.uint64) >> np.uint64(5)) << np.uint64(26)) | (np.asarray(o1, np.uint64) >> np.uint64(6))
    return bits.astype(np.float64) * 2.0 ** -53


def _u64(v, what):
    a = np.asarray(v)
    if a.dtype.kind not in "iu" and not (a.dtype == object and all(isinstance(i, int) for i in a.ravel())):
        raise TypeError(f"{what} must be integers")
    if a.dtype.kind != "u" and a.size and min(a.ravel()) < 0:
        raise ValueError(f"{what} must not be negative")
    return a.astype(np.uint64)


def obstacle_uniform(seed, ego, epoch):
    """The uniform u in [0, 1) behind the obstacle's policy choice: seed the sampler's 64-bit seed,
    ego the GLOBAL ego index (the plan's ego_base + its row), epoch = t // hold.  Vectorised:
    the three broadcast against each other."""
    s, g, ep = np.broadcast_arrays(_u64(seed, "seed"), _u64(ego, "ego"), _u64(epoch, "epoch"))
    if ep.size and ep.max() >= 2 ** 32:
        raise ValueError("epoch must fit 32 bits")
    counter = np.stack([g & _MASK, g >> _S32, ep, np.full(g.shape, PURPOSE_OBSTACLE_POLICY, np.uint64)], axis=-1)
    key = np.stack([s & _MASK, s >> _S32], axis=-1)
    o = philox4x32(counter, key)
    return uniform53(o[..., 0], o[..., 1])


def ih4(o):
    """The disturbance's variate from four output words o [..., 4]: the centred integer sum
    s = o0 + o1 + o2 + o3 - 2 (2^32 - 1), exact, times sqrt(3) / 2^32 -- one rounding, the double
    ``rng_ih4`` of ``csrc/bmpc_rng.h`` gives.  Irwin-Hall with four terms: mean 0, variance
    1 - 2^-64, kurtosis 2.7, |xi| <= 2 sqrt(3)."""
    s = np.asarray(o, dtype=np.uint32).astype(np.int64).sum(axis=-1) - 2 * (2 ** 32 - 1)
    return s.astype(np.float64) * DISTURBANCE_SCALE


def _ih4_at(seed, ego, step, purpose0, k):
    """ih4 [..., k] at the counters {lo32(ego), hi32(ego), step, purpose0 + c}, c < k, key = seed."""
    s, g, t = np.broadcast_arrays(_u64(seed, "seed"), _u64(ego, "ego"), _u64(step, "step"))
    if t.size and t.max() >= 2 ** 32:
        raise ValueError("step must fit 32 bits")
    s, g, t = (np.broadcast_to(a[..., None], a.shape + (int(k),)) for a in (s, g, t))
    purpose = np.broadcast_to(np.arange(int(k), dtype=np.uint64) + np.uint64(purpose0), g.shape)
    counter = np.stack([g & _MASK, g >> _S32, t, purpose], axis=-1)
    key = np.stack([s & _MASK, s >> _S32], axis=-1)
    return ih4(philox4x32(counter, key))


def disturbance(seed, ego, step, vehicle, d):
    """xi [..., d] of the actuation disturbance (``BatchPlan.set_disturbance``): seed its 64-bit
    seed, ego the GLOBAL ego index (the plan's ego_base + its row), step the closed-loop step t
    whose input is disturbed, vehicle "obstacle" or "ego", d the input dimension (<= 4).  The input
    a vehicle applies at step t is ``nominal + sigma * disturbance(...)``, the product rounded before
    it is added -- what NumPy computes.  Vectorised like ``obstacle_uniform``."""
    if vehicle not in DISTURBANCE_PURPOSE:
        raise ValueError(f"vehicle {vehicle!r}: one of {sorted(DISTURBANCE_PURPOSE)}")
    if int(d) != d or not 1 <= int(d) <= 4:
        raise ValueError("d must be an integer in 1..4")
    return _ih4_at(seed, ego, step, DISTURBANCE_PURPOSE[vehicle], d)


def observation(seed, ego, step, vehicle, n):
    """xi [..., n] of the observation noise (``BatchPlan.set_observation``): seed its 64-bit seed, ego
    the GLOBAL ego index (the plan's ego_base + its row), step the closed-loop step t whose solve sees
    the observation, vehicle "obstacle" or "ego", n the state dimension (<= 8).  The state handed to
    the solve of step t is ``true state + sigma * observation(...)``, the product rounded before it is
    added -- what NumPy computes; a component with sigma == 0 passes through
    (``np.where(sigma != 0, ...)``).  The variate is ``disturbance``'s, at purposes of its own.
    Vectorised like ``obstacle_uniform``."""
    if vehicle not in OBSERVATION_PURPOSE:
        raise ValueError(f"vehicle {vehicle!r}: one of {sorted(OBSERVATION_PURPOSE)}")
    if int(n) != n or not 1 <= int(n) <= 8:
        raise ValueError("n must be an integer in 1..8")
    return _ih4_at(seed, ego, step, OBSERVATION_PURPOSE[vehicle], n)


def inverse_cdf(p, u):
    """The scene's choice rule: the smallest j with u < p_0 + ... + p_j (partial sums in that
    order), m - 1 if none.  p [..., m] probabilities, u [...].  Also returns the partial sums
    [..., m] (a decision is as sure as |u - partial sum| is large)."""
    cum = np.cumsum(np.asarray(p, float), axis=-1)
    below = np.asarray(u, float)[..., None] < cum
    return np.where(below.any(-1), below.argmax(-1), cum.shape[-1] - 1), cum
