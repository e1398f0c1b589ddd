"""The population resampling's ancestor rule in NumPy and Python integers, as ``csrc/bmpc_resample.h``
computes it on the device (``BatchPlan.resample``, ``plan.population_ancestors``).

The rule is exact integer arithmetic, so the GPU, a host build and this module give the same
ancestors from the same integer weights k:

* ``quantise``: M = max logw, k_i = floor(exp(logw_i - M) 2^40) (``exp`` may differ in its last place
  between libraries, so k can differ by one unit between paths: the entries hand out the k they used);
* ``offset``: the 53-bit integer u53 of the one draw of a resampling, Philox4x32-10 at counter
  {lo32(ego_base), hi32(ego_base), round, purpose 1}, key = seed;
* ``ancestors``: systematic resampling -- child j's raw ancestor is the smallest i with
  C_i B > U0 + j S, U0 = (u53 S) >> 53, C the inclusive prefix sums of k -- arranged so that survivors
  stay where they are and the dead slots, in increasing order, take the surplus list;
* ``ess`` = float(S) float(S) / float(sum k^2) and ``new_logw`` = M + log S - log B - 40 log 2.

Anyone can audit a resampling of a run from the recorded log-weights without a GPU."""
from __future__ import annotations

import math

import numpy as np

from . import rng

BITS = 40
PURPOSE_RESAMPLE = 1      # counter word 3 of the resampling draw
MAX_BATCH = 1 << 20


def quantise(logw):
    """(k, M): the integer weights k [B] (uint64) and the maximum M of log-weights logw [B] (finite or
    -inf).  M = -inf (every ego dead) gives k = 0."""
    lw = np.asarray(logw, np.float64).ravel()
    if lw.size < 1 or lw.size > MAX_BATCH:
        raise ValueError("1 .. 2^20 egos")
    if np.isnan(lw).any() or np.isposinf(lw).any():
        raise ValueError("logw must be finite or -inf")
    M = float(lw.max())
    if M == -np.inf:
        return np.zeros(lw.size, np.uint64), M
    with np.errstate(under="ignore"):
        k = np.floor(np.exp(lw - M) * 2.0 ** BITS)
    return k.astype(np.uint64), M


def offset(seed, ego_base, round):
    """u53, the 53-bit integer of the resampling draw of (seed, ego_base, round): the numerator of
    bmpc.rng.uniform53 at purpose 1."""
    seed, g, r = int(seed), int(ego_base), int(round)
    if not (0 <= seed < 2 ** 64 and 0 <= g < 2 ** 63 and 0 <= r < 2 ** 32):
        raise ValueError("seed in [0, 2^64), ego_base in [0, 2^63), round in [0, 2^32)")
    o = rng.philox4x32([g & 0xFFFFFFFF, g >> 32, r, PURPOSE_RESAMPLE], [seed & 0xFFFFFFFF, seed >> 32])
    return ((int(o[0]) >> 5) << 26) | (int(o[1]) >> 6)


def raw_ancestors(k, u53):
    """The raw (unarranged) systematic ancestors [B] of integer weights k: non-decreasing."""
    ks = [int(v) for v in np.asarray(k).ravel()]
    B, S = len(ks), sum(ks)
    if S <= 0:
        raise ValueError("every weight is zero")
    U0 = (int(u53) * S) >> 53
    out, i, C = np.zeros(B, np.int64), 0, ks[0]
    for j in range(B):
        thr = U0 + j * S
        while not C * B > thr:
            i += 1
            C += ks[i]
        out[j] = i
    return out


def ancestors(k, u53):
    """(ancestor, counts) of integer weights k [B] at the draw u53: counts[i] = n_i children have raw
    ancestor i; ancestor[i] = i where n_i >= 1, and the dead slots (n_i = 0), in increasing order,
    receive the surplus list -- each i repeated n_i - 1 times, in increasing i."""
    raw = raw_ancestors(k, u53)
    B = len(raw)
    counts = np.bincount(raw, minlength=B).astype(np.int64)
    anc = np.arange(B, dtype=np.int32)
    surplus = np.repeat(np.arange(B), np.maximum(counts - 1, 0))
    dead = np.flatnonzero(counts == 0)
    assert len(surplus) == len(dead)
    anc[dead] = surplus
    return anc, counts


def ess(k):
    """float(S) float(S) / float(Q) with S = sum k and Q = sum k^2 exact Python integers."""
    ks = [int(v) for v in np.asarray(k).ravel()]
    S, Q = sum(ks), sum(v * v for v in ks)
    return float(S) * float(S) / float(Q)


def new_logw(M, S, B):
    """Every ego's log-weight after a resampling: the log of the mean weight."""
    return float(M) + math.log(float(int(S))) - math.log(float(int(B))) - 40.0 * math.log(2.0)


def resample(logw, seed=0, ego_base=0, round=0, ess_fraction=0.5, k=None):
    """The whole rule on the host: (ancestor [B] int32, info [8]) as bmpc_resample_device reports them --
    info = (resampled, ess, M, new log-weight, float(S), survivors, non-finite log-weights seen, 0).
    k: integer weights to use instead of quantise(logw)'s (e.g. the device's own)."""
    lw = np.asarray(logw, np.float64).ravel()
    B = lw.size
    ident = np.arange(B, dtype=np.int32)
    bad = int(np.isnan(lw).sum() + np.isposinf(lw).sum())
    M = float(np.max(np.where(np.isnan(lw) | np.isposinf(lw), -np.inf, lw)))
    if bad or M == -np.inf:
        return ident, np.array([0.0, 0.0, M, 0.0, 0.0, B, bad, 0.0])
    kk = quantise(lw)[0] if k is None else np.asarray(k, np.uint64)
    S = sum(int(v) for v in kk)
    e = ess(kk)
    info = np.array([0.0, e, M, new_logw(M, S, B), float(S), B, 0.0, 0.0])
    if not e < float(ess_fraction) * B:
        return ident, info
    anc, counts = ancestors(kk, offset(seed, ego_base, round))
    info[0], info[5] = 1.0, float((counts > 0).sum())
    return anc, info
