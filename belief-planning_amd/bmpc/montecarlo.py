"""Weighted Monte-Carlo estimates over a closed-loop population (host, NumPy only).

An ego of a population run with ``BatchPlan.set_obstacle_sampling("tilted")`` or ``("script")``
carries, in its scene row's slot ``abi.ENV_LOGW``, the logarithm of a weight w:

* tilted: w = p(path) / q(path), the likelihood ratio of the obstacle's realised choice sequence
  under the model's branch distribution p against the tilted proposal q it was drawn from.  For a
  per-ego quantity f, ``estimate(f, logw)`` is the importance-sampling estimate of E_p[f];
* script: w = p(path), the model's probability of the prescribed sequence.  Over the full enumeration
  ``enumerate_scripts(m, epochs)`` from one initial state the weights sum to one and
  sum_paths w f -- ``estimate(f, logw)[0] * len(f)``, or ``exact_expectation`` -- is the exact
  closed-loop expectation over the scenario tree.

A sharded population reduces ``reduce_terms`` with ``distributed.reduce_stats(v, max_slots=())`` and
hands the sum to ``estimate_from_terms``: the result is the unsharded one."""
from __future__ import annotations

import numpy as np

# slots of reduce_terms' vector
T_N, T_W, T_WF, T_W2, T_WF2, T_W2F, T_COUNT = 0, 1, 2, 3, 4, 5, 6


def enumerate_scripts(m, epochs):
    """All m ** epochs choice sequences as an int32 array [m ** epochs, epochs], rows in lexicographic
    order (epoch 0 is the most significant digit): the script table of a full enumeration."""
    m, epochs = int(m), int(epochs)
    if m < 1 or epochs < 1:
        raise ValueError("m >= 1 and epochs >= 1")
    if m ** epochs > 2 ** 24:
        raise ValueError(f"{m} ** {epochs} paths: too many to enumerate")
    idx = np.arange(m ** epochs)
    return np.stack([(idx // m ** (epochs - 1 - c)) % m for c in range(epochs)], axis=1).astype(np.int32)


def _args(values, logw):
    f, lw = np.asarray(values, np.float64).ravel(), np.asarray(logw, np.float64).ravel()
    if f.shape != lw.shape or f.size == 0:
        raise ValueError(f"values and logw must hold one entry per ego, got {f.shape} and {lw.shape}")
    if np.isnan(lw).any() or np.isposinf(lw).any():
        raise ValueError("logw must be finite or -inf")
    return f, lw


def reduce_terms(values, logw, shift=0.0):
    """The sums an estimate needs, as a float64 vector that adds over shards:
    [n, sum w, sum w f, sum w^2, sum (w f)^2, sum w^2 f] with w = exp(logw - shift) (slots T_*).
    Every shard passes the same `shift` (0, or a bound on the population's logw when exp(logw)
    would overflow); estimate_from_terms takes it back out."""
    f, lw = _args(values, logw)
    w = np.exp(lw - float(shift))
    return np.array([f.size, w.sum(), (w * f).sum(), (w * w).sum(), ((w * f) ** 2).sum(), (w * w * f).sum()])


def estimate_from_terms(terms, self_normalised=False, shift=0.0):
    """(mean, standard error, effective sample size) from reduce_terms' vector (summed over shards).
    Plain: mean = sum(w f) / n, the unbiased estimate when w is a likelihood ratio, with the standard
    error of the sample mean of w f.  Self-normalised: mean = sum(w f) / sum(w), with the
    delta-method error sqrt(sum w^2 (f - mean)^2) / sum(w).  The effective sample size is
    (sum w)^2 / sum(w^2) either way."""
    v = np.asarray(terms, np.float64)
    n, sw, swf, sw2, swf2, sw2f = (float(v[i]) for i in range(T_COUNT))
    ess = sw * sw / sw2 if sw2 > 0 else 0.0
    if self_normalised:
        if not sw > 0:
            raise ValueError("every weight is zero")
        mean = swf / sw
        var = max(swf2 - 2.0 * mean * sw2f + mean * mean * sw2, 0.0)
        return mean, float(np.sqrt(var) / sw), ess
    scale = float(np.exp(shift))
    mean = swf / n
    var = max(swf2 / n - mean * mean, 0.0) * (n / (n - 1.0)) if n > 1 else 0.0
    return mean * scale, float(np.sqrt(var / n)) * scale, ess


def estimate(values, logw, self_normalised=False):
    """(mean, standard error, effective sample size) of the weighted estimate of E[values] from per-ego
    values and log-weights (estimate_from_terms' two forms).  Safe for large |logw|: the weights are
    taken relative to the largest one, which the self-normalised form cancels and the plain form
    multiplies back in at the end."""
    f, lw = _args(values, logw)
    shift = float(lw.max())
    if not np.isfinite(shift):
        shift = 0.0
    return estimate_from_terms(reduce_terms(f, lw, shift), self_normalised, shift)


def lineage(ancestor_history):
    """The slots a resampled population's final egos lived in.  ancestor_history: the ancestor arrays
    [B] of R resamplings in time order (BatchPlan.resample; number r was applied between loop
    segments r and r + 1).  Returns int64 [B, R + 1]: entry (e, s) is the slot final ego e occupied
    during segment s -- its last column is e itself, and column s is ancestor_s[column s + 1].  An
    ego's full trajectory is read out of a LoopRecording (whose rows stay addressed by slot) as the
    rows of segment s at slot lineage[e, s]."""
    hist = [np.asarray(a).ravel().astype(np.int64) for a in ancestor_history]
    if not hist:
        raise ValueError("at least one ancestor array")
    B = hist[0].size
    if any(a.size != B for a in hist) or any(a.min() < 0 or a.max() >= B for a in hist):
        raise ValueError(f"every ancestor array must hold {B} entries in [0, {B})")
    out = np.empty((B, len(hist) + 1), np.int64)
    out[:, -1] = np.arange(B)
    for s in range(len(hist) - 1, -1, -1):
        out[:, s] = hist[s][out[:, s + 1]]
    return out


def exact_expectation(values, logp):
    """sum_paths exp(logp) values over a full enumeration (script mode's ENV_LOGW), and the total
    probability sum_paths exp(logp), which is 1 up to rounding when every path is there."""
    f, lw = _args(values, logp)
    w = np.exp(lw)
    return float((w * f).sum()), float(w.sum())


def paired_difference(a, b):
    """(mean of a - b, its standard error, the sample correlation of a and b) for per-ego values of
    two runs over the same episodes (scenarios.controller_comparison: the same initial states and
    the same seeds, so ego e of both runs meets the same draws).  The standard error is that of the
    sample mean of the differences, sqrt(var(a - b) / n) with the n - 1 variance (0 for n = 1): the
    positive correlation of paired episodes is what makes it smaller than that of two independent
    runs.  The correlation is nan when either side is constant.  Plain and unweighted on purpose:
    the log-weights of a tilted run are likelihood ratios of each ego's realised choice sequence,
    which depend on the states the choices were drawn at, hence on the controller -- two controllers'
    weighted runs have different weights per ego, and a difference of their per-ego values is no
    estimate of anything; compare montecarlo.estimate's two results instead."""
    x, y = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    if x.shape != y.shape or x.size == 0:
        raise ValueError(f"a and b must hold one entry per ego, got {x.shape} and {y.shape}")
    d = x - y
    n = d.size
    se = float(np.sqrt(d.var(ddof=1) / n)) if n > 1 else 0.0
    sx, sy = x.std(), y.std()
    corr = float(((x - x.mean()) * (y - y.mean())).mean() / (sx * sy)) if sx > 0 and sy > 0 else float("nan")
    return float(d.mean()), se, corr
