"""Shared by tests/test_resample.py and tests/test_resample_gpu.py: the host build of the population
resampling's rules (tests/hostsim/resample_host.cpp), the weight families of the ancestor tests and
the checks both sides apply to a set of ancestors."""
import ctypes as C
import os

import numpy as np

import hostbuild
from bmpc import resample
from common import HERE

SRC = os.path.join(HERE, "hostsim", "resample_host.cpp")
_shim = None


def shim():
    """The shared-library build of the host file (hostbuild.shared), with its prototypes."""
    global _shim
    if _shim is None:
        _shim = hostbuild.shared("resample", [SRC])
        _shim.rs_u53.restype = C.c_uint64
        _shim.rs_u53.argtypes = [C.c_uint64, C.c_int64, C.c_uint32]
        _shim.rs_ess.restype = C.c_double
        _shim.rs_new_logw.restype = C.c_double
        _shim.rs_new_logw.argtypes = [C.c_double, C.c_uint64, C.c_int]
        _shim.rs_to_double.restype = C.c_double
        _shim.rs_to_double.argtypes = [C.c_uint64, C.c_uint64]
    return _shim


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_quantise(logw):
    lw = np.ascontiguousarray(logw, np.float64)
    k, M = np.zeros(lw.size, np.uint64), C.c_double()
    bad = shim().rs_quantise(lw.size, _p(lw), _p(k), C.byref(M))
    return k, M.value, bad


def host_ancestors(k, u53):
    k = np.ascontiguousarray(k, np.uint64)
    anc, counts = np.zeros(k.size, np.int32), np.zeros(k.size, np.int32)
    shim().rs_ancestors(k.size, _p(k), C.c_uint64(int(u53)), _p(anc), _p(counts))
    return anc, counts


def host_ess(k):
    k = np.ascontiguousarray(k, np.uint64)
    return shim().rs_ess(k.size, _p(k))


FAMILIES = ("equal", "sd1", "sd5", "sd30", "sd100", "half_dead")


def family(name, B, seed=0):
    """Log-weights [B] of one of the issue's families (deterministic)."""
    g = np.random.default_rng([seed, B, FAMILIES.index(name)])
    if name == "equal":
        return np.full(B, -2.75)
    if name == "half_dead":
        lw = g.normal(0.0, 1.0, B)
        lw[g.permutation(B)[:B // 2]] = -np.inf
        return lw
    return g.normal(0.0, float(name[2:]), B)


def check_properties(k, u53, anc, counts):
    """The properties of the rule for integer weights k at the draw u53 (exact Python integers)."""
    ks = [int(v) for v in k]
    B, S = len(ks), sum(ks)
    raw = resample.raw_ancestors(k, u53)
    assert np.all(np.diff(raw) >= 0)
    assert np.array_equal(np.bincount(raw, minlength=B), counts) and int(np.sum(counts)) == B
    for i in range(B):
        assert (B * ks[i]) // S <= counts[i] <= -((-B * ks[i]) // S), (i, ks[i], counts[i])
    alive = np.asarray(counts) > 0
    assert np.array_equal(np.asarray(anc)[alive], np.flatnonzero(alive))
    assert np.array_equal(np.asarray(anc)[~alive], np.repeat(np.arange(B), np.maximum(np.asarray(counts) - 1, 0)))
    assert alive[np.asarray(anc)].all()          # sources are never destinations


def mean_weight_bound(B):
    """The relative bound on |mean(exp(new logw)) / mean(exp(logw)) - 1| after a resampling: every k_i
    loses less than one unit of 2^-40 against exp(logw_i - M) <= 1 while the mean of exp(logw - M) is at
    least 1 / B (the maximum contributes 1), so the quantisation costs at most B 2^-40 relative; the
    exp / log / sum roundings of the two sides (a few ulp each, the NumPy pairwise sum's log2(B) ulp)
    are covered by 64 ulp."""
    return B * 2.0 ** -40 + 64 * 2.0 ** -52
