"""Resampling a weighted population (bmpc_population_ancestors / bmpc_gather_egos /
bmpc_resample_device), host side.

The per-element rules of csrc/bmpc_resample.h as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/hostsim/resample_host.cpp); the same file as a shared library
against bmpc/resample.py -- equal integers given the library's own k; the properties of the NumPy
restatement itself; the draw; montecarlo.lineage; the preservation of the mean weight; the ctypes
mirror, the validation and the population entries' signatures.  The GPU side is
tests/test_resample_gpu.py."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import hostbuild
import resample_common as R
from bmpc import abi, montecarlo, plan, resample, rng, scenarios
from common import REPO

SIZES = (1, 2, 3, 63, 64, 65, 257, 1000)
DRAWS = (0, 1, 2 ** 53 - 1, 0x123456789ABCD, 0x1F0E0D0C0B0A09)


def test_host_program_under_sanitizers(tmp_path):
    """The rule over the batch sizes and weight families with its properties, the conversion's rounding,
    the refusals, and synthetic slabs gathered through a permutation, a broadcast, clamped entries and
    the rule's own arrangement, compiled with -fsanitize=address,undefined and run once."""
    r = hostbuild.sanitized_program("resample_host.cpp", tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def test_resample_desc_layout_matches_header(tmp_path):
    fields = ("scheme", "round", "ess_fraction", "seed", "ego_base")
    offs = ", ".join(f"offsetof(bmpc_resample_desc, {f})" for f in fields)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("' + "%zu " * (2 + len(fields)) + '%d %d %d\\n", sizeof(bmpc_resample_desc), '
            + offs + ', sizeof(bmpc_ego_buffers), (int)BMPC_RESAMPLE_NINFO, (int)BMPC_RESAMPLE_SYSTEMATIC, '
            '(int)BMPC_RESAMPLE_MAX_BATCH);return 0;}\n')
    got = hostbuild.header_program(tmp_path, code, cxx=True)
    D = abi.ResampleDesc
    assert [n for n, _ in D._fields_] == list(fields)
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields] + [
        C.sizeof(abi.EgoBuffers), abi.RESAMPLE_NINFO, abi.RESAMPLE_SYSTEMATIC, abi.RESAMPLE_MAX_BATCH]
    assert got == [32, 0, 4, 8, 16, 24, 72, 8, 0, 1 << 20]
    assert [n for n, _ in abi.EgoBuffers._fields_] == ["scene", "upred", "x", "z", "xref", "J", "status", "iters", "stats"]
    assert "static_assert(sizeof(bmpc_resample_desc) == 32" in open(os.path.join(REPO, "include", "bmpc.h")).read()


@pytest.mark.parametrize("B", SIZES)
def test_host_rule_equals_numpy_given_its_k(B):
    """Per family and draw: ancestors and counts of the host build are bmpc.resample's, as equal
    integers, from the host build's own k; that k is NumPy's within one unit; ess is bit-equal given k;
    the new log-weight agrees within 1e-15 relative."""
    for fam in R.FAMILIES:
        lw = R.family(fam, B)
        k, M, bad = R.host_quantise(lw)
        kn, Mn = resample.quantise(lw)
        assert bad == 0 and M == Mn
        assert np.abs(k.astype(np.int64) - kn.astype(np.int64)).max() <= 1
        assert int(k.max()) == 2 ** 40 and np.all(k[np.isneginf(lw)] == 0)
        assert R.host_ess(k) == resample.ess(k)
        S = sum(int(v) for v in k)
        got, want = R.shim().rs_new_logw(M, S, B), resample.new_logw(M, S, B)
        assert abs(got - want) <= 1e-15 * max(abs(want), 1.0)
        for u53 in DRAWS:
            anc, counts = R.host_ancestors(k, u53)
            want_anc, want_counts = resample.ancestors(k, u53)
            assert np.array_equal(anc, want_anc) and np.array_equal(counts, want_counts), (fam, u53)
            assert anc.dtype == want_anc.dtype == np.int32


@pytest.mark.parametrize("B", SIZES)
def test_restatement_properties(B):
    """bmpc.resample by itself: raw ancestors non-decreasing, counts sum to B, floor(B k / S) <= n <=
    ceil(B k / S), survivors stay, the dead slots take the surplus list in order, sources are never
    destinations, and equal weights give the identity for every draw."""
    for fam in R.FAMILIES:
        k, _ = resample.quantise(R.family(fam, B))
        for u53 in DRAWS:
            anc, counts = resample.ancestors(k, u53)
            R.check_properties(k, u53, anc, counts)
            if fam == "equal":
                assert np.array_equal(anc, np.arange(B))


def test_conversion_rounds_like_python():
    g = np.random.default_rng(3)
    vals = [2 ** 64, 2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 + 1, 2 ** 64 + 3 * 2 ** 11, 2 ** 100 - 1, 2 ** 128 - 1]
    vals += [int(g.integers(1, 2 ** 62)) * int(g.integers(1, 2 ** 62)) + int(g.integers(0, 2 ** 40)) for _ in range(200)]
    for v in vals:
        assert R.shim().rs_to_double(v >> 64, v & (2 ** 64 - 1)) == float(v), v


def test_the_draw():
    """resample.offset is Philox4x32-10 at counter {lo32(ego_base), hi32(ego_base), round, 1}, key = seed;
    the host build draws the same integer; purpose 1 is not the obstacle's draw of the same address."""
    for seed, base, rnd in ((7, 0, 0), (7, 32, 4), (2 ** 64 - 1, 2 ** 40 + 5, 2 ** 32 - 1), (0, 1, 2)):
        o = rng.philox4x32([base & 0xFFFFFFFF, base >> 32, rnd, 1], [seed & 0xFFFFFFFF, seed >> 32])
        u53 = resample.offset(seed, base, rnd)
        assert u53 == ((int(o[0]) >> 5) << 26) | (int(o[1]) >> 6) and 0 <= u53 < 2 ** 53
        assert u53 * 2.0 ** -53 == float(rng.uniform53(o[0], o[1]))
        assert R.shim().rs_u53(seed, base, rnd) == u53
        assert u53 * 2.0 ** -53 != float(rng.obstacle_uniform(seed, base, rnd))
    assert resample.PURPOSE_RESAMPLE == 1 != rng.PURPOSE_OBSTACLE_POLICY
    assert resample.offset(7, 0, 1) != resample.offset(7, 32, 1) != resample.offset(7, 32, 2)
    for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 2 ** 32), (2 ** 64, 0, 0)):
        with pytest.raises(ValueError):
            resample.offset(*bad)


def test_lineage():
    a1 = [0, 0, 2, 2]          # after segment 0: slot 1 continues ego 0, slot 3 ego 2
    a2 = [0, 1, 1, 3]          # after segment 1: slot 2 continues slot 1
    lin = montecarlo.lineage([a1, a2])
    assert lin.dtype == np.int64 and lin.tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 2], [2, 3, 3]]
    assert montecarlo.lineage([np.arange(5)] * 3).tolist() == [[e] * 4 for e in range(5)]
    for bad in ([], [[0, 1], [0, 1, 2]], [[0, 2]], [[-1, 0]]):
        with pytest.raises(ValueError):
            montecarlo.lineage(bad)


@pytest.mark.parametrize("B", (2, 65, 1000))
def test_mean_weight_is_preserved(B):
    """mean(exp(new logw)) = mean(exp(logw)) within resample_common.mean_weight_bound(B): B 2^-40 of
    quantisation plus 64 ulp of rounding, relative."""
    for fam in ("sd1", "sd5", "sd30", "half_dead"):
        lw = R.family(fam, B)
        anc, info = resample.resample(lw, seed=3, round=5, ess_fraction=2.0)
        assert info[abi.R_RESAMPLED] == 1.0 and info[abi.R_SURVIVORS] == len(np.unique(anc))
        before, after = np.exp(lw).mean(), math.exp(info[abi.R_NEW_LOGW])
        print(fam, B, "relative change of the mean weight", after / before - 1.0, "bound", R.mean_weight_bound(B))
        assert abs(after / before - 1.0) <= R.mean_weight_bound(B)
        # ... and the decision: ess_fraction 0 never resamples, the identity comes back
        same, info0 = resample.resample(lw, seed=3, round=5, ess_fraction=0.0)
        assert info0[abi.R_RESAMPLED] == 0.0 and np.array_equal(same, np.arange(B)) and info0[abi.R_ESS] == info[abi.R_ESS]


def test_refusing_log_weights():
    for bad in (np.nan, np.inf):
        lw = np.array([0.0, -1.0, bad, -2.0])
        anc, info = resample.resample(lw, ess_fraction=2.0)
        assert np.array_equal(anc, np.arange(4)) and info[abi.R_RESAMPLED] == 0.0 and info[abi.R_NONFINITE] == 1.0
        assert R.host_quantise(lw)[2] == 1
        with pytest.raises(ValueError):
            resample.quantise(lw)
    anc, info = resample.resample(np.full(3, -np.inf), ess_fraction=2.0)
    assert np.array_equal(anc, np.arange(3)) and info[abi.R_RESAMPLED] == 0.0 and info[abi.R_MAX] == -np.inf
    k, M = resample.quantise(np.full(3, -np.inf))
    assert M == -np.inf and not k.any()


def test_make_resample_desc_validates():
    d = abi.make_resample_desc(12, seed=2 ** 64 - 1, ess_fraction=0.25, ego_base=32)
    assert (d.scheme, d.round, d.ess_fraction, d.seed, d.ego_base) == (0, 12, 0.25, 2 ** 64 - 1, 32)
    for bad in (dict(round=-1), dict(round=2 ** 32), dict(round=1.5), dict(round=0, seed=-1), dict(round=0, seed=2 ** 64),
                dict(round=0, ess_fraction=-0.1), dict(round=0, ess_fraction=np.nan), dict(round=0, ess_fraction=np.inf),
                dict(round=0, ego_base=-1), dict(round=0, scheme=1)):
        with pytest.raises(ValueError):
            abi.make_resample_desc(**bad)
    e = abi.make_ego_buffers(scene=4096, J=None, status=8192)
    assert (e.scene, e.J, e.status, e.upred) == (4096, None, 8192, None)
    with pytest.raises(ValueError):
        abi.make_ego_buffers(scenes=1)


def test_entries_are_declared_and_plumbed():
    from bmpc import _lib
    for name in ("bmpc_population_ancestors", "bmpc_gather_egos", "bmpc_resample_device"):
        assert name in _lib.EXPORTED
    assert list(inspect.signature(plan.BatchPlan.resample).parameters) == [
        "self", "buffers", "round", "seed", "ess_fraction", "ego_base", "stream"]
    assert list(inspect.signature(plan.BatchPlan.gather_egos).parameters) == ["self", "ancestor", "buffers", "stream"]
    assert callable(plan.population_ancestors)
    weighted = list(inspect.signature(scenarios.weighted_overtake_population).parameters)
    for fn in (scenarios.resampled_overtake_population, scenarios.resampled_quadruped_population):
        names = list(inspect.signature(fn).parameters)
        assert names[:6] == ["B", "steps", "resample_every", "ess_fraction", "resample_seed", "tilt"], fn.__name__
        assert sorted(names[6:]) == sorted(a for a in weighted if a not in ("B", "steps", "tilt"))
        assert inspect.signature(fn).parameters["ess_fraction"].default == 0.5
        assert "distributed.shard" in fn.__doc__
