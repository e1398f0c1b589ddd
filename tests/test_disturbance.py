"""The actuation disturbance of the device closed loops (bmpc_set_disturbance), host side.

The variate of csrc/bmpc_rng.h as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/hostsim/disturbance_host.cpp); the scene steps' host build
(tests/hostsim/scene_host.cpp) as a shared library: its draws against bmpc/rng.py exactly, the variate's moments, the three scene functions with a disturbance against an
undisturbed call on NumPy-perturbed inputs bit for bit, and law NONE / sigma 0 against the scene
functions' former argument list; the ctypes mirror, the argument validation and the population
entries' plumbing.  The GPU side is tests/test_disturbance_gpu.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import disturbance_common as D
import hostbuild
import scene_common as SC
from bmpc import abi, plan, rng, scenarios
from common import REPO

STEPS, B = 8, 65


def test_host_program_under_sanitizers(tmp_path):
    """Known answers of xi through bmpc_rng.h, its extremes -+ 2 (2^32 - 1) K at the all-zero and
    all-ones output words, counters with g >= 2^32 and seed >= 2^32, and sigma = 0 changing nothing."""
    r = hostbuild.sanitized_program("disturbance_host.cpp", tmp_path, flags=["-ffp-contract=off"])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def test_variate_known_answers():
    """bmpc/rng.py's own extremes and scale, and the values the C++ program holds."""
    K = rng.DISTURBANCE_SCALE
    assert K == float.fromhex("0x1.bb67ae8584caap-32") and abs(K * 2.0 ** 32 - np.sqrt(3.0)) < 1e-15
    assert rng.ih4([0] * 4) == -2 * (2 ** 32 - 1) * K and rng.ih4([0xffffffff] * 4) == 2 * (2 ** 32 - 1) * K
    assert rng.ih4([0xffffffff, 0, 0xffffffff, 0]) == 0.0
    assert rng.ih4([0xffffffff] * 4) < 2 * np.sqrt(3.0)
    got = rng.disturbance(7, 0, 3, "ego", 2)
    assert [float(v).hex() for v in got] == ["0x1.46d85550b5cdfp+1", "-0x1.167cc2e809c2fp+0"]
    assert float(rng.disturbance(2 ** 64 - 1, 2 ** 32, 4, "obstacle", 1)[0]).hex() == "-0x1.223920708af30p+0"
    assert rng.DISTURBANCE_PURPOSE == {"obstacle": 8, "ego": 12} and rng.PURPOSE_OBSTACLE_POLICY == 0
    for bad in (dict(vehicle="both"), dict(d=0), dict(d=5), dict(seed=-1)):
        with pytest.raises(ValueError):
            rng.disturbance(**{**dict(seed=0, ego=0, step=0, vehicle="ego", d=2), **bad})


def test_draws_equal_numpy_restatement():
    """xi of the C++ header equals bmpc/rng.py's exactly over 1,000 random (seed, ego, step) addresses
    x all 8 purposes, egos and seeds beyond 2^32 among them."""
    g = np.random.default_rng(11)
    n = 1000
    seed = g.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, n, dtype=np.uint64)
    ego = g.integers(0, 2 ** 40, n, dtype=np.uint64)
    step = g.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seed[:4] = [0, 7, 2 ** 32, 2 ** 64 - 1]
    ego[:4] = [65535, 2 ** 33 + 5, 0, 2 ** 32]
    step[:4] = [0, 1, 2 ** 32 - 1, 4]
    want = np.concatenate([rng.disturbance(seed, ego, step, v, 4) for v in ("obstacle", "ego")], axis=-1)   # [n, 8]
    assert want.shape == (n, 8)
    got = np.zeros((n, 8))
    for c in range(8):
        col = np.zeros(n)
        SC.shim().dh_xi(n, SC._p(seed), SC._p(ego), SC._p(step), SC._p(np.full(n, 8 + c, np.uint32)), SC._p(col))
        got[:, c] = col
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(got)) == got.size and np.all(np.abs(got) <= 2 * np.sqrt(3.0))
    # vectorised like obstacle_uniform: the arguments broadcast, the components are the last axis
    grid = rng.disturbance(7, np.arange(5)[:, None], np.arange(3)[None, :], "ego", 2)
    assert grid.shape == (5, 3, 2) and np.array_equal(grid[4, 2], rng.disturbance(7, 4, 2, "ego", 2))
    assert np.array_equal(rng.disturbance(7, 4, 2, "ego", 4)[:2], grid[4, 2])


def test_moments():
    """Seed 7, egos 0..4095, steps 0..15: n = 65,536 per purpose (deterministic: purposes 8 / 9 / 12 / 13
    have means 0.0017 / 0.0053 / 0.0044 / -0.0038, variances 1.0008 / 1.0088 / 0.9914 / 0.9933, kurtosis
    2.69-2.71, max |xi| 3.31, correlations below 0.006).  Bars: |mean| <= 4 / sqrt(n) = 0.0156,
    |var - 1| <= 0.02 (4 standard errors), kurtosis in [2.6, 2.8], |xi| <= 2 sqrt(3), |corr| <= 0.016
    between purposes and at lag 1 over the steps."""
    e, t = np.arange(4096)[:, None], np.arange(16)[None, :]
    xi = np.concatenate([rng.disturbance(7, e, t, v, 2) for v in ("obstacle", "ego")], axis=-1)   # [4096, 16, 4]
    n = 4096 * 16
    flat = xi.reshape(n, 4)
    mean, var = flat.mean(0), flat.var(0)
    kurt = ((flat - mean) ** 4).mean(0) / var ** 2
    print("means", mean, "variances", var, "kurtosis", kurt, "max", np.abs(flat).max())
    assert np.all(np.abs(mean) <= 4 / np.sqrt(n))
    assert np.all(np.abs(var - 1) <= 0.02)
    assert np.all((kurt >= 2.6) & (kurt <= 2.8))
    assert np.abs(flat).max() <= 2 * np.sqrt(3.0)
    corr = np.corrcoef(flat.T)
    lag = [np.corrcoef(xi[:, :-1, c].ravel(), xi[:, 1:, c].ravel())[0, 1] for c in range(4)]
    print("corr", np.abs(corr - np.eye(4)).max(), "lag-1", lag)
    assert np.abs(corr - np.eye(4)).max() <= 0.016 and np.max(np.abs(lag)) <= 0.016


@pytest.mark.parametrize("kind", SC.KINDS)
def test_host_scene_equals_perturbed_inputs(kind):
    """65 egos, 8 teacher-forced steps: a disturbed call equals an undisturbed call whose u0 and
    obstacle-input slot hold nominal + sigma * bmpc.rng.disturbance(...) formed in NumPy, bit for bit
    in scene, x, z and xref (merge: S and bx too); a shard with ego_base = 40 takes the rows of the
    whole batch; an undisturbed run differs."""
    sc = SC.Scene(kind, B)
    dist = D.make(kind)
    got, pol = SC.host_run(sc, STEPS, dist=dist)
    twin, pol_t = SC.host_run(sc, STEPS, twin=D.twin(kind, dist))
    D.assert_same_but_uobs(kind, got, twin)
    assert (pol is None and pol_t is None) or bytes(pol) == bytes(pol_t)
    plain, _ = SC.host_run(sc, STEPS)
    assert not np.array_equal(plain[-1]["x"], got[-1]["x"]) and not np.array_equal(plain[-1]["z"], got[-1]["z"])
    assert np.array_equal(plain[0]["scene"], got[0]["scene"])          # step 0 has no Euler step
    part, _ = SC.host_run(sc, STEPS, dist=D.make(kind, ego_base=40), egos=slice(40, 60))
    for a, b in zip(got, part):
        for k in set(b) - {"pol"}:
            assert np.array_equal(a[k][40:60], b[k]), k
    # one channel at a time: sigma_ego alone leaves the obstacle alone, and the other way round
    zero = (0.0,) * D.slot(kind)[1]
    ego_only, _ = SC.host_run(sc, STEPS, dist=D.make(kind, sigma_obs=zero))
    obs_only, _ = SC.host_run(sc, STEPS, dist=D.make(kind, sigma_ego=zero))
    if kind == "merge":   # (the other scenes' obstacles react to the ego)
        assert np.array_equal(ego_only[-1]["z"], plain[-1]["z"]) and np.array_equal(obs_only[-1]["x"], plain[-1]["x"])
    assert not np.array_equal(ego_only[-1]["x"], plain[-1]["x"]) and not np.array_equal(obs_only[-1]["z"], plain[-1]["z"])


@pytest.mark.parametrize("kind", SC.KINDS)
def test_off_is_the_former_function(kind):
    """Law NONE with non-zero sigmas, law IH4 with all sigmas zero and no disturbance at all reproduce
    the scene function's former argument list bit for bit over the same 8 steps."""
    sc = SC.Scene(kind, B)
    ref, ref_pol = SC.host_run(sc, STEPS, arglist=1)
    zero = (0.0,) * D.slot(kind)[1]
    for dist in (D.make(kind, law=abi.DISTURB_NONE, seed=2 ** 63 + 99, ego_base=12),
                 D.make(kind, sigma_ego=zero, sigma_obs=zero), None):
        got, got_pol = SC.host_run(sc, STEPS, dist=dist)
        D.assert_same_but_uobs(kind, ref, got)
        assert (ref_pol is None and got_pol is None) or bytes(ref_pol) == bytes(got_pol)


# ---- the Python surface -----------------------------------------------------------------------

FIELDS = ("law", "reserved", "seed", "ego_base", "sigma_ego", "sigma_obs")


def test_disturbance_layout_matches_header(tmp_path):
    offs = ", ".join(f"offsetof(bmpc_disturbance, {f})" for f in FIELDS)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("' + "%zu " * (1 + len(FIELDS)) + '%d %d %d\\n", sizeof(bmpc_disturbance), ' + offs
            + ', (int)BMPC_DISTURB_NONE, (int)BMPC_DISTURB_IH4, (int)BMPC_MAX_D);return 0;}\n')
    got = hostbuild.header_program(tmp_path, code, cxx=True)   # (C++: the header's own static_assert)
    S = abi.Disturbance
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [abi.DISTURB_NONE, abi.DISTURB_IH4, abi.MAX_D]
    assert got[:7] == [88, 0, 4, 8, 16, 24, 56]
    assert "static_assert(sizeof(bmpc_disturbance) ==" in open(os.path.join(REPO, "include", "bmpc.h")).read()


def test_make_disturbance_validates():
    s = abi.make_disturbance((0.3, 0.01), (0.5,), seed=2 ** 64 - 1, ego_base=2 ** 40)
    assert (s.law, s.reserved, s.seed, s.ego_base) == (abi.DISTURB_IH4, 0, 2 ** 64 - 1, 2 ** 40)
    assert list(s.sigma_ego) == [0.3, 0.01, 0, 0] and list(s.sigma_obs) == [0.5, 0, 0, 0]
    assert list(abi.make_disturbance(None, 0.25).sigma_obs) == [0.25, 0, 0, 0]
    assert abi.make_disturbance(law=abi.DISTURB_NONE).law == 0
    for bad in (dict(sigma_ego=(-0.1,)), dict(sigma_obs=(np.nan,)), dict(sigma_ego=(np.inf,)), dict(sigma_ego=(1,) * 5),
                dict(sigma_ego=(1, 1, 1), d=2), dict(sigma_obs=np.ones((2, 2))), dict(law=2), dict(seed=-1),
                dict(seed=2 ** 64), dict(ego_base=-1), dict(ego_base=1.5)):
        with pytest.raises(ValueError):
            abi.make_disturbance(**bad)


class FakeLib:
    """bmpc_set_disturbance of a library that is not there: records what it was handed."""

    def __init__(self):
        self.calls = []

    def bmpc_set_disturbance(self, h, ref):
        s = None if ref is None else ref._obj
        self.calls.append(None if s is None else (s.law, s.seed, s.ego_base, list(s.sigma_ego), list(s.sigma_obs)))
        return 0


def test_plan_set_disturbance_marshals(monkeypatch):
    from bmpc import _lib
    assert "bmpc_set_disturbance" in _lib.EXPORTED
    fake = FakeLib()
    monkeypatch.setattr(plan, "lib", lambda: fake)
    pl = object.__new__(plan.BatchPlan)
    pl._h = None                                    # (nothing to destroy)
    pl.desc = scenarios.highway_desc(N=6, NB=1)
    pl.set_disturbance((0.3, 0.01), (0.5, 0.02), seed=9, ego_base=40)
    assert pl.disturbance.ego_base == 40
    pl.set_disturbance(sigma_obs=(0.5,))
    pl.set_disturbance(abi.make_disturbance((1.0,), law=abi.DISTURB_NONE))
    pl.set_disturbance()
    assert pl.disturbance is None
    assert fake.calls == [(1, 9, 40, [0.3, 0.01, 0, 0], [0.5, 0.02, 0, 0]), (1, 0, 0, [0.0] * 4, [0.5, 0, 0, 0]),
                          (0, 0, 0, [1.0, 0, 0, 0], [0.0] * 4), None]
    for bad in (dict(sigma_ego=(0.1, 0.1, 0.1)), dict(sigma_ego=(-1,)), dict(sigma_ego=(1,), seed=-1)):
        with pytest.raises(ValueError):
            pl.set_disturbance(**bad)
    assert len(fake.calls) == 4                     # refused before the library saw it


def test_population_entries_plumb_the_disturbance():
    """disturbed_*_population take sigma_ego / sigma_obs / disturbance_seed and the sampled entries'
    ego_base / population (overtake and quadruped: obstacle / obstacle_seed / hold too); the attach
    helper hands them to the plan; the existing entries keep their parameter lists."""
    common = ["B", "steps", "sigma_ego", "sigma_obs", "disturbance_seed", "seed", "device", "record"]
    for fn in (scenarios.disturbed_overtake_population, scenarios.disturbed_quadruped_population):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == common + ["obstacle", "obstacle_seed", "hold", "ego_base", "population",
                                                 "desc"], fn.__name__
        d = {k: v.default for k, v in sig.parameters.items()}
        assert (d["sigma_ego"], d["sigma_obs"], d["disturbance_seed"], d["obstacle"], d["hold"], d["ego_base"]) == \
            (None, None, 0, None, 1, 0)
    assert list(inspect.signature(scenarios.disturbed_merge_population).parameters) == common + ["ego_base", "population"]
    assert list(inspect.signature(scenarios.merge_population).parameters) == ["B", "steps", "seed", "device", "record"]
    # one driver takes every scene's plan: no scene has a loop of its own with its own parameter list
    assert list(inspect.signature(scenarios._closed_loop).parameters)[:5] == ["pl", "scene0", "steps", "record", "device"]
    assert not [n for n in vars(scenarios) if n.endswith("_loop") and n != "_closed_loop"]

    class Plan:
        def set_disturbance(self, sigma_ego, sigma_obs, seed, ego_base):
            self.disturbance = (sigma_ego, sigma_obs, seed, ego_base)

    pl = Plan()
    assert scenarios._attach_disturbance(pl, None, None, 1, 3) is None and not hasattr(pl, "disturbance")
    assert scenarios._attach_disturbance(pl, (0.3,), None, 5, 40) == ((0.3,), None, 5, 40)
    assert scenarios._attach_disturbance(pl, None, (0.5, 0.02), 6, 0) == (None, (0.5, 0.02), 6, 0)
