"""The observation noise of the device closed loops (bmpc_set_observation), host side.

The variate at the two new purpose bases and rng_observe_state as a stand-alone program under the
address and undefined-behaviour sanitizers (tests/hostsim/observation_host.cpp); the device header's
draws through the shared host build against bmpc/rng.py exactly; the variate's moments over the 16
purposes; the three scene functions with an observation model against the plain call plus NumPy's
noise, bit for bit; null, law NONE and sigma 0 against the scene functions' former argument list; the
ctypes mirror, the argument validation and the population entries' plumbing.  The GPU side is
tests/test_observation_gpu.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import hostbuild
import observation_common as O
import scene_common as SC
from bmpc import abi, plan, rng, scenarios
from common import REPO

STEPS, B = 8, 65


def test_host_program_under_sanitizers(tmp_path):
    """Known answers of xi at purposes 16.. and 24.., its extremes -+ 2 (2^32 - 1) K at the all-zero and
    all-ones output words, counters with g >= 2^32 and seed >= 2^32, sigma = 0 changing nothing, and one
    step of each scene with arrays of their exact sizes -- nothing preloaded."""
    r = hostbuild.sanitized_program("observation_host.cpp", tmp_path, flags=["-ffp-contract=off"])
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


FIELDS = ("law", "reserved", "seed", "ego_base", "sigma_x", "sigma_z")


def test_observation_layout_matches_header(tmp_path):
    offs = ", ".join(f"offsetof(bmpc_observation, {f})" for f in FIELDS)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("' + "%zu " * (1 + len(FIELDS)) + '%d %d %d %d\\n", sizeof(bmpc_observation), ' + offs
            + ', (int)BMPC_OBSERVE_NONE, (int)BMPC_OBSERVE_IH4, (int)BMPC_MAX_N, (int)BMPC_ABI_VERSION);return 0;}\n')
    got = hostbuild.header_program(tmp_path, code, cxx=True)   # (C++: the header's own static_assert)
    S = abi.Observation
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [abi.OBSERVE_NONE, abi.OBSERVE_IH4,
                                                                              abi.MAX_N, 2]
    assert got[:7] == [152, 0, 4, 8, 16, 24, 88] and got[7:9] == [0, 1]
    assert "static_assert(sizeof(bmpc_observation) ==" in open(os.path.join(REPO, "include", "bmpc.h")).read()


def test_draws_equal_numpy_restatement():
    """xi of the C++ header equals bmpc/rng.py's exactly over 1,000 random (seed, ego, step) addresses
    x the 16 purposes 16..31, egos and seeds beyond 2^32 among them; component c of a vehicle's
    observation is the variate of purpose base + c, and no draw is the disturbance's."""
    g = np.random.default_rng(13)
    n = 1000
    seed = g.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, n, dtype=np.uint64)
    ego = g.integers(0, 2 ** 40, n, dtype=np.uint64)
    step = g.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seed[:4] = [0, 7, 2 ** 32, 2 ** 64 - 1]
    ego[:4] = [65535, 2 ** 33 + 5, 0, 2 ** 32]
    step[:4] = [0, 1, 2 ** 32 - 1, 4]
    want = np.concatenate([rng.observation(seed, ego, step, v, 8) for v in ("obstacle", "ego")], axis=-1)   # [n, 16]
    assert want.shape == (n, 16)
    got = np.zeros((n, 16))
    for c in range(16):
        col = np.zeros(n)
        SC.shim().dh_xi(n, SC._p(seed), SC._p(ego), SC._p(step), SC._p(np.full(n, 16 + c, np.uint32)), SC._p(col))
        got[:, c] = col
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(got)) == got.size and np.all(np.abs(got) <= 2 * np.sqrt(3.0))
    assert rng.OBSERVATION_PURPOSE == {"obstacle": 16, "ego": 24}
    # component c is the IH4 of purpose base + c, whatever n
    for vehicle, base in rng.OBSERVATION_PURPOSE.items():
        for c in (0, 2, 7):
            counter = np.array([7, 0, 3, base + c], np.uint32)
            one = rng.ih4(rng.philox4x32(counter, np.array([9, 0], np.uint32)))
            assert rng.observation(9, 7, 3, vehicle, 8)[c] == one
            if c < 3:
                assert rng.observation(9, 7, 3, vehicle, 3)[c] == one
    # other purposes than the disturbance's: different numbers at the same (seed, g, t)
    for vehicle in ("obstacle", "ego"):
        assert not np.any(rng.observation(seed, ego, step, vehicle, 4) == rng.disturbance(seed, ego, step, vehicle, 4))
    # vectorised like disturbance: the arguments broadcast, the components are the last axis
    grid = rng.observation(7, np.arange(5)[:, None], np.arange(3)[None, :], "ego", 4)
    assert grid.shape == (5, 3, 4) and np.array_equal(grid[4, 2], rng.observation(7, 4, 2, "ego", 4))
    assert [float(v).hex() for v in rng.observation(7, 1, 3, "obstacle", 2)] == ["-0x1.fb612af7eee0fp-2",
                                                                                 "-0x1.5d417cb0ecdbdp-1"]
    for bad in (dict(vehicle="both"), dict(n=0), dict(n=9), dict(seed=-1), dict(step=2 ** 32)):
        with pytest.raises(ValueError):
            rng.observation(**{**dict(seed=0, ego=0, step=0, vehicle="ego", n=4), **bad})


def test_moments():
    """Seed 11, egos 0..4095, steps 0..15: n = 65,536 draws per purpose, the 16 purposes 16..31.  Bars
    (those of the disturbance's check): |mean| <= 4 / sqrt(n) = 0.0156, |var - 1| <= 0.02 (4 standard
    errors of the variance of a kurtosis-2.7 variate: 4 sqrt(1.7 / n) = 0.0204), kurtosis in [2.6, 2.8],
    |xi| <= 2 sqrt(3), |corr| <= 4 / sqrt(n) between purposes and at lag 1 over the steps."""
    e, t = np.arange(4096)[:, None], np.arange(16)[None, :]
    xi = np.concatenate([rng.observation(O.SEED, e, t, v, 8) for v in ("obstacle", "ego")], axis=-1)   # [4096, 16, 16]
    n = 4096 * 16
    flat = xi.reshape(n, 16)
    mean, var = flat.mean(0), flat.var(0)
    kurt = ((flat - mean) ** 4).mean(0) / var ** 2
    print("means", mean, "variances", var, "kurtosis", kurt, "max", np.abs(flat).max())
    assert np.all(np.abs(mean) <= 4 / np.sqrt(n))
    assert np.all(np.abs(var - 1) <= 0.02)
    assert np.all((kurt >= 2.6) & (kurt <= 2.8))
    assert np.abs(flat).max() <= 2 * np.sqrt(3.0)
    corr = np.corrcoef(flat.T)
    lag = [np.corrcoef(xi[:, :-1, c].ravel(), xi[:, 1:, c].ravel())[0, 1] for c in range(16)]
    print("corr", np.abs(corr - np.eye(16)).max(), "lag-1", lag)
    assert np.abs(corr - np.eye(16)).max() <= 4 / np.sqrt(n) and np.max(np.abs(lag)) <= 4 / np.sqrt(n - 4096)


@pytest.fixture(scope="module", params=SC.KINDS)
def runs(request):
    """One scene at 65 egos over 8 teacher-forced steps: the plain run (the former argument list) and
    the run under the suggested observation model, computed once and never modified."""
    kind = request.param
    sc = SC.Scene(kind, B)
    return kind, sc, O.host_run(sc, STEPS, plain=True), O.host_run(sc, STEPS, O.make(kind))


KEPT = ("scene", "xref", "S", "bx", "stats", "pol")


def assert_truth_kept(plain, got):
    for t, (a, b) in enumerate(zip(plain, got)):
        for k in KEPT:
            if a.get(k) is not None:
                assert np.array_equal(a[k], b[k]) if not isinstance(a[k], bytes) else a[k] == b[k], (t, k)


def test_host_scene_equals_plain_plus_numpy_noise(runs):
    """The observed call's x_out / z_out equal the plain call's plus sigma * bmpc.rng.observation formed
    in NumPy, bit for bit, at every step (step 0 too: its solve sees an observation); scene row, x_ref,
    S, bx, policies and statistics equal the plain call's; a shard with ego_base = 40 takes the rows of
    the whole batch."""
    kind, sc, plain, got = runs
    obs = O.make(kind)
    assert_truth_kept(plain, got)
    n = O.width(kind)
    for t, (a, b) in enumerate(zip(plain, got)):
        x, z = O.observed(kind, obs, t, a["x"], a["z"], np.arange(B))
        assert np.array_equal(b["x"], x) and np.array_equal(b["z"], z), t
        assert np.all(b["x"] != a["x"]) and np.all(b["z"] != a["z"]), t
        # the plain outputs are the row's true states, so the observation is reproducible from the row
        xr, zr = O.observed_rows(kind, obs, t, b["scene"])
        assert np.array_equal(xr, b["x"]) and np.array_equal(zr, b["z"]), t
        assert np.array_equal(x, a["x"] + np.array(obs.sigma_x[:n]) * rng.observation(O.SEED, np.arange(B), t, "ego", n))
    part = O.host_run(sc, STEPS, O.make(kind, ego_base=40), egos=slice(40, 60))
    for a, b in zip(got, part):
        for k in ("x", "z", "xref", "scene"):
            assert np.array_equal(a[k][40:60], b[k]), k
    wrong = O.host_run(sc, 1, O.make(kind), egos=slice(40, 60))
    assert not np.array_equal(wrong[0]["z"], got[0]["z"][40:60])
    other = O.host_run(sc, 1, O.make(kind, seed=O.SEED + 1))
    assert np.all(other[0]["z"] != got[0]["z"]) and np.array_equal(other[0]["scene"], got[0]["scene"])


def test_off_is_the_former_function(runs):
    """A null pointer, law NONE with non-zero sigmas and law IH4 with all sigmas zero reproduce the
    scene function's former argument list bit for bit over the same 8 steps, x_out and z_out too."""
    kind, sc, plain, _ = runs
    zero = (0.0,) * O.width(kind)
    for obs in (None, O.make(kind, law=abi.OBSERVE_NONE, seed=2 ** 63 + 99, ego_base=12),
                O.make(kind, sigma_x=zero, sigma_z=zero)):
        got = O.host_run(sc, STEPS, obs)
        assert_truth_kept(plain, got)
        for a, b in zip(plain, got):
            assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["z"], b["z"])


def test_one_component_moves_that_component_only(runs):
    """A single non-zero sigma moves its component of its vector and nothing else; sigma_z only leaves
    x_out the row's x, sigma_x only leaves z_out the row's z."""
    kind, sc, plain, _ = runs
    n = O.width(kind)
    zero = (0.0,) * n
    for vehicle, key, other in (("sigma_x", "x", "z"), ("sigma_z", "z", "x")):
        for c in range(n):
            sg = tuple(0.25 if i == c else 0.0 for i in range(n))
            obs = O.make(kind, **{"sigma_x": zero, "sigma_z": zero, vehicle: sg})
            got = O.host_run(sc, 3, obs)
            assert_truth_kept(plain[:3], got)
            for t, (a, b) in enumerate(zip(plain, got)):
                assert np.array_equal(a[other], b[other])
                keep = np.arange(n) != c
                assert np.array_equal(a[key][:, keep], b[key][:, keep]) and np.all(a[key][:, c] != b[key][:, c])
                xi = rng.observation(O.SEED, np.arange(B), t, "ego" if key == "x" else "obstacle", n)[:, c]
                assert np.array_equal(b[key][:, c], a[key][:, c] + 0.25 * xi)


def test_observation_rides_beside_the_other_options():
    """Overtake with the tilted sampler (hold 2) and the disturbance attached: the observation model
    changes x_out / z_out alone -- the choices, ENV_LOGW and the Euler steps are the unobserved run's."""
    import disturbance_common as D
    sc = SC.Scene("overtake", B)
    prop = abi.make_obstacle_proposal(tilt=(1.0, 4.0, 0.25), m=3)
    smp = abi.make_obstacle_sampling("tilted", seed=5, hold=2)
    opts = dict(smp=smp, prop=prop, dist=D.make("overtake"))
    plain = O.host_run(sc, STEPS, plain=True, **opts)
    got = O.host_run(sc, STEPS, O.make("overtake"), **opts)
    assert_truth_kept(plain, got)
    assert np.any(got[-1]["scene"][:, abi.ENV_LOGW] != 0) and len(np.unique(got[-1]["scene"][:, abi.ENV_OBSPOL])) > 1
    for t, (a, b) in enumerate(zip(plain, got)):
        x, z = O.observed("overtake", O.make("overtake"), t, a["x"], a["z"], np.arange(B))
        assert np.array_equal(b["x"], x) and np.array_equal(b["z"], z)


# ---- the Python surface -----------------------------------------------------------------------

def test_make_observation_validates():
    s = abi.make_observation((0.05, 0.02), (0.2,), seed=2 ** 64 - 1, ego_base=2 ** 40)
    assert (s.law, s.reserved, s.seed, s.ego_base) == (abi.OBSERVE_IH4, 0, 2 ** 64 - 1, 2 ** 40)
    assert list(s.sigma_x) == [0.05, 0.02] + [0] * 6 and list(s.sigma_z) == [0.2] + [0] * 7
    assert list(abi.make_observation(None, 0.25).sigma_z) == [0.25] + [0] * 7
    assert abi.make_observation(law=abi.OBSERVE_NONE).law == 0
    assert len(abi.make_observation((1,) * 8).sigma_x) == abi.MAX_N == 8
    for bad in (dict(sigma_x=(-0.1,)), dict(sigma_z=(np.nan,)), dict(sigma_x=(np.inf,)), dict(sigma_x=(1,) * 9),
                dict(sigma_x=(1, 1, 1, 1), n=3), dict(sigma_z=np.ones((2, 2))), dict(law=2), dict(seed=-1),
                dict(seed=2 ** 64), dict(ego_base=-1), dict(ego_base=1.5)):
        with pytest.raises(ValueError):
            abi.make_observation(**bad)


class FakeLib:
    """bmpc_set_observation of a library that is not there: records what it was handed."""

    def __init__(self):
        self.calls = []

    def bmpc_set_observation(self, h, ref):
        s = None if ref is None else ref._obj
        self.calls.append(None if s is None else (s.law, s.seed, s.ego_base, list(s.sigma_x)[:4], list(s.sigma_z)[:4]))
        return 0


def test_plan_set_observation_marshals(monkeypatch):
    from bmpc import _lib
    assert "bmpc_set_observation" in _lib.EXPORTED
    fake = FakeLib()
    monkeypatch.setattr(plan, "lib", lambda: fake)
    pl = object.__new__(plan.BatchPlan)
    pl._h = None                                    # (nothing to destroy)
    pl.desc = scenarios.highway_desc(N=6, NB=1)
    pl.set_observation((0.05, 0.02), (0.2, 0.1, 0.2, 0.01), seed=9, ego_base=40)
    assert pl.observation.ego_base == 40
    pl.set_observation(sigma_z=(0.5,))
    pl.set_observation(abi.make_observation((1.0,), law=abi.OBSERVE_NONE))
    pl.set_observation()
    assert pl.observation is None
    assert fake.calls == [(1, 9, 40, [0.05, 0.02, 0, 0], [0.2, 0.1, 0.2, 0.01]), (1, 0, 0, [0.0] * 4, [0.5, 0, 0, 0]),
                          (0, 0, 0, [1.0, 0, 0, 0], [0.0] * 4), None]
    for bad in (dict(sigma_x=(0.1,) * 5), dict(sigma_z=(-1,)), dict(sigma_x=(1,), seed=-1)):
        with pytest.raises(ValueError):
            pl.set_observation(**bad)
    assert len(fake.calls) == 4                     # refused before the library saw it


def test_population_entries_plumb_the_observation():
    """observed_*_population take sigma_x / sigma_z / observation_seed and then the disturbed entries'
    arguments in their order, so the three options combine; the attach helper hands them to the plan."""
    own = ["sigma_x", "sigma_z", "observation_seed"]
    for name in ("overtake", "merge", "quadruped"):
        base = list(inspect.signature(getattr(scenarios, f"disturbed_{name}_population")).parameters)
        sig = inspect.signature(getattr(scenarios, f"observed_{name}_population"))
        assert list(sig.parameters) == base[:2] + own + base[2:], name
        assert [sig.parameters[k].default for k in own] == [None, None, 0]

    class Plan:
        def set_observation(self, sigma_x, sigma_z, seed, ego_base):
            self.observation = (sigma_x, sigma_z, seed, ego_base)

    pl = Plan()
    assert scenarios._attach_observation(pl, None, None, 1, 3) is None and not hasattr(pl, "observation")
    assert scenarios._attach_observation(pl, (0.05,), None, 5, 40) == ((0.05,), None, 5, 40)
    assert scenarios._attach_observation(pl, None, (0.2, 0.1), 6, 0) == (None, (0.2, 0.1), 6, 0)
