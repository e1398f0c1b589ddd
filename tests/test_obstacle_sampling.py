"""The sampled obstacle of the device closed loops (bmpc_set_obstacle_sampling), host side.

The generator and the choice rule of csrc/bmpc_rng.h as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/hostsim/obstacle_sampling_host.cpp); the scene steps' host build
(tests/hostsim/scene_host.cpp) as a shared library: its draws against bmpc/rng.py, the two scene functions with a sampler against the inverse
CDF of oracle.model's branch_eval, the draws' frequencies, and mode 0 against the scene functions'
former argument list bit for bit; the ctypes mirror, the argument validation and the population
entries' plumbing.  The GPU side is tests/test_obstacle_sampling_gpu.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import hostbuild
import obstacle_sampling_common as S
import scene_common as SC
from bmpc import abi, plan, rng, scenarios
from common import REPO

STEPS, HOLD, SEED = 12, 3, 7


def test_generator_known_answers():
    """Philox4x32-10 of bmpc/rng.py at the three (counter, key) pairs a pure-Python restatement gave."""
    for c, k, want in (([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                       ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
                        "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % v for v in rng.philox4x32(c, k)) == want
    assert rng.uniform53(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53 and rng.uniform53(0, 0) == 0.0


def test_host_program_under_sanitizers(tmp_path):
    """The known answers through bmpc_rng.h, the uniform's bounds at the all-ones output, counters with
    g >= 2^32 and seed >= 2^32, the inverse CDF just below and at a partial sum and its m - 1
    fallback, and the choice kept inside an epoch."""
    r = hostbuild.sanitized_program("obstacle_sampling_host.cpp", tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def test_draws_equal_numpy_restatement():
    """obstacle_uniform of the C++ header equals bmpc/rng.py's exactly over 1,000 (seed, ego, epoch)
    triples, ego 65,535 and 2^33 + 5 and seeds beyond 2^32 among them."""
    g = np.random.default_rng(3)
    n = 1000
    seed = g.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, n, dtype=np.uint64)
    ego = g.integers(0, 2 ** 40, n, dtype=np.uint64)
    epoch = g.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seed[:4] = [0, 7, 2 ** 32, 2 ** 64 - 1]
    ego[:4] = [65535, 2 ** 33 + 5, 0, 2 ** 32]
    epoch[:4] = [0, 1, 2 ** 32 - 1, 4]
    out = np.zeros(n)
    SC.shim().os_uniforms(n, SC._p(seed), SC._p(ego), SC._p(epoch), SC._p(out))
    want = rng.obstacle_uniform(seed, ego, epoch)
    assert want.shape == (n,) and np.all((want >= 0) & (want < 1))
    np.testing.assert_array_equal(out, want)
    assert len(np.unique(out)) == n
    # vectorised over egos and epochs, and plain Python integers beyond 2^63 are taken as they are
    grid = rng.obstacle_uniform(7, np.arange(5)[:, None], np.arange(3)[None, :])
    assert grid.shape == (5, 3) and grid[4, 2] == rng.obstacle_uniform(7, 4, 2)
    assert rng.obstacle_uniform(2 ** 64 - 1, 2 ** 32, 4) == out[3]
    with pytest.raises(ValueError):
        rng.obstacle_uniform(-1, 0, 0)


@pytest.fixture(scope="module", params=["overtake", "quadruped"])
def sampled_run(request):
    sc = SC.Scene(request.param, 65)
    smp = abi.make_obstacle_sampling("model", seed=SEED, hold=HOLD)
    return sc, smp, SC.host_run(sc, STEPS, smp)[0]


def test_host_scene_samples_the_models_distribution(sampled_run):
    """65 egos, hold 3, 12 teacher-forced steps: every epoch start's choice is the inverse CDF of
    oracle.model's branch_eval at the recorded pre-step state (with the policies in force before the
    step's re-targeting) under bmpc/rng.py's u, every other step keeps its epoch's first; a decision
    within 1e-9 of a partial sum is left out, at most 1 % of them (none expected: the first-step
    states keep 1.4e-3 / 5.2e-3).  All three overtake policies (both quadruped ones) are drawn."""
    sc, smp, run = sampled_run
    choices = [r["scene"][:, abi.ENV_OBSPOL].astype(int) for r in run]
    pre = [(r["pol"], r["x"], r["z"]) if t % HOLD == 0 else None for t, r in enumerate(run)]
    compared = S.check_choices(sc, smp, choices, pre)
    print(f"{sc.kind}: {compared} of {65 * STEPS // HOLD} draws compared; counts",
          np.bincount(np.concatenate(choices[::HOLD]), minlength=sc.m))
    assert compared == 65 * STEPS // HOLD
    assert np.all(np.bincount(np.concatenate(choices[::HOLD]), minlength=sc.m) >= 1)
    for t, r in enumerate(run):
        assert np.all(r["scene"][:, abi.ENV_STEPS] == t + 1)


def test_host_scene_downstream_of_the_choice(sampled_run):
    """The obstacle's input is the chosen backup's from the env's own list, as under the argmax rule."""
    sc, smp, run = sampled_run
    for r in run:
        st, c = r["scene"], r["scene"][:, abi.ENV_OBSPOL].astype(int)
        if sc.kind == "quadruped":
            np.testing.assert_array_equal(st[:, abi.QENV_UOBS:abi.QENV_UOBS + 3],
                                          np.where(c[:, None] == 0, [0.2, 0, 0], 0.0))
        else:
            z = st[:, abi.ENV_Z:abi.ENV_Z + 4]
            u = st[:, abi.ENV_UOBS:abi.ENV_UOBS + 2]
            np.testing.assert_array_equal(u[c == 0, 0], 0.0)
            np.testing.assert_allclose(u[c < 2, 1], -0.1 * z[c < 2, 3], rtol=0, atol=1e-15)
            tg = np.array(sc.env.target[:4])
            np.testing.assert_allclose(u[c == 2, 0], -0.8558 * (z[c == 2, 2] - tg[2]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind,bound", [("overtake", 13.82), ("quadruped", 10.83)])
def test_draw_frequencies(kind, bound):
    """4,096 egos at one fixed (x, z) -- the scene's row 0, the reference's own initial state --, one
    epoch: Pearson's chi^2 of the choice counts against 4096 p lies below the 99.9 % quantile for
    m - 1 degrees of freedom.  The draws are deterministic; seed 7 gives chi^2 = 9.11 (overtake:
    p = 0.404 / 0.410 / 0.185, counts 1733 / 1669 / 694) and 5.28 (quadruped: p = 0.400 / 0.600, counts
    1711 / 2385) -- one and the same 4,096 uniforms, so one draw from the statistic's tail, not two; over
    seeds 0..11 the overtake statistic has the spread chi^2 with 2 degrees of freedom should."""
    B = 4096
    sc = SC.Scene(kind, 1)
    scene = np.repeat(sc.scene0, B, 0)
    pol = abi.policy_array([sc.rows[0]] * B)
    smp = abi.make_obstacle_sampling("model", seed=SEED, hold=1)
    x, z, _ = SC.host_step(sc, 0, scene, pol, None, smp)
    p = sc.oracle_p(abi.policy_array([sc.rows[0]]), 0, x[0], z[0])
    counts = np.bincount(scene[:, abi.ENV_OBSPOL].astype(int), minlength=sc.m)
    chi2 = float(((counts - B * p) ** 2 / (B * p)).sum())
    print(kind, "p", p, "counts", counts, "chi2", chi2)
    assert counts.sum() == B and chi2 < bound
    # ... and they are bmpc/rng.py's draws
    want, sure = S.expected_choice(p[None], rng.obstacle_uniform(SEED, np.arange(B), 0))
    np.testing.assert_array_equal(scene[sure, abi.ENV_OBSPOL], want[sure])


@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_mode_argmax_is_the_unsampled_function(kind):
    """mode 0 with an arbitrary hold and seed, and no sampler at all, reproduce the scene function's
    former argument list bit for bit over the same 12 steps: scene, outputs and policies."""
    sc = SC.Scene(kind, 65)
    ref, ref_pol = SC.host_run(sc, STEPS, arglist=3)
    off = abi.make_obstacle_sampling("argmax", seed=2 ** 63 + 99, hold=5, ego_base=12)
    for smp in (off, None):
        got, got_pol = SC.host_run(sc, STEPS, smp)
        for a, b in zip(ref, got):
            for k in ("scene", "x", "z", "xref"):
                np.testing.assert_array_equal(a[k], b[k])
        assert bytes(ref_pol) == bytes(got_pol)
    sampled = SC.host_run(sc, STEPS, abi.make_obstacle_sampling("model", seed=SEED, hold=HOLD))[0]
    assert any((a["scene"][:, abi.ENV_OBSPOL] != b["scene"][:, abi.ENV_OBSPOL]).any() for a, b in zip(ref, sampled))


def test_host_scene_shard_invariance():
    """Egos 40..59 of the 65 in a scene batch of their own with ego_base = 40 take the rows they have
    in the whole batch, bit for bit."""
    sc = SC.Scene("overtake", 65)
    whole = SC.host_run(sc, STEPS, abi.make_obstacle_sampling("model", seed=SEED, hold=HOLD))[0]
    part = SC.host_run(sc, STEPS, abi.make_obstacle_sampling("model", seed=SEED, hold=HOLD, ego_base=40),
                      egos=slice(40, 60))[0]
    for a, b in zip(whole, part):
        for k in ("scene", "x", "z", "xref"):
            np.testing.assert_array_equal(a[k][40:60], b[k])


# ---- the Python surface -----------------------------------------------------------------------

FIELDS = ("mode", "hold", "seed", "ego_base")


def test_obstacle_sampling_layout_matches_header(tmp_path):
    offs = ", ".join(f"offsetof(bmpc_obstacle_sampling, {f})" for f in FIELDS)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("' + "%zu " * (1 + len(FIELDS)) + '%d %d\\n", sizeof(bmpc_obstacle_sampling), ' + offs
            + ', (int)BMPC_OBS_ARGMAX, (int)BMPC_OBS_SAMPLE_MODEL);return 0;}\n')
    got = hostbuild.header_program(tmp_path, code, cxx=True)   # (C++: the header's own static_assert on the size)
    D = abi.ObstacleSampling
    assert [name for name, _ in D._fields_] == list(FIELDS)
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in FIELDS] + [abi.OBS_ARGMAX, abi.OBS_SAMPLE_MODEL]
    assert got[:5] == [24, 0, 4, 8, 16]
    assert "static_assert(sizeof(bmpc_obstacle_sampling) == 24" in open(os.path.join(REPO, "include", "bmpc.h")).read()


def test_make_obstacle_sampling_validates():
    s = abi.make_obstacle_sampling("model", seed=2 ** 64 - 1, hold=3, ego_base=2 ** 40)
    assert (s.mode, s.hold, s.seed, s.ego_base) == (abi.OBS_SAMPLE_MODEL, 3, 2 ** 64 - 1, 2 ** 40)
    assert abi.make_obstacle_sampling("argmax").mode == abi.OBS_ARGMAX
    assert abi.make_obstacle_sampling(abi.OBS_SAMPLE_MODEL).mode == 1
    for bad in (dict(mode="softmax"), dict(mode=7), dict(hold=0), dict(hold=1.5), dict(ego_base=-1), dict(seed=-1),
                dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            abi.make_obstacle_sampling(**bad)


class FakeLib:
    """bmpc_set_obstacle_sampling of a library that is not there: records what it was handed."""

    def __init__(self):
        self.calls = []

    def bmpc_set_obstacle_sampling(self, h, ref):
        s = None if ref is None else ref._obj
        self.calls.append(None if s is None else (s.mode, s.hold, s.seed, s.ego_base))
        return 0


def test_plan_set_obstacle_sampling_marshals(monkeypatch):
    from bmpc import _lib
    assert "bmpc_set_obstacle_sampling" in _lib.EXPORTED
    fake = FakeLib()
    monkeypatch.setattr(plan, "lib", lambda: fake)
    pl = object.__new__(plan.BatchPlan)
    pl._h = None                                    # (nothing to destroy)
    pl.set_obstacle_sampling()
    pl.set_obstacle_sampling("model", seed=9, hold=4, ego_base=40)
    assert pl.obstacle_sampling.ego_base == 40
    pl.set_obstacle_sampling(abi.make_obstacle_sampling("argmax", seed=1))
    pl.set_obstacle_sampling(None)
    assert pl.obstacle_sampling is None
    assert fake.calls == [(1, 1, 0, 0), (1, 4, 9, 40), (0, 1, 1, 0), None]
    with pytest.raises(ValueError):
        pl.set_obstacle_sampling("model", hold=0)
    assert len(fake.calls) == 4                     # refused before the library saw it


def test_population_entries_plumb_the_sampler():
    """sampled_*_population take obstacle / obstacle_seed / hold / ego_base / population after the
    population entries' own arguments; the attach helper hands them to the plan; a shard's rows are
    the whole population's."""
    for fn in (scenarios.sampled_overtake_population, scenarios.sampled_quadruped_population):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["B", "steps", "seed", "device", "record", "obstacle", "obstacle_seed", "hold",
                                        "ego_base", "population", "desc"], fn.__name__
        d = {k: v.default for k, v in sig.parameters.items()}
        assert (d["obstacle"], d["obstacle_seed"], d["hold"], d["ego_base"], d["record"]) == ("model", 0, 1, 0, False)
        assert "distributed.shard" in fn.__doc__
    assert "obstacle" not in inspect.signature(scenarios.merge_population).parameters

    class Plan:
        def set_obstacle_sampling(self, mode, seed, hold, ego_base):
            self.obstacle_sampling = (mode, seed, hold, ego_base)

    pl = Plan()
    assert scenarios._attach_obstacle(pl, None, 1, 2, 3) is None and not hasattr(pl, "obstacle_sampling")
    assert scenarios._attach_obstacle(pl, "model", 5, 2, 40) == ("model", 5, 2, 40)
    with pytest.raises(ValueError):
        scenarios._attach_obstacle(pl, "argmax-ish", 0, 1, 0)
    assert scenarios._shard_rows(20, 40, 65) == (65, slice(40, 60))
    assert scenarios._shard_rows(8, 0, None) == (8, slice(0, 8))
    with pytest.raises(ValueError):
        scenarios._shard_rows(20, 50, 65)


def test_lane_change_targets_from_recorded_rows():
    """The GPU tests rebuild the policies in force before a step from recorded scene rows
    (Scene.lc_targets); here against the policy arrays the host scene function actually held."""
    sc = SC.Scene("overtake", 65)
    run = SC.host_run(sc, 40, abi.make_obstacle_sampling("model", seed=SEED, hold=HOLD))[0]
    got = sc.lc_targets(np.stack([r["scene"] for r in run], 1))
    want = np.array([[list(r["pol"][e * 3 + 2].p) for r in run] for e in range(65)])
    np.testing.assert_array_equal(got, want)
    assert (want[:, 1:] != want[:, :-1]).any()        # some obstacle changed lanes: the rule was exercised
