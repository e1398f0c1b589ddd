"""The weighted obstacle modes of the device closed loops (bmpc_set_obstacle_proposal), host side.

The tilted and the scripted rule of csrc/bmpc_env.h as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/hostsim/obstacle_proposal_host.cpp); the scene steps' host build
(tests/hostsim/scene_host.cpp) as a shared library: a tilt of ones against mode 1 bit for bit, tilted and scripted choices and log-weights against
NumPy over oracle.model's branch_eval, a full enumeration's probabilities summing to one, the
likelihood ratio's mean, bmpc.montecarlo, the ctypes mirror, the argument validation and the population
entries' plumbing.  The GPU side is tests/test_obstacle_proposal_gpu.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import hostbuild
import obstacle_proposal_common as P
import scene_common as SC
from bmpc import abi, montecarlo, plan, scenarios
from common import REPO

SEED = 7


def sampling(mode, hold=1, seed=SEED, ego_base=0):
    return abi.make_obstacle_sampling(mode, seed=seed, hold=hold, ego_base=ego_base)


def stack(run, key="scene"):
    return np.stack([r[key] for r in run], 1)


# ---- the host program -----------------------------------------------------------------------------

def test_host_program_under_sanitizers(tmp_path):
    """A tilt of ones against mode 1, the log-weight of a tilted and of a scripted choice, the script's
    clamps at a heap table of exactly its size, the epochs' untouched steps and whole scene steps of
    both scenes in both modes, compiled with -fsanitize=address,undefined and run once."""
    r = hostbuild.sanitized_program("obstacle_proposal_host.cpp", tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


# ---- 1: layout ------------------------------------------------------------------------------------

FIELDS = ("tilt", "script", "script_epochs", "epoch0")


def test_obstacle_proposal_layout_matches_header(tmp_path):
    offs = ", ".join(f"offsetof(bmpc_obstacle_proposal, {f})" for f in FIELDS)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("' + "%zu " * (1 + len(FIELDS)) + '%d %d %d %d\\n", sizeof(bmpc_obstacle_proposal), '
            + offs + ', (int)BMPC_ENV_LOGW, (int)BMPC_OBS_SAMPLE_TILTED, (int)BMPC_OBS_SCRIPT, (int)BMPC_ENV_STRIDE);'
            'return 0;}\n')
    got = hostbuild.header_program(tmp_path, code, cxx=True)
    D = abi.ObstacleProposal
    assert [name for name, _ in D._fields_] == list(FIELDS)
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in FIELDS] + [abi.ENV_LOGW, abi.OBS_SAMPLE_TILTED,
                                                                           abi.OBS_SCRIPT, abi.ENV_STRIDE]
    assert got == [48, 0, 32, 40, 44, 15, 2, 3, 16]
    # (cxx: the header's own static_asserts -- this struct's and the sampler's, still 24 bytes -- hold as C++)
    header = open(os.path.join(REPO, "include", "bmpc.h")).read()
    assert "static_assert(sizeof(bmpc_obstacle_proposal) ==" in header
    assert "static_assert(sizeof(bmpc_obstacle_sampling) == 24" in header and C.sizeof(abi.ObstacleSampling) == 24


# ---- 2: a tilt of ones is mode 1 --------------------------------------------------------------------

@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_tilt_of_ones_is_mode_model(kind, hold):
    """64 egos, 8 teacher-forced steps: mode 2 with b == 1 gives mode 1's scene rows, outputs and
    policies bit for bit, and ENV_LOGW is exactly 0.0 in every row."""
    sc = SC.Scene(kind, 64)
    ref = SC.host_run(sc, 8, sampling("model", hold), None)[0]
    prop, _ = P.proposal(sc, np.ones(sc.m))
    got = SC.host_run(sc, 8, sampling("tilted", hold), prop)[0]
    for a, b in zip(ref, got):
        for k in ("scene", "x", "z"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert bytes(a["pol"]) == bytes(b["pol"])
        assert np.all(b["scene"][:, abi.ENV_LOGW] == 0.0) and not np.signbit(b["scene"][:, abi.ENV_LOGW]).any()
    # ... and another tilt gives other choices somewhere
    prop, _ = P.proposal(sc, P.TILTS[kind])
    other = SC.host_run(sc, 8, sampling("tilted", hold), prop)[0]
    assert (stack(other)[:, :, abi.ENV_OBSPOL] != stack(ref)[:, :, abi.ENV_OBSPOL]).any()


# ---- 3: tilted choices and weights -----------------------------------------------------------------

@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_tilted_choices_and_weights(kind, hold):
    """b = (1, 4, 0.25) / (1, 5), 64 egos, 8 steps: every epoch start's choice is bmpc.rng's inverse CDF of
    oracle.model's p_j b_j at the recorded pre-step state, and ENV_LOGW after every step is NumPy's
    running sum of log(p_j / q_j) within 1e-9.  Decisions within 1e-9 of a partial sum are left out, at
    most 1 % of them; with seed 7 the NumPy side alone leaves out none (asserted here), so every decision
    is compared."""
    sc = SC.Scene(kind, 64)
    smp = sampling("tilted", hold)
    prop, _ = P.proposal(sc, P.TILTS[kind])
    run = SC.host_run(sc, 8, smp, prop)[0]
    p_at = P.oracle_probabilities(sc, run)
    cache = {}
    p_once = lambda r: cache[r] if r in cache else cache.setdefault(r, p_at(r))   # noqa: E731
    left, total = P.numpy_left_out(smp, p_once, P.TILTS[kind], 8)
    assert left == 0 and total == 64 * len(range(0, 8, hold))
    compared, logw = P.check_weighted(smp, sc.m, stack(run), p_once, tilt=P.TILTS[kind])
    assert compared == total
    assert np.abs(logw).max() > 0.1 and len(np.unique(stack(run)[:, ::hold, abi.ENV_OBSPOL])) == sc.m
    print(kind, "hold", hold, "logw range", logw.min(), logw.max())


# ---- 4: script --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_script_is_followed(kind):
    """A random script with hold 2 and epoch0 = 3 under a run of steps 6..13: followed exactly, entries
    outside [0, m) clamped, ENV_LOGW the NumPy sum of log p_j (oracle.model) within 1e-9 on top of the
    row's starting value, the second step of every epoch leaving choice and weight alone; the seed
    changes nothing."""
    sc = SC.Scene(kind, 64)
    g = np.random.default_rng(11)
    script = g.integers(0, sc.m, (64, 4))
    script[g.integers(0, 64, 12), g.integers(0, 4, 12)] = g.choice([-3, -1, sc.m, sc.m + 5], 12)
    assert (script < 0).any() and (script >= sc.m).any()
    prop, table = P.proposal(sc, None, script, epoch0=3)
    sc.scene0[:, abi.ENV_LOGW] = -0.5          # (accumulates onto what the row holds)
    run = SC.host_run(sc, 8, sampling("script", 2), prop, t0=6)[0]
    _, logw = P.check_weighted(sampling("script", 2), sc.m, stack(run), P.oracle_probabilities(sc, run), script=script,
                               epoch0=3, t0=6, logw0=-0.5)
    assert np.all(logw < -0.5)
    again = SC.host_run(sc, 8, sampling("script", 2, seed=12345), prop, t0=6)[0]
    assert stack(again).tobytes() == stack(run).tobytes()


# ---- 5: the enumeration sums to one -----------------------------------------------------------------

@pytest.mark.parametrize("kind,epochs,hold", [("overtake", 4, 2), ("quadruped", 5, 1)])
def test_enumeration_sums_to_one(kind, epochs, hold):
    """One initial state (the scene's row 0) against all m ** epochs scripts (81 / 32 paths) under one
    scripted input: sum over paths of exp(ENV_LOGW) is 1 within 1e-12 per path.  A tilted population
    from the same state realises some of these paths; for each of its egos log q(path), from the
    weights at its recorded states, plus its ENV_LOGW equals the scripted run's log p(path) within 1e-9."""
    m = 3 if kind == "overtake" else 2
    paths = montecarlo.enumerate_scripts(m, epochs)
    n = len(paths)
    assert n == (81 if kind == "overtake" else 32)
    sc = SC.Scene(kind, n)
    sc.scene0[:] = sc.scene0[0]
    sc.rows = [sc.rows[0]] * n
    steps = epochs * hold
    prop, table = P.proposal(sc, None, paths)
    run = SC.host_run(sc, steps, sampling("script", hold), prop, same_input=True)[0]
    logp = run[-1]["scene"][:, abi.ENV_LOGW]
    total = np.exp(logp).sum()
    print(kind, "sum of path probabilities - 1 =", total - 1.0)
    assert abs(total - 1.0) <= 1e-12 * n
    assert np.array_equal(stack(run)[:, ::hold, abi.ENV_OBSPOL], paths)
    assert montecarlo.exact_expectation(np.ones(n), logp)[1] == pytest.approx(1.0, abs=1e-12 * n)
    # the tilted population from the same state
    b = np.array(P.TILTS[kind])
    B = 256
    pop = SC.Scene(kind, B)
    pop.scene0[:] = pop.scene0[0]
    pop.rows = [pop.rows[0]] * B
    tprop, _ = P.proposal(pop, b)
    trun = SC.host_run(pop, steps, sampling("tilted", hold), tprop, same_input=True)[0]
    chosen = stack(trun)[:, ::hold, abi.ENV_OBSPOL].astype(int)
    index = (chosen * m ** np.arange(epochs - 1, -1, -1)).sum(1)
    assert np.array_equal(paths[index], chosen) and len(np.unique(index)) >= 8
    logq = np.zeros(B)
    for c, r in enumerate(range(0, steps, hold)):
        w = P.host_weights(pop, trun[r]["pol"], trun[r]["x"], trun[r]["z"])
        logq += np.log(w[np.arange(B), chosen[:, c]] * b[chosen[:, c]] / (w * b).sum(1))
    np.testing.assert_allclose(logq + trun[-1]["scene"][:, abi.ENV_LOGW], logp[index], rtol=0, atol=1e-9)


# ---- 6: unbiasedness --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_likelihood_ratio_is_unbiased(kind):
    """4,096 host egos (the scene's seeded batch), the tilt of test 3, seed 7, 4 epochs of one step: the
    mean of exp(ENV_LOGW) lies within 5 of its own standard errors of 1, and montecarlo.estimate of "the
    obstacle chose policy 1 in epoch 0" under the tilt lies within 5 of its standard errors of the plain
    (mode 1) frequency's 5-sigma band.  Deterministic; the NumPy restatement of the same run -- choices
    and weights from the recorded model weights and bmpc.rng -- reproduces ENV_LOGW within 1e-9 and
    passes the same two bounds."""
    B = 4096
    sc = SC.Scene(kind, B)
    b = np.array(P.TILTS[kind])
    smp = sampling("tilted")
    prop, _ = P.proposal(sc, b)
    run = SC.host_run(sc, 4, smp, prop)[0]

    def p_at(r):
        w = P.host_weights(sc, run[r]["pol"], run[r]["x"], run[r]["z"])
        return w / w.sum(1, keepdims=True)

    _, numpy_logw = P.check_weighted(smp, sc.m, stack(run), p_at, tilt=b)
    plain = SC.host_run(sc, 1, sampling("model"), None)[0]
    hit_plain = plain[0]["scene"][:, abi.ENV_OBSPOL] == 1
    freq = hit_plain.mean()
    band = 5.0 * np.sqrt(freq * (1.0 - freq) / B)
    hit = run[0]["scene"][:, abi.ENV_OBSPOL] == 1
    assert hit.mean() > freq + band            # (the tilt does favour policy 1: the estimate needs its weights)
    for logw in (run[-1]["scene"][:, abi.ENV_LOGW], numpy_logw):
        mean, se, ess = montecarlo.estimate(np.ones(B), logw)
        print(kind, "mean weight", mean, "+-", se, "ess", ess)
        assert abs(mean - 1.0) <= 5.0 * se and 0 < ess < B
        est, est_se, _ = montecarlo.estimate(hit, logw)
        print(kind, "P(policy 1 in epoch 0): tilted estimate", est, "+-", est_se, "plain frequency", freq, "+-", band / 5)
        assert abs(est - freq) <= 5.0 * est_se + band


# ---- 7: montecarlo ----------------------------------------------------------------------------------

def test_montecarlo_estimates():
    g = np.random.default_rng(5)
    f, lw = g.normal(1.0, 2.0, 500), g.normal(0.0, 0.7, 500)
    w = np.exp(lw)
    mean, se, ess = montecarlo.estimate(f, lw)
    assert mean == pytest.approx((w * f).mean(), rel=1e-13)
    assert se == pytest.approx((w * f).std(ddof=1) / np.sqrt(500), rel=1e-10)
    assert ess == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-13)
    mean, se, ess2 = montecarlo.estimate(f, lw, self_normalised=True)
    mu = (w * f).sum() / w.sum()
    assert mean == pytest.approx(mu, rel=1e-13) and ess2 == pytest.approx(ess, rel=1e-13)
    assert se == pytest.approx(np.sqrt((w * w * (f - mu) ** 2).sum()) / w.sum(), rel=1e-9)
    # log-weights near +-700: exp(2 logw) overflows (underflows) a double, the estimates do not
    for shift in (700.0, -700.0):
        big = lw + shift
        ld = np.exp(big.astype(np.longdouble))
        m2, s2, e2 = montecarlo.estimate(f, big, self_normalised=True)
        assert (m2, e2) == (pytest.approx(mu, rel=1e-12), pytest.approx(ess, rel=1e-12))
        assert s2 == pytest.approx(se, rel=1e-9)
        m1, s1, e1 = montecarlo.estimate(f, big)
        assert np.isfinite([m1, s1, e1]).all()
        assert m1 == pytest.approx(float((ld * f).mean()), rel=1e-12) and e1 == pytest.approx(ess, rel=1e-12)
        assert s1 == pytest.approx(float((ld * f).std(ddof=1) / np.sqrt(np.longdouble(500))), rel=1e-9)
    # equal weights: the plain sample mean and its error
    mean, se, ess = montecarlo.estimate(f, np.zeros(500))
    assert (mean, se, ess) == (pytest.approx(f.mean()), pytest.approx(f.std(ddof=1) / np.sqrt(500)), pytest.approx(500))
    with pytest.raises(ValueError):
        montecarlo.estimate(f, lw[:10])
    with pytest.raises(ValueError):
        montecarlo.estimate(f, np.full(500, np.nan))


def test_montecarlo_terms_add_over_shards():
    g = np.random.default_rng(6)
    f, lw = g.normal(0.0, 1.0, 300), g.normal(0.0, 0.5, 300)
    whole = montecarlo.reduce_terms(f, lw)
    parts = montecarlo.reduce_terms(f[:120], lw[:120]) + montecarlo.reduce_terms(f[120:], lw[120:])
    assert whole.shape == (montecarlo.T_COUNT,) and whole.dtype == np.float64
    np.testing.assert_allclose(parts, whole, rtol=1e-13, atol=0)
    w = np.exp(lw)
    np.testing.assert_allclose(whole[[montecarlo.T_W, montecarlo.T_WF, montecarlo.T_W2, montecarlo.T_WF2]],
                               [w.sum(), (w * f).sum(), (w * w).sum(), ((w * f) ** 2).sum()], rtol=1e-13)
    for sn in (False, True):
        np.testing.assert_allclose(montecarlo.estimate_from_terms(parts, sn), montecarlo.estimate(f, lw, sn), rtol=1e-10)
    # the vector is what distributed.reduce_stats all-reduces (no flag slots): one rank leaves it as it is
    from bmpc import distributed
    import torch
    v = torch.tensor(whole)
    assert np.array_equal(distributed.reduce_stats(v, max_slots=()).numpy(), whole)


def test_enumerate_scripts():
    s = montecarlo.enumerate_scripts(3, 4)
    assert s.shape == (81, 4) and s.dtype == np.int32
    assert [tuple(r) for r in s] == sorted({tuple(r) for r in s}) and len({tuple(r) for r in s}) == 81
    assert s[0].tolist() == [0, 0, 0, 0] and s[1].tolist() == [0, 0, 0, 1] and s[-1].tolist() == [2, 2, 2, 2]
    assert montecarlo.enumerate_scripts(2, 1).tolist() == [[0], [1]]
    with pytest.raises(ValueError):
        montecarlo.enumerate_scripts(0, 3)
    with pytest.raises(ValueError):
        montecarlo.enumerate_scripts(4, 20)


# ---- 8: validation and plumbing ---------------------------------------------------------------------

def test_make_obstacle_proposal_validates():
    q = abi.make_obstacle_proposal((1, 4, 0.25), m=3)
    assert list(q.tilt) == [1.0, 4.0, 0.25, 1.0] and not q.script and (q.script_epochs, q.epoch0) == (0, 0)
    assert list(abi.make_obstacle_proposal(m=2).tilt) == [1.0] * 4
    q = abi.make_obstacle_proposal(None, (4096, 5), epoch0=3, m=2)
    assert (q.script, q.script_epochs, q.epoch0) == (4096, 5, 3)
    for bad in (dict(tilt=(1, 0, 1)), dict(tilt=(1, -2)), dict(tilt=(1, np.inf)), dict(tilt=(1, np.nan)),
                dict(tilt=(1, 1), m=3), dict(tilt=(1,) * 5), dict(tilt=[[1, 1]]), dict(tilt=()), dict(epoch0=-1),
                dict(epoch0=1.5), dict(script=(0, 4)), dict(script=(4096, 0)), dict(script=(4096, -2))):
        with pytest.raises(ValueError):
            abi.make_obstacle_proposal(**bad)
    assert abi.make_obstacle_sampling("tilted").mode == abi.OBS_SAMPLE_TILTED == 2
    assert abi.make_obstacle_sampling("script", hold=2).mode == abi.OBS_SCRIPT == 3
    assert abi.make_obstacle_sampling(abi.OBS_SCRIPT).mode == 3


class FakeLib:
    """bmpc_set_obstacle_proposal / _sampling of a library that is not there: records what it was handed."""

    def __init__(self):
        self.calls = []

    def bmpc_set_obstacle_proposal(self, h, ref):
        q = None if ref is None else ref._obj
        self.calls.append(None if q is None else (list(q.tilt), q.script, q.script_epochs, q.epoch0))
        return 0


def test_plan_set_obstacle_proposal_marshals(monkeypatch):
    from bmpc import _lib
    assert "bmpc_set_obstacle_proposal" in _lib.EXPORTED
    fake = FakeLib()
    monkeypatch.setattr(plan, "lib", lambda: fake)
    pl = object.__new__(plan.BatchPlan)
    pl._h = None                                    # (nothing to destroy)
    pl.desc, pl.batch, pl.device = scenarios.highway_desc(N=6), 4, 0
    pl.set_obstacle_proposal(tilt=(1, 4, 0.25), epoch0=2)
    assert pl.obstacle_proposal.epoch0 == 2
    pl.set_obstacle_proposal(abi.make_obstacle_proposal((2, 2, 2), m=3))
    pl.set_obstacle_proposal()
    assert pl.obstacle_proposal is None
    assert fake.calls == [([1.0, 4.0, 0.25, 1.0], None, 0, 2), ([2.0, 2.0, 2.0, 1.0], None, 0, 0), None]
    ok = np.zeros((4, 3), np.int64)
    for bad in (dict(tilt=(1, 1)), dict(tilt=(1, 0, 1)), dict(tilt=(1, 1, 1, 1)), dict(script=ok[:3]),
                dict(script=ok[:, :0]), dict(script=ok[0]), dict(script=ok + 3), dict(script=ok - 1),
                dict(script=ok.astype(float)), dict(script=ok, epoch0=-1)):
        with pytest.raises(ValueError):
            pl.set_obstacle_proposal(**bad)
    assert len(fake.calls) == 3                     # refused before the library saw it (and before any upload)


def test_population_entries_plumb_the_proposal():
    """weighted_*_population take the sampled entries' arguments (without `obstacle`) plus tilt;
    enumerated_*_population take the state, epochs and hold, then device / record / desc; the attach
    helpers hand the proposal to the plan before the mode that needs it."""
    sampled = list(inspect.signature(scenarios.sampled_overtake_population).parameters)
    for fn in (scenarios.weighted_overtake_population, scenarios.weighted_quadruped_population):
        assert list(inspect.signature(fn).parameters) == [a for a in sampled if a != "obstacle"] + ["tilt"], fn.__name__
        assert "distributed.shard" in fn.__doc__
    assert list(inspect.signature(scenarios.enumerated_overtake_population).parameters) == [
        "x0", "z0", "epochs", "hold", "device", "record", "desc"]
    assert list(inspect.signature(scenarios.enumerated_quadruped_population).parameters) == [
        "x0", "z0", "x_des", "epochs", "hold", "device", "record", "desc"]

    class Plan:
        batch = 9

        def __init__(self):
            self.calls = []

        def set_obstacle_proposal(self, tilt=None, script=None, epoch0=0):
            self.calls.append(("proposal", tilt, script))

        def set_obstacle_sampling(self, mode, seed=0, hold=1, ego_base=0):
            self.calls.append(("sampling", mode, seed, hold, ego_base))

    pl = Plan()
    scenarios._attach_tilt(pl, (1, 4, 0.25), 5, 2, 40)
    assert pl.calls == [("proposal", (1, 4, 0.25), None), ("sampling", "tilted", 5, 2, 40)]
    pl = Plan()
    script = scenarios._attach_script(pl, 3, 2, 4)
    assert np.array_equal(script, montecarlo.enumerate_scripts(3, 2))
    assert pl.calls[0][0] == "proposal" and pl.calls[0][2] is script and pl.calls[1] == ("sampling", "script", 0, 4, 0)
    with pytest.raises(ValueError):
        scenarios._attach_script(Plan(), 3, 3, 1)    # 9 egos are not 27 paths
    stats, scene = np.zeros((2, abi.ENV_NSTAT)), np.arange(32.0).reshape(2, 16)
    out = scenarios._with_logw((stats, scene, "rec"))
    assert out[0] is stats and out[1] is scene and out[2].tolist() == [15.0, 31.0] and out[3] == "rec"
