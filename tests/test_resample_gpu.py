"""Resampling a weighted population on the GPU (bmpc_population_ancestors, bmpc_gather_egos,
bmpc_resample_device).

Shapes follow the obstacle tests': overtake N = 6, NB = 1, m = 3 and quadruped N = 6, NB = 2, m = 2;
the launch paths are selected as tests/loop_common.py does.

Yardsticks: bmpc/resample.py's exact integer rule fed the device's own integer weights k (equal
integers, no tolerance); an un-gathered run of the same plan on the same launch path (bit for bit: a
child continues as its ancestor does there); the mean weight before a resampling
(resample_common.mean_weight_bound)."""
import ctypes as C

import numpy as np
import pytest

import resample_common as R
from bmpc import abi, resample, scenarios
from bmpc._lib import lib
from bmpc.scenarios import highway_desc, merge_desc, quadruped_desc
from loop_common import FINALS, PATHS, Loop, assert_all_solved, gpu, overtake_case, quad_case, set_path  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 11
TILE = 1024          # the ancestor kernel walks the population in tiles of this many egos
BUFFERS = dict(scene="scene", upred="up", x="x", z="z", xref="xref", J="J", status="st", iters="it", stats="stats")


def buffers(d):
    return {k: getattr(d, v) for k, v in BUFFERS.items()}


def device_rule(plan, logw, rnd, seed=SEED, ess_fraction=2.0, ego_base=0):
    """bmpc_population_ancestors of host log-weights: ancestors, the k used (uint64) and info on the host."""
    import torch
    anc, k, info = plan.population_ancestors(logw, rnd, seed, ess_fraction, ego_base)
    torch.cuda.synchronize()
    return anc.cpu().numpy(), k.cpu().numpy().view(np.uint64), info.cpu().numpy()


# ---- 1: the rule against NumPy, given the device's k --------------------------------------------------

@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 256, 257, 1000, TILE + 1, 4097])
def test_ancestors_equal_numpy_given_the_device_k(gpu, B):
    """Per weight family: the device's ancestors are bmpc.resample.ancestors of the device's own k at the
    stated draw, its k is NumPy's within one unit, its ess is float(S)^2 / float(Q) of that k bit for bit
    and its info vector is the restatement's.  TILE + 1 = 1025 is the first size past one tile of the
    kernel's scans."""
    ident = np.arange(B)
    fams = {f: R.family(f, B) for f in ("equal", "half_dead", "sd30")}
    dom = np.full(B, -300.0)
    dom[B // 3] = 2.5
    fams["dominant"] = dom
    for name, lw in fams.items():
        rnd = 3 + len(name)
        anc, k, info = device_rule(gpu, lw, rnd)
        kn, M = resample.quantise(lw)
        assert np.abs(k.astype(np.int64) - kn.astype(np.int64)).max() <= 1, name
        S = sum(int(v) for v in k)
        assert info[abi.R_ESS] == resample.ess(k) and info[abi.R_MAX] == M and info[abi.R_SUM] == float(S), name
        want_lw = resample.new_logw(M, S, B)
        assert abs(info[abi.R_NEW_LOGW] - want_lw) <= 1e-15 * max(abs(want_lw), 1.0)
        want, counts = resample.ancestors(k, resample.offset(SEED, 0, rnd))
        assert info[abi.R_RESAMPLED] == 1.0 and info[abi.R_NONFINITE] == 0.0 and info[7] == 0.0
        assert np.array_equal(anc, want), (name, np.flatnonzero(anc != want)[:8])
        assert info[abi.R_SURVIVORS] == (counts > 0).sum()
        R.check_properties(k, resample.offset(SEED, 0, rnd), anc, counts)
        if name == "equal":
            assert np.array_equal(anc, ident)
            # ... and unforced, equal weights are not resampled at all (ess = B)
            anc0, _, info0 = device_rule(gpu, lw, rnd, ess_fraction=0.5)
            assert info0[abi.R_RESAMPLED] == 0.0 and info0[abi.R_ESS] == B and np.array_equal(anc0, ident)
        if name == "dominant":
            assert np.all(anc == B // 3) and info[abi.R_SURVIVORS] == 1
        if name == "half_dead":
            assert np.all(k[np.isneginf(lw)] == 0) and np.all(np.isfinite(lw[anc]))
    # another shard's draw differs and equals its own restatement
    if B > 2:
        anc, k, _ = device_rule(gpu, fams["sd30"], 4, ego_base=32)
        assert np.array_equal(anc, resample.ancestors(k, resample.offset(SEED, 32, 4))[0])
    # a NaN (a +inf) refuses: the identity, and the info vector says so
    for bad in (np.nan, np.inf):
        lw = fams["sd30"].copy()
        lw[B // 2] = bad
        anc, k, info = device_rule(gpu, lw, 1)
        assert np.array_equal(anc, ident) and info[abi.R_RESAMPLED] == 0.0 and info[abi.R_NONFINITE] == 1.0
        assert not k.any()
    # every ego dead: nothing to resample
    anc, k, info = device_rule(gpu, np.full(B, -np.inf), 1)
    assert np.array_equal(anc, ident) and info[abi.R_RESAMPLED] == 0.0 and info[abi.R_MAX] == -np.inf


@pytest.mark.parametrize("B", [65, 1000])
def test_threshold_on_each_side(gpu, B):
    """ess_fraction just above and just below ess / B: resampled, and not (the comparison is
    ess < ess_fraction * B in double, checked here on the host for the same two numbers)."""
    lw = R.family("sd1", B)
    _, k, info = device_rule(gpu, lw, 0)
    ess = info[abi.R_ESS]
    assert 1.0 < ess < B and ess == resample.ess(k)
    above, below = ess / B * (1 + 1e-12), ess / B * (1 - 1e-12)
    assert ess < above * B and not ess < below * B
    anc_a, _, info_a = device_rule(gpu, lw, 0, ess_fraction=above)
    anc_b, _, info_b = device_rule(gpu, lw, 0, ess_fraction=below)
    assert info_a[abi.R_RESAMPLED] == 1.0 and np.array_equal(anc_a, resample.ancestors(k, resample.offset(SEED, 0, 0))[0])
    assert info_b[abi.R_RESAMPLED] == 0.0 and np.array_equal(anc_b, np.arange(B)) and info_b[abi.R_ESS] == ess
    assert (anc_a != np.arange(B)).any()


# ---- 2: a gathered ego continues as its ancestor does --------------------------------------------------

GATHER_B = 8
GATHER_MAP = np.array([0, 0, 0, 4, 3, 5, 6, 5], np.int32)   # a broadcast of ego 0, a swap 3 <-> 4, 5 also into 7; 5, 6 fixed
K1 = K2 = 4


def run_segments(plan, case, amap, setup=None, between=None):
    """K1 steps, then (amap given) gather_egos, then K2 steps, one recorder attached throughout: the
    finals, the policies, the record on the host and the kernels of the two calls."""
    import torch
    d = Loop(plan, case)
    if setup:
        setup(d.pl)
    rec = d.pl.new_loop_record(K1 + K2, 0, predictions=True)
    d.pl.set_loop_record(rec)
    kernels = []
    d.loop(K1)
    d.stream.synchronize()
    kernels.append(d.pl.last_kernel())
    pol_mid = d.pl.get_policies()
    if amap is not None:
        a = torch.tensor(amap, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        d.pl.gather_egos(a, buffers(d), d.stream.cuda_stream)
        if between:
            d.stream.synchronize()
            between(d.pl)
    d.loop(K2)
    d.stream.synchronize()
    kernels.append(d.pl.last_kernel())
    return d.finals(), d.pl.get_policies(), rec.host(), kernels, pol_mid


def assert_children_continue(case, amap, ref, got):
    fin_r, pol_r, rec_r, _, pol_mid = ref
    fin_g, pol_g, rec_g, _, _ = got
    a = np.asarray(amap)
    assert_all_solved(case["desc"], rec_r.col("status"))
    assert np.all(fin_r["scene"][:, abi.ENV_STEPS] == K1 + K2)
    for k in FINALS:
        assert np.array_equal(fin_g[k], fin_r[k][a]), k
    for kk in fin_r["ws"]:
        assert np.array_equal(fin_g["ws"][kk], fin_r["ws"][kk][a]), ("warm start", kk)
    assert pol_g == [pol_r[i] for i in a]
    for k in rec_r.cols:
        assert np.array_equal(rec_g.col(k)[:, :K1], rec_r.col(k)[:, :K1]), (k, "before the gather")
        assert np.array_equal(rec_g.col(k)[:, K1:], rec_r.col(k)[a][:, K1:]), (k, "after the gather")
    # the test can see a forgotten part: the moved egos differ from their ancestors in every part
    moved = np.flatnonzero(a != np.arange(len(a)))
    assert len(moved) >= 4
    for k in ("scene", "up", "J", "x", "z"):
        assert all(not np.array_equal(fin_r[k][j], fin_r[k][a[j]]) for j in moved), k
    for kk in fin_r["ws"]:
        if fin_r["ws"][kk].any() and kk != "p":   # (a PROX plan keeps no Jcons: all zero)
            assert any(not np.array_equal(fin_r["ws"][kk][j], fin_r["ws"][kk][a[j]]) for j in moved), kk
    return moved, pol_mid


GATHER_CASES = [("overtake", "wave", None), ("overtake", "lean", None), ("overtake", "wave", 0), ("overtake", "blk", None),
                ("robust", None, None), ("quadruped", "wave", None), ("quadruped", "lean", None),
                ("quadruped", "wave", 0)]


def gather_case(kind):
    if kind == "quadruped":
        return quad_case(GATHER_B)
    return overtake_case(6, 1, GATHER_B, robust=(kind == "robust"))


@pytest.mark.parametrize("kind,path,fused", GATHER_CASES,
                         ids=[f"{k}-{p}-{'per_step' if f == 0 else 'loop'}" for k, p, f in GATHER_CASES])
def test_gathered_egos_continue_as_their_ancestors(gpu, monkeypatch, kind, path, fused):
    """K1 = 4 steps under the argmax obstacle, gather_egos with a map holding a broadcast, a swap and
    fixed points, K2 = 4 more steps: child j's scene rows, outputs, statistics, policies, record rows
    and final warm start equal, bit for bit, those of ego a[j] in an un-gathered run of 8 steps.  The
    overtake CVaR plan (per-ego lane-change targets that differ), the overtake robustMPC plan (xLin, the
    per-step path) and the quadruped PROX plan (OldInput); fused rich, fused lean, BMPC_LOOP_FUSED=0
    and the small-batch path."""
    case = gather_case(kind)
    if kind == "robust":
        set_path(monkeypatch)
        want = {abi.KERNEL_QP_RICH, abi.KERNEL_QP_LEAN}
    else:
        egos, rich, k_step, k_loop = PATHS[kind, path]
        set_path(monkeypatch, egos, rich, fused)
        want = set(k_step if fused == 0 else k_loop)
    ref = run_segments(gpu, case, None)
    got = run_segments(gpu, case, GATHER_MAP)
    assert set(ref[3]) <= want and set(got[3]) <= want, (ref[3], got[3])
    moved, pol_mid = assert_children_continue(case, GATHER_MAP, ref, got)
    if kind == "overtake":   # a forgotten policy row would show: lane-change targets differ at the gather
        assert any(pol_mid[j] != pol_mid[GATHER_MAP[j]] for j in moved)
    print(kind, path, fused, "kernels", got[3], "moved", moved.tolist())


@pytest.mark.parametrize("kind,path", [("overtake", "wave"), ("quadruped", "wave")])
def test_gathered_egos_continue_in_script_mode(gpu, monkeypatch, kind, path):
    """The same in mode "script" (hold 1): after the gather the script's rows are gathered too
    (script[j] = script[a[j]]), and child j follows ego a[j] of the un-gathered scripted run, its
    log-weight included."""
    case = gather_case(kind)
    m = case["desc"].m
    script = np.random.default_rng(5).integers(0, m, (GATHER_B, K1 + K2)).astype(np.int32)
    egos, rich, _, k_loop = PATHS[kind, path]
    set_path(monkeypatch, egos, rich)

    def setup(pl):
        pl.set_obstacle_proposal(script=script)
        pl.set_obstacle_sampling("script", hold=1)

    ref = run_segments(gpu, case, None, setup)
    got = run_segments(gpu, case, GATHER_MAP, setup, between=lambda pl: pl.set_obstacle_proposal(script=script[GATHER_MAP]))
    assert set(got[3]) <= set(k_loop)
    assert_children_continue(case, GATHER_MAP, ref, got)
    logw = ref[0]["scene"][:, abi.ENV_LOGW]
    assert np.all(logw < 0.0) and np.array_equal(got[0]["scene"][:, abi.ENV_LOGW], logw[GATHER_MAP])


# ---- 3: bmpc_resample_device end to end ----------------------------------------------------------------

def snapshot(d):
    d.stream.synchronize()
    return d.finals(), d.pl.get_policies()


def tilted_loop(plan, case, ego_base=0):
    d = Loop(plan, case)
    d.pl.set_obstacle_proposal(tilt=(1.0, 4.0, 0.25))
    d.pl.set_obstacle_sampling("tilted", seed=7, hold=1, ego_base=ego_base)
    return d


def resample_round(plan, d, t, ess_fraction=2.0, ego_base=0):
    """One resampling of loop `d` at round t: (log-weights before, the device's k for them, ancestors,
    info, log-weights after) on the host."""
    import torch
    logw0 = d.host("scene")[0][:, abi.ENV_LOGW]
    _, k, _ = plan.population_ancestors(d.scene.view(-1)[abi.ENV_LOGW:], t, SEED, ess_fraction, ego_base,
                                        stride=abi.ENV_STRIDE, batch=d.B)
    torch.cuda.synchronize()
    anc, info = d.pl.resample(buffers(d), t, SEED, ess_fraction, ego_base, d.stream.cuda_stream)
    d.stream.synchronize()
    return logw0, k.cpu().numpy().view(np.uint64), anc.cpu().numpy(), info.cpu().numpy(), d.host("scene")[0][:, abi.ENV_LOGW]


def test_resample_device_end_to_end(gpu, monkeypatch):
    """Tilted mode at 64 overtake egos, resampled after every epoch with ess_fraction 2: every round's
    ancestors are bmpc.resample.ancestors of the device's k at the stated draw, every ego's slot 15 holds
    info[3], the mean weight is preserved within resample_common.mean_weight_bound, and a moved ego's
    buffers are its ancestor's.  With ess_fraction 0 no byte of scene, outputs, statistics, policies
    or warm start changes."""
    B = 64
    case = overtake_case(6, 1, B)
    set_path(monkeypatch, 0, 1)
    d = tilted_loop(gpu, case)
    moved_total = 0
    for t in range(1, 5):
        d.loop(1)
        before, _ = snapshot(d)
        logw0, k, anc, info, logw1 = resample_round(gpu, d, t)
        want, counts = resample.ancestors(k, resample.offset(SEED, 0, t))
        assert info[abi.R_RESAMPLED] == 1.0 and np.array_equal(anc, want), t
        assert info[abi.R_ESS] == resample.ess(k) and info[abi.R_SURVIVORS] == (counts > 0).sum()
        assert np.all(logw1 == info[abi.R_NEW_LOGW])
        ratio = np.exp(info[abi.R_NEW_LOGW]) / np.exp(logw0).mean()
        print("round", t, "ess", info[abi.R_ESS], "survivors", info[abi.R_SURVIVORS], "mean weight ratio - 1", ratio - 1.0)
        assert abs(ratio - 1.0) <= R.mean_weight_bound(B)
        after, _ = snapshot(d)
        for key in ("up", "J", "st", "it", "stats", "x", "z", "xref"):
            assert np.array_equal(after[key], before[key][anc]), key
        assert np.array_equal(after["scene"][:, :abi.ENV_LOGW], before["scene"][anc][:, :abi.ENV_LOGW])
        for kk in before["ws"]:
            assert np.array_equal(after["ws"][kk], before["ws"][kk][anc]), kk
        moved_total += int((anc != np.arange(B)).sum())
    assert moved_total > 0
    assert d.pl.last_kernel() == abi.KERNEL_LOOP_RICH
    # unforced to never: nothing changes
    d.loop(1)
    before, pol0 = snapshot(d)
    logw0, _, anc, info, logw1 = resample_round(gpu, d, 5, ess_fraction=0.0)
    after, pol1 = snapshot(d)
    assert info[abi.R_RESAMPLED] == 0.0 and np.array_equal(anc, np.arange(B)) and pol0 == pol1
    for key in before:
        if key == "ws":
            assert all(before["ws"][kk].tobytes() == after["ws"][kk].tobytes() for kk in before["ws"])
        else:
            assert before[key].tobytes() == after[key].tobytes(), key


def test_sharded_pair_draws_its_own_offsets(gpu, monkeypatch):
    """Two plans of 32 egos, ego_base 0 and 32 (rows 0..31 and 32..63 of the 64-ego case): each shard's
    ancestors equal its own restatement, and the two draws differ."""
    whole = overtake_case(6, 1, 64)
    set_path(monkeypatch, 0, 1)
    assert resample.offset(SEED, 0, 2) != resample.offset(SEED, 32, 2)
    for base in (0, 32):
        case = dict(whole, scene=whole["scene"][base:base + 32], policies=whole["policies"][base:base + 32])
        d = tilted_loop(gpu, case, ego_base=base)
        d.loop(2)
        _, k, anc, info, _ = resample_round(gpu, d, 2, ego_base=base)
        assert info[abi.R_RESAMPLED] == 1.0
        assert np.array_equal(anc, resample.ancestors(k, resample.offset(SEED, base, 2))[0]), base


# ---- 4: refusals ------------------------------------------------------------------------------------

def raw_desc(scheme=0, rnd=0, ess_fraction=0.5, seed=0, ego_base=0):
    D = abi.ResampleDesc()
    D.scheme, D.round, D.ess_fraction, D.seed, D.ego_base = scheme, rnd, ess_fraction, seed, ego_base
    return D


def test_refusals(gpu, monkeypatch):
    """Every -22 of the three entries, with a message; none of them enqueues anything (the output buffers
    keep their sentinels)."""
    import torch
    from bmpc import plan as P
    set_path(monkeypatch)
    B = 8
    logw = torch.zeros(B * 2, dtype=torch.float64, device="cuda")
    anc = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((abi.RESAMPLE_NINFO,), -7.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx = P.context(0)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def ancestors(desc=None, batch=B, lw=logw, stride=1, a=anc, i=info, c=ctx):
        rc = lib().bmpc_population_ancestors(c, None if desc is False else C.byref(desc or raw_desc()), batch, vp(lw), stride,
                                             vp(a), None, vp(i), None)
        return rc, lib().bmpc_last_error().decode()

    assert ancestors()[0] == 0
    torch.cuda.synchronize()
    assert np.array_equal(anc.cpu().numpy(), np.arange(B))
    anc.fill_(-7), info.fill_(-7.5)
    torch.cuda.synchronize()
    for kw, word in ((dict(batch=0), "batch"), (dict(batch=-3), "batch"), (dict(batch=(1 << 20) + 1), "batch"),
                     (dict(stride=0), "stride"), (dict(desc=raw_desc(scheme=1)), "scheme"),
                     (dict(desc=raw_desc(ess_fraction=-0.5)), "ess_fraction"), (dict(desc=raw_desc(ess_fraction=np.nan)), "ess_fraction"),
                     (dict(desc=raw_desc(ess_fraction=np.inf)), "ess_fraction"), (dict(desc=raw_desc(ego_base=-1)), "ego_base"),
                     (dict(desc=False), "null"), (dict(lw=None), "null"), (dict(a=None), "null"), (dict(i=None), "null"),
                     (dict(c=None), "null")):
        rc, msg = ancestors(**kw)
        assert rc == -22 and word in msg and "bmpc_population_ancestors" in msg, (kw, rc, msg)
    d = Loop(gpu, overtake_case(6, 1, B))
    bufs = abi.make_ego_buffers(buffers(d))

    def resample_rc(pl=d.pl, desc=None, b=bufs, a=anc, i=info):
        rc = lib().bmpc_resample_device(pl._h if pl else None, None if desc is False else C.byref(desc or raw_desc()),
                                        None if b is None else C.byref(b), vp(a), vp(i), None)
        return rc, lib().bmpc_last_error().decode()

    no_scene = abi.make_ego_buffers(dict(buffers(d), scene=None))
    merge = gpu.BatchPlan(merge_desc(N=12), B)
    xdesc = highway_desc(N=6)
    xdesc.flags = abi.PLAN_TRANSFORM
    xform = gpu.BatchPlan(xdesc, B)
    for kw, word in ((dict(pl=None), "null"), (dict(desc=False), "null"), (dict(b=None), "null"), (dict(b=no_scene), "null"),
                     (dict(a=None), "null"), (dict(i=None), "null"), (dict(desc=raw_desc(scheme=2)), "scheme"),
                     (dict(desc=raw_desc(ess_fraction=-1.0)), "ess_fraction"), (dict(desc=raw_desc(ego_base=-5)), "ego_base"),
                     (dict(pl=merge), "merge scene's obstacle never chooses"), (dict(pl=xform), "BMPC_PLAN_TRANSFORM")):
        rc, msg = resample_rc(**kw)
        assert rc == -22 and word in msg and "bmpc_resample_device" in msg, (kw, rc, msg)
    rc = lib().bmpc_gather_egos(d.pl._h, None, C.byref(bufs), None)
    assert rc == -22 and "bmpc_gather_egos" in lib().bmpc_last_error().decode()
    rc = lib().bmpc_gather_egos(None, vp(anc), C.byref(bufs), None)
    assert rc == -22
    with pytest.raises(ValueError):
        d.pl.gather_egos(anc[:4], buffers(d))
    with pytest.raises(ValueError):
        d.pl.resample(buffers(d), -1)
    torch.cuda.synchronize()
    assert np.all(anc.cpu().numpy() == -7) and np.all(info.cpu().numpy() == -7.5)
    # every plan kind gathers: the merge and the transform plan take the identity and a swap
    swap = torch.tensor([1, 0] + list(range(2, B)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for pl in (merge, xform):
        pl.gather_egos(swap)
    torch.cuda.synchronize()


# ---- 5: the population entries -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["overtake", "quadruped"])
def test_resampled_population_keeps_more_effective_samples(gpu, monkeypatch, kind):
    """resampled_*_population against weighted_*_population with the same tilt and seeds at the same step
    count: the effective sample size after the last round is at least the unresampled one."""
    from bmpc import montecarlo
    set_path(monkeypatch)
    B, steps, every = 256, 8, 2
    if kind == "overtake":
        kw = dict(desc=highway_desc(N=6), tilt=(1.0, 4.0, 0.25), obstacle_seed=7)
        plain = scenarios.weighted_overtake_population(B, steps, **kw)
        got = scenarios.resampled_overtake_population(B, steps, every, ess_fraction=0.5, resample_seed=SEED, record=True, **kw)
    else:
        kw = dict(desc=quadruped_desc(N=6), tilt=(1.0, 5.0), obstacle_seed=7)
        plain = scenarios.weighted_quadruped_population(B, steps, **kw)
        got = scenarios.resampled_quadruped_population(B, steps, every, ess_fraction=0.5, resample_seed=SEED, record=True, **kw)
    stats, scene, logw, rec, rounds = got
    assert stats.shape == (B, abi.ENV_NSTAT) and scene.shape == (B, abi.ENV_STRIDE) and len(rounds) == steps // every - 1
    assert np.array_equal(logw, scene[:, abi.ENV_LOGW]) and np.all(scene[:, abi.ENV_STEPS] == steps)
    ess_plain = montecarlo.estimate(np.ones(B), plain[2])[2]
    ess_res = montecarlo.estimate(np.ones(B), logw)[2]
    print(kind, "effective sample size after", steps, "steps: resampled", ess_res, "plain", ess_plain,
          "resampled in rounds", [int(i[abi.R_RESAMPLED]) for _, i in rounds])
    assert ess_res >= ess_plain
    for r, (anc, info) in enumerate(rounds):
        t = (r + 1) * every
        assert anc.shape == (B,) and info.shape == (abi.RESAMPLE_NINFO,)
        if info[abi.R_RESAMPLED]:   # the record's scene rows just after the resampling carry the mean weight's history
            assert np.all(np.isfinite(rec.logw[:, t]))
        else:
            assert np.array_equal(anc, np.arange(B))
    lin = montecarlo.lineage([a for a, _ in rounds])
    assert lin.shape == (B, len(rounds) + 1) and np.array_equal(lin[:, -1], np.arange(B))
