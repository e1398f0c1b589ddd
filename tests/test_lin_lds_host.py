"""BMPC_LIN_LDS (csrc/bmpc_core.h, csrc/bmpc_ipm.h lin_A / lin_fill): the IPM reads A of the solve's
linearisation -- the input nodes' state matrices, written once per solve by the tree step -- through an
accessor over a compact per-solve copy of the entries that vary from node to node; every other entry is a
constant of the model's description (csrc/bmpc_model.h HighwayLin), checked against the slab when the copy
is filled.  The host build runs the same accessor over its LDS stand-in, following what the plan carved
(Plan::nlin_a).

Every term of every sum stays in place, so the default host build must give exactly the results of the
build with -DBMPC_LIN_LDS=0 over the every-exit closed loops of tests/test_ipm_lean_passes.py, on a small
merge plan, on a plan that judges the cache on its lean launch and on one whose cache does not fit.  The
guard's precondition is checked on the slab itself after the tree step, the guard is tripped by overwriting
one constant entry of one ego's A between the tree step and the IPM (tests/hostsim/lin_lds_host.cpp splits
the solve there), and a plan with a table value outside 16 bits gets no cache."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import hostsim_lib as H1
from bmpc import abi
from common import golden, highway_desc, highway_policy_rows, seeded_batch
from test_ipm_lean_passes import _desc, _loop
from test_merge import NAME as MERGE, merge_desc, merge_rows, replay_inputs

OFF = "-DBMPC_LIN_LDS=0"
EXIT_GUARD = -9
KEYS = ("status", "iters", "J", "upred", "xpred")


def _module(name, flags):
    old = os.environ.get("BMPC_HOSTSIM_FLAGS")
    os.environ["BMPC_HOSTSIM_FLAGS"] = flags
    try:
        spec = importlib.util.spec_from_file_location(name, H1.__file__)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["BMPC_HOSTSIM_FLAGS"]
        else:
            os.environ["BMPC_HOSTSIM_FLAGS"] = old
    return mod


@pytest.fixture(scope="module")
def H0():
    """hostsim_lib over the =0 build (the module reads its flag set when it is imported)."""
    mod = _module("hostsim_lib_lin_lds_0", OFF)
    assert mod.FLAGS == [OFF] and mod.SO != H1.SO
    mod.lib()
    H1.lib()
    with open(mod.SO, "rb") as f0, open(H1.SO, "rb") as f1:   # the default build really is the cache's code
        assert f0.read() != f1.read(), "the default host build compiles the BMPC_LIN_LDS=0 code"
    return mod


@pytest.fixture(scope="module")
def HL():
    """hostsim_lib over tests/hostsim/lin_lds_host.cpp: the default build plus hs_lin_info and the solve
    in two halves (hs_tree_only, hs_ipm_only)."""
    assert H1.FLAGS == []
    mod = _module("hostsim_lib_lin_lds_split", "")
    hs_dir = os.path.join(H1.HERE, "hostsim")
    mod.HDRS = mod.HDRS + mod.SRCS            # (the sources it includes: part of its stamp)
    mod.SRCS = [os.path.join(hs_dir, "lin_lds_host.cpp")]
    mod.SO = os.path.join(hs_dir, "libbmpc_hostsim_lin_lds.so")
    mod.lib()
    return mod


def _info(HL, hs):
    out = np.zeros(7, np.int32)
    HL.lib().hs_lin_info(hs.h, out.ctypes.data_as(C.c_void_p))
    return dict(zip(("lds_lin", "nlin_a", "tab16", "nlds", "ntab", "na", "on"), map(int, out)))


def _same(ref, new):
    for s, (a, b) in enumerate(zip(ref, new)):
        for k in a:
            assert np.array_equal(a[k], b[k]), (s, k)


@pytest.mark.parametrize("N,NB,maxit,lean", [(4, 1, 26, 0), (3, 2, 32, 0), (4, 1, 26, 1), (3, 2, 32, 1)])
def test_lin_lds_bit_identical(H0, HL, monkeypatch, N, NB, maxit, lean):
    assert H1.FLAGS == [], "the default host build is the =1 side of this comparison"
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", str(lean))
    hs = HL.HostSim(_desc(N, NB, maxit), 1)
    i = _info(HL, hs)
    assert i["on"] == 1 and i["nlin_a"] == 4 * hs.U, i   # the plan has the cache
    ref = _loop(H0, N, NB, maxit)
    new = _loop(H1, N, NB, maxit)
    st, it = ref[0]["status"], ref[0]["iters"]
    assert ((st == 0) & (it < maxit)).any(), "no ego exits optimal"
    assert (it == maxit).any(), "no ego ends at maxit"
    assert (((st == 10) | (st < 0)) & (it < maxit)).any(), "no ego ends through the backtrack"
    assert not (st == EXIT_GUARD).any()
    _same(ref, new)


def _merge_small(H, N=5, egos=8, solves=2):
    g = golden(MERGE)
    rb = replay_inputs(g, egos)
    d = merge_desc(g)
    d.N = N
    hs = H.HostSim(d, egos)
    hs.set_policies(merge_rows(g, egos))
    hs.set_transform(rb["S"], rb["bx"])
    out = []
    for _ in range(solves):   # (the second solve starts from the first one's warm start)
        r = hs.solve(rb["x"], rb["z"], rb["xref"])
        out.append({k: r[k] for k in KEYS})
    return hs, out


def test_merge_plan(H0, HL, monkeypatch):
    """A small merge plan with the state transformation on: A is the highway models', and cached."""
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    hs, _ = _merge_small(HL, solves=0)
    i = _info(HL, hs)
    assert i["nlin_a"] == 4 * hs.U, i
    _, ref = _merge_small(H0)
    _, new = _merge_small(H1)
    assert (ref[0]["status"] >= 0).all(), ref[0]["status"]
    _same(ref, new)


def _highway_once(H, N, egos=2):
    x, z, xref, tgt = seeded_batch(egos, 2)
    hs = H.HostSim(highway_desc(N, 1), egos)
    hs.set_policies(highway_policy_rows(tgt))
    r = hs.solve(x, z, xref)
    return hs, [{k: r[k] for k in KEYS}]


@pytest.mark.parametrize("N,cached", [(40, True), (30, False)])
def test_longer_horizons(H0, HL, monkeypatch, N, cached):
    """The cache must fit the 9,984 bytes beside the other LDS of the launch that keeps 16 egos per CU:
    N=40 judges it on its lean launch (no coupling matrix, no tables) and has the room, N=30 on its rich
    one (with the tree-solve staging) and has not: that plan's IPM reads A from the slab."""
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    hs = HL.HostSim(highway_desc(N, 1), 1)
    i = _info(HL, hs)
    assert i["nlin_a"] == (4 * hs.U if cached else 0), i
    _, ref = _highway_once(H0, N)
    _, new = _highway_once(H1, N)
    assert (ref[0]["status"] >= 0).all(), ref[0]["status"]
    _same(ref, new)


def _split_loop(HL, N, NB, maxit, corrupt=None, egos=16, steps=3, check=None):
    """test_ipm_lean_passes._loop with each solve in its two halves; check(hs) runs between them, and
    corrupt = (step, ego, offset into Ad, value) overwrites one double of that ego's A there."""
    x, z, xref, tgt = seeded_batch(egos, 2)
    for e in (3, 7, 11):   # on top of the obstacle
        z[e] = x[e]
        z[e, 0] += 0.5 * (e % 3)
    hs = HL.HostSim(_desc(N, NB, maxit), egos)
    hs.set_policies(highway_policy_rows(tgt))
    env = abi.make_env()
    scene = np.zeros((egos, abi.ENV_STRIDE))
    scene[:, 0:4], scene[:, 4:8] = x, z
    lay, p = hs.layout(), lambda a: a.ctypes.data_as(C.c_void_p)
    out, r = [], None
    for t in range(steps):
        x, z, xref = hs.env_step(env, t, scene, *(() if r is None else (r["upred"], r["J"], r["status"], r["iters"])))
        x, z, xref = (np.ascontiguousarray(v) for v in (x, z, xref))
        HL.lib().hs_tree_only(hs.h, p(x), p(z), p(xref))
        if check is not None:
            check(hs, lay)
        if corrupt is not None and corrupt[0] == t:
            hs.workspace(corrupt[1])[lay["Ad"] + corrupt[2]] = corrupt[3]
        r = dict(upred=np.zeros((egos, hs.U, 2)), xpred=np.zeros((egos, hs.T, 4)), J=np.zeros(egos),
                 status=np.zeros(egos, np.int32), iters=np.zeros(egos, np.int32))
        HL.lib().hs_ipm_only(hs.h, 0, p(r["upred"]), p(r["xpred"]), p(r["J"]), p(r["status"]), p(r["iters"]))
        out.append(r)
    return out


def test_guard_precondition_on_the_slab(HL, monkeypatch):
    """After the tree step of the every-exit population, on every step: A is the identity outside
    (0,2), (0,3), (1,2), (1,3) -- what lin_fill compares -- and the two halves together are hs_solve.
    B's pattern (dt at (2,0), (3,1), zero elsewhere) and dh's zero columns 2 and 3 are checked with it: the
    IPM reads both from the slab today, and these are the facts that reading them as constants would need."""
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", "0")
    N, NB, maxit = 4, 1, 26
    dt = _desc(N, NB, maxit).dt
    seen = []

    def check(hs, lay):
        for e in range(hs.batch):
            w = hs.workspace(e)
            A = w[lay["Ad"]:lay["Ad"] + hs.U * 16].reshape(hs.U, 4, 4).copy()
            seen.append(np.abs(A[:, :2, 2:]).max())
            A[:, :2, 2:] = 0.0
            assert np.array_equal(A, np.broadcast_to(np.eye(4), A.shape)), e
            Bm = w[lay["Bd"]:lay["Bd"] + hs.U * 8].reshape(hs.U, 4, 2)
            want = np.zeros((4, 2))
            want[2, 0] = want[3, 1] = dt
            assert np.array_equal(Bm, np.broadcast_to(want, Bm.shape)), e
            dh = w[lay["dh"]:lay["dh"] + hs.T * 4].reshape(hs.T, 4)
            assert np.array_equal(dh[:, 2:], np.zeros((hs.T, 2))), e

    new = _split_loop(HL, N, NB, maxit, check=check)
    assert max(seen) > 0.0   # (the varying entries do vary)
    ref = _loop(HL, N, NB, maxit)
    _same([{k: a[k] for k in KEYS} for a in ref], new)


@pytest.mark.parametrize("off,val", [(5, 1.0 + 2.0 ** -40), (1, 1e-300), (4 * 16 + 12, float("nan"))])
def test_guard_trips_on_a_changed_constant(HL, monkeypatch, off, val):
    """One constant entry of ego 5's A overwritten between the tree step and the IPM of step 1: that ego
    ends with EXIT_GUARD and keeps its previous solution, every other ego's bits are unchanged."""
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", "0")
    N, NB, maxit, ego = 4, 1, 26, 5
    ref = _split_loop(HL, N, NB, maxit, steps=2)
    new = _split_loop(HL, N, NB, maxit, steps=2, corrupt=(1, ego, off, val))
    _same(ref[:1], new[:1])
    assert new[1]["status"][ego] == EXIT_GUARD and new[1]["iters"][ego] == 0
    assert ref[1]["status"][ego] != EXIT_GUARD
    assert np.array_equal(new[1]["upred"][ego], new[0]["upred"][ego])   # the previous solution stays
    others = np.arange(16) != ego
    for k in KEYS:
        assert np.array_equal(ref[1][k][others], new[1][k][others]), k


def test_tables_outside_16_bits_get_no_cache(HL):
    """The launches with the cache hold their LDS copy of the topology tables in 16 bits: a plan with a
    table value beyond them (here the cones' row offsets of a 2,000-step horizon) is marked at plan build
    and carves no cache, so it never takes them; the plans the suite runs are far inside."""
    big = _info(HL, HL.HostSim(highway_desc(2000, 1), 1))
    assert big["tab16"] == 0 and big["nlin_a"] == 0, big
    for N, NB in ((20, 1), (8, 2), (30, 2)):
        assert _info(HL, HL.HostSim(highway_desc(N, NB), 1))["tab16"] == 1, (N, NB)
