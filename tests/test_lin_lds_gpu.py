"""BMPC_LIN_LDS (csrc/bmpc_core.h, csrc/bmpc_ipm.h lin_A / lin_fill) on the device: the one-wave kernels
read A of the solve's linearisation from a compact copy in the wave's LDS (the entries that vary from node
to node; the others are the model's constants), filled and checked against the slab at the start of each
solve, and keep their LDS copy of the topology tables in 16 bits.  The library takes these kernels for
batches beyond 8 egos per CU; BMPC_LIN_CACHE=1 asks for them at the tests' sizes.  No floating-point operation changes;
what can go wrong is the cache overlapping another LDS area, a table value cut by the narrower copy, a
stale cache in the fused loop (it is refilled after every tree step) or the guard tripping on a slab the
description does hold for.  The every-exit closed loops of tests/test_ipm_lean_passes.py (N=4 NB=1 maxit 26
and N=3 NB=2 maxit 32, tolerances 1e-10, 16 egos, 3 steps, egos 3, 7 and 11 on their obstacle) on the rich
and lean one-wave launches and on the fused loop's rich and lean instantiations:

  * no status is -9 (lin_fill's guard, the best-iterate guard) and none is outside the IPM's exit codes;
  * the three exit kinds occur on the device too;
  * the fused loop equals the per-step launches bit for bit;
  * per step, at least as many egos agree with the host build (hostsim_lib) in status and in iteration
    count as tests/test_phase_calls_gpu.py's PARENT counts.

The default library equals the library built with -DBMPC_LIN_LDS=0 (libbmpc_lin0.so, which
__graft_entry__.build() compiles beside the product; loaded through BMPC_LIBRARY by tools/variant_check.py
in a process of its own) in status, iterations, J and uPred, bit for bit: 65 egos N=20 NB=1 on the rich
launch, 5 egos N=8 NB=2 on the lean one, and three closed-loop steps of 6 egos of the merge scene at N=10
(the fused loop's merge instantiation).  And the small-batch kernel, which has no cache, runs one ego at
N=4 NB=1 as libbmpc_lin0.so does.  Which launch read the cache is asked of the plan (bmpc_last_lin_cache):
the forced launches above, and the library's own rule on 4,096 egos (the cache, on the rich kernel, at
N=20 and at N=22, where the launch with the cache must be priced with its 16-bit tables to stay rich) and
on 1,024 (the parent's kernel).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from bmpc import _lib, abi, plan, scenarios
from bmpc.scenarios import highway_desc
from common import REPO, highway_policy_rows, seeded_batch
from loop_common import PATHS, assert_record_equals, assert_same_finals, gpu, manual, recorded, set_path  # noqa: F401
from test_phase_calls_gpu import ALLOWED, PARENT, STEPS, _case, _host

pytestmark = pytest.mark.gpu

ONE_WAVE = {"rich": {"BMPC_BLOCK_EGOS": "0", "BMPC_LDS_RICH": "1"}, "lean": {"BMPC_BLOCK_EGOS": "0", "BMPC_LDS_RICH": "0"},
            "blk": {}}
KERNELS = {"rich": (abi.KERNEL_IPM_RICH,), "lean": (abi.KERNEL_IPM_LEAN,), "blk": (abi.KERNEL_IPM_BLK4, abi.KERNEL_IPM_BLK8)}


@pytest.mark.parametrize("path", ["rich", "lean"])
@pytest.mark.parametrize("N,NB,maxit", [(4, 1, 26), (3, 2, 32)])
def test_lin_lds_every_exit(gpu, monkeypatch, N, NB, maxit, path):
    block_egos, rich, k_step, k_loop = PATHS[("overtake", "wave" if path == "rich" else path)]
    set_path(monkeypatch, block_egos, rich)
    monkeypatch.setenv("BMPC_LIN_CACHE", "1")
    cols, kernels, fin = manual(gpu, _case(N, NB, maxit), STEPS)
    assert kernels <= set(k_step), (path, kernels)
    st, it = cols["status"], cols["iters"]
    hst, hit = _host(N, NB, maxit, 1 if path == "lean" else 0)
    agree_st = (st == hst).sum(0).tolist()
    agree_it = (it == hit).sum(0).tolist()
    print(f"N={N} NB={NB} {path}: host agreement per step, status {agree_st} iters {agree_it}")
    print("  status", st.T.tolist(), "\n  iters", it.T.tolist())
    assert not (st == -9).any(), ("guard", np.argwhere(st == -9).tolist())
    assert np.isin(st, ALLOWED).all(), np.unique(st, return_counts=True)
    st0, it0 = st[:, 0], it[:, 0]   # the first step, where the host build asserts them
    assert ((st0 == 0) & (it0 < maxit)).any(), "no ego exits optimal"
    assert (it0 == maxit).any(), "no ego ends at maxit"
    assert (((st0 == 10) | (st0 < 0)) & (it0 < maxit)).any(), "no ego ends through the backtrack"
    want_st, want_it = PARENT[(N, NB, path)]
    assert all(a >= w for a, w in zip(agree_st, want_st)), (agree_st, want_st)
    assert all(a >= w for a, w in zip(agree_it, want_it)), (agree_it, want_it)
    rec, kf, ffin = recorded(gpu, _case(N, NB, maxit), [STEPS])
    assert set(kf) <= set(k_loop), (path, kf)
    assert_record_equals(rec, cols)
    assert_same_finals(fin, ffin)


def _lin0(tmp_path, env, *args):
    """tools/variant_check.py over libbmpc_lin0.so in a process of its own: its saved arrays."""
    lin0 = os.path.join(os.path.dirname(_lib.SO_PATH), "libbmpc_lin0.so")
    assert _lib.stamp(lin0) == _lib.source_hash(), "libbmpc_lin0.so is not built from this tree (__graft_entry__.build())"
    assert os.path.abspath(os.environ.get("BMPC_LIBRARY", _lib.SO_PATH)) != os.path.abspath(lin0)
    out = tmp_path / "lin0.npz"
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "variant_check.py"), str(out), *map(str, args)],
                   check=True, env=dict(os.environ, BMPC_LIBRARY=lin0, **env), timeout=120)
    return np.load(out)


def _equal(ref, got):
    for k in ("status", "iters", "J", "upred"):
        assert np.array_equal(ref[k], got[k]), (k, np.argwhere(np.asarray(ref[k] != got[k]))[:8].tolist())


@pytest.mark.parametrize("path,B,N,NB", [("rich", 65, 20, 1), ("lean", 5, 8, 2), ("blk", 1, 4, 1)])
def test_lin_lds_equals_slab_build(gpu, tmp_path, monkeypatch, path, B, N, NB):
    for k in ("BMPC_BLOCK_EGOS", "BMPC_LDS_RICH"):
        monkeypatch.delenv(k, raising=False)
    env = dict(ONE_WAVE[path], BMPC_LIN_CACHE="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref = _lin0(tmp_path, env, B, N, NB)
    x, z, xref, tgt = seeded_batch(B, seed=0)   # (tools/variant_check.py's batch)
    pl = plan.BatchPlan(highway_desc(N=N, NB=NB), B)
    pl.set_policies(highway_policy_rows(tgt))
    r = pl.solve(x, z, xref)
    assert pl.last_kernel() in KERNELS[path], (path, pl.last_kernel())
    assert pl.last_lin_cache() == (path != "blk"), path
    assert (r["status"] != -9).all(), r["status"]
    _equal(ref, r)


@pytest.mark.parametrize("B,N,cache", [(4096, 20, True), (4096, 22, True), (1024, 20, False)])
def test_lin_lds_default_rule(gpu, monkeypatch, B, N, cache):
    """The library's own choice: batches beyond 8 egos per CU of a plan with room take the cache, and
    stay on the rich kernel as at the parent commit; smaller ones run the parent's kernel."""
    for k in ("BMPC_BLOCK_EGOS", "BMPC_LDS_RICH", "BMPC_LIN_CACHE"):
        monkeypatch.delenv(k, raising=False)
    x, z, xref, tgt = seeded_batch(B, seed=0)
    pl = plan.BatchPlan(highway_desc(N=N, NB=1), B)
    pl.set_policies(highway_policy_rows(tgt))
    r = pl.solve(x, z, xref)
    assert pl.last_kernel() == abi.KERNEL_IPM_RICH, pl.last_kernel()
    assert pl.last_lin_cache() == cache
    assert (r["status"] != -9).all(), np.unique(r["status"], return_counts=True)


def test_lin_lds_merge_equals_slab_build(gpu, tmp_path, monkeypatch):
    monkeypatch.delenv("BMPC_LDS_RICH", raising=False)
    monkeypatch.delenv("BMPC_LOOP_FUSED", raising=False)
    monkeypatch.setenv("BMPC_BLOCK_EGOS", "0")   # the one-wave kernels: the merge k_loop
    monkeypatch.setenv("BMPC_LIN_CACHE", "1")
    B, N = 6, 10
    ref = _lin0(tmp_path, {"BMPC_BLOCK_EGOS": "0"}, B, N, 1, "merge")
    pl, scene0 = scenarios._seeded_plan("merge", B, 0, 0, desc=scenarios.merge_desc(N=N, NB=1))
    _, scene, rec = scenarios._closed_loop(pl, scene0, 3, "predictions", 0)
    got = {k: rec.col(k) for k in ("status", "iters", "J", "upred")}
    assert (got["status"] >= 0).all(), got["status"]
    _equal(ref, got)
    assert np.array_equal(ref["scene"], scene)
