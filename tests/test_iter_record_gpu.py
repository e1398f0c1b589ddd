"""BMPC_ITER_RECORD (csrc/bmpc_core.h, csrc/bmpc_ipm.h): the one-wave kernels keep the IPM loop's
wave-uniform state (tau, kappa, the residual scales, the best iterate's figures, the step quantities)
in a record in the wave's LDS (Plan::lds_it) and fetch it as scalar operands where a pass uses it; the
small-batch kernel keeps the loop with locals.  No floating-point operation changes; what can go wrong is a
slot read before it is written, an LDS area overlapping another's, or a product that the compiler
contracts differently around a value that now comes from memory.  The every-exit closed loops of
tests/test_ipm_lean_passes.py (N=4 NB=1 maxit 26 and N=3 NB=2 maxit 32, tolerances 1e-10, 16 egos,
3 steps, egos 3, 7 and 11 on their obstacle) on the rich, lean and small-batch (blk) launches and on
the fused loop's rich and lean instantiations:

  * no status is -9 (the best-iterate guard: the record against its slab mirror) and none is
    outside the IPM's exit codes;
  * the three exit kinds occur on the device too;
  * the fused loop equals the per-step launches bit for bit;
  * per step, at least as many egos agree with the host build (hostsim_lib) in status and in
    iteration count as at the parent commit.

The parent commit on this same test (profiles/iter_record/parent_agreement.txt), egos of 16 that
agree with the host build per step, status / iterations -- the counts of tests/test_phase_calls_gpu.py,
since no arithmetic changed in between:
    N=4 NB=1  rich [15, 14, 14] / [11, 11, 11]   lean [15, 14, 14] / [11, 11, 11]   blk [14, 14, 13] / [11, 11, 11]
    N=3 NB=2  rich [14, 14, 14] / [12, 13, 10]   lean [14, 14, 14] / [12, 13, 10]   blk [15, 15, 13] / [13, 13, 13]

And a 65-ego N=20 NB=1 solve (two blocks' worth of the wave launch and an odd ego) and a 3-ego
N=8 NB=2 solve of the default library equal those of the library built with -DBMPC_ITER_RECORD=0
(libbmpc_rec0.so, which __graft_entry__.build() compiles beside the product; loaded through
BMPC_LIBRARY in a process of its own) in status, iterations, J and uPred, bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from bmpc import _lib, plan
from bmpc.scenarios import highway_desc
from common import REPO, highway_policy_rows, seeded_batch
from loop_common import PATHS, assert_record_equals, assert_same_finals, gpu, manual, recorded, set_path  # noqa: F401
from test_phase_calls_gpu import ALLOWED, EGOS, PARENT, STEPS, _case, _host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", ["rich", "lean", "blk"])
@pytest.mark.parametrize("N,NB,maxit", [(4, 1, 26), (3, 2, 32)])
def test_iter_record_every_exit(gpu, monkeypatch, N, NB, maxit, path):
    block_egos, rich, k_step, k_loop = PATHS[("overtake", "wave" if path == "rich" else path)]
    set_path(monkeypatch, block_egos, rich)
    cols, kernels, fin = manual(gpu, _case(N, NB, maxit), STEPS)
    assert kernels <= set(k_step), (path, kernels)
    st, it = cols["status"], cols["iters"]
    hst, hit = _host(N, NB, maxit, 1 if path == "lean" else 0)
    agree_st = (st == hst).sum(0).tolist()
    agree_it = (it == hit).sum(0).tolist()
    print(f"N={N} NB={NB} {path}: host agreement per step, status {agree_st} iters {agree_it}")
    print("  status", st.T.tolist(), "\n  iters", it.T.tolist())
    assert not (st == -9).any(), ("best-iterate guard", np.argwhere(st == -9).tolist())
    assert np.isin(st, ALLOWED).all(), np.unique(st, return_counts=True)
    st0, it0 = st[:, 0], it[:, 0]   # the first step, where the host build asserts them
    assert ((st0 == 0) & (it0 < maxit)).any(), "no ego exits optimal"
    assert (it0 == maxit).any(), "no ego ends at maxit"
    assert (((st0 == 10) | (st0 < 0)) & (it0 < maxit)).any(), "no ego ends through the backtrack"
    want_st, want_it = PARENT[(N, NB, path)]
    assert all(a >= w for a, w in zip(agree_st, want_st)), (agree_st, want_st)
    assert all(a >= w for a, w in zip(agree_it, want_it)), (agree_it, want_it)
    if path == "blk":   # small batches keep their launches per step: no fused instantiation
        return
    rec, kf, ffin = recorded(gpu, _case(N, NB, maxit), [STEPS])
    assert set(kf) <= set(k_loop), (path, kf)
    assert_record_equals(rec, cols)
    assert_same_finals(fin, ffin)


@pytest.mark.parametrize("B,N,NB", [(65, 20, 1), (3, 8, 2)])
def test_iter_record_equals_locals_build(tmp_path, B, N, NB):
    rec0 = os.path.join(os.path.dirname(_lib.SO_PATH), "libbmpc_rec0.so")
    assert _lib.stamp(rec0) == _lib.source_hash(), "libbmpc_rec0.so is not built from this tree (__graft_entry__.build())"
    out = tmp_path / "rec0.npz"
    env = dict(os.environ, BMPC_LIBRARY=rec0)
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "variant_check.py"), str(out), str(B), str(N), str(NB)],
                   check=True, env=env, timeout=120)
    ref = np.load(out)
    x, z, xref, tgt = seeded_batch(B, seed=0)   # (tools/variant_check.py's batch)
    pl = plan.BatchPlan(highway_desc(N=N, NB=NB), B)
    pl.set_policies(highway_policy_rows(tgt))
    r = pl.solve(x, z, xref)
    assert os.path.abspath(os.environ.get("BMPC_LIBRARY", _lib.SO_PATH)) != os.path.abspath(rec0)
    for k in ("status", "iters", "J", "upred"):
        assert np.array_equal(ref[k], r[k]), (k, np.argwhere(np.asarray(ref[k] != r[k]))[:8].tolist())
