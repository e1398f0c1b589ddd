"""BMPC_PHASE_NOCSR (csrc/bmpc_core.h): the solver's out-of-line phase functions are never tail
called, so the compiler drops their callee-saved register saves and every caller keeps what it
needs across a call itself.  No floating-point operation changes; what can go wrong is a register
lost across a call.  The every-exit closed loops of tests/test_ipm_lean_passes.py (N=4 NB=1 maxit
26 and N=3 NB=2 maxit 32, tolerances 1e-10, 16 egos, 3 steps, egos 3, 7 and 11 on their obstacle)
reach the optimal exit, the maxit exit and the backtrack exit, both refinement depths, and at NB=2
the tree solve of eight and more right-hand sides and the wave LU on the slab.  On the rich, lean
and small-batch (blk) launches, and on the fused loop's rich and lean instantiations:

  * no status is -9 (the best-iterate guard: a register lost across a phase call) and none is
    outside the IPM's exit codes;
  * the three exit kinds occur on the device too;
  * the fused loop equals the per-step launches bit for bit (separately register-allocated
    instantiations of the same templates);
  * per step, at least as many egos agree with the host build (hostsim_lib) in status and in
    iteration count as at the parent commit.

The parent commit on this same test (profiles/phase_calls/parent_agreement.log), egos of 16 that
agree with the host build per step, status / iterations (DESIGN.md §4.1 on why a device exit can
differ from the host's; these 1e-10 loops sit on such borders by construction.  The calling mode
changes no arithmetic, so this build reaches the same counts):
    N=4 NB=1  rich [15, 14, 14] / [11, 11, 11]   lean [15, 14, 14] / [11, 11, 11]   blk [14, 14, 13] / [11, 11, 11]
    N=3 NB=2  rich [14, 14, 14] / [12, 13, 10]   lean [14, 14, 14] / [12, 13, 10]   blk [15, 15, 13] / [13, 13, 13]
"""
import functools
import os

import numpy as np
import pytest

import hostsim_lib as H1
from bmpc import abi
from bmpc.scenarios import _overtake_scene
from common import highway_policy_rows, seeded_batch
from loop_common import PATHS, assert_record_equals, assert_same_finals, gpu, manual, recorded, set_path  # noqa: F401
from test_ipm_lean_passes import _desc, _loop

pytestmark = pytest.mark.gpu

EGOS, STEPS = 16, 3
ALLOWED = (0, 1, 2, 10, 11, 12, -1, -2)   # optimal, the certificates, their inaccurate forms, maxit, numerics
# egos of EGOS agreeing with the host at the parent commit, per step: (status, iterations)
PARENT = {
    (4, 1, "rich"): ([15, 14, 14], [11, 11, 11]), (4, 1, "lean"): ([15, 14, 14], [11, 11, 11]),
    (4, 1, "blk"): ([14, 14, 13], [11, 11, 11]),
    (3, 2, "rich"): ([14, 14, 14], [12, 13, 10]), (3, 2, "lean"): ([14, 14, 14], [12, 13, 10]),
    (3, 2, "blk"): ([15, 15, 13], [13, 13, 13]),
}


@functools.lru_cache(maxsize=None)
def _host(N, NB, maxit, lean):
    """The host build's loop (computed once per shape and coupling-system placement, read only)."""
    old = {k: os.environ.get(k) for k in ("BMPC_HOST_PHASED", "BMPC_HOST_LEAN")}
    os.environ["BMPC_HOST_PHASED"], os.environ["BMPC_HOST_LEAN"] = "0", str(lean)
    try:
        out = _loop(H1, N, NB, maxit, egos=EGOS, steps=STEPS)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return np.stack([r["status"] for r in out], 1), np.stack([r["iters"] for r in out], 1)


def _case(N, NB, maxit):
    x, z, _, tgt = seeded_batch(EGOS, 2)
    for e in (3, 7, 11):   # on top of the obstacle (test_ipm_lean_passes._loop)
        z[e] = x[e]
        z[e, 0] += 0.5 * (e % 3)
    return dict(kind="overtake", desc=_desc(N, NB, maxit), scene=_overtake_scene(x, z),
                policies=highway_policy_rows(tgt), env=abi.make_env())


@pytest.mark.parametrize("path", ["rich", "lean", "blk"])
@pytest.mark.parametrize("N,NB,maxit", [(4, 1, 26), (3, 2, 32)])
def test_phase_calls_every_exit(gpu, monkeypatch, N, NB, maxit, path):
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
