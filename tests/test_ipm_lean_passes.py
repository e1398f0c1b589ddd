"""BMPC_IPM_LEAN_PASSES (csrc/bmpc_ipm.h): the IPM iteration without the passes and re-reads its
result does not need -- the LP rows' step-length search inside the direction passes, dx / dy formed
in the update (the finiteness flag with them, so a failed step is seen after x was written), the
affine step's two dot pairs in one pass, -e_J written once and -rx formed with rx.  Every value
comes from the same expression as before, so the host build with -DBMPC_IPM_LEAN_PASSES=1 (the
default) must give exactly the results of the build with =0, bit for bit, over closed-loop steps:
statuses, iteration counts, J, the predicted inputs and states and the warm start carried to the
next solve.

The plans are small (N=4 NB=1 and N=3 NB=2, 16 egos, 3 steps), so their descriptor is changed to
reach every exit of the loop in one batch: the tolerances are tightened to 1e-10 (some egos meet
them, the others run into the step-length floor and leave through the backtrack to the best
iterate) and maxit is lowered to 26 / 32 (inside the batch's range of iteration counts, so some
egos end there).  Three egos start on top of their obstacle.  The test asserts that the =0 build's first step shows all three kinds."""
import importlib.util
import os

import numpy as np
import pytest

import hostsim_lib as H1
from bmpc import abi
from common import highway_desc, highway_policy_rows, seeded_batch

OFF = "-DBMPC_IPM_LEAN_PASSES=0"


@pytest.fixture(scope="module")
def H0():
    """hostsim_lib over the =0 build (the module reads its flag set when it is imported)."""
    old = os.environ.get("BMPC_HOSTSIM_FLAGS")
    os.environ["BMPC_HOSTSIM_FLAGS"] = OFF
    try:
        spec = importlib.util.spec_from_file_location("hostsim_lib_lean_passes_0", H1.__file__)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["BMPC_HOSTSIM_FLAGS"]
        else:
            os.environ["BMPC_HOSTSIM_FLAGS"] = old
    assert mod.FLAGS == [OFF] and mod.SO != H1.SO
    mod.lib()
    return mod


def _desc(N, NB, maxit):
    d = highway_desc(N, NB)
    d.maxit = maxit
    d.feastol = d.abstol = d.reltol = 1e-10
    return d


def _loop(H, N, NB, maxit, egos=16, steps=3):
    x, z, xref, tgt = seeded_batch(egos, 2)
    for e in (3, 7, 11):   # on top of the obstacle
        z[e] = x[e]
        z[e, 0] += 0.5 * (e % 3)
    hs = H.HostSim(_desc(N, NB, maxit), egos)
    hs.set_policies(highway_policy_rows(tgt))
    env = abi.make_env()
    scene = np.zeros((egos, abi.ENV_STRIDE))
    scene[:, 0:4], scene[:, 4:8] = x, z
    lay = hs.layout()
    U, d = hs.U, hs.desc.d
    warm = {"uLin": (U + 1) * d, "pprev": hs.bdim * hs.desc.m, "misc": 2 + d}   # MISC_INIT, MISC_JCONS, MISC_OLDU
    out, r = [], None
    for t in range(steps):
        x, z, xref = hs.env_step(env, t, scene, *(() if r is None else (r["upred"], r["J"], r["status"], r["iters"])))
        r = hs.solve(x, z, xref)
        for k, cnt in warm.items():
            r["warm_" + k] = np.array([hs.workspace(e)[lay[k]:lay[k] + cnt] for e in range(egos)])
        out.append(r)
    return out


@pytest.mark.parametrize("N,NB,maxit,lean", [(4, 1, 26, 0), (3, 2, 32, 0), (4, 1, 26, 1), (3, 2, 32, 1)])
def test_lean_passes_bit_identical(H0, monkeypatch, N, NB, maxit, lean):
    assert H1.FLAGS == [], "the default host build is the =1 side of this comparison"
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", str(lean))
    ref = _loop(H0, N, NB, maxit)
    new = _loop(H1, N, NB, maxit)
    st, it = ref[0]["status"], ref[0]["iters"]
    print("=0 build, step 0: status", st.tolist(), "iters", it.tolist())
    assert ((st == 0) & (it < maxit)).any(), "no ego exits optimal"
    assert (it == maxit).any(), "no ego ends at maxit"
    assert (((st == 10) | (st < 0)) & (it < maxit)).any(), "no ego ends through the backtrack"
    for s, (a, b) in enumerate(zip(ref, new)):
        for k in ("status", "iters", "J", "upred", "xpred", "warm_uLin", "warm_pprev", "warm_misc"):
            assert np.array_equal(a[k], b[k]), (s, k)


@pytest.mark.gpu
def test_lean_passes_gpu_kernels(monkeypatch):
    """The product library's rich, lean and small-batch kernels run the lean passes to an allowed
    status (the bit-for-bit comparison of two GPU builds is the A/B's, tools/ab_pmc.sh)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from bmpc import plan
    B = 8
    want = {"rich": (abi.KERNEL_IPM_RICH,), "lean": (abi.KERNEL_IPM_LEAN,),
            "blk": (abi.KERNEL_IPM_BLK4, abi.KERNEL_IPM_BLK8)}
    for path, env in (("rich", {"BMPC_BLOCK_EGOS": "0", "BMPC_LDS_RICH": "1"}),
                      ("lean", {"BMPC_BLOCK_EGOS": "0", "BMPC_LDS_RICH": "0"}), ("blk", {})):
        for k in ("BMPC_BLOCK_EGOS", "BMPC_LDS_RICH", "BMPC_BLOCK_WAVES", "BMPC_BLK_LDS", "BMPC_IPM_PHASED"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        x, z, xref, tgt = seeded_batch(B, seed=0)
        pl = plan.BatchPlan(highway_desc(4, 1), B)
        pl.set_policies(highway_policy_rows(tgt))
        for _ in range(2):
            r = pl.solve(x, z, xref)
            assert pl.last_kernel() in want[path], (path, pl.last_kernel())
            assert (r["status"] >= 0).all(), (path, r["status"])   # as the other GPU tests: no failed solve
            u0 = r["upred"][:, 0]
            x = x + 0.1 * np.stack([x[:, 2] * np.cos(x[:, 3]), x[:, 2] * np.sin(x[:, 3]), u0[:, 0], u0[:, 1]], 1)
            z = z + 0.1 * np.stack([z[:, 2], 0 * z[:, 0], 0 * z[:, 0], 0 * z[:, 0]], 1)
