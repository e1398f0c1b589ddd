"""BMPC_THIN_CALLERS (csrc/bmpc_ipm.h): a KKT solve as its front calls, its back half and its
refinement, the refinements' corrections as a tree solve and a back-half leaf, the coupling
build apart from its tree solve.  Only where a function begins and ends changes, so the default
host build (BMPC_PHASE_NOCSR is 1 in every build, csrc/bmpc_core.h, and BMPC_THIN_CALLERS follows it;
the fixture checks that the two shared objects differ) must give exactly the results of the build
with -DBMPC_THIN_CALLERS=0 over the every-exit closed loops of tests/test_ipm_lean_passes.py (optimal, maxit and
backtrack exits, both refinement depths, the rich and the slab coupling system)."""
import importlib.util
import os

import numpy as np
import pytest

import hostsim_lib as H1
from test_ipm_lean_passes import _loop

OFF = "-DBMPC_THIN_CALLERS=0"


@pytest.fixture(scope="module")
def H0():
    """hostsim_lib over the =0 build (the module reads its flag set when it is imported)."""
    old = os.environ.get("BMPC_HOSTSIM_FLAGS")
    os.environ["BMPC_HOSTSIM_FLAGS"] = OFF
    try:
        spec = importlib.util.spec_from_file_location("hostsim_lib_thin_callers_0", H1.__file__)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["BMPC_HOSTSIM_FLAGS"]
        else:
            os.environ["BMPC_HOSTSIM_FLAGS"] = old
    assert mod.FLAGS == [OFF] and mod.SO != H1.SO
    mod.lib()
    H1.lib()
    with open(mod.SO, "rb") as f0, open(H1.SO, "rb") as f1:   # the default build really is the other call structure
        assert f0.read() != f1.read(), "the default host build compiles the BMPC_THIN_CALLERS=0 code"
    return mod


@pytest.mark.parametrize("N,NB,maxit,lean", [(4, 1, 26, 0), (3, 2, 32, 0), (4, 1, 26, 1), (3, 2, 32, 1)])
def test_thin_callers_bit_identical(H0, monkeypatch, N, NB, maxit, lean):
    assert H1.FLAGS == [], "the default host build is the =1 side of this comparison"
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", str(lean))
    ref = _loop(H0, N, NB, maxit)
    new = _loop(H1, N, NB, maxit)
    st, it = ref[0]["status"], ref[0]["iters"]
    assert ((st == 0) & (it < maxit)).any() and (it == maxit).any()
    assert (((st == 10) | (st < 0)) & (it < maxit)).any()
    for s, (a, b) in enumerate(zip(ref, new)):
        for k in ("status", "iters", "J", "upred", "xpred", "warm_uLin", "warm_pprev", "warm_misc"):
            assert np.array_equal(a[k], b[k]), (s, k)
