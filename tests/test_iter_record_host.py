"""BMPC_ITER_RECORD (csrc/bmpc_core.h, csrc/bmpc_ipm.h): the IPM loop's wave-uniform state -- tau, kappa,
the residual scales, the best iterate's figures, the step quantities -- in one record of named slots
behind an accessor (IterRec) instead of in locals, and the slab's arrays addressed where they are used.
The host build runs the same accessor code over a local struct (the one-wave kernels keep the record
in LDS).  No floating-point operation changes, so the default host build must give exactly the
results of the build with -DBMPC_ITER_RECORD=0 (the fixture checks that the two shared objects differ)
over the every-exit closed loops of tests/test_ipm_lean_passes.py: optimal, maxit and backtrack exits,
both refinement depths, the rich and the slab coupling system.  The host code is also compiled with a
stand-alone driver under the address and undefined-behaviour sanitizers and run over the N=4 loop."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import hostbuild
import hostsim_lib as H1
from bmpc import abi
from common import highway_policy_rows, seeded_batch
from test_ipm_lean_passes import _desc, _loop

OFF = "-DBMPC_ITER_RECORD=0"


@pytest.fixture(scope="module")
def H0():
    """hostsim_lib over the =0 build (the module reads its flag set when it is imported)."""
    old = os.environ.get("BMPC_HOSTSIM_FLAGS")
    os.environ["BMPC_HOSTSIM_FLAGS"] = OFF
    try:
        spec = importlib.util.spec_from_file_location("hostsim_lib_iter_record_0", H1.__file__)
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
    with open(mod.SO, "rb") as f0, open(H1.SO, "rb") as f1:   # the default build really is the record's code
        assert f0.read() != f1.read(), "the default host build compiles the BMPC_ITER_RECORD=0 code"
    return mod


@pytest.mark.parametrize("N,NB,maxit,lean", [(4, 1, 26, 0), (3, 2, 32, 0), (4, 1, 26, 1), (3, 2, 32, 1)])
def test_iter_record_bit_identical(H0, monkeypatch, N, NB, maxit, lean):
    assert H1.FLAGS == [], "the default host build is the =1 side of this comparison"
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", str(lean))
    ref = _loop(H0, N, NB, maxit)
    new = _loop(H1, N, NB, maxit)
    st, it = ref[0]["status"], ref[0]["iters"]
    assert ((st == 0) & (it < maxit)).any(), "no ego exits optimal"
    assert (it == maxit).any(), "no ego ends at maxit"
    assert (((st == 10) | (st < 0)) & (it < maxit)).any(), "no ego ends through the backtrack"
    for s, (a, b) in enumerate(zip(ref, new)):
        for k in ("status", "iters", "J", "upred", "xpred", "warm_uLin", "warm_pprev", "warm_misc"):
            assert np.array_equal(a[k], b[k]), (s, k)


def test_iter_record_sanitized(tmp_path, monkeypatch):
    """The N=4 NB=1 loop through the stand-alone sanitized program: the inputs of its three steps as the
    default build's loop produced them (test_ipm_lean_passes._loop's scene), the same exits out."""
    monkeypatch.setenv("BMPC_HOST_PHASED", "0")
    monkeypatch.setenv("BMPC_HOST_LEAN", "0")
    N, NB, maxit, egos, steps = 4, 1, 26, 16, 3
    x, z, _, tgt = seeded_batch(egos, 2)
    for e in (3, 7, 11):
        z[e] = x[e]
        z[e, 0] += 0.5 * (e % 3)
    desc = _desc(N, NB, maxit)
    hs = H1.HostSim(desc, egos)
    pol = abi.policy_array(highway_policy_rows(tgt))
    H1.lib().hs_set_policies(hs.h, pol)
    env = abi.make_env()
    scene = np.zeros((egos, abi.ENV_STRIDE))
    scene[:, 0:4], scene[:, 4:8] = x, z
    blob, want, r = [np.array([egos, steps], np.int32).tobytes(), bytes(desc)], [], None
    for t in range(steps):
        xs = hs.env_step(env, t, scene, *(() if r is None else (r["upred"], r["J"], r["status"], r["iters"])))
        r = hs.solve(*xs)
        blob.append(bytes(hs.get_policies()))   # (the scene step re-targets them)
        blob += [np.ascontiguousarray(v, np.float64).tobytes() for v in xs]
        want.append("status " + " ".join(map(str, r["status"])) + " iters " + " ".join(map(str, r["iters"])))
    assert C.sizeof(desc) == len(bytes(desc))
    case = tmp_path / "case.bin"
    case.write_bytes(b"".join(blob))
    monkeypatch.setenv("BMPC_ITER_RECORD_CASE", str(case))
    run = hostbuild.sanitized_program("iter_record_host.cpp", tmp_path, flags=["-I" + H1.EXP, "-I" + os.path.join(H1.HERE, "hostsim")])
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.splitlines() == want, run.stdout + run.stderr
