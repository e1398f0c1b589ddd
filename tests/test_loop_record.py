"""The closed loops' per-step recorder (bmpc_set_loop_record), host side: the ctypes mirror of
bmpc_loop_record against the header, the row writer of csrc/bmpc_record.h as a stand-alone program
under the address and undefined-behaviour sanitizers (tests/hostsim/loop_record_host.cpp), the views
of plan.LoopRecording on synthetic arrays, and the *_population signatures.  The GPU side is
tests/test_loop_record_gpu.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

import hostbuild
from bmpc import abi, plan, scenarios

FIELDS = ("capacity", "t_base", "scene", "xref", "u", "J", "status", "iters", "upred", "xpred", "zpred", "branch_w")


def test_loop_record_layout_matches_header(tmp_path):
    offs = ", ".join(f"offsetof(bmpc_loop_record, {f})" for f in FIELDS)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmpc.h"\n'
            'int main(){printf("' + "%zu " * (1 + len(FIELDS)) + '\\n", sizeof(bmpc_loop_record), ' + offs
            + ');return 0;}\n')
    got = hostbuild.header_program(tmp_path, code)
    D = abi.LoopRecord
    assert [name for name, _ in D._fields_] == list(FIELDS)
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in FIELDS]


def test_row_writer_host_program_under_sanitizers(tmp_path):
    """B = 3, capacity 3 from step 1, steps 0..4 over a fake slab: rows hold steps 1..3, steps 0 and 4
    write nothing, every guard margin keeps its sentinel, NULL optional columns are skipped, and the
    offset of ego 65,535's last row at capacity 4,096 and width 1,480 (beyond 2^32) is exact."""
    r = hostbuild.sanitized_program("loop_record_host.cpp", tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def synthetic(kind, B=2, cap=3, n=4, d=2):
    rng = np.random.default_rng(0)
    cols = dict(scene=rng.normal(size=(B, cap, abi.ENV_STRIDE)), xref=rng.normal(size=(B, cap, n)),
                u=rng.normal(size=(B, cap, d)), J=rng.normal(size=(B, cap)),
                status=np.zeros((B, cap), np.int32), iters=np.ones((B, cap), np.int32))
    return plan.LoopRecording(kind, cap, 5, cols), cols["scene"]


@pytest.mark.parametrize("kind", ["overtake", "merge"])
def test_recording_views_highway_scenes(kind):
    rec, s = synthetic(kind)
    assert rec.struct is None and rec.capacity == 3 and rec.t_base == 5
    np.testing.assert_array_equal(rec.x, s[:, :, abi.ENV_X:abi.ENV_X + 4])
    np.testing.assert_array_equal(rec.z, s[:, :, abi.ENV_Z:abi.ENV_Z + 4])
    np.testing.assert_array_equal(rec.u_obs, s[:, :, abi.ENV_UOBS:abi.ENV_UOBS + 2])
    np.testing.assert_array_equal(rec.obs_policy, s[:, :, abi.ENV_OBSPOL])
    np.testing.assert_array_equal(rec.collided, s[:, :, abi.ENV_COLL])
    np.testing.assert_array_equal(rec.steps, s[:, :, abi.ENV_STEPS])
    assert rec.x.shape == (2, 3, 4) and rec.obs_policy.shape == (2, 3)
    assert np.shares_memory(rec.x, s) and np.shares_memory(rec.steps, s)     # views, not copies
    if kind == "merge":
        np.testing.assert_array_equal(rec.merged, s[:, :, abi.ENV_MERGED])
    else:
        with pytest.raises(AttributeError):
            rec.merged
    with pytest.raises(AttributeError):
        rec.x_des
    assert rec.nbytes == 2 * 3 * ((16 + 4 + 2 + 1) * 8 + 2 * 4)
    snap = rec.host()
    assert snap.kind == kind and all(np.array_equal(snap.col(k), rec.col(k)) for k in rec.cols)


def test_recording_views_quadruped_scene():
    rec, s = synthetic("quadruped", n=3, d=3)
    np.testing.assert_array_equal(rec.x, s[:, :, abi.QENV_X:abi.QENV_X + 3])
    np.testing.assert_array_equal(rec.z, s[:, :, abi.QENV_Z:abi.QENV_Z + 3])
    np.testing.assert_array_equal(rec.u_obs, s[:, :, abi.QENV_UOBS:abi.QENV_UOBS + 3])
    np.testing.assert_array_equal(rec.x_des, s[:, :, abi.QENV_XDES:abi.QENV_XDES + 3])
    np.testing.assert_array_equal(rec.obs_policy, s[:, :, abi.ENV_OBSPOL])
    np.testing.assert_array_equal(rec.steps, s[:, :, abi.ENV_STEPS])
    assert np.shares_memory(rec.x_des, s)
    with pytest.raises(AttributeError):
        rec.merged


def test_recording_rejects_bad_input():
    _, s = synthetic("overtake")
    with pytest.raises(ValueError, match="scene kind"):
        plan.LoopRecording("belief", 3, 0, dict(scene=s))
    with pytest.raises(ValueError, match="core columns missing"):
        plan.LoopRecording("overtake", 3, 0, dict(scene=s))


def test_population_signatures_keep_their_default_return():
    """record defaults to False (the 2-tuple of statistics and scene) in all three entries, and the
    overtake scene has its population entry."""
    for fn in (scenarios.overtake_population, scenarios.merge_population, scenarios.quadruped_population):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["B", "steps", "seed", "device", "record"], fn.__name__
        assert sig.parameters["record"].default is False
        assert sig.parameters["seed"].default == 0 and sig.parameters["device"].default == 0
