"""The closed loops' per-step recorder (bmpc_set_loop_record) on the GPU.

The yardstick everywhere is manual stepping on the same launch path: the scene's *_env_step_device,
then solve_device with its xpred / branch_w outputs, a host copy after every step and get_tree for
the tree's obstacle predictions.  The existing tests pin that path to the reference's recordings, and
the recorder copies what that path computes, so a record equals it bit for bit: no tolerance.

Equality must not be equality between failures: every status of the manual path is asserted to be a
success (>= 0 for the CVaR controller, 1 for the OSQP-class ones).  The egos are the first rows of the
batches whose loops the existing tests already hold to that: seeded_batch(300, seed=5)
(tests/test_loop_gpu.py), seeded_merge_batch, test_quad_loop.loop_batch.

Small batches reach the one-wave kernels and the fused k_loop with BMPC_BLOCK_EGOS=0, as conftest's
solver_path fixture does; every case asserts the kernel the plan reports (BMPC_INFO_SOLVER)."""
import numpy as np
import pytest

from bmpc import abi
from bmpc.scenarios import highway_desc
from loop_common import (BLK, Loop, assert_record_equals, assert_same_finals, gpu, manual, merge_case,  # noqa: F401
                         overtake_case, quad_case, recorded, set_path)

pytestmark = pytest.mark.gpu


def assert_solved(case, ref):
    """No equality between failures: every solve of the manual path succeeded."""
    st = ref["status"]
    print(f"{case['kind']} B {st.shape[0]}: statuses {np.unique(st, return_counts=True)}, iterations "
          f"{ref['iters'].min()}-{ref['iters'].max()}")
    if case["desc"].controller == abi.CTRL_CVAR:
        assert np.all(st >= 0), np.argwhere(st < 0)
    else:
        assert np.all(st == 1), np.argwhere(st != 1)
    assert np.all(np.isfinite(ref["J"])) and np.all(np.isfinite(ref["xpred"]))
    assert np.array_equal(ref["scene"][:, :, abi.ENV_STEPS], np.tile(np.arange(1, st.shape[1] + 1.0), (st.shape[0], 1)))


_REF = {}


def reference(plan, key, case, steps):
    """The manual path of a case, computed once per launch path and shared (never modified)."""
    if key not in _REF:
        _REF[key] = manual(plan, case, steps)
        assert_solved(case, _REF[key][0])
    return _REF[key]


# ---- overtake ------------------------------------------------------------------------------------

# (BMPC_BLOCK_EGOS, BMPC_LDS_RICH, the per-step solver kernels, the loop's kernels)
OVERTAKE_PATHS = {
    "blk": (None, None, BLK, BLK),                               # small batches keep their launches per step
    "wave": (0, 1, (abi.KERNEL_IPM_RICH,), (abi.KERNEL_LOOP_RICH,)),
    "lean": (0, 0, (abi.KERNEL_IPM_LEAN,), (abi.KERNEL_LOOP_LEAN,)),
}
# N, NB, B, steps: the headline tree on one partial wave of egos; several branch weights, T = 106 and a
# batch that crosses a wave boundary in any thread-per-ego grid
OVERTAKE_SHAPES = {"n20nb1_b3": (20, 1, 3, 5), "n8nb2_b65": (8, 2, 65, 3)}


@pytest.mark.parametrize("shape", list(OVERTAKE_SHAPES))
@pytest.mark.parametrize("path", list(OVERTAKE_PATHS))
def test_overtake_record_equals_manual_stepping(gpu, monkeypatch, path, shape):
    """One call, a loop split over two calls on one attached recorder, and the per-step path of the same
    call (BMPC_LOOP_FUSED=0) all record what manual stepping on the same kernels copies out."""
    egos, rich, k_step, k_loop = OVERTAKE_PATHS[path]
    N, NB, B, steps = OVERTAKE_SHAPES[shape]
    case = overtake_case(N, NB, B)
    set_path(monkeypatch, egos, rich)
    ref, kr, fin = reference(gpu, ("overtake", path, shape), case, steps)
    assert kr <= set(k_step), kr
    assert ref["branch_w"].shape[2] == (3 if NB == 1 else 12) and ref["zpred"].shape == ref["xpred"].shape
    rec, k1, f1 = recorded(gpu, case, [steps])
    assert set(k1) <= set(k_loop), k1
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    rec, k2, f2 = recorded(gpu, case, [2, steps - 2])
    assert set(k2) <= set(k_loop) and len(k2) == 2, k2
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f2)
    set_path(monkeypatch, egos, rich, fused=0)
    rec, k3, f3 = recorded(gpu, case, [steps])
    assert set(k3) <= set(k_step), k3
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f3)


GUARD = 24   # doubles (int32 entries) kept at the sentinel before and after every column


@pytest.mark.parametrize("fused", [None, 0], ids=["fused", "per_step"])
def test_window_guards_and_detach(gpu, monkeypatch, fused):
    """Capacity 3 from step 1 under a 5-step loop: rows hold steps 1..3, steps 0 and 4 touch nothing,
    and the margins around the columns (interior pointers into larger buffers) keep their sentinel.
    After a detach, further steps leave every buffer as it was."""
    import torch
    case = overtake_case(20, 1, 3)
    set_path(monkeypatch, 0, 1)
    ref, _, _ = reference(gpu, ("overtake", "wave", "n20nb1_b3"), case, 5)
    set_path(monkeypatch, 0, 1, fused)
    d = Loop(gpu, case)
    B, cap, n, dd, T, U, nbw = 3, 3, 4, 2, d.pl.T, d.pl.U, d.pl.nbranch - 1
    widths = dict(scene=abi.ENV_STRIDE, xref=n, u=dd, J=1, status=1, iters=1, upred=U * dd, xpred=T * n, zpred=T * n,
                  branch_w=nbw)
    bufs, struct = {}, abi.LoopRecord(capacity=cap, t_base=1)
    for k, w in widths.items():
        i32 = k in ("status", "iters")
        bufs[k] = torch.full((B * cap * w + 2 * GUARD,), -7777 if i32 else -7777.25,
                             dtype=torch.int32 if i32 else torch.float64, device="cuda")
        setattr(struct, k, bufs[k].data_ptr() + GUARD * (4 if i32 else 8))
    torch.cuda.synchronize()
    d.pl.set_loop_record(struct)
    d.loop(5)
    d.stream.synchronize()
    assert d.pl.last_kernel() == (abi.KERNEL_LOOP_RICH if fused is None else abi.KERNEL_IPM_RICH)
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, w in widths.items():
        sentinel = -7777 if k in ("status", "iters") else -7777.25
        assert np.all(host[k][:GUARD] == sentinel) and np.all(host[k][-GUARD:] == sentinel), k
        got = host[k][GUARD:-GUARD].reshape(ref[k][:, 1:4].shape)
        assert np.array_equal(got, ref[k][:, 1:4]), k
    d.pl.set_loop_record(None)
    d.loop(2)
    d.stream.synchronize()
    for k, v in bufs.items():
        assert np.array_equal(v.cpu().numpy(), host[k]), k


@pytest.mark.parametrize("fused", [None, 0], ids=["fused", "per_step"])
def test_recorder_changes_nothing_else(gpu, monkeypatch, fused):
    """Scene, uPred, J, status, iterations, statistics, solve inputs and warm start after 5 steps: the
    same bits with all columns, with the core columns only and without a recorder."""
    case = overtake_case(20, 1, 3)
    set_path(monkeypatch, 0, 1, fused)
    _, k0, plain = recorded(gpu, case, [2, 3], attach=False)
    assert set(k0) == {abi.KERNEL_LOOP_RICH if fused is None else abi.KERNEL_IPM_RICH}
    assert np.all(plain["st"] >= 0) and np.all(plain["scene"][:, abi.ENV_STEPS] == 5)
    full, _, f_full = recorded(gpu, case, [2, 3])
    core, _, f_core = recorded(gpu, case, [2, 3], predictions=False)
    assert_same_finals(plain, f_full)
    assert_same_finals(plain, f_core)
    assert sorted(core.cols) == sorted(core.CORE)
    for k in core.CORE:
        assert np.array_equal(core.col(k), full.col(k)), k
    # the last row is the loop's final state
    assert np.array_equal(full.col("scene")[:, -1], plain["scene"]) and np.array_equal(full.col("J")[:, -1], plain["J"])
    assert np.array_equal(full.col("upred")[:, -1], plain["up"]) and np.array_equal(full.x[:, -1], plain["x"])


# ---- merge, quadruped, robust --------------------------------------------------------------------

@pytest.mark.parametrize("rich", [1, 0], ids=["rich", "lean"])
def test_merge_record_equals_manual_stepping(gpu, monkeypatch, rich):
    """merge_desc(N=12), the first 3 egos of seeded_merge_batch, 4 steps, fused."""
    case = merge_case(3)
    set_path(monkeypatch, 0, rich)
    ref, kr, fin = reference(gpu, ("merge", rich), case, 4)
    assert kr == {abi.KERNEL_IPM_RICH if rich else abi.KERNEL_IPM_LEAN}, kr
    rec, k1, f1 = recorded(gpu, case, [1, 3])
    assert set(k1) == {abi.KERNEL_LOOP_RICH if rich else abi.KERNEL_LOOP_LEAN}, k1
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    assert np.array_equal(rec.merged, ref["scene"][:, :, abi.ENV_MERGED])


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("rich", [1, 0], ids=["rich", "lean"])
def test_quadruped_record_equals_manual_stepping(gpu, monkeypatch, rich, B):
    """The quadruped fixture's plan at N=6, NB=2 (OSQP-class plans fuse at any batch), the first rows
    of test_quad_loop.loop_batch, 4 steps."""
    case = quad_case(B)
    set_path(monkeypatch, None, rich)
    ref, kr, fin = reference(gpu, ("quadruped", rich, B), case, 4)
    assert kr == {abi.KERNEL_QP_RICH if rich else abi.KERNEL_QP_LEAN}, kr
    rec, k1, f1 = recorded(gpu, case, [4])
    assert k1 == [abi.KERNEL_LOOP_RICH if rich else abi.KERNEL_LOOP_LEAN], k1
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    assert np.array_equal(rec.x_des[:, 0], case["scene"][:, abi.QENV_XDES:abi.QENV_XDES + 3])


def test_robust_record_on_the_per_step_path(gpu, monkeypatch):
    """A robustMPC highway plan through bmpc_loop_device (never fused), B=3, 3 steps; its tree keeps no
    zbar, so a zpred column is refused and new_loop_record leaves it out."""
    case = overtake_case(8, 2, 3, robust=True)
    set_path(monkeypatch)
    ref, kr, fin = reference(gpu, ("robust",), case, 3)
    assert kr <= {abi.KERNEL_QP_RICH, abi.KERNEL_QP_LEAN} and "zpred" not in ref
    rec, k1, f1 = recorded(gpu, case, [3])
    assert set(k1) == kr, k1
    assert "zpred" not in rec.cols and "xpred" in rec.cols
    assert_record_equals(rec, ref)
    assert_same_finals(fin, f1)
    d = Loop(gpu, case)
    bad = d.pl.new_loop_record(2).struct
    bad.zpred = bad.scene
    with pytest.raises(RuntimeError, match=r"\(-22\).*zpred"):
        d.pl.set_loop_record(bad)


def test_record_refusals(gpu):
    pl = gpu.BatchPlan(highway_desc(N=8, NB=1), 2)
    good = pl.new_loop_record(2, predictions=True)
    pl.set_loop_record(good)
    pl.set_loop_record(None)
    for cap in (0, -1):
        s = pl.new_loop_record(2).struct
        s.capacity = cap
        with pytest.raises(RuntimeError, match=r"\(-22\).*capacity"):
            pl.set_loop_record(s)
    for k in ("scene", "xref", "u", "J", "status", "iters"):
        s = pl.new_loop_record(2).struct
        setattr(s, k, None)
        with pytest.raises(RuntimeError, match=r"\(-22\).*null core column"):
            pl.set_loop_record(s)
    with pytest.raises(ValueError, match="capacity"):
        pl.new_loop_record(0)
    with pytest.raises(ValueError, match="not on a device"):
        pl.set_loop_record(good.host())


def test_populations_return_their_record(gpu, monkeypatch):
    from bmpc import scenarios
    set_path(monkeypatch)
    for fn, kind in ((scenarios.overtake_population, "overtake"), (scenarios.merge_population, "merge"),
                     (scenarios.quadruped_population, "quadruped")):
        stats, scene, rec = fn(4, 3, record=True)
        assert rec.kind == kind and rec.struct is None and sorted(rec.cols) == sorted(rec.CORE)
        assert stats.shape == (4, abi.ENV_NSTAT) and rec.col("scene").shape == (4, 3, abi.ENV_STRIDE)
        assert np.array_equal(rec.col("scene")[:, -1], scene), kind
        assert np.array_equal(rec.steps, np.tile([1.0, 2.0, 3.0], (4, 1))), kind
        assert np.all(np.isfinite(rec.col("J"))) and np.all(stats[:, abi.ENVS_SOLVES] == 2)
    out = scenarios.overtake_population(4, 2)
    assert len(out) == 2 and out[1].shape == (4, abi.ENV_STRIDE)
    _, _, rec = scenarios.overtake_population(4, 2, record="predictions")
    assert rec.col("xpred").shape[:2] == (4, 2) and "zpred" in rec.cols
