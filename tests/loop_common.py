"""The GPU tests' harness of the device closed loops: the three scenes' small cases, a plan with its
loop's device buffers (Loop), the launch-path switch, and the two ways every closed-loop feature test
runs a case -- `manual`, the scene's *_env_step_device then solve_device with a host copy after every
step, and `recorded`, the loop entry in chunks with a recorder attached -- each with a `setup(loop)`
callback that attaches the feature under test after the plan is made and before the first step."""
import numpy as np
import pytest

from bmpc import abi
from bmpc.scenarios import (_overtake_scene, highway_desc, highway_policy_rows, merge_desc, merge_lane_ref,
                            merge_policy_rows, quad_scene, quadruped_policy_rows, seeded_batch, seeded_merge_batch)
from common import golden

COLUMNS = ("scene", "xref", "u", "J", "status", "iters", "upred", "xpred", "zpred", "branch_w")
FINALS = ("scene", "up", "J", "st", "it", "stats", "x", "z", "xref")
BLK = (abi.KERNEL_IPM_BLK4, abi.KERNEL_IPM_BLK8)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from bmpc import plan
    plan.context(0)
    return plan


def set_path(monkeypatch, block_egos=None, rich=None, fused=None):
    """The launch path of the plans made next (read from the environment on every launch)."""
    for k, v in (("BMPC_BLOCK_EGOS", block_egos), ("BMPC_LDS_RICH", rich), ("BMPC_LOOP_FUSED", fused),
                 ("BMPC_BLOCK_WAVES", None)):
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, str(v))


# ---- the scenes ----------------------------------------------------------------------------------

def overtake_case(N, NB, B, robust=False):
    x, z, _, tgt = (a[:B] for a in seeded_batch(300, seed=5))
    desc = highway_desc(N=N, NB=NB)
    if robust:
        desc.controller = abi.CTRL_ROBUST
    return dict(kind="overtake", desc=desc, scene=_overtake_scene(x, z), policies=highway_policy_rows(tgt),
                env=abi.make_env())


def merge_case(B):
    return dict(kind="merge", desc=merge_desc(N=12), scene=_overtake_scene(*seeded_merge_batch(B)),
                policies=merge_policy_rows(B), env=None)


def quad_case(B):
    from test_quad_loop import NAME, fixture_desc, loop_batch, scene_env
    g = golden(NAME)
    x, z, x_des = (a[:B] for a in loop_batch(300))
    return dict(kind="quadruped", desc=fixture_desc(g, 6), scene=quad_scene(x, z, x_des),
                policies=quadruped_policy_rows(B, float(g["v0"])), env=scene_env(g))


class Loop:
    """A plan of one of the scenes with the device buffers of its closed loop."""

    def __init__(self, plan, case):
        import torch
        self.torch, self.kind, self.env = torch, case["kind"], case["env"]
        B = self.B = len(case["scene"])
        self.pl = pl = plan.BatchPlan(case["desc"], B)
        pl.set_policies(case["policies"])
        if self.kind == "merge":
            pl.set_merge_scene(abi.make_merge_env(), *merge_lane_ref())
        n, d = pl.desc.n, pl.desc.d
        dev = torch.device("cuda", 0)
        f64 = dict(dtype=torch.float64, device=dev)
        self.scene = torch.tensor(case["scene"], **f64)
        self.up = torch.zeros((B, pl.U, d), **f64)
        self.J = torch.zeros(B, **f64)
        self.st = torch.zeros(B, dtype=torch.int32, device=dev)
        self.it = torch.zeros(B, dtype=torch.int32, device=dev)
        self.stats = torch.zeros((B, abi.ENV_NSTAT), **f64)
        self.x, self.z, self.xref = (torch.zeros((B, n), **f64) for _ in range(3))
        self.xpred = torch.zeros((B, pl.T, n), **f64)
        self.bw = torch.zeros((B, max(pl.nbranch - 1, 1)), **f64)
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream(dev)
        self.t = 0

    def _ptrs(self, *names):
        return [getattr(self, n).data_ptr() for n in names]

    def env_step(self):
        args = self._ptrs("scene", "up", "x", "z", "xref", "J", "st", "it", "stats")
        s = self.stream.cuda_stream
        if self.kind == "overtake":
            self.pl.env_step_device(self.env, self.t, *args, stream=s)
        elif self.kind == "merge":
            self.pl.merge_env_step_device(self.t, *args, stream=s)
        else:
            self.pl.quad_env_step_device(self.env, self.t, *args, stream=s)
        self.t += 1

    def solve(self):
        self.pl.solve_device(*self._ptrs("x", "z", "xref", "up", "xpred", "bw", "J", "st", "it"), self.stream.cuda_stream)

    def loop(self, n):
        args = self._ptrs("scene", "up", "x", "z", "xref", "J", "st", "it", "stats")
        s = self.stream.cuda_stream
        if self.kind == "overtake":
            self.pl.loop_device(self.env, self.t, n, *args, s)
        elif self.kind == "merge":
            self.pl.merge_loop_device(self.t, n, *args, s)
        else:
            self.pl.quad_loop_device(self.env, self.t, n, *args, s)
        self.t += n

    def host(self, *names):
        self.stream.synchronize()
        return [getattr(self, n).cpu().numpy().copy() for n in names]

    def finals(self):
        out = dict(zip(FINALS, self.host(*FINALS)))
        if self.pl.desc.controller == abi.CTRL_ROBUST:
            out["ws"] = self.pl.get_robust_warm_start()
        else:
            out["ws"] = self.pl.get_warm_start()
        return out


def manual(plan, case, steps, setup=None):
    """`steps` closed-loop steps as their launches with a host copy after each: the columns a record of
    the same loop must hold [B, steps, ...], the kernels taken and the loop's final state."""
    d = Loop(plan, case)
    if setup is not None:
        setup(d)
    robust = d.pl.desc.controller == abi.CTRL_ROBUST
    rows = {k: [] for k in COLUMNS}
    kernels = set()
    for _ in range(steps):
        d.env_step()
        d.solve()
        scene, xref, up, J, st, it, xpred, bw = d.host("scene", "xref", "up", "J", "st", "it", "xpred", "bw")
        kernels.add(d.pl.last_kernel())
        for k, v in zip(COLUMNS, (scene, xref, up[:, 0], J, st, it, up, xpred,
                                  None if robust else d.pl.tree()["zbar"], bw[:, :d.pl.nbranch - 1])):
            rows[k].append(v)
    cols = {k: np.stack(v, axis=1) for k, v in rows.items() if v[0] is not None}
    return cols, kernels, d.finals()


def recorded(plan, case, chunks, predictions=True, attach=True, setup=None):
    """The loop in `chunks` calls with one recorder attached throughout: the record on the host, the
    kernel reported after each call and the loop's final state."""
    d = Loop(plan, case)
    if setup is not None:
        setup(d)
    rec = None
    if attach:
        rec = d.pl.new_loop_record(sum(chunks), 0, predictions=predictions)
        d.pl.set_loop_record(rec)
    kernels = []
    for c in chunks:
        d.loop(c)
        d.stream.synchronize()
        kernels.append(d.pl.last_kernel())
    out = d.finals()
    return (None if rec is None else rec.host()), kernels, out


def assert_record_equals(rec, ref, rows=None):
    names = [k for k in COLUMNS if k in ref]
    assert sorted(rec.cols) == sorted(names)
    for k in names:
        want = ref[k] if rows is None else ref[k][:, rows]
        assert rec.col(k).shape == want.shape and rec.col(k).dtype == want.dtype, k
        assert np.array_equal(rec.col(k), want), (k, np.argwhere(rec.col(k) != want)[:4])


def assert_same_finals(a, b):
    for k in a:
        if k == "ws":
            for kk in a[k]:
                assert np.array_equal(a[k][kk], b[k][kk]), ("warm start", kk)
        else:
            assert np.array_equal(a[k], b[k]), k


# (BMPC_BLOCK_EGOS, BMPC_LDS_RICH, the per-step solver kernels, the loop's kernels)
PATHS = {
    ("overtake", "wave"): (0, 1, (abi.KERNEL_IPM_RICH,), (abi.KERNEL_LOOP_RICH,)),
    ("overtake", "lean"): (0, 0, (abi.KERNEL_IPM_LEAN,), (abi.KERNEL_LOOP_LEAN,)),
    ("overtake", "blk"): (None, None, BLK, BLK),              # small batches keep their launches per step
    ("quadruped", "wave"): (None, 1, (abi.KERNEL_QP_RICH,), (abi.KERNEL_LOOP_RICH,)),
    ("quadruped", "lean"): (None, 0, (abi.KERNEL_QP_LEAN,), (abi.KERNEL_LOOP_LEAN,)),
}


def assert_all_solved(desc, status):
    status = np.asarray(status)
    if desc.controller == abi.CTRL_CVAR:
        assert np.all((status == 0) | (status == 10)), np.unique(status, return_counts=True)
    else:
        assert np.all(status == 1), np.unique(status, return_counts=True)


def model_p(plan, sc, targets, x, z):
    """bmpc_model_eval's branch probabilities at (x, z) [B, n] under the scene's policies (overtake: the
    lane-change targets [B, 4] in force)."""
    if sc.kind == "overtake":
        rows = [[r[0], r[1], (abi.POL_LC, tuple(map(float, tg)))] for r, tg in zip(sc.rows, targets)]
    else:
        rows = sc.rows
    return plan.model_eval(sc.desc, rows, x, np.zeros((len(x), sc.desc.d)), z)["p"]
