"""A/B of the closed loops' recorder (bmpc_set_loop_record) at two shapes:

  overtake   the headline shape: seeded overtake egos, N=20, NB=1 (bmpc_loop_device, fused k_loop);
  quadruped  BASELINE config 4's shape: quadruped egos, N=25, NB=2 (bmpc_quad_loop_device, fused).

Four variants, alternated within every repetition of one process (the order rotates from one
repetition to the next, so with --reps 4 every variant takes every place once):

  parent     the parent commit's library, built beforehand and named by --parent (skipped without it);
  off        this library, no recorder attached;
  core       this library, the core columns (scene, xref, u, J, status, iters);
  full       this library, all columns (uPred, xPred, zPred, branch_w too).

Every repetition starts a fresh plan from the same seeded population, runs --warmup steps and times
the next --steps with HIP events on the loop's stream.  The gate: `off` must lie within
the spread `parent`'s own repetitions show; `core` and `full` are reported.  Prints one JSON line per
shape and variant: ms per step of each repetition, the mean iterations and a checksum of uPred[0]
(the same for every variant: the recorder changes no result).

    python tools/loop_record_ab.py [--parent PATH/libbmpc_parent.so] [--this PATH/libbmpc_TAG.so] [--reps 4]
                                   [--shape overtake|quadruped|both]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "belief-planning_amd")]

from bmpc import _lib, abi, plan  # noqa: E402
from bmpc.scenarios import (highway_desc, highway_policy_rows, quad_scene, quadruped_desc,  # noqa: E402
                            quadruped_policy_rows, seeded_batch, seeded_quadruped_batch, seeded_quadruped_goals)

SHAPES = {"overtake": dict(egos=4096, steps=20), "quadruped": dict(egos=1024, steps=10)}


class Libraries:
    """The libraries of the A/B, each with its own contexts: use() makes one the package's."""

    def __init__(self, parent, this=None):
        if this:   # another in-tree build of this source (e.g. tools/build_variant.py's)
            self.libs = {"this": _lib.load(this, strict=False)}
        else:
            self.libs = {"this": _lib.load(_lib.SO_PATH)}
            _lib.check_stamp(_lib.SO_PATH)
        if parent:
            self.libs["parent"] = _lib.load(parent, strict=False)
        self.ctx = {k: {} for k in self.libs}

    def use(self, name):
        _lib._LIB = self.libs[name]
        plan._CTX = self.ctx[name]


def run(shape, egos, steps, warmup, seed, record, obstacle=None, proposal=None):
    """One repetition: a fresh plan, `warmup` steps, then `steps` timed ones.  record: None, "core", "full";
    obstacle: None or the keyword arguments of BatchPlan.set_obstacle_sampling (tools/obstacle_sampling_ab.py);
    proposal: None or those of BatchPlan.set_obstacle_proposal, attached first (tools/obstacle_proposal_ab.py)."""
    import torch
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    if shape == "overtake":
        x, z, _, tgt = seeded_batch(egos, seed)
        pl = plan.BatchPlan(highway_desc(), egos)
        pl.set_policies(highway_policy_rows(tgt))
        scene = torch.zeros((egos, abi.ENV_STRIDE), **f64)
        scene[:, abi.ENV_X:abi.ENV_X + 4] = torch.tensor(x, **f64)
        scene[:, abi.ENV_Z:abi.ENV_Z + 4] = torch.tensor(z, **f64)
        env = abi.make_env()
        loop = pl.loop_device
    else:
        x, z, _ = seeded_quadruped_batch(egos, seed)
        pl = plan.BatchPlan(quadruped_desc(), egos)
        pl.set_policies(quadruped_policy_rows(egos))
        scene = torch.tensor(quad_scene(x, z, seeded_quadruped_goals(egos, seed)), **f64)
        env = abi.make_quad_env()
        loop = pl.quad_loop_device
    n, d = pl.desc.n, pl.desc.d
    up = torch.zeros((egos, pl.U, d), **f64)
    J = torch.zeros(egos, **f64)
    st, it = (torch.zeros(egos, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.zeros((egos, abi.ENV_NSTAT), **f64)
    tx, tz, tr = (torch.zeros((egos, n), **f64) for _ in range(3))
    if proposal:
        pl.set_obstacle_proposal(**proposal)
    if obstacle:
        pl.set_obstacle_sampling(**obstacle)
    rec = None
    if record:
        rec = pl.new_loop_record(warmup + steps, 0, predictions=(record == "full"))
        pl.set_loop_record(rec)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)

    def go(t0, k):
        loop(env, t0, k, scene.data_ptr(), up.data_ptr(), tx.data_ptr(), tz.data_ptr(), tr.data_ptr(), J.data_ptr(),
             st.data_ptr(), it.data_ptr(), stats.data_ptr(), stream.cuda_stream)

    go(0, warmup)
    stream.synchronize()
    before = stats.cpu().numpy().copy()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    go(warmup, steps)
    e1.record(stream)
    stream.synchronize()
    dlt = stats.cpu().numpy() - before   # a step books the solve before it
    out = dict(ms=e0.elapsed_time(e1) / steps, iters=float(dlt[:, abi.ENVS_ITERS].sum() / dlt[:, abi.ENVS_SOLVES].sum()),
               J=float(dlt[:, abi.ENVS_J].sum() / dlt[:, abi.ENVS_SOLVES].sum()), kernel=pl.last_kernel(),
               check=float(up[:, 0].sum().item()), record_mb=0.0 if rec is None else rec.nbytes / 2**20)
    if rec is not None:   # the record's last row is the loop's last step
        assert bool((rec.cols["scene"][:, -1] == scene).all()), "the record's last row is not the final scene"
    pl.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's libbmpc.so (variant `parent`)")
    ap.add_argument("--this", default=None, help="the library under test instead of the product libbmpc.so")
    ap.add_argument("--shape", default="both", choices=["overtake", "quadruped", "both"])
    ap.add_argument("--egos", type=int, default=0, help="override the shape's batch")
    ap.add_argument("--steps", type=int, default=0, help="override the shape's timed steps")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    os.environ.pop("BMPC_LOOP_FUSED", None)
    import torch
    if not torch.cuda.is_available():   # (torch's runtime first, as in the tests)
        raise SystemExit("no HIP device")
    libs = Libraries(args.parent, args.this)
    variants = [("parent", "parent", None)] if args.parent else []
    variants += [("off", "this", None), ("core", "this", "core"), ("full", "this", "full")]
    for shape in (SHAPES if args.shape == "both" else [args.shape]):
        egos = args.egos or SHAPES[shape]["egos"]
        steps = args.steps or SHAPES[shape]["steps"]

        def one(lib, record):
            libs.use(lib)
            return run(shape, egos, steps, args.warmup, args.seed, record)

        for _, lib, record in variants:   # every variant once: module load, LDS opt-in, allocator
            one(lib, record)
        res = {name: [] for name, _, _ in variants}
        # the order rotates: at the quadruped shape a run's place in a fixed sequence moved its time
        # by 2 ms, the parent's own runs included
        for i in range(max(args.reps, 3)):
            k = i % len(variants)
            for name, lib, record in variants[k:] + variants[:k]:
                res[name].append(one(lib, record))
        if not args.parent:
            print(json.dumps(dict(shape=shape, variant="parent", ms_per_step="not measured (no --parent library)")))
        for name, rs in res.items():
            print(json.dumps(dict(shape=shape, variant=name, egos=egos, steps=steps, warmup=args.warmup,
                                  ms_per_step=[round(r["ms"], 4) for r in rs], mean_iters=round(rs[-1]["iters"], 4),
                                  mean_J=rs[-1]["J"], kernel=rs[-1]["kernel"], upred0_sum=rs[-1]["check"],
                                  record_mb=round(rs[-1]["record_mb"], 1))), flush=True)
        if args.parent:
            a, b = [r["ms"] for r in res["parent"]], [r["ms"] for r in res["off"]]
            mean_b = sum(b) / len(b)
            print(json.dumps(dict(shape=shape, gate="off within parent's spread", parent_min=round(min(a), 4),
                                  parent_max=round(max(a), 4), off_mean=round(mean_b, 4),
                                  passed=bool(mean_b <= max(a)))), flush=True)   # (faster than parent passes too)


if __name__ == "__main__":
    main()
