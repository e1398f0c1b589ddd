"""A/B of the overtake closed loop under the OSQP-class controllers at the headline shape (4,096 seeded
egos, N=20, NB=1), per controller ("branch": BranchMPC, "robust": robustMPC):

  fused     bmpc_loop_device as one k_loop launch (OvertakeQpScene: scene + tree + QP per step, per
            ego), asked for with BMPC_LOOP_FUSED=2 so that robust plans take it too;
  per-step  the same call with BMPC_LOOP_FUSED=0 (k_env + k_tree + k_qp per step).

Every repetition starts a fresh plan from the same seeded population, runs --warmup steps through its
path and times the next --steps with HIP events on the loop's stream.  Every path runs once before
anything is timed; the paths alternate within a repetition.  Prints one JSON line per path: ms per
step (each repetition), the mean iterations, the solves not returning status 1, the kernel and the sum
of uPred[0] (equal between the two paths of a controller, to the bit).

    python tools/overtake_qp_loop_ab.py [--egos 4096] [--steps 10] [--warmup 2] [--reps 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "belief-planning_amd")]

from bmpc import abi, plan  # noqa: E402
from bmpc.scenarios import _overtake_scene, highway_desc, highway_policy_rows, seeded_batch  # noqa: E402


def device_loop(args, controller, fused):
    import torch
    os.environ["BMPC_LOOP_FUSED"] = "2" if fused else "0"
    B = args.egos
    x, z, _, tgt = seeded_batch(B, args.seed)
    pl = plan.BatchPlan(highway_desc(N=args.N, NB=args.NB, controller=controller), B)
    pl.set_policies(highway_policy_rows(tgt))
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    scene = torch.tensor(_overtake_scene(x, z), **f64)
    up = torch.zeros((B, pl.U, 2), **f64)
    J = torch.zeros(B, **f64)
    st, it = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.zeros((B, abi.ENV_NSTAT), **f64)
    tx, tz, tr = (torch.zeros((B, 4), **f64) for _ in range(3))
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    env = abi.make_env()

    def go(t0, n):
        pl.loop_device(env, t0, n, scene.data_ptr(), up.data_ptr(), tx.data_ptr(), tz.data_ptr(), tr.data_ptr(),
                       J.data_ptr(), st.data_ptr(), it.data_ptr(), stats.data_ptr(), stream.cuda_stream)

    go(0, args.warmup)
    stream.synchronize()
    before = stats.cpu().numpy().copy()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    go(args.warmup, args.steps)
    e1.record(stream)
    stream.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    d = stats.cpu().numpy() - before    # a step books the solve before it: `steps` solves, the last warm-up's first
    out = dict(ms=ms, iters=float(d[:, abi.ENVS_ITERS].sum() / d[:, abi.ENVS_SOLVES].sum()),
               unsolved=int(d[:, abi.ENVS_INFEAS].sum()), kernel=pl.last_kernel(), check=float(up[:, 0].sum().item()))
    pl.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=4096)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--NB", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    paths = {(c, name): (lambda c=c, f=f: device_loop(args, c, f))
             for c in ("branch", "robust") for name, f in (("fused", True), ("per-step", False))}
    for f in paths.values():   # every path once: module load, LDS opt-in, allocator
        f()
    res = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, f in paths.items():
            res[k].append(f())
    for (c, name), rs in res.items():
        print(json.dumps(dict(controller=c, path=name, egos=args.egos, N=args.N, NB=args.NB, steps=args.steps,
                              warmup=args.warmup, ms_per_step=[round(r["ms"], 4) for r in rs],
                              mean_iters=round(rs[-1]["iters"], 3), unsolved=rs[-1]["unsolved"],
                              kernel=rs[-1]["kernel"], upred0_sum=rs[-1]["check"])))


if __name__ == "__main__":
    main()
