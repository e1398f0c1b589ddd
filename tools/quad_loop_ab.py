"""A/B of the quadruped closed loop at BASELINE config 4's shape (BranchMPCProx, N=25, NB=2):

  fused     bmpc_quad_loop_device as one k_loop launch (scene + tree + QP per step, per ego);
  per-step  the same call with BMPC_LOOP_FUSED=0 (k_env_quad + k_tree + k_qp per step);
  host      the loop driven from the host: a NumPy scene over the batch and BatchPlan.solve per step.

Every repetition starts a fresh plan from the same seeded population, runs --warmup steps through
its path and times the next --steps: HIP events on the loop's stream for the two device paths, a
host clock around the synchronous calls for the host-driven one.  The three paths alternate within
a repetition.  Prints one JSON line per path: ms per step (each repetition) and the mean iterations.

    python tools/quad_loop_ab.py [--egos 1024] [--steps 10] [--warmup 2] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "belief-planning_amd")]

from bmpc import abi, plan  # noqa: E402
from bmpc.scenarios import (quad_scene, quadruped_desc, quadruped_policy_rows, seeded_quadruped_batch,  # noqa: E402
                            seeded_quadruped_goals)

DT, V0, N = 0.2, 0.2, 25
CLEAR = (0.5 + 1.0) / 2 + 0.2   # (L1 + L2) / 2 + col_tol


def euler(x, u):
    c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
    return x + DT * np.stack([u[:, 0] * c - u[:, 1] * s, u[:, 1] * c + u[:, 0] * s, u[:, 2]], 1)


def numpy_scene(x, z, uobs, x_des, u0):
    """quadruped_env.Quad_env.step's rules over the batch (csrc/bmpc_env_quad.h, vectorised)."""
    if u0 is not None:
        x, z = euler(x, u0), euler(z, uobs)
    fwd = np.tile([V0, 0.0, 0.0], (len(x), 1))
    xe, zf = x.copy(), z.copy()
    hi = np.full((len(x), 2), np.inf)
    for _ in range(N):
        xe, zf = euler(xe, fwd), euler(zf, fwd)
        hi[:, 0] = np.minimum(hi[:, 0], np.linalg.norm(xe[:, :2] - zf[:, :2], axis=1) - CLEAR)
        hi[:, 1] = np.minimum(hi[:, 1], np.linalg.norm(xe[:, :2] - z[:, :2], axis=1) - CLEAR)
    stop = (hi[:, 0] <= 0.5) & (hi[:, 1] > hi[:, 0])
    uobs = np.where(stop[:, None], 0.0, fwd)
    dx = x_des[:, :2] - x[:, :2]
    nrm = np.linalg.norm(dx, axis=1)
    dx = dx / nrm[:, None] * np.minimum(nrm, 5.0)[:, None]
    psi = np.arctan2(dx[:, 1], dx[:, 0])
    psi = psi - 2 * np.pi * np.ceil((psi - x_des[:, 2] - np.pi) / (2 * np.pi))    # into (des - pi, des + pi]
    psi = np.where(np.linalg.norm(dx, axis=1) > 0.1, psi, x[:, 2])
    return x, z, uobs, np.column_stack([x[:, :2] + dx, psi])


def device_loop(args, fused):
    import torch
    os.environ["BMPC_LOOP_FUSED"] = "1" if fused else "0"
    B = args.egos
    x, z, _ = seeded_quadruped_batch(B, args.seed)
    pl = plan.BatchPlan(quadruped_desc(), B)
    pl.set_policies(quadruped_policy_rows(B))
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    scene = torch.tensor(quad_scene(x, z, seeded_quadruped_goals(B, args.seed)), **f64)
    up = torch.zeros((B, pl.U, 3), **f64)
    J = torch.zeros(B, **f64)
    st, it = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.zeros((B, abi.ENV_NSTAT), **f64)
    tx, tz, tr = (torch.zeros((B, 3), **f64) for _ in range(3))
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    env = abi.make_quad_env()

    def go(t0, n):
        pl.quad_loop_device(env, t0, n, scene.data_ptr(), up.data_ptr(), tx.data_ptr(), tz.data_ptr(), tr.data_ptr(),
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


def host_loop(args):
    B = args.egos
    x, z, _ = seeded_quadruped_batch(B, args.seed)
    x_des = seeded_quadruped_goals(B, args.seed)
    pl = plan.BatchPlan(quadruped_desc(), B)
    pl.set_policies(quadruped_policy_rows(B))
    uobs, u0, iters, r = np.zeros((B, 3)), None, [], None
    t_start = 0.0
    for t in range(args.warmup + args.steps):
        if t == args.warmup:
            t_start = time.perf_counter()
        x, z, uobs, xr = numpy_scene(x, z, uobs, x_des, u0)
        r = pl.solve(x, z, xr)
        u0 = r["upred"][:, 0]
        if t >= args.warmup - 1 and t < args.warmup + args.steps - 1:
            iters.append(r["iters"].mean())
    ms = (time.perf_counter() - t_start) * 1e3 / args.steps
    out = dict(ms=ms, iters=float(np.mean(iters)), unsolved=int((r["status"] != 1).sum()), kernel=pl.last_kernel(),
               check=float(u0.sum()))
    pl.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    paths = {"fused": lambda: device_loop(args, True), "per-step": lambda: device_loop(args, False),
             "host": lambda: host_loop(args)}
    for f in paths.values():   # every path once: module load, LDS opt-in, allocator
        f()
    res = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, f in paths.items():
            res[k].append(f())
    for k, rs in res.items():
        print(json.dumps(dict(path=k, egos=args.egos, steps=args.steps, warmup=args.warmup,
                              ms_per_step=[round(r["ms"], 4) for r in rs], mean_iters=round(rs[-1]["iters"], 3),
                              unsolved=rs[-1]["unsolved"], kernel=rs[-1]["kernel"], upred0_sum=rs[-1]["check"])))


if __name__ == "__main__":
    main()
