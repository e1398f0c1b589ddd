"""Measurements of the actuation disturbance (bmpc_set_disturbance).

--mode ab: the A/B of tools/loop_record_ab.py's method -- a fresh plan per repetition, warm-up steps,
HIP events on the loop's stream, the variants alternated and their order rotated -- at three shapes:

  overtake   4,096 egos, N=20, NB=1, 20 steps (bmpc_loop_device, fused k_loop);
  quadruped  1,024 egos, N=25, NB=2, 10 steps (bmpc_quad_loop_device, fused);
  merge      4,096 egos, N=40, NB=1, 10 steps (bmpc_merge_loop_device, fused).

Variants: `parent` (the parent commit's library, built beforehand and named by --parent), `off` (this
library, nothing attached) and `on` (this library, the suggested sigmas).  The gate: `off`'s mean ms
per step lies within the parent's own min-max and its mean J, mean iterations and uPred[0] checksum
equal the parent's to the bit; `on` is another episode and is reported.

--mode sweep: the collided and infeasible fractions of a 4,096-ego merge and overtake population
against the disturbance's scale (multiples of the suggested sigmas), through
scenarios.disturbed_*_population.

    python tools/disturbance_measure.py --mode ab --parent PATH/libbmpc_parent.so [--reps 4] [--shape ...]
    python tools/disturbance_measure.py --mode sweep [--egos 4096] [--steps 40]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loop_record_ab import Libraries  # noqa: E402  (puts the package on sys.path)

from bmpc import abi, plan, scenarios  # noqa: E402

SHAPES = {"overtake": dict(egos=4096, steps=20), "quadruped": dict(egos=1024, steps=10),
          "merge": dict(egos=4096, steps=10)}
SIGMAS = {"overtake": ((0.3, 0.01), (0.5, 0.02)), "merge": ((0.3, 0.01), (0.5, 0.02)),
          "quadruped": ((0.02, 0.01, 0.05), (0.02, 0.01, 0.05))}


def run(shape, egos, steps, warmup, seed, sigmas=None, attach=None):
    """One repetition: a fresh plan of the shape's seeded population, `warmup` steps, then `steps` timed
    ones.  sigmas: None or (sigma_ego, sigma_obs) attached with seed `seed`; attach: None or a function
    of the plan that attaches another scene option (tools/observation_measure.py)."""
    import torch
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    if shape == "quadruped":
        x, z, _ = scenarios.seeded_quadruped_batch(egos, seed)
        pl = plan.BatchPlan(scenarios.quadruped_desc(), egos)
        pl.set_policies(scenarios.quadruped_policy_rows(egos))
        scene0 = scenarios.quad_scene(x, z, scenarios.seeded_quadruped_goals(egos, seed))
        env = abi.make_quad_env()
        loop = lambda *a: pl.quad_loop_device(env, *a)   # noqa: E731
    else:
        if shape == "overtake":
            x, z, _, tgt = scenarios.seeded_batch(egos, seed)
            pl = plan.BatchPlan(scenarios.highway_desc(), egos)
            pl.set_policies(scenarios.highway_policy_rows(tgt))
            env = abi.make_env()
            loop = lambda *a: pl.loop_device(env, *a)   # noqa: E731
        else:
            x, z = scenarios.seeded_merge_batch(egos, seed)
            pl = plan.BatchPlan(scenarios.merge_desc(), egos)
            pl.set_policies(scenarios.merge_policy_rows(egos))
            pl.set_merge_scene(abi.make_merge_env(), *scenarios.merge_lane_ref())
            loop = pl.merge_loop_device
        scene0 = scenarios._overtake_scene(x, z)
    if sigmas is not None:
        pl.set_disturbance(*sigmas, seed=seed)
    if attach is not None:
        attach(pl)
    n, d = pl.desc.n, pl.desc.d
    scene = torch.tensor(scene0, **f64)
    up = torch.zeros((egos, pl.U, d), **f64)
    J = torch.zeros(egos, **f64)
    st, it = (torch.zeros(egos, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.zeros((egos, abi.ENV_NSTAT), **f64)
    tx, tz, tr = (torch.zeros((egos, n), **f64) for _ in range(3))
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)

    def go(t0, k):
        loop(t0, k, scene.data_ptr(), up.data_ptr(), tx.data_ptr(), tz.data_ptr(), tr.data_ptr(), J.data_ptr(),
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
    solves = dlt[:, abi.ENVS_SOLVES].sum()
    out = dict(ms=e0.elapsed_time(e1) / steps, iters=float(dlt[:, abi.ENVS_ITERS].sum() / solves),
               J=float(dlt[:, abi.ENVS_J].sum() / solves), infeasible=float(dlt[:, abi.ENVS_INFEAS].sum() / solves),
               kernel=pl.last_kernel(), check=float(up[:, 0].sum().item()))
    pl.close()
    return out


def ab(args):
    os.environ.pop("BMPC_LOOP_FUSED", None)
    libs = Libraries(args.parent, args.this)
    for shape in (SHAPES if args.shape == "all" else [args.shape]):
        egos, steps = args.egos or SHAPES[shape]["egos"], args.steps or SHAPES[shape]["steps"]
        variants = [("parent", "parent", None)] if args.parent else []
        variants += [("off", "this", None), ("on", "this", SIGMAS[shape])]

        def one(lib, sigmas):
            libs.use(lib)
            return run(shape, egos, steps, args.warmup, args.seed, sigmas)

        for _, lib, sigmas in variants:   # every variant once: module load, LDS opt-in, allocator
            one(lib, sigmas)
        res = {v[0]: [] for v in variants}
        for i in range(max(args.reps, 3)):
            k = i % len(variants)
            for name, lib, sigmas in variants[k:] + variants[:k]:
                res[name].append(one(lib, sigmas))
        for name, rs in res.items():
            print(json.dumps(dict(shape=shape, variant=name, egos=egos, steps=steps, warmup=args.warmup,
                                  ms_per_step=[round(r["ms"], 4) for r in rs], mean_iters=rs[-1]["iters"],
                                  mean_J=rs[-1]["J"], infeasible=rs[-1]["infeasible"], kernel=rs[-1]["kernel"],
                                  upred0_sum=rs[-1]["check"])), flush=True)
        if args.parent:
            a, b = [r["ms"] for r in res["parent"]], [r["ms"] for r in res["off"]]
            mean_b = sum(b) / len(b)
            same = all(res["parent"][-1][k] == res["off"][-1][k] for k in ("iters", "J", "check"))
            print(json.dumps(dict(shape=shape, gate="off within parent's min-max, its results", parent_min=round(min(a), 4),
                                  parent_max=round(max(a), 4), off_mean=round(mean_b, 4), same_results=same,
                                  passed=bool(min(a) <= mean_b <= max(a) and same),
                                  not_slower=bool(mean_b <= max(a)))), flush=True)


def sweep(args):
    egos, steps = args.egos or 4096, args.steps or 40
    for shape, fn in (("merge", scenarios.disturbed_merge_population), ("overtake", scenarios.disturbed_overtake_population)):
        for scale in (0.0, 0.5, 1.0, 2.0, 4.0):
            se, so = (tuple(scale * v for v in s) for s in SIGMAS[shape])
            stats, scene = fn(egos, steps, se, so, disturbance_seed=args.seed, seed=args.seed)
            solves = stats[:, abi.ENVS_SOLVES].sum()
            print(json.dumps(dict(shape=shape, egos=egos, steps=steps, scale=scale, sigma_ego=se, sigma_obs=so,
                                  collided=float(stats[:, abi.ENVS_COLLIDED].mean()),
                                  infeasible=float(stats[:, abi.ENVS_INFEAS].sum() / solves),
                                  egos_with_an_infeasible_solve=float((stats[:, abi.ENVS_INFEAS] > 0).mean()),
                                  mean_J=float(stats[:, abi.ENVS_J].sum() / solves),
                                  mean_iters=float(stats[:, abi.ENVS_ITERS].sum() / solves))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="ab", choices=["ab", "sweep"])
    ap.add_argument("--parent", default=None, help="the parent commit's libbmpc.so (variant `parent`)")
    ap.add_argument("--this", default=None, help="the library under test instead of the product libbmpc.so")
    ap.add_argument("--shape", default="all", choices=["overtake", "quadruped", "merge", "all"])
    ap.add_argument("--egos", type=int, default=0)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device")
    (ab if args.mode == "ab" else sweep)(args)


if __name__ == "__main__":
    main()
