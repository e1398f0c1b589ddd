"""Measurements of the observation noise (bmpc_set_observation).

--mode ab: tools/disturbance_measure.py's A/B (its shapes, its repetition: a fresh plan, warm-up steps,
HIP events on the loop's stream, the variants alternated and their order rotated) with the variants
`parent` (the parent commit's library, built beforehand and named by --parent), `off` (this library,
nothing attached) and `on` (this library, the suggested sigmas of the observed states).  The
condition: `off`'s mean J, mean iterations and uPred[0] checksum equal the parent's to the bit; its
mean ms per step is reported against the parent's own min-max; `on` is another episode and is
reported.

--mode sweep: the collided and infeasible fractions of a 4,096-ego merge and overtake population
against the noise's scale (multiples of the suggested sigmas), through
scenarios.observed_*_population.

    python tools/observation_measure.py --mode ab --parent PATH/libbmpc_parent.so [--reps 4] [--shape ...]
    python tools/observation_measure.py --mode sweep [--egos 4096] [--steps 40]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from disturbance_measure import SHAPES, run  # noqa: E402  (puts the package on sys.path)
from loop_record_ab import Libraries  # noqa: E402

from bmpc import abi, scenarios  # noqa: E402

# (sigma_x, sigma_z): of (X, Y, v, psi) on the highway and the merge, of (x, y, psi) for the quadrupeds
SIGMAS = {"overtake": ((0.05, 0.02, 0.05, 0.002), (0.2, 0.1, 0.2, 0.01)),
          "merge": ((0.05, 0.02, 0.05, 0.002), (0.2, 0.1, 0.2, 0.01)),
          "quadruped": ((0.005, 0.005, 0.005), (0.02, 0.02, 0.02))}


def ab(args):
    os.environ.pop("BMPC_LOOP_FUSED", None)
    libs = Libraries(args.parent, args.this)
    for shape in (SHAPES if args.shape == "all" else [args.shape]):
        egos, steps = args.egos or SHAPES[shape]["egos"], args.steps or SHAPES[shape]["steps"]
        variants = [("parent", "parent", None)] if args.parent else []
        variants += [("off", "this", None),
                     ("on", "this", lambda pl, s=SIGMAS[shape]: pl.set_observation(*s, seed=args.seed))]

        def one(lib, attach):
            libs.use(lib)
            return run(shape, egos, steps, args.warmup, args.seed, attach=attach)

        for _, lib, attach in variants:   # every variant once: module load, LDS opt-in, allocator
            one(lib, attach)
        res = {v[0]: [] for v in variants}
        for i in range(max(args.reps, 3)):
            k = i % len(variants)
            for name, lib, attach in variants[k:] + variants[:k]:
                res[name].append(one(lib, attach))
        for name, rs in res.items():
            print(json.dumps(dict(shape=shape, variant=name, egos=egos, steps=steps, warmup=args.warmup,
                                  ms_per_step=[round(r["ms"], 4) for r in rs], mean_iters=rs[-1]["iters"],
                                  mean_J=rs[-1]["J"], infeasible=rs[-1]["infeasible"], kernel=rs[-1]["kernel"],
                                  upred0_sum=rs[-1]["check"])), flush=True)
        if args.parent:
            a, b = [r["ms"] for r in res["parent"]], [r["ms"] for r in res["off"]]
            mean_a, mean_b = sum(a) / len(a), sum(b) / len(b)
            same = all(p[k] == o[k] for p, o in zip(res["parent"], res["off"]) for k in ("iters", "J", "check"))
            print(json.dumps(dict(shape=shape, condition="off reproduces the parent's J, iterations and uPred[0] checksum",
                                  same_results=same, parent_min=round(min(a), 4), parent_max=round(max(a), 4),
                                  parent_mean=round(mean_a, 4), off_mean=round(mean_b, 4),
                                  off_mean_within_parent_spread=bool(min(a) <= mean_b <= max(a)),
                                  off_mean_over_parent_max_percent=round(100 * (mean_b / max(a) - 1), 3))), flush=True)


def sweep(args):
    egos, steps = args.egos or 4096, args.steps or 40
    for shape, fn in (("merge", scenarios.observed_merge_population), ("overtake", scenarios.observed_overtake_population)):
        for scale in (0.0, 0.5, 1.0, 2.0, 4.0):
            sx, sz = (tuple(scale * v for v in s) for s in SIGMAS[shape])
            stats, scene = fn(egos, steps, sx, sz, observation_seed=args.seed, seed=args.seed)
            solves = stats[:, abi.ENVS_SOLVES].sum()
            print(json.dumps(dict(shape=shape, egos=egos, steps=steps, scale=scale, sigma_x=sx, sigma_z=sz,
                                  collided=float(stats[:, abi.ENVS_COLLIDED].mean()),
                                  collided_egos=int(stats[:, abi.ENVS_COLLIDED].sum()),
                                  infeasible=float(stats[:, abi.ENVS_INFEAS].sum() / solves),
                                  infeasible_solves=int(stats[:, abi.ENVS_INFEAS].sum()),
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
