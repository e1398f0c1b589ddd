"""A/B of the scenes' obstacle sampler (bmpc_set_obstacle_sampling) at the two shapes of
tools/loop_record_ab.py (overtake: 4,096 egos, N=20, NB=1; quadruped: 1,024 egos, N=25, NB=2; fused).

Three variants by that tool's method -- a fresh plan per repetition, warm-up steps, HIP events on the
loop's stream, the variants alternated and their order rotated from one repetition to the next:

  parent     the parent commit's library, built beforehand and named by --parent;
  off        this library, no sampler attached;
  sampled    this library, mode "model", hold 1: a draw and m rollouts of N steps on every step.

The gate: `off` must lie within the spread `parent`'s own repetitions show, and computes
the parent's results (mean iterations, mean J and the uPred[0] checksum are printed); `sampled` is
reported -- its trajectories are other ones, so its iterations and checksum differ.

    python tools/obstacle_sampling_ab.py --parent PATH/libbmpc_parent.so [--reps 4] [--shape overtake|quadruped|both]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loop_record_ab import SHAPES, Libraries, run  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's libbmpc.so (variant `parent`)")
    ap.add_argument("--this", default=None, help="the library under test instead of the product libbmpc.so")
    ap.add_argument("--shape", default="both", choices=["overtake", "quadruped", "both"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hold", type=int, default=1)
    args = ap.parse_args()
    os.environ.pop("BMPC_LOOP_FUSED", None)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device")
    libs = Libraries(args.parent, args.this)
    variants = [("parent", "parent", None)] if args.parent else []
    variants += [("off", "this", None), ("sampled", "this", dict(mode="model", seed=args.seed, hold=args.hold))]
    for shape in (SHAPES if args.shape == "both" else [args.shape]):
        egos, steps = SHAPES[shape]["egos"], SHAPES[shape]["steps"]

        def one(lib, obstacle):
            libs.use(lib)
            return run(shape, egos, steps, args.warmup, args.seed, None, obstacle)

        for _, lib, obstacle in variants:   # every variant once: module load, LDS opt-in, allocator
            one(lib, obstacle)
        res = {name: [] for name, _, _ in variants}
        for i in range(max(args.reps, 3)):
            k = i % len(variants)
            for name, lib, obstacle in variants[k:] + variants[:k]:
                res[name].append(one(lib, obstacle))
        for name, rs in res.items():
            print(json.dumps(dict(shape=shape, variant=name, egos=egos, steps=steps, warmup=args.warmup,
                                  ms_per_step=[round(r["ms"], 4) for r in rs], mean_iters=round(rs[-1]["iters"], 4),
                                  mean_J=rs[-1]["J"], kernel=rs[-1]["kernel"], upred0_sum=rs[-1]["check"])), flush=True)
        if args.parent:
            a, b = [r["ms"] for r in res["parent"]], [r["ms"] for r in res["off"]]
            mean_b = sum(b) / len(b)
            same = all(res["parent"][-1][k] == res["off"][-1][k] for k in ("iters", "J", "check"))
            print(json.dumps(dict(shape=shape, gate="off within parent's spread, the parent's results",
                                  parent_min=round(min(a), 4), parent_max=round(max(a), 4), off_mean=round(mean_b, 4),
                                  same_results=same, passed=bool(mean_b <= max(a) and same))), flush=True)


if __name__ == "__main__":
    main()
