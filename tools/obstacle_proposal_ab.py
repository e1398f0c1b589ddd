"""A/B of the weighted obstacle modes (bmpc_set_obstacle_proposal) at the two shapes of
tools/loop_record_ab.py (overtake: 4,096 egos, N=20, NB=1; quadruped: 1,024 egos, N=25, NB=2; fused).

Five variants by that tool's method -- a fresh plan per repetition, warm-up steps, HIP events on the
loop's stream, the variants alternated and their order rotated from one repetition to the next:

  parent     the parent commit's library, built beforehand and named by --parent;
  off        this library, nothing attached;
  model      this library, mode "model", hold 1 (no proposal attached);
  tilted     this library, mode "tilted", hold 1, the tilt (1, 4, 0.25) / (1, 5);
  script     this library, mode "script", hold 1, a seeded random script.

The gate: `off` and `model` must lie within the spread `parent`'s own repetitions show and
compute the parent's results (mean iterations, mean J and the uPred[0] checksum are printed; `parent`
runs twice, with and without its sampler); `tilted` and `script` are other episodes and are reported.

    python tools/obstacle_proposal_ab.py --parent PATH/libbmpc_parent.so [--reps 4] [--shape overtake|quadruped|both]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loop_record_ab import SHAPES, Libraries, run  # noqa: E402

TILTS = {"overtake": (1.0, 4.0, 0.25), "quadruped": (1.0, 5.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's libbmpc.so (variants `parent`, `parent_model`)")
    ap.add_argument("--this", default=None, help="the library under test instead of the product libbmpc.so")
    ap.add_argument("--shape", default="both", choices=["overtake", "quadruped", "both"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    os.environ.pop("BMPC_LOOP_FUSED", None)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device")
    libs = Libraries(args.parent, args.this)
    for shape in (SHAPES if args.shape == "both" else [args.shape]):
        egos, steps = SHAPES[shape]["egos"], SHAPES[shape]["steps"]
        m = len(TILTS[shape])
        script = np.random.default_rng(args.seed).integers(0, m, (egos, args.warmup + steps))
        model = dict(mode="model", seed=args.seed, hold=1)
        # (name, library, sampler, proposal)
        variants = [("parent", "parent", None, None), ("parent_model", "parent", model, None)] if args.parent else []
        variants += [("off", "this", None, None), ("model", "this", model, None),
                     ("tilted", "this", dict(mode="tilted", seed=args.seed, hold=1), dict(tilt=TILTS[shape])),
                     ("script", "this", dict(mode="script", hold=1), dict(script=script))]

        def one(lib, obstacle, proposal):
            libs.use(lib)
            return run(shape, egos, steps, args.warmup, args.seed, None, obstacle, proposal)

        for _, lib, obstacle, proposal in variants:   # every variant once: module load, LDS opt-in, allocator
            one(lib, obstacle, proposal)
        res = {v[0]: [] for v in variants}
        for i in range(max(args.reps, 3)):
            k = i % len(variants)
            for name, lib, obstacle, proposal in variants[k:] + variants[:k]:
                res[name].append(one(lib, obstacle, proposal))
        for name, rs in res.items():
            print(json.dumps(dict(shape=shape, variant=name, egos=egos, steps=steps, warmup=args.warmup,
                                  ms_per_step=[round(r["ms"], 4) for r in rs], mean_iters=round(rs[-1]["iters"], 4),
                                  mean_J=rs[-1]["J"], kernel=rs[-1]["kernel"], upred0_sum=rs[-1]["check"])), flush=True)
        if args.parent:
            for ref, name in (("parent", "off"), ("parent_model", "model")):
                a, b = [r["ms"] for r in res[ref]], [r["ms"] for r in res[name]]
                mean_b = sum(b) / len(b)
                same = all(res[ref][-1][k] == res[name][-1][k] for k in ("iters", "J", "check"))
                print(json.dumps(dict(shape=shape, gate=f"{name} within {ref}'s spread, its results",
                                      parent_min=round(min(a), 4), parent_max=round(max(a), 4),
                                      mean=round(mean_b, 4), same_results=same,
                                      passed=bool(mean_b <= max(a) and same))), flush=True)


if __name__ == "__main__":
    main()
