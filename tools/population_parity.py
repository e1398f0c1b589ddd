"""Bit-for-bit parity of the closed-loop population entries (bmpc.scenarios.*_population) between two
builds of the package, e.g. a commit and its parent.

  dump OUT.npz       calls every *_population entry through the public API and saves every returned array
                     (statistics, final scene, log-weights, scripts, ancestors and resampling info, and
                     every column of the record).  Needs a GPU.  The shapes are the smallest that reach
                     every path: descriptions with N=6 (merge N=12), 4 steps, hold 2, resample_every 2,
                     record="predictions"; B=3 as is (the small-batch launches per step) and B=65 with
                     BMPC_BLOCK_EGOS=0 (the fused k_loop, one ego past a wave); the sharded entries as
                     rows [2, 2 + B) of a population of B + 5; the enumerated entries from one state with
                     2 epochs.  merge_population takes no description: scenarios.merge_desc is bound to
                     N=12 for the run.
  compare A.npz B.npz  on the CPU: equal key sets, shapes, dtypes and np.array_equal for every key; prints
                     the first differing index otherwise and exits 1.

The tool imports only public names, so the same file runs against a worktree of another commit:

    python tools/population_parity.py dump OUT.npz [--package PATH/belief-planning_amd]
"""
import argparse
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS, HOLD, EVERY, EPOCHS = 4, 2, 2, 2
EGO_BASE, EXTRA = 2, 5
# tests/disturbance_common.SIGMAS and tests/obstacle_proposal_common.TILTS
SIGMAS = {"overtake": ((0.3, 0.01), (0.5, 0.02)), "merge": ((0.3, 0.01), (0.5, 0.02)),
          "quadruped": ((0.02, 0.01, 0.05), (0.02, 0.01, 0.05))}
TILTS = {"overtake": (1.0, 4.0, 0.25), "quadruped": (1.0, 5.0)}


def flatten(prefix, value, out):
    """Every array reachable from one returned value, under a key that names its place."""
    if value is None:
        return
    if isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            flatten(f"{prefix}.{i}", v, out)
    elif isinstance(value, np.ndarray):
        out[prefix] = value
    elif hasattr(value, "cols") and hasattr(value, "col"):   # plan.LoopRecording: every column
        for name in sorted(value.cols):
            out[f"{prefix}.{name}"] = np.asarray(value.col(name))
    else:
        out[prefix] = np.asarray(value)


def dump(path, package):
    sys.path[:0] = [os.path.dirname(package), package]
    from bmpc import scenarios as sc
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device")
    sc.merge_desc = functools.partial(sc.merge_desc, N=12)
    hw, qd = sc.highway_desc(N=6), sc.quadruped_desc(N=6)
    rec = "predictions"
    out = {}
    for B, blk in ((3, None), (65, "0")):
        if blk is None:
            os.environ.pop("BMPC_BLOCK_EGOS", None)
        else:
            os.environ["BMPC_BLOCK_EGOS"] = blk
        shard = dict(ego_base=EGO_BASE, population=B + EXTRA)
        so, sq = dict(desc=hw, **shard), dict(desc=qd, **shard)
        (se_o, sz_o), (se_m, sz_m), (se_q, sz_q) = (SIGMAS[k] for k in ("overtake", "merge", "quadruped"))
        calls = {
            "sampled_overtake.rule": lambda: sc.sampled_overtake_population(B, STEPS, record=rec, obstacle=None, **so),
            "sampled_overtake": lambda: sc.sampled_overtake_population(B, STEPS, seed=3, record=rec, obstacle_seed=5,
                                                                       hold=HOLD, **so),
            "merge": lambda: sc.merge_population(B, STEPS, seed=1, record=rec),
            "sampled_quadruped.rule": lambda: sc.sampled_quadruped_population(B, STEPS, record=rec, obstacle=None, **sq),
            "sampled_quadruped": lambda: sc.sampled_quadruped_population(B, STEPS, seed=3, record=rec, obstacle_seed=5,
                                                                         hold=HOLD, **sq),
            "weighted_overtake": lambda: sc.weighted_overtake_population(B, STEPS, seed=3, record=rec, obstacle_seed=5,
                                                                         hold=HOLD, tilt=TILTS["overtake"], **so),
            "weighted_quadruped": lambda: sc.weighted_quadruped_population(B, STEPS, seed=3, record=rec, obstacle_seed=5,
                                                                           hold=HOLD, tilt=TILTS["quadruped"], **sq),
            "resampled_overtake": lambda: sc.resampled_overtake_population(
                B, STEPS, EVERY, ess_fraction=2.0, resample_seed=4, tilt=TILTS["overtake"], seed=3, record=rec,
                obstacle_seed=5, hold=HOLD, **so),
            "resampled_quadruped": lambda: sc.resampled_quadruped_population(
                B, STEPS, EVERY, ess_fraction=2.0, resample_seed=4, tilt=TILTS["quadruped"], seed=3, record=rec,
                obstacle_seed=5, hold=HOLD, **sq),
            "disturbed_overtake": lambda: sc.disturbed_overtake_population(
                B, STEPS, se_o, sz_o, disturbance_seed=7, seed=3, record=rec, obstacle="model", obstacle_seed=5,
                hold=HOLD, **so),
            "disturbed_merge": lambda: sc.disturbed_merge_population(B, STEPS, se_m, sz_m, disturbance_seed=7, seed=1,
                                                                     record=rec, **shard),
            "disturbed_quadruped": lambda: sc.disturbed_quadruped_population(
                B, STEPS, se_q, sz_q, disturbance_seed=7, seed=3, record=rec, obstacle="model", obstacle_seed=5,
                hold=HOLD, **sq),
        }
        if B == 3:      # the entries without a description or a batch argument: once, at their own shapes
            x, z, _, _ = sc.seeded_batch(1)
            qx, qz, _ = sc.seeded_quadruped_batch(1)
            calls.update({
                "overtake": lambda: sc.overtake_population(B, STEPS, seed=2, record=rec),
                "quadruped": lambda: sc.quadruped_population(B, STEPS, seed=2, record=rec),
                "merge.norecord": lambda: sc.merge_population(B, STEPS),
                "enumerated_overtake": lambda: sc.enumerated_overtake_population(x[0], z[0], EPOCHS, HOLD, record=rec,
                                                                                 desc=hw),
                "enumerated_quadruped": lambda: sc.enumerated_quadruped_population(qx[0], qz[0], sc.QUAD_X_DES, EPOCHS,
                                                                                   HOLD, record=rec, desc=qd),
            })
        for name, call in calls.items():
            n0 = len(out)
            flatten(f"B{B}.{name}", call(), out)
            print(f"B{B}.{name}: {len(out) - n0} arrays", flush=True)
    np.savez(path, **out)
    print(f"saved {len(out)} arrays to {path}")


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = 0
    for k in sorted(set(A.files) ^ set(Bz.files)):
        print(f"DIFF {k}: only in {a if k in A.files else b}")
        bad += 1
    for k in sorted(set(A.files) & set(Bz.files)):
        u, v = A[k], Bz[k]
        if u.shape != v.shape or u.dtype != v.dtype:
            print(f"DIFF {k}: {u.dtype}{u.shape} against {v.dtype}{v.shape}")
            bad += 1
        elif not np.array_equal(u, v, equal_nan=u.dtype.kind == "f"):
            same = (u == v) | ((u != u) & (v != v)) if u.dtype.kind == "f" else u == v
            idx = np.unravel_index(int(np.argmin(same)), u.shape) if u.ndim else ()
            print(f"DIFF {k}: first at {tuple(int(i) for i in idx)}: {u[idx]!r} against {v[idx]!r}")
            bad += 1
    print(f"{len(A.files)} against {len(Bz.files)} arrays, {bad} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--package", default=os.path.join(REPO, "belief-planning_amd"),
                   help="the belief-planning_amd directory of the build to run (default: this tree's)")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(args.out, os.path.abspath(args.package))
    else:
        sys.exit(compare(args.a, args.b))


if __name__ == "__main__":
    main()
