"""Measurements of the population resampling (bmpc_resample_device) at the two shapes of
tools/loop_record_ab.py (overtake: 4,096 egos, N=20, NB=1; quadruped: 1,024 egos, N=25, NB=2; fused),
tilted obstacle (1, 4, 0.25) / (1, 5), hold 1.

  cost   a fresh plan, --warmup steps, --steps timed steps (ms per closed-loop step), then --reps times
         one more step followed by one bmpc_resample_device call between HIP events on the loop's stream:
         forced (ess_fraction 2: every stage runs) and not forced (ess_fraction 0: the ancestor kernel
         decides, the gather kernels return at once).  Reported beside the step as a share of it.
  ess    the effective sample size of the population after every epoch over --epochs epochs, without
         resampling and with a resampling after every epoch at ess_fraction 0.5 -- the same tilt, seeds
         and initial states --, and the survivors of every resampling.

Prints one JSON line per measurement.

    python tools/resample_measure.py [--shape overtake|quadruped|both] [--reps 5] [--epochs 8]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "belief-planning_amd")]

from bmpc import abi, montecarlo, plan  # noqa: E402
from bmpc.scenarios import (_overtake_scene, highway_desc, highway_policy_rows, quad_scene, quadruped_desc,  # noqa: E402
                            quadruped_policy_rows, seeded_batch, seeded_quadruped_batch, seeded_quadruped_goals)

SHAPES = {"overtake": dict(egos=4096, steps=8), "quadruped": dict(egos=1024, steps=6)}
TILTS = {"overtake": (1.0, 4.0, 0.25), "quadruped": (1.0, 5.0)}


class Population:
    """A tilted population of one of the two shapes with the loop's device buffers."""

    def __init__(self, shape, egos, seed):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        f64 = dict(dtype=torch.float64, device=dev)
        if shape == "overtake":
            x, z, _, tgt = seeded_batch(egos, seed)
            self.pl = pl = plan.BatchPlan(highway_desc(), egos)
            pl.set_policies(highway_policy_rows(tgt))
            scene = _overtake_scene(x, z)
            self.env, self.loop = abi.make_env(), pl.loop_device
        else:
            x, z, _ = seeded_quadruped_batch(egos, seed)
            self.pl = pl = plan.BatchPlan(quadruped_desc(), egos)
            pl.set_policies(quadruped_policy_rows(egos))
            scene = quad_scene(x, z, seeded_quadruped_goals(egos, seed))
            self.env, self.loop = abi.make_quad_env(), pl.quad_loop_device
        pl.set_obstacle_proposal(tilt=TILTS[shape])
        pl.set_obstacle_sampling("tilted", seed=seed, hold=1)
        n, d = pl.desc.n, pl.desc.d
        self.b = dict(scene=torch.tensor(scene, **f64), upred=torch.zeros((egos, pl.U, d), **f64),
                      x=torch.zeros((egos, n), **f64), z=torch.zeros((egos, n), **f64), xref=torch.zeros((egos, n), **f64),
                      J=torch.zeros(egos, **f64), status=torch.zeros(egos, dtype=torch.int32, device=dev),
                      iters=torch.zeros(egos, dtype=torch.int32, device=dev), stats=torch.zeros((egos, abi.ENV_NSTAT), **f64))
        torch.cuda.synchronize(dev)
        self.stream = torch.cuda.Stream(dev)
        self.t = 0

    def go(self, k):
        self.loop(self.env, self.t, k, *(self.b[n].data_ptr() for n in ("scene", "upred", "x", "z", "xref", "J", "status",
                                                                       "iters", "stats")), self.stream.cuda_stream)
        self.t += k

    def timed(self, fn):
        e0, e1 = (self.torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record(self.stream)
        out = fn()
        e1.record(self.stream)
        self.stream.synchronize()
        return e0.elapsed_time(e1), out

    def logw(self):
        self.stream.synchronize()
        return self.b["scene"][:, abi.ENV_LOGW].cpu().numpy()


def cost(shape, egos, steps, warmup, reps, seed):
    p = Population(shape, egos, seed)
    p.go(warmup)
    p.stream.synchronize()
    step_ms = p.timed(lambda: p.go(steps))[0] / steps
    res = {"forced": [], "not_forced": []}
    moved = []
    for r in range(reps):
        for name, frac in (("not_forced", 0.0), ("forced", 2.0)):
            p.go(1)
            p.stream.synchronize()
            ms, (anc, info) = p.timed(lambda: p.pl.resample(p.b, p.t, seed, frac, 0, p.stream.cuda_stream))
            res[name].append(ms)
            assert info.cpu().numpy()[abi.R_RESAMPLED] == (1.0 if frac else 0.0)
            if frac:
                moved.append(int((anc.cpu().numpy() != np.arange(egos)).sum()))
    kernel = p.pl.last_kernel()
    p.pl.close()
    for name, v in res.items():
        v = v[1:] if len(v) > 1 else v   # (the first call allocates the scratch)
        mean = sum(v) / len(v)
        print(json.dumps(dict(measure="cost", shape=shape, egos=egos, variant=name, ms_per_call=[round(x, 4) for x in v],
                              mean_ms=round(mean, 4), step_ms=round(step_ms, 4), share_of_a_step=round(mean / step_ms, 5),
                              egos_moved=moved[1:] if name == "forced" else None, kernel=kernel)), flush=True)


def ess_history(shape, egos, epochs, seed):
    for resampled in (False, True):
        p = Population(shape, egos, seed)
        ess, survivors = [], []
        for t in range(1, epochs + 1):
            p.go(1)
            ess.append(round(montecarlo.estimate(np.ones(egos), p.logw())[2], 2))
            if resampled and t < epochs:
                _, info = p.pl.resample(p.b, t, seed, 0.5, 0, p.stream.cuda_stream)
                p.stream.synchronize()
                info = info.cpu().numpy()
                survivors.append(int(info[abi.R_SURVIVORS]) if info[abi.R_RESAMPLED] else None)
        mean_w = float(np.exp(p.logw()).mean())
        p.pl.close()
        print(json.dumps(dict(measure="ess", shape=shape, egos=egos, tilt=TILTS[shape], resampled=resampled,
                              ess_after_epoch=ess, survivors=survivors if resampled else None, mean_weight=mean_w)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["overtake", "quadruped", "both"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    os.environ.pop("BMPC_LOOP_FUSED", None)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device")
    for shape in (SHAPES if args.shape == "both" else [args.shape]):
        cost(shape, SHAPES[shape]["egos"], SHAPES[shape]["steps"], args.warmup, args.reps, args.seed)
    for shape in (SHAPES if args.shape == "both" else [args.shape]):
        ess_history(shape, SHAPES[shape]["egos"], args.epochs, args.seed)


if __name__ == "__main__":
    main()
