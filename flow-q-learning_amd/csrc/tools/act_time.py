"""Population acting timing (developer tool): one Population.act call for every member against
what a user had to do before it, one Population.sample_actions call per member.

  python act_time.py [--reps 5] [--iters 200] [--members 16] [--envs 50] [--loop-only] [--root CHECKOUT]

Shapes: cube (28, 5) and antsoccer (42, 8), hidden (512,) * 4, 16 members x 50 envs (an online
loop's environment step).  Each path is warmed up (20 calls) first; a repetition is the mean
over --iters back-to-back calls, and --reps repetitions give the run-to-run spread.  Both
calls synchronise, so a host clock is valid.  Prints one JSON line per shape, path and
repetition: the wall time per environment step (one act call, or --members sample_actions
calls) in microseconds and, for act, the kernel time of the last call from HIP events
(fqlpop_act_time).  --loop-only times the per-member loop alone; --root imports the package
from another checkout (an A/B against the commit before act existed, which has only the loop).
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--members", type=int, default=16)
ap.add_argument("--envs", type=int, default=50)
ap.add_argument("--loop-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path[:0] = [args.root, os.path.join(args.root, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

from fqlpop import Population, PopulationConfig  # noqa: E402

SHAPES = {"cube": (28, 5), "antsoccer": (42, 8)}
M, E = args.members, args.envs

for name, (D, A) in SHAPES.items():
    pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(512,) * 4, batch_size=256),
                     np.logspace(0.5, 3, M).tolist(), list(range(1, M + 1)))
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((M, E, D)).astype(np.float32)

    def loop(t):
        for m in range(M):
            pop.sample_actions(m, obs[m], seed=t)

    def act(t):
        pop.act(obs, seed=7, t=t)

    paths = [("loop", loop)] if args.loop_only else [("act", act), ("loop", loop)]
    for path, fn in paths:
        for t in range(1, 21):  # warm-up
            fn(t)
        for rep in range(args.reps):
            t0 = time.perf_counter()
            for t in range(1, args.iters + 1):
                fn(t)
            wall = (time.perf_counter() - t0) / args.iters
            out = {"label": args.label, "shape": name, "members": M, "envs": E, "path": path, "rep": rep,
                   "wall_us": round(1e6 * wall, 1)}
            if path == "act":
                out["kernel_us"] = round(pop.last_act_us(), 1)
                out["blocks"] = M * ((E + 15) // 16)
            print(json.dumps(out), flush=True)
    pop.close()
