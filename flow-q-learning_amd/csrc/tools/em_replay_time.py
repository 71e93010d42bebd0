"""Recorded-action replay timing (developer tool): one Population.envmodel_replay call over
n episodes x T steps against what a user had to do before it, T Population.envmodel_step
calls over the same episodes.

  python em_replay_time.py [--reps 3] [--T 1000] [--per-step] [--root CHECKOUT]

Shapes: cube (28, 5) and antsoccer (42, 8), the default models (128, 256, 128) / (128, 128),
n in {50, 1000}.  Each shape is warmed up first.  Prints one JSON line per shape and
repeat: the wall time of the call (it synchronises, so a host clock is valid), the kernel
time from HIP events (fqlpop_envmodel_replay_time) and the achieved FLOP/s from
2 (K0 h1 + h1 h2 + ... + h_last D + D t1 + ... + t_last) per episode-step.  --per-step times
the T-call path instead; --root imports the package from another checkout (an A/B against
the commit before the replay existed, which has only the per-step path).
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--T", type=int, default=1000)
ap.add_argument("--per-step", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path[:0] = [args.root, os.path.join(args.root, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

import envmodel as em  # noqa: E402
from fqlpop import Population, PopulationConfig  # noqa: E402

SHAPES = {"cube": (28, 5), "antsoccer": (42, 8)}
T = args.T


def flops_per_episode_step(spec):
    sd, td = spec.sp_dims(), spec.tp_dims()
    return 2.0 * (sum(a * b for a, b in zip(sd, sd[1:])) + sum(a * b for a, b in zip(td, td[1:])))


for name, (D, A) in SHAPES.items():
    spec = em.EnvModelSpec(D, A, (128, 256, 128), (128, 128))
    sp = em.init_state_predictor(spec, 0, scale=0.1)
    tp = em.init_termination_predictor(spec, 1)
    pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(64,) * 4, batch_size=64), [1.0], [0])
    pop.set_env_model(em.flatten_state_predictor(spec, sp), em.flatten_termination_predictor(spec, tp),
                      spec.sp_hidden, spec.tp_hidden)
    for n in (50, 1000):
        rng = np.random.default_rng(n)
        init = rng.standard_normal((n, D)).astype(np.float32)
        act = rng.uniform(-1, 1, (n, T, A)).astype(np.float32)
        nxt = rng.standard_normal((n, T, D)).astype(np.float32)
        row = {"label": args.label, "shape": name, "n": n, "T": T}
        if args.per_step:
            def run():
                x = init
                for t in range(T):
                    x, _ = pop.envmodel_step(x, act[:, t])
            x, _ = pop.envmodel_step(init, act[:, 0])  # warm-up
        else:
            def run():
                pop.envmodel_replay(init, act, next_obs=nxt)
            pop.envmodel_replay(init[:, :], act[:, :8], next_obs=nxt[:, :8])  # warm-up
            run()
        for rep in range(args.reps):
            t0 = time.perf_counter()
            run()
            wall = time.perf_counter() - t0
            out = dict(row, path="per_step" if args.per_step else "replay", rep=rep, wall_ms=round(1e3 * wall, 3))
            if not args.per_step:
                k_us = pop.replay_kernel_us()
                out["kernel_ms"] = round(k_us / 1e3, 3)
                out["kernel_gflops"] = round(flops_per_episode_step(spec) * n * T / (k_us * 1e-6) / 1e9, 1)
                out["blocks"] = (n + 15) // 16
            print(json.dumps(out), flush=True)
    pop.close()
