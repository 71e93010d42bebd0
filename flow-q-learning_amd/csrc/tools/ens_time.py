"""Ensemble rollout timing (developer tool) at benchmark configuration 5's evaluation shape:
32 antsoccer members (obs 42, act 8, 512 x 4) x 50 envs x 1000 steps, K = 5 env models of
the default shape (128, 256, 128) / (128, 128), a termination predictor that never fires
(every episode runs all its steps) and the device's noise.

  python ens_time.py [--reps 3] [--K 5] [--steps 1000] [--members 32] [--envs 50]

(a) per_model: ONE Population.rollout_ensemble(mode="per_model") launch against what a user
    had to do before it for the same numbers, K x (Population.set_env_model +
    Population.rollout) in the same process.
(b) mixed: ONE rollout_ensemble(mode="mixed") launch (the device draws a model per env and
    step) against ONE single-model Population.rollout.

Every path is warmed up first.  Prints one JSON line per path and repeat: the wall time of
the call(s) (they synchronise, so a host clock is valid) and, for the ensemble launches, the
kernel time from HIP events (fqlpop_rollout_ensemble_time); then one summary line with the
medians, the two ratios and the GPU's clocks and power right after the last timed call.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--K", type=int, default=5)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--members", type=int, default=32)
ap.add_argument("--envs", type=int, default=50)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path[:0] = [args.root, os.path.join(args.root, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
import envmodel as em  # noqa: E402
from fqlpop import Population, PopulationConfig  # noqa: E402

D, A, K, T, N, E = 42, 8, args.K, args.steps, args.members, args.envs
spec = em.EnvModelSpec(D, A, (128, 256, 128), (128, 128))
sps = [em.flatten_state_predictor(spec, em.init_state_predictor(spec, k, scale=0.1)) for k in range(K)]
tps = []
for k in range(K):
    tp = em.init_termination_predictor(spec, 100 + k, bias=-50.0)
    last = tp[f"Dense_{len(spec.tp_dims()) - 2}"]
    last["kernel"] = np.zeros_like(last["kernel"])  # logit = -50 whatever the state: never > 0
    tps.append(em.flatten_termination_predictor(spec, tp))
pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(512,) * 4, batch_size=64),
                 [10.0] * N, list(range(1, N + 1)))
pop.set_env_model_ensemble(sps, tps, spec.sp_hidden, spec.tp_hidden)
obs0 = np.random.default_rng(0).standard_normal((E, D)).astype(np.float32)
tiles = (E + 15) // 16


def loop():
    for k in range(K):
        pop.set_env_model(sps[k], tps[k], spec.sp_hidden, spec.tp_hidden)
        pop.rollout(obs0, T, seed=1)


def per_model():
    return pop.rollout_ensemble(obs0, T, seed=1, mode="per_model")


def single():
    return pop.rollout(obs0, T, seed=1)


def mixed():
    return pop.rollout_ensemble(obs0, T, seed=1, mode="mixed")


PATHS = (("loop", loop, N * tiles, False), ("per_model", per_model, N * K * tiles, True),
         ("single", single, N * tiles, False), ("mixed", mixed, N * tiles, True))
row = {"label": args.label, "members": N, "envs": E, "steps": T, "K": K}
med = {}
for name, fn, blocks, timed in PATHS:
    if name == "single":
        pop.set_env_model(sps[0], tps[0], spec.sp_hidden, spec.tp_hidden)
    res = fn()  # warm-up
    if res is not None:
        assert (res[1] == T).all(), "an episode ended early: the paths would not run the same steps"
    walls, kernels = [], []
    for rep in range(args.reps):
        t0 = time.perf_counter()
        fn()
        walls.append(1e3 * (time.perf_counter() - t0))
        out = dict(row, path=name, rep=rep, blocks_per_launch=blocks, wall_ms=round(walls[-1], 3))
        if timed:
            kernels.append(pop.ensemble_kernel_us() / 1e3)
            out["kernel_ms"] = round(kernels[-1], 3)
        print(json.dumps(out), flush=True)
    med[name] = statistics.median(walls)
    if timed:
        med[name + "_kernel"] = statistics.median(kernels)
print(json.dumps(dict(row, summary=True, **{k + "_ms": round(v, 3) for k, v in med.items()},
                      per_model_over_loop=round(med["per_model"] / med["loop"], 4),
                      mixed_over_single=round(med["mixed"] / med["single"], 4),
                      gpu_clock=bench.gpu_clock_power(0))), flush=True)
pop.close()
