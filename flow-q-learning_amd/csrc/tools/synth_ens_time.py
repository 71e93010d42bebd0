"""Timings of branching under the world-model ensemble (developer tool), at bench config C2
as synth_time.py: cube (28, 5), 16 members, hidden (512,) x 4; 512 branches of horizon 5 per
collect, the default env-model widths with a termination predictor that never fires (every
branch runs its 5 steps: 2 560 transitions per member and collect).

  python synth_ens_time.py [--reps 10] [--models 5] [--out profiles/synth_ens/synth_ens_time.json]

One JSON line per measurement, all of them also written to --out.  Each is BURST collects
enqueued back to back, then one sync(), per call (a host clock around work that ends in a
device synchronise; the launch and synchronise latency amortised), median, min and max of
--reps repetitions after a warm-up, the three variants alternating within a repetition:
 (a) "collect_single":   Population.collect under set_env_model's model (the baseline);
 (b) "collect_ensemble": collect(ensemble=True) under --models models (only the models some
     column of a tile chose run in a tile-step);
 (c) "collect_ensemble_penalty": the same with penalty = 1 (every model runs in every tile-step).
Then one summary line: the ratios of the medians to (a), and the mean number of env-model
chains per tile-step of (b), counted from the device's own model draw (traj_model of one
recorded rollout of the same branches).
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--models", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

import envmodel as em  # noqa: E402
from fqlpop import Population, PopulationConfig  # noqa: E402

D, A, H, L, B, N = 28, 5, 512, 4, 256, 16
BRANCHES, HORIZON, ROWS, SEED = 512, 5, 100_000, 7
BURST = 20
K = args.models
results = []


def emit(**row):
    results.append(row)
    print(json.dumps(row), flush=True)


def dataset(n, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    rew = np.where(rng.uniform(size=n) < 0.05, 0.0, -1.0).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32), "rewards": rew,
            "masks": (1.0 - (rew == 0)).astype(np.float32),
            "next_observations": (obs + 0.05 * rng.standard_normal((n, D))).astype(np.float32)}


def summary(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
            "max_ms": round(1e3 * max(ts), 4), "reps": len(ts)}


data = dataset(ROWS, 0)
pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * L, batch_size=B),
                 np.logspace(np.log10(3), np.log10(1000), N).tolist(), list(range(N)))
pop.set_dataset(data)
spec = em.EnvModelSpec(D, A)
sps = [em.flatten_state_predictor(spec, em.init_state_predictor(spec, k)) for k in range(K)]
tp = em.flatten_termination_predictor(spec, em.init_termination_predictor(spec, 1, scale=0.1, bias=-50.0))
pop.set_env_model(sps[0], tp, spec.sp_hidden, spec.tp_hidden)
pop.set_env_model_ensemble(sps, tp, spec.sp_hidden, spec.tp_hidden)
pop.step(5)
pop.sync()
pop.synth_create(4 * BRANCHES * HORIZON)
start = np.random.default_rng(1).integers(0, ROWS, BRANCHES)
shape = {"members": N, "branches": BRANCHES, "horizon": HORIZON, "calls_per_sync": BURST}
variants = {"collect_single": dict(), "collect_ensemble": dict(ensemble=True),
            "collect_ensemble_penalty": dict(ensemble=True, penalty=1.0)}


def burst(kw):
    t0 = time.perf_counter()
    for _ in range(BURST):
        pop.collect(BRANCHES, HORIZON, SEED, start_rows=start, **kw)
    pop.sync()
    return (time.perf_counter() - t0) / BURST


times = {name: [] for name in variants}
for rep in range(args.reps + 2):
    for name, kw in variants.items():
        t = burst(kw)
        if rep >= 2:  # two warm-up rounds (the workspace grows on the first penalised collect)
            times[name].append(t)
for name in variants:
    emit(what=name, models=1 if name == "collect_single" else K, **shape, **summary(times[name]))
info = pop.synth_info(0)
assert info["rows"] == 4 * BRANCHES * HORIZON and info["appended"] % (BRANCHES * HORIZON) == 0, info
assert (pop.synth_read(0)["rewards"] < -1).any()  # the last collect was penalised

# chains per tile-step of the unpenalised ensemble collect: the distinct models among a tile's 16 columns
rec = pop.rollout_ensemble(data["observations"][start], HORIZON, seed=SEED, mode="mixed", record=True)
tm = rec[4][0].reshape(HORIZON, BRANCHES // 16, 16)
chains = float(np.mean([[len(set(tile.tolist())) for tile in step] for step in tm]))
med = {name: statistics.median(times[name]) for name in variants}
emit(what="summary", models=K, chains_per_tile_step_single=1.0, chains_per_tile_step_ensemble=round(chains, 3),
     chains_per_tile_step_penalty=float(K),
     ensemble_over_single=round(med["collect_ensemble"] / med["collect_single"], 3),
     penalty_over_single=round(med["collect_ensemble_penalty"] / med["collect_single"], 3))
pop.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
