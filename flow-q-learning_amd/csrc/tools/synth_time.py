"""Timings of training on world-model branches (developer tool), at bench config C2: cube
(28, 5), 16 members, B = 256, hidden (512,) x 4; 512 branches of horizon 5 per collect, the
default env-model widths with a termination predictor that never fires (every branch runs
its 5 steps: 2 560 transitions per member and collect).

  python synth_time.py [--reps 10] [--steps 300] [--record-only] [--out profiles/synth/synth_time.json]

One JSON line per measurement, all of them also written to --out:
 (a) "collect_burst": 20 Population.collect calls enqueued back to back, then one sync(), per
     call (a host clock around work that ends in a device synchronise; the launch and
     synchronise latency amortised: the GPU time of the start gather, the rollout, the append
     and the commit).  "collect_sync": one collect followed by sync().  Median, min and max of
     --reps repetitions after a warm-up.
 (b) "rollout_record": wall time of Population.rollout(record=True, return_obs=True) with the
     same observations, branches, horizon and seed -- before collect, the only way to those
     transitions, and it ends on the host.  --record-only measures just this, so that the same
     file run from a checkout of the parent commit gives the parent's figure.
 (c) "step_rate": member-steps/s of --steps population steps plus sync() with the rings filled,
     at real_ratio 1 and at 0.5, alternating, in this process.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--record-only", action="store_true")
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


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def summary(ts, scale=1.0):
    ts = [t / scale for t in ts]
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
            "max_ms": round(1e3 * max(ts), 4), "reps": len(ts)}


data = dataset(ROWS, 0)
pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * L, batch_size=B),
                 np.logspace(np.log10(3), np.log10(1000), N).tolist(), list(range(N)))
pop.set_dataset(data)
spec = em.EnvModelSpec(D, A)
pop.set_env_model(em.flatten_state_predictor(spec, em.init_state_predictor(spec, 0)),
                  em.flatten_termination_predictor(spec, em.init_termination_predictor(spec, 1, scale=0.1, bias=-50.0)),
                  spec.sp_hidden, spec.tp_hidden)
pop.step(5)
pop.sync()
shape = {"members": N, "branches": BRANCHES, "horizon": HORIZON}
start = np.random.default_rng(1).integers(0, ROWS, BRANCHES)
obs0 = data["observations"][start]


def record():
    pop.rollout(obs0, HORIZON, seed=SEED, record=True, return_obs=True)


emit(what="rollout_record", **shape, **summary(timed(record, args.reps, 3)))

if not args.record_only:
    pop.synth_create(4 * BRANCHES * HORIZON)

    def collect_sync():
        pop.collect(BRANCHES, HORIZON, SEED, start_rows=start)
        pop.sync()

    def collect_burst():
        for _ in range(BURST):
            pop.collect(BRANCHES, HORIZON, SEED, start_rows=start)
        pop.sync()

    emit(what="collect_sync", **shape, **summary(timed(collect_sync, args.reps, 3)))
    emit(what="collect_burst", calls_per_sync=BURST, **shape, **summary(timed(collect_burst, args.reps, 2), BURST))
    info = pop.synth_info(0)
    assert info["rows"] == 4 * BRANCHES * HORIZON and info["appended"] % (BRANCHES * HORIZON) == 0, info

    def steps():
        pop.step(args.steps)
        pop.sync()

    rates = {1.0: [], 0.5: []}
    pop.step(50)
    pop.sync()
    for _ in range(3):
        for rho in (1.0, 0.5):
            pop.set_real_ratio(rho)
            t = timed(steps, 1, 0)[0]
            rates[rho].append(N * args.steps / t)
    for rho, r in rates.items():
        emit(what="step_rate", real_ratio=rho, members=N, steps=args.steps, ring_rows=info["rows"],
             member_steps_per_s=[round(x, 1) for x in r], median=round(statistics.median(r), 1))
    assert np.all(np.isfinite(pop.read_info_array()[:, :13]))
pop.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
