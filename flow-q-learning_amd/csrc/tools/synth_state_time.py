"""Time of a ring checkpoint (developer tool): Population.synth_state of every member, then
Population.load_synth_state of every member into a second population, for 16 cube members
(28, 5) with full rings of the default capacity (100 000 rows of 63 floats: 25.2 MB a member).

  python synth_state_time.py [--reps 5] [--out synth_state_time.json]

One JSON line per measurement, all of them also written to --out:
 "synth_state": the 16 reads (each synchronises and copies five fields to the host);
 "load_synth_state": the 16 writes plus one sync() (each stages its rows in mapped host memory,
   which the placement kernel reads over the bus);
 "append_full": 16 Population.synth_append calls of `capacity` rows plus one sync(), the same
   traffic through the wrapping path.
Median, min and max of --reps repetitions after a warm-up; wall clock around work that ends in
a device synchronise.  The rings are checked to be byte-equal afterwards.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

from fqlpop import Population, PopulationConfig  # noqa: E402

D, A, H, L, B, N, CAP = 28, 5, 512, 4, 256, 16, 100_000
results = []


def emit(**row):
    results.append(row)
    print(json.dumps(row), flush=True)


def rows(n, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
            "rewards": -np.ones(n, np.float32), "masks": np.ones(n, np.float32),
            "next_observations": obs[::-1].copy()}


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * statistics.median(out), 3), "min_ms": round(1e3 * min(out), 3),
            "max_ms": round(1e3 * max(out), 3), "reps": reps}


def population():
    pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * L, batch_size=B),
                     np.logspace(np.log10(3), np.log10(1000), N).tolist(), list(range(N)))
    pop.synth_create(CAP)
    return pop


src, dst = population(), population()
for m in range(N):                       # full rings that have wrapped: head in the middle
    src.synth_append(m, rows(CAP, m))
    src.synth_append(m, rows(CAP // 3, 100 + m))
src.sync()
states = []


def save():
    states[:] = [src.synth_state(m) for m in range(N)]


def load():
    for m in range(N):
        dst.load_synth_state(m, states[m])
    dst.sync()


piece = rows(CAP, 999)


def append_full():
    for m in range(N):
        dst.synth_append(m, piece)
    dst.sync()


shape = {"members": N, "capacity": CAP, "mbytes_per_member": round(CAP * (2 * D + A + 2) * 4 / 1e6, 1)}
emit(what="synth_state", **shape, **timed(save, args.reps, 1))
emit(what="load_synth_state", **shape, **timed(load, args.reps, 1))
for m in range(N):
    got = dst.synth_state(m)
    assert got["appended"] == states[m]["appended"] == CAP + CAP // 3
    assert all(got[k].tobytes() == states[m][k].tobytes() for k in got if k not in ("appended", "capacity")), m
emit(what="append_full", **shape, **timed(append_full, args.reps, 1))
src.close()
dst.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
