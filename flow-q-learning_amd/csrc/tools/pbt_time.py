"""Population-based training timings (developer tool), at bench config C2: cube (28, 5),
16 members, B = 256, hidden (512,) x 4.

  python pbt_time.py [--reps 20] [--steps 4000] [--eval_interval 500] [--skip-tune]

Prints one JSON line per measurement:
 (a) "clone": wall time of Population.clone_members of 1, 4 and 8 pairs followed by sync()
     (a host clock around work that ends in a device synchronise): median, min and max of
     --reps repetitions after a warm-up, the bytes moved (read + write of every arena the
     clone copies, computed from the shapes below) and their rate as a fraction of the
     8 TB/s HBM peak.  "clone_burst": 20 such calls enqueued back to back before one sync,
     per call -- the launch and synchronise latency amortised, i.e. the kernel's own rate.
 (b) "state_dict": the same member copies through state_dict() / load_state_dict(), the only
     path there was before clone_members (three get_state and three set_state calls, each a
     device synchronise and a staged host copy, and a set_count).
 (c) "tune": one tune_alpha.py --task synthetic run each with --strategy successive_halving
     and --strategy pbt, 16 alphas, the same steps, eval_interval and seed, in this process
     after a small warm-up run: member-updates done / wall seconds.
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--eval_interval", type=int, default=500)
ap.add_argument("--skip-tune", action="store_true")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

from fqlpop import Population, PopulationConfig  # noqa: E402

HBM_PEAK = 8.0e12
D, A, H, L, B, E, N = 28, 5, 512, 4, 256, 2, 16


def align_up(x, a=64):
    return (x + a - 1) // a * a


def net_floats(in_dim, out_dim, ln):
    """One ensemble member of runtime.cpp's NetLayout: every leaf rounded up to 64 floats."""
    o = 0
    for layer in range(L + 1):
        k, n = (in_dim if layer == 0 else H), (out_dim if layer == L else H)
        o = align_up(o + k * n)
        o = align_up(o + n)
        if layer < L and ln:
            o = align_up(align_up(o + H) + H)
    return o


def clone_bytes_per_member():
    """Bytes the clone reads (and as many it writes) per pair: both parameter buffers, Adam m
    and v (P floats each), the target critic (PT) and both W^T arenas (PTT)."""
    critic = net_floats(D + A, 1, True) * E
    bc_off = align_up(critic)
    os_off = align_up(bc_off + net_floats(D + A + 1, A, False))
    P = align_up(os_off + net_floats(D + A, A, False))
    PT = align_up(critic)
    PTT = (E + 2) * (L - 1) * H * H
    return 4 * (4 * P + PT + 2 * PTT)


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


def summary(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4),
            "max_ms": round(1e3 * max(ts), 4), "reps": len(ts)}


pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * L, batch_size=B),
                 np.logspace(np.log10(3), np.log10(1000), N).tolist(), list(range(N)))
pop.set_dataset(dataset(100_000, 0))
pop.step(5)
pop.sync()
per_member = clone_bytes_per_member()
BURST = 20
for k in (1, 4, 8):
    src, dst = list(range(k)), list(range(8, 8 + k))

    def clone():
        pop.clone_members(src, dst)
        pop.sync()

    def burst():
        for _ in range(BURST):
            pop.clone_members(src, dst)
        pop.sync()

    def via_state_dict():
        for s, d in zip(src, dst):
            pop.load_state_dict(d, pop.state_dict(s))
        pop.sync()
    moved = 2 * k * per_member
    row = {"pairs": k, "bytes_moved": moved}
    a = summary(timed(clone, max(10, args.reps), 5))
    a["hbm_peak_fraction"] = round(moved / (a["median_ms"] * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(dict(row, what="clone", **a)), flush=True)
    ts = [t / BURST for t in timed(burst, max(10, args.reps), 2)]
    bb = summary(ts)
    bb["hbm_peak_fraction"] = round(moved / (bb["median_ms"] * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(dict(row, what="clone_burst", calls_per_sync=BURST, **bb)), flush=True)
    b = summary(timed(via_state_dict, 10, 1))
    print(json.dumps(dict(row, what="state_dict", ratio_to_clone=round(b["median_ms"] / a["median_ms"], 1), **b)),
          flush=True)
pop.step(2)  # the population still trains after the copies
pop.sync()
assert np.all(np.isfinite(pop.read_info_array()[:, :13]))
pop.close()

if not args.skip_tune:
    import tune_alpha  # noqa: E402
    rounds = args.steps // args.eval_interval

    def tune(strategy, steps, eval_interval, save):
        argv = [f"--save_directory={save}", f"--steps={steps}", f"--eval_interval={eval_interval}",
                f"--log_interval={eval_interval}", "--agent.layer_norm", "--eval_episodes=4", "--seed=0",
                "--number_of_alphas=16", "--number_of_seeds=1", "--max_evaluations=100000", "--task=synthetic",
                f"--strategy={strategy}", f"--halving_horizon={steps // eval_interval}"]
        t0 = time.perf_counter()
        tune_alpha.main(argv)
        wall = time.perf_counter() - t0
        with open(os.path.join(save, "cube-single-play-singletask-task2-v0", "checkpoint.pkl"), "rb") as f:
            tr = pickle.load(f)["trainer"]
        done = sum(e["current_step"] for e in tr["experiments"].values())
        done += sum(r["current_step"] for r in tr.get("retired", []))
        done -= sum(r["step"] for r in tr.get("lineage", []))  # inherited, not trained
        return wall, done, len(tr.get("lineage", []))
    with tempfile.TemporaryDirectory() as tmp:
        tune("pbt", 40, 20, os.path.join(tmp, "warm"))
        out = {}
        for strategy in ("successive_halving", "pbt"):
            wall, done, clones = tune(strategy, args.steps, args.eval_interval, os.path.join(tmp, strategy))
            out[strategy] = done / wall
            print(json.dumps({"what": "tune", "strategy": strategy, "steps": args.steps, "rounds": rounds,
                              "member_updates": done, "clones": clones, "wall_s": round(wall, 3),
                              "member_updates_per_s": round(done / wall, 1)}), flush=True)
        print(json.dumps({"what": "tune_ratio", "pbt_over_successive_halving":
                          round(out["pbt"] / out["successive_halving"], 3)}), flush=True)
