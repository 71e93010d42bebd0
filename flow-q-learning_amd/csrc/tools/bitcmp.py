"""Bit-identity check between builds (developer tool, on the GPU box from the repo root).

Runs device-sampled population steps (default: 20 steps of the cube headline shape, 4 members,
B = 256, H = 512), then one validation pass, and prints a SHA-256 over the train and val info
rows and every member's parameters (the flat state, which holds the target critic too), Adam m
and Adam v.  Run it once per build (FQLPOP_LIB selects a second library) and compare the digests:
    python flow-q-learning_amd/csrc/tools/bitcmp.py
    FQLPOP_LIB=$PWD/flow-q-learning_amd/csrc/devlib/libfqlpop_ref.so python flow-q-learning_amd/csrc/tools/bitcmp.py
Other shapes and code paths:
    ... bitcmp.py --members 2 --hidden 512 --batch 64 --steps 4 --engine-option stream_fwd=0
    ... bitcmp.py --hidden 64 --batch 64 --no-layer-norm --eager
The line also shows the wall time of the first step (graph capture included).
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "flow-q-learning_amd"))

from fqlpop import Population, PopulationConfig  # noqa: E402
from fqlpop._lib import STATE_ADAM_M, STATE_ADAM_V, STATE_PARAMS, set_engine_option  # noqa: E402


def dataset(n, D, A, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, D), dtype=np.float32)
    rew = (rng.random(n) < 0.05).astype(np.float32) - 1.0
    return {
        "observations": obs,
        "actions": rng.uniform(-1 + 1e-5, 1 - 1e-5, (n, A)).astype(np.float32),
        "rewards": rew,
        "masks": (1.0 - (rew == 0)).astype(np.float32),
        "next_observations": (obs + 0.05 * rng.standard_normal((n, D))).astype(np.float32),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-layer-norm", action="store_true", help="critic without LayerNorm")
    ap.add_argument("--engine-option", action="append", default=[], metavar="K=V")
    ap.add_argument("--eager", action="store_true", help="no graph capture: launch every step")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()

    for kv in args.engine_option:
        k, v = kv.split("=")
        set_engine_option(k, int(v))
    D, A, m = 28, 5, args.members
    cfg = PopulationConfig(hidden_dims=(args.hidden,) * 4, batch_size=args.batch,
                           layer_norm=not args.no_layer_norm, use_graph=not args.eager)
    alphas = [(3.0, 10.0, 100.0, 1000.0)[i % 4] * (1 + i // 4) for i in range(m)]
    pop = Population(cfg, alphas, [11 + i for i in range(m)], device=0)
    pop.set_dataset(dataset(50_000, D, A, 0))
    pop.set_dataset(dataset(5_000, D, A, 1), "val")
    t0 = time.perf_counter()
    pop.step(1)
    pop.sync()
    first_ms = 1e3 * (time.perf_counter() - t0)
    pop.step(args.steps - 1)
    pop.total_loss()
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pop.read_info_array()).tobytes())
    h.update(np.ascontiguousarray(pop.read_info_array("val")).tobytes())
    for i in range(m):
        for which in (STATE_PARAMS, STATE_ADAM_M, STATE_ADAM_V):
            h.update(np.ascontiguousarray(pop.get_flat(i, which)).tobytes())
    pop.close()
    case = f"m{m} H{args.hidden} B{args.batch} ln{int(not args.no_layer_norm)} steps{args.steps}" \
           f"{' eager' if args.eager else ''} {' '.join(args.engine_option)}".rstrip()
    print("bitcmp", os.environ.get("FQLPOP_LIB", "in-tree"), f"[{case}]", h.hexdigest(), f"first step {first_ms:.1f} ms")


if __name__ == "__main__":
    main()
