"""Initial-observation VAE timings (developer tool): microseconds per device-sampled train
step at B = 256 with hidden (128,) and (128, 256, 128), and per fqlpop_initobs_sample call of
50 and of 4 096 rows (host clock around work that ends in a device synchronise; the sample
call includes its device-to-host copy).

  python initobs_time.py [obs_dim] [repeats]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

from envmodel import initial_observation as io  # noqa: E402
from envmodel.trainer import EnvModelTrainerConfig  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 28
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
STEPS, CALLS = 2000, 200


class _Loader:
    def __init__(self, obs):
        self.dataset = {"observations": obs}


def main():
    rng = np.random.default_rng(0)
    data = rng.standard_normal((1000, D)).astype(np.float32)  # ~1 000 episode starts
    for hidden in ((128,), (128, 256, 128)):
        spec = io.InitialObservationSpec(D, 4, hidden)
        cfg = EnvModelTrainerConfig(steps=STEPS * (REPEATS + 1), batch_size=256, reconstruction_weight=10.0)
        tr = io.InitialObservationTrainer(spec, io.init_initial_observation(spec, 0), _Loader(data), None, cfg)
        tr.steps(STEPS)  # warm-up
        tr.sync()
        step_us = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            tr.steps(STEPS)
            tr.sync()
            step_us.append((time.perf_counter() - t0) / STEPS * 1e6)
        row = {"obs_dim": D, "latent_dim": 4, "hidden": list(hidden), "batch_size": 256,
               "train_step_us": [round(t, 2) for t in step_us]}
        for n in (50, 4096):
            tr.sample(n, seed=0)  # warm-up (and the buffers' allocation)
            us = []
            for r in range(REPEATS):
                t0 = time.perf_counter()
                for c in range(CALLS):
                    tr.sample(n, seed=c)
                us.append((time.perf_counter() - t0) / CALLS * 1e6)
            row[f"sample_{n}_us"] = [round(t, 2) for t in us]
        tr.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
