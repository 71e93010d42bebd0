"""Compare generated initial observations with the dataset's (stands in for the PCA plots of
the reference's distribution_visualizer.py:24-104; sklearn and seaborn are absent).

Reads ``<data_directory>/<dataset>.npz`` and the trained VAE under
``<save_directory>/<env_name>/env_models/`` (train_env_model.py --model initial_observation),
decodes ``--num_samples`` latents z ~ N(0, 1) on the GPU (the visualiser draws 1 100) and
writes ``initial_observation_distribution.csv`` there: per feature the mean and standard
deviation of the real episode starts (rows 0, 1000, ...) and of the generated ones, then the
same statistics of both sets projected on the two leading principal directions of the real
data (numpy SVD of the centred real starts).  Prints one JSON summary line.
"""
from __future__ import annotations

import csv
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from argparser import build_env_model_config_from_args, get_env_model_argparser  # noqa: E402
from envmodel.initial_observation import InitialObservationSampler, load_initial_observation_model  # noqa: E402
from task.offline_task_npz import load_npz_dataset  # noqa: E402


def distribution_rows(real: np.ndarray, generated: np.ndarray):
    """[(name, real_mean, real_std, generated_mean, generated_std)]: every feature, then the
    projections on the real data's two leading principal directions."""
    real, generated = np.asarray(real, np.float64), np.asarray(generated, np.float64)
    rows = [(f"feature_{i}", real[:, i].mean(), real[:, i].std(), generated[:, i].mean(), generated[:, i].std())
            for i in range(real.shape[1])]
    centre = real.mean(0)
    _, _, vt = np.linalg.svd(real - centre, full_matrices=False)
    for j in range(min(2, len(vt))):
        pr, pg = (real - centre) @ vt[j], (generated - centre) @ vt[j]
        rows.append((f"pc_{j}", pr.mean(), pr.std(), pg.mean(), pg.std()))
    return rows


def main(argv=None):
    p = get_env_model_argparser()
    p.add_argument("--num_samples", type=int, default=1100)
    args = p.parse_args(argv)
    config = build_env_model_config_from_args(args)
    base = config.env_name.replace("-singletask", "").rsplit("-task", 1)[0]
    real = load_npz_dataset(Path(config.data_directory) / f"{base}.npz")["observations"][::1000]
    d = Path(config.save_directory) / config.env_name / "env_models"
    sampler = InitialObservationSampler(*load_initial_observation_model(d))
    generated = sampler.sample(args.num_samples, seed=config.seed)
    sampler.close()
    rows = distribution_rows(real, generated)
    path = d / "initial_observation_distribution.csv"
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("name", "real_mean", "real_std", "generated_mean", "generated_std"))
        for r in rows:
            wr.writerow([r[0]] + [repr(float(x)) for x in r[1:]])
    feat = np.array([r[1:] for r in rows if r[0].startswith("feature_")])
    print(json.dumps({"env_name": config.env_name, "real_rows": int(len(real)), "generated_rows": int(len(generated)),
                      "max_mean_gap": float(np.abs(feat[:, 0] - feat[:, 2]).max()),
                      "std_ratio_min": float((feat[:, 3] / np.maximum(feat[:, 1], 1e-12)).min()),
                      "std_ratio_max": float((feat[:, 3] / np.maximum(feat[:, 1], 1e-12)).max()),
                      "csv": str(path)}))
    return path


if __name__ == "__main__":
    main()
