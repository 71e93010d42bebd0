"""Evaluate a trained world model on recorded episodes (the reference's
evaluate_env_model.py:1-47 + evaluator/env_model_evaluator.py, the stage between
train_env_model.py and tune_alpha.py): replay the dataset's recorded actions through
``--model`` (baseline | multistep) and the termination predictor on the GPU, all
episodes in one launch, and report the per-step MSE / MAE drift and the real2sim
success rate.

Flags: the reference's (train_env_model.py's, plus --eval_episodes), and --horizon
(steps replayed from each episode's start) and --anchor_every (0: open loop; k: reset to
the recorded state every k steps).  Reads ``<data_directory>/<dataset>.npz`` and the
models under ``<save_directory>/<env_name>/env_models/`` as train_env_model.py wrote
them; needs no agent and no real environment.  Writes
``<save_directory>/<env_name>/env_models/<model>_trajectory_comparison.csv`` (one row per
step) and prints one JSON summary line.
"""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import envmodel as em  # noqa: E402
from argparser import build_env_model_config_from_args, get_env_model_argparser  # noqa: E402
from evaluator.env_model_evaluator import EnvModelEvaluator  # noqa: E402
from task.offline_task_npz import load_npz_dataset  # noqa: E402
from task.offline_task_simulated import load_reference_env_model  # noqa: E402

HOST_WIDTH = 64  # the replay runs no actor: host the env model in the smallest population


def get_argparser():
    p = get_env_model_argparser()
    p.add_argument("--eval_episodes", type=int, default=50,
                   help="Number of evaluation episodes for the environment model.")
    p.add_argument("--horizon", type=int, default=1000)
    p.add_argument("--anchor_every", type=int, default=0)
    return p


def main(argv=None):
    args = get_argparser().parse_args(argv)
    config = build_env_model_config_from_args(args)
    base = config.env_name.replace("-singletask", "").rsplit("-task", 1)[0]
    dataset = load_npz_dataset(Path(config.data_directory) / f"{base}.npz")
    sp_tree, tp_tree = load_reference_env_model(config.save_directory, config.env_name, config.model)
    spec = em.spec_from_trees(sp_tree, tp_tree)

    from fqlpop import Population, PopulationConfig
    pop = Population(PopulationConfig(obs_dim=spec.obs_dim, action_dim=spec.action_dim,
                                      hidden_dims=(HOST_WIDTH,) * 4, batch_size=64), [1.0], [config.seed])
    try:
        pop.set_env_model(em.flatten_state_predictor(spec, sp_tree), em.flatten_termination_predictor(spec, tp_tree),
                          spec.sp_hidden, spec.tp_hidden)
        ev = EnvModelEvaluator(dataset, pop)
        res = ev.evaluate(args.horizon, n_episodes=args.eval_episodes, anchor_every=args.anchor_every,
                          seed=config.seed)
        path = ev.write_csv(Path(config.save_directory) / config.env_name / "env_models" /
                            f"{config.model}_trajectory_comparison.csv")
    finally:
        pop.close()
    last = len(res["n_valid"]) - 1
    print(json.dumps({"env_name": config.env_name, "model": config.model, "episodes": args.eval_episodes,
                      "horizon": last + 1, "anchor_every": args.anchor_every,
                      "mse_mean_first": float(res["mse_mean"][0]), "mse_mean_last": float(res["mse_mean"][last]),
                      "mae_mean_first": float(res["mae_mean"][0]), "mae_mean_last": float(res["mae_mean"][last]),
                      "real2sim_success": res["real2sim_success"], "recorded_success": res["recorded_success"],
                      "csv": str(path)}))
    return path


if __name__ == "__main__":
    main()
