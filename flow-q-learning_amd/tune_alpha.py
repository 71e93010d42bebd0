"""alpha-sweep driver (reference tune_alpha.py:14-95), same flags and flow:
alpha = logspace(log10 3, log10 1000, --number_of_alphas), seeds =
random.sample(range(10000), --number_of_seeds) after random.seed(--seed);
--single_experiment --job_id=i runs one (alpha, seed) to completion with a
checkpoint every eval_interval; otherwise an Identity-strategy Trainer trains
the whole population (here: all members together on the GPU) and writes
<save>/<env>/checkpoint.pkl.  --strategy successive_halving selects halving,
--strategy pbt population-based training of alpha (hpo/pbt.py: the worst members are
replaced by on-device clones of the best under a perturbed alpha, the population stays
full; one GPU only; <save>/<env>/pbt_lineage.csv records every clone).

--lrs / --discounts / --taus (each one or more values) extend the grid to alpha x seed x
those: every combination is its own ExperimentConfig and trains as one member of the same
population under its own learning rate, discount and target-EMA tau (the engine keeps the
three per member).  Without them the grid, the seeds and --job_id are the reference's.
--strategy pbt --pbt_explore alpha lr discount tau perturbs the named fields (default: alpha),
within --pbt_{lr,discount,tau}_{min,max}.

Data: --task synthetic (default; SURVEY.md 8d transitions + a toy evaluation
env), --task npz (local OGBench .npz files under --data_directory) or --task
simulated (candidates scored by world-model rollouts on the GPU).

Training on world-model branches (--task simulated, one GPU): --model_rollout_branches N
--model_rollout_horizon H --model_rollout_interval I [--model_rollout_warmup W]
[--model_real_ratio R] [--model_buffer_rows C]: every I updates each member rolls N branches
of H steps in the env model into its own on-device ring, and its minibatches take the share
R from the offline data, the rest from the ring (trainer/trainer.py; off by default).
--env_model_ensemble 5 --model_rollout_ensemble --model_rollout_penalty 1.0
runs the branches under the K-model ensemble instead (a model drawn per branch and step) and
lowers every synthetic reward by the penalty times the models' disagreement about that step.

Offline-to-online fine-tuning (--task synthetic, one GPU; strategies identity and
successive_halving): --online_steps N [--online_envs E] [--online_utd U]
[--online_buffer_rows C] [--online_real_ratio auto|R]: the last N of --steps updates are
online.  For every U updates each member acts once in its own E environments (one
Population.act launch for the whole population), the observed transitions go into its
on-device ring, and its minibatches draw offline and online rows uniformly over both ("auto")
or with the offline share R (trainer/trainer.py; off by default).

Multi-GPU (BASELINE configs 4 / 5): launched by torch.distributed.run with one
process per GPU (``python -m torch.distributed.run --nproc-per-node 8
--master-addr 127.0.0.1 tune_alpha.py ...``), the population is sharded over the
ranks by trainer.distributed_trainer.DistributedTrainer (RCCL over xGMI gathers
the scores and moves members after pruning); rank 0 writes the checkpoint.
"""
from __future__ import annotations

import itertools
import os
import pickle
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from argparser import (build_config_from_args, build_model_rollout_config_from_args,  # noqa: E402
                       build_online_config_from_args, get_argparser)
from hpo.identity import Identity  # noqa: E402
from hpo.pbt import PopulationBasedTraining  # noqa: E402
from hpo.successive_halving import SuccessiveHalving  # noqa: E402
from trainer.config import ExperimentConfig  # noqa: E402
from trainer.experiment import Experiment  # noqa: E402
from trainer.trainer import Trainer  # noqa: E402


def make_task(args, config):
    if args.task == "simulated":
        # world-model evaluation on the GPU (BASELINE config 5): the reference's env-model files
        # under <save>/<env>/env_models if present, else a seeded synthetic model
        from task.offline_task_simulated import (OfflineTaskWithSimulatedEvaluations, load_env_model_ensemble,
                                                 select_elites)
        env_dir = config.save_directory / config.env_name / "env_models"
        if args.env_model_elites:
            # the E models with the lowest out-of-bag loss, handed over as if E had been trained
            elites = select_elites(env_dir, args.env_model, args.env_model_ensemble, args.env_model_elites)
            return OfflineTaskWithSimulatedEvaluations(
                config.env_name, model=args.env_model, save_directory=config.save_directory,
                n_rows=args.synthetic_rows, num_evaluation_envs=config.eval_episodes,
                max_episode_steps=args.max_episode_steps, seed=config.seed,
                initial_observations=args.initial_observations, ensemble_score=args.ensemble_score,
                env_models=load_env_model_ensemble(config.save_directory, config.env_name, args.env_model,
                                                   args.env_model_ensemble, members=elites))
        return OfflineTaskWithSimulatedEvaluations(
            config.env_name, model=args.env_model, save_directory=config.save_directory if env_dir.exists() else None,
            n_rows=args.synthetic_rows, num_evaluation_envs=config.eval_episodes,
            max_episode_steps=args.max_episode_steps, seed=config.seed,
            initial_observations=args.initial_observations,
            ensemble_size=args.env_model_ensemble, ensemble_score=args.ensemble_score)
    if args.task == "npz":
        from task.offline_task_npz import OfflineTaskNpz
        return OfflineTaskNpz(config.env_name, config.data_directory)
    from task.offline_task_synthetic import OfflineTaskSynthetic
    return OfflineTaskSynthetic(config.env_name, n_rows=args.synthetic_rows,
                                num_evaluation_envs=min(config.eval_episodes, 64), seed=config.seed)


def build_parser():
    """The reference's flags (argparser.py) plus this driver's own."""
    parser = get_argparser()
    parser.add_argument("--max_evaluations", type=int, default=200)
    parser.add_argument("--number_of_seeds", type=int, default=1)
    parser.add_argument("--number_of_alphas", type=int, default=1)
    parser.add_argument("--task", choices=("synthetic", "npz", "simulated"), default="synthetic")
    parser.add_argument("--env_model", choices=("baseline", "multistep"), default="multistep")
    # --task simulated: episode starts from the dataset (rows 0, 1000, ...) or decoded from the
    # initial-observation VAE saved by train_env_model.py --model initial_observation
    parser.add_argument("--initial_observations", choices=("dataset", "model"), default="dataset")
    parser.add_argument("--max_episode_steps", type=int, default=1000)
    parser.add_argument("--synthetic_rows", type=int, default=100_000)
    parser.add_argument("--strategy", choices=("identity", "successive_halving", "pbt"), default="identity")
    parser.add_argument("--fraction", type=float, default=0.5)
    parser.add_argument("--history_length", type=int, default=1)
    # SuccessiveHalving's evaluation horizon E (hpo/successive_halving.py milestones).  The
    # reference passes --max_evaluations, which Trainer.train spends per candidate: with N
    # candidates evaluated every round the milestones (in evaluations per candidate, >= h)
    # are then out of reach for N >= 8 at h = 4.  The reference's StrategyEvaluator counts E in
    # rounds (steps / eval_interval); --halving_horizon selects that reading.  Default: the
    # reference wiring.
    parser.add_argument("--halving_horizon", type=int, default=None)
    # population-based training (hpo/pbt.py); --history_length is shared with halving
    parser.add_argument("--pbt_ready_interval", type=int, default=1)
    parser.add_argument("--pbt_truncation", type=float, default=0.25)
    parser.add_argument("--pbt_alpha_min", type=float, default=None)
    parser.add_argument("--pbt_alpha_max", type=float, default=None)
    parser.add_argument("--pbt_explore", nargs="+", choices=("alpha", "lr", "discount", "tau"), default=["alpha"])
    for f in ("lr", "discount", "tau"):
        parser.add_argument(f"--pbt_{f}_min", type=float, default=None)
        parser.add_argument(f"--pbt_{f}_max", type=float, default=None)
    # per-member lr / discount / tau grids (none given: the alpha x seed grid alone)
    parser.add_argument("--lrs", type=float, nargs="+", default=None)
    parser.add_argument("--discounts", type=float, nargs="+", default=None)
    parser.add_argument("--taus", type=float, nargs="+", default=None)
    # --task simulated: score under the K env models saved by train_env_model.py --ensemble_size K
    # (0: the single model); --ensemble_score: the mean or the min of the per-model success rates,
    # or mixed episodes that draw a model afresh at every step (task/offline_task_simulated.py)
    parser.add_argument("--env_model_ensemble", type=int, default=0)
    parser.add_argument("--ensemble_score", choices=("mean", "min", "mixed"), default="mean")
    # keep only the E of the K models with the lowest out-of-bag loss (<model>_ens_oob.csv of
    # train_env_model.py --bootstrap); 0: all K
    parser.add_argument("--env_model_elites", type=int, default=0)
    return parser


def experiment_grid(combinations, lrs=None, discounts=None, taus=None):
    """The ExperimentConfigs of a run: the (alpha, seed) combinations in their order, each
    crossed with the given lr, discount and tau values (innermost); an axis left None stays
    out of the grid and its field None."""
    axes = [v if v else [None] for v in (lrs, discounts, taus)]
    return [ExperimentConfig(seed=seed, alpha=alpha, lr=lr, discount=discount, tau=tau)
            for (alpha, seed), lr, discount, tau in itertools.product(combinations, *axes)]


def main(argv=None):
    args = build_parser().parse_args(argv)
    config = build_config_from_args(args)
    model_rollouts = build_model_rollout_config_from_args(args)
    online = build_online_config_from_args(args)
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    device = 0
    if world_size > 1 and online.enabled and not args.single_experiment:
        from trainer.trainer import ONLINE_DISTRIBUTED_MSG
        sys.exit(ONLINE_DISTRIBUTED_MSG)  # before any process group exists
    if args.single_experiment and online.enabled:
        sys.exit("--online_steps needs the population Trainer (drop --single_experiment)")
    if world_size > 1 and model_rollouts.enabled and not args.single_experiment:
        from trainer.trainer import MODEL_ROLLOUT_DISTRIBUTED_MSG
        sys.exit(MODEL_ROLLOUT_DISTRIBUTED_MSG)  # before any process group exists
    if args.single_experiment and model_rollouts.enabled:
        sys.exit("--model_rollout_branches needs the population Trainer (drop --single_experiment)")
    if world_size > 1 and args.strategy == "pbt" and not args.single_experiment:
        from trainer.trainer import PBT_DISTRIBUTED_MSG
        sys.exit(PBT_DISTRIBUTED_MSG)  # before any process group exists
    if world_size > 1 and not args.single_experiment:
        import torch
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        n_dev = torch.cuda.device_count()
        if n_dev >= world_size:  # one GPU per rank: RCCL (the "nccl" backend) over xGMI
            device = local_rank
            torch.cuda.set_device(device)
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:  # fewer GPUs than ranks (a rehearsal on a small box): ranks share GPUs, gloo
            device = local_rank % max(n_dev, 1)
            dist.init_process_group("gloo")

    random.seed(config.seed)
    np.random.seed(config.seed)
    alpha_values = np.logspace(np.log10(3), np.log10(1000), num=args.number_of_alphas).tolist()
    seeds = random.sample(range(10000), args.number_of_seeds)
    combinations = list(itertools.product(alpha_values, seeds))
    configs = experiment_grid(combinations, args.lrs, args.discounts, args.taus)
    task = make_task(args, config)

    if args.single_experiment:
        experiment = Experiment(task, config, configs[args.job_id])
        done = False
        while not done:
            done = experiment.train(config.eval_interval)
            experiment.save_agent(checkpoint=True)
        experiment.stop()
        return

    ckpt = config.save_directory / config.env_name / "checkpoint.pkl"
    state = {}
    if ckpt.exists():
        with open(ckpt, "rb") as f:  # written by this script
            state = pickle.load(f)
    if args.strategy == "identity":
        strategy = Identity(population=configs, total_evaluations=0, state_dict=state.get("strategy"))
    elif args.strategy == "pbt":
        bounds = None
        if args.pbt_alpha_min is not None or args.pbt_alpha_max is not None:
            bounds = (args.pbt_alpha_min, args.pbt_alpha_max)
        hp_bounds = {f: (getattr(args, f"pbt_{f}_min"), getattr(args, f"pbt_{f}_max"))
                     for f in ("lr", "discount", "tau")
                     if getattr(args, f"pbt_{f}_min") is not None or getattr(args, f"pbt_{f}_max") is not None}
        strategy = PopulationBasedTraining(population=set(configs), total_evaluations=args.max_evaluations,
                                           ready_interval=args.pbt_ready_interval, truncation=args.pbt_truncation,
                                           alpha_bounds=bounds, history_length=args.history_length,
                                           seed=config.seed, state_dict=state.get("strategy"),
                                           explore=tuple(args.pbt_explore), bounds=hp_bounds,
                                           base={"lr": config.agent.lr, "discount": config.agent.discount,
                                                 "tau": config.agent.tau})
    else:
        horizon = args.max_evaluations if args.halving_horizon is None else args.halving_horizon
        strategy = SuccessiveHalving(population=set(configs), total_evaluations=horizon,
                                     fraction=args.fraction, history_length=args.history_length,
                                     state_dict=state.get("strategy"))
    if world_size > 1:
        from trainer.distributed_trainer import DistributedTrainer
        trainer = DistributedTrainer(task, strategy, config, state_dict=state.get("trainer"), device=device,
                                     model_rollouts=model_rollouts)
    else:
        # (without --online_steps the call is the one it was: no online argument)
        extra = {"online": online} if online.enabled else {}
        trainer = Trainer(task, strategy, config, state_dict=state.get("trainer"), model_rollouts=model_rollouts,
                          **extra)
    trainer.train(max_evaluations=args.max_evaluations)
    trainer_state = trainer.state_dict()  # collective under DistributedTrainer (rank 0 gets it)
    if trainer_state is not None:
        ckpt.parent.mkdir(parents=True, exist_ok=True)
        with open(ckpt, "wb") as f:
            pickle.dump({"trainer": trainer_state, "strategy": trainer.strategy.state_dict()}, f)
    if world_size > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
