"""Train a world model on the GPU: the reference's train_env_model.py:1-137
(`--model baseline | termination_predictor`, same flags), over a local
OGBench-style .npz dataset (ogbench / wandb are absent: data must already be in
--data_directory; logs go to a CSV under --save_directory).

Saves ``<save_directory>/<env_name>/env_models/<model>.pt`` (flax
``to_bytes`` of the params tree, readable by utils/envmodel.py:load_model) and
``<model>_config.yaml``, as train_env_model.py:127-137 does.  ``multistep`` trains
the baseline cell through a ``--sequence_length`` scan (BPTT on the GPU) and saves
it under ``params/ScanCell_0/cell`` like flax's ``nn.scan`` tree.
``initial_observation`` trains the VAE of envmodel/initial_observation.py on the episode
starts (InitialObservationLoader), honouring ``--model.hidden_dims``, ``--model.latent_dim``
and ``--reconstruction_weight``, and saves ``{"params": {"encoder", "decoder"}}`` with
``hidden_dims`` and ``latent_dim`` in the yaml: the files distribution_visualizer.py:62-99 reads.

``--ensemble_size K`` trains K models, member k with seed ``--seed + k``, and saves them as
``<model>_ens<k>.pt`` / ``<model>_ens<k>_config.yaml`` / ``<model>_ens<k>_log.csv``: the
files task/offline_task_simulated.py loads with ``ensemble_size=K``.  With K >= 2 the K
models of the kinds in ``BATCHED_KINDS`` train as one launch per step
(envmodel.trainer.*EnsembleTrainer; K <= 16) and the files are byte for byte those of K runs
one after the other, which ``--ensemble_sequential`` still does.  Without
``--ensemble_size`` names and behaviour are the reference's.

``--bootstrap`` (PETS / MBPO / MOPO; not for ``initial_observation``) trains every model on
its own resample of the dataset, drawn on the device from the model's seed, and evaluates it
on the rows (multistep: episodes) the resample missed: ``oob/`` rows join the log CSVs at every
validation interval, and ``<model>_ens_oob.csv`` lists ``model, seed, n_units, n_oob`` and the
final out-of-bag losses of every model -- what ``--env_model_elites`` of tune_alpha.py and
evaluate_env_model.py ranks.  Without ``--bootstrap`` no file changes.
"""
from __future__ import annotations

import csv
import os
import sys
from pathlib import Path

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import envmodel as em  # noqa: E402
from argparser import build_env_model_config_from_args, get_env_model_argparser  # noqa: E402
from envmodel import initial_observation as iobs  # noqa: E402
from envmodel.flax_msgpack import msgpack_serialize  # noqa: E402
from envmodel.trainer import (StatePredictorEnsembleTrainer, StatePredictorTrainer,  # noqa: E402
                              TerminationPredictorEnsembleTrainer, TerminationPredictorTrainer)
from task.offline_task_npz import load_npz_dataset  # noqa: E402
from utils.logger import CsvLogger  # noqa: E402


class StepLoader:
    """utils/data_loader.py:47-52: uniform minibatches of single transitions."""

    def __init__(self, dataset: dict, rng=None):
        self.dataset = {k: dataset[k] for k in ("observations", "actions", "rewards", "next_observations")}
        self.rng = rng  # a np.random.RandomState; None: the global numpy stream

    def sample(self, batch_size: int, rng=None) -> dict:
        rng = rng or self.rng or np.random
        idx = rng.randint(len(self.dataset["observations"]), size=batch_size)
        return {k: v[idx] for k, v in self.dataset.items()}


class MultistepLoader:
    """utils/data_loader.py:25-39: the dataset as [n / 1000][1000] episodes; a batch is
    batch_size windows of sequence_length steps (uniform episode, uniform start in
    [0, 1000 - sequence_length))."""

    episode_length = 1000

    def __init__(self, dataset: dict, sequence_length: int = 128, rng=None):
        self.sequence_length = sequence_length
        self.rng = rng  # as StepLoader
        n = len(dataset["observations"])
        if n % self.episode_length:
            raise ValueError(f"multistep: {n} rows is not a whole number of {self.episode_length}-step episodes")
        shape = (n // self.episode_length, self.episode_length)
        self.dataset = {k: np.asarray(dataset[k]).reshape(shape + np.shape(dataset[k])[1:])
                        for k in ("observations", "actions", "rewards", "next_observations")}

    def sample(self, batch_size: int, rng=None) -> dict:
        rng = rng or self.rng or np.random
        ep = rng.randint(len(self.dataset["observations"]), size=batch_size)
        start = rng.randint(0, self.episode_length - self.sequence_length, size=batch_size)
        idx = start[:, None] + np.arange(self.sequence_length)
        return {k: v[ep[:, None], idx] for k, v in self.dataset.items()}


class InitialObservationLoader:
    """utils/data_loader.py:14-22: the episode starts, rows 0, 1000, 2000, ... of every array."""

    episode_length = 1000

    def __init__(self, dataset: dict, rng=None):
        idx = np.arange(0, len(dataset["observations"]), self.episode_length)
        self.indices = idx
        self.dataset = {k: np.asarray(v)[idx] for k, v in dataset.items() if len(v) == len(dataset["observations"])}
        self.rng = rng  # as StepLoader

    def sample(self, batch_size: int, rng=None) -> dict:
        rng = rng or self.rng or np.random
        idx = rng.randint(len(self.dataset["observations"]), size=batch_size)
        return {k: v[idx] for k, v in self.dataset.items()}


class _CsvRunLogger:
    """wandb.log stand-in: long-format CSV (step, key, value) -- train and val rows carry
    different keys, so a fixed-header CSV would drop some."""

    def __init__(self, path: Path):
        self.csv = CsvLogger(str(path))

    def log(self, row: dict, step: int):
        for k, v in row.items():
            self.csv.log({"key": k, "value": v}, step=step)


def build_parser():
    """The reference's flags (argparser.py) plus --ensemble_size and --ensemble_sequential."""
    parser = get_env_model_argparser()
    parser.add_argument("--ensemble_size", type=int, default=0)
    parser.add_argument("--ensemble_sequential", action="store_true",
                        help="train the --ensemble_size models one after the other (K runs) instead of "
                             "as one launch per step; the files are the same")
    parser.add_argument("--bootstrap", action="store_true",
                        help="train every model on its own bootstrap resample of the dataset and log its "
                             "out-of-bag losses (oob/ rows, <model>_ens_oob.csv)")
    return parser


def member_config(args, k: int | None):
    """(trainer config, saved name) of ensemble member k; k None: the plain run."""
    config = build_env_model_config_from_args(args)
    if k is None:
        return config, config.model
    config.seed = args.seed + k
    return config, f"{config.model}_ens{k}"


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.ensemble_size < 0:
        raise ValueError("--ensemble_size must be >= 0")
    if args.ensemble_size > 0 and args.model == "initial_observation":
        raise ValueError("--ensemble_size is for baseline, multistep and termination_predictor")
    if args.bootstrap and args.model == "initial_observation":
        raise ValueError("--bootstrap is for baseline, multistep and termination_predictor")
    oob = [] if args.bootstrap else None  # one row per model, in model order
    if args.ensemble_size == 0:
        save_dir = train_one(*member_config(args, None), oob=oob)
    elif args.ensemble_size >= 2 and not args.ensemble_sequential and args.model in BATCHED_KINDS:
        save_dir = train_ensemble([member_config(args, k) for k in range(args.ensemble_size)], oob=oob)
    else:
        for k in range(args.ensemble_size):
            save_dir = train_one(*member_config(args, k), oob=oob)
    if oob is not None:
        write_oob_csv(save_dir / f"{args.model}_ens_oob.csv", oob)
    return save_dir


def oob_row(k: int, seed: int, trainer, logs: dict, model: int = 0) -> dict:
    """The ``<model>_ens_oob.csv`` row of saved model k: trainer-side model ``model``."""
    return {"model": k, "seed": seed, "n_units": trainer.n_units, "n_oob": len(trainer.oob_rows(model)), **logs}


def write_oob_csv(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


# the model kinds whose ensembles train batched by default (the ensemble
# training table: batched is the default only where it beats the loop at K = 5)
BATCHED_KINDS = ("baseline", "multistep", "termination_predictor")


def _load_data(config):
    """(train, val, save_dir) of a run."""
    base = config.env_name.replace("-singletask", "").rsplit("-task", 1)[0]
    d = Path(config.data_directory)
    train = load_npz_dataset(d / f"{base}.npz")
    val_path = d / f"{base}-val.npz"
    val = load_npz_dataset(val_path) if val_path.exists() else train
    save_dir = Path(config.save_directory) / config.env_name / "env_models"
    save_dir.mkdir(parents=True, exist_ok=True)
    return train, val, save_dir


def _state_predictor_spec(config, D, A, hidden, save_dir):
    """(spec, frozen termination predictor tree or None) of a baseline / multistep run."""
    spec = em.EnvModelSpec(D, A, hidden, em.DEFAULT_HIDDEN)
    tp = None
    if config.termination_weight > 0:  # utils/envmodel.py load_model("termination_predictor")
        tp = em.load_flax_msgpack(save_dir / "termination_predictor.pt")
        tp = tp.get("params", tp)
        n = sum(1 for k in tp if k.startswith("Dense_"))
        spec.tp_hidden = tuple(int(np.asarray(tp[f"Dense_{i}"]["kernel"]).shape[1]) for i in range(n - 1))
    return spec, tp


def _save(save_dir, name, config, params):
    with open(save_dir / f"{name}_config.yaml", "w") as f:
        yaml.safe_dump({k: list(v) if isinstance(v, tuple) else v for k, v in config.model_config.items()}, f)
    with open(save_dir / f"{name}.pt", "wb") as f:
        if config.model == "multistep":  # nn.scan(Cell) tree (envmodel/multistep.py:41-52)
            params = {"ScanCell_0": {"cell": params}}
        f.write(msgpack_serialize({"params": params}))


def train_ensemble(members, oob=None):
    """The K runs ``train_one(config_k, name_k)`` as one batched trainer: model k starts from
    the tree of seed_k, draws its minibatches and dropout mask from seed_k on the device and
    its val batches from ``RandomState(seed_k)`` (what ``np.random.seed(seed_k)`` gives the
    sequential run), and logs to its own CSV.  The saved files are those of the K runs."""
    configs, names = [c for c, _ in members], [n for _, n in members]
    config = configs[0]
    train, val, save_dir = _load_data(config)
    D, A = train["observations"].shape[-1], train["actions"].shape[-1]
    hidden = tuple(config.model_config.get("hidden_dims", em.DEFAULT_HIDDEN))
    seeds = [c.seed for c in configs]
    loggers = [_CsvRunLogger(save_dir / f"{name}_log.csv") for name in names]
    if config.model in ("baseline", "multistep"):
        spec, tp = _state_predictor_spec(config, D, A, hidden, save_dir)
        if config.model == "multistep":
            loaders = (MultistepLoader(train, config.sequence_length), MultistepLoader(val, config.sequence_length))
        else:
            loaders = (StepLoader(train), StepLoader(val))
        trainer = StatePredictorEnsembleTrainer(spec, [em.init_state_predictor(spec, s) for s in seeds], *loaders,
                                                config, seeds, loggers=loggers, tp_params=tp,
                                                bootstrap=oob is not None)
    elif config.model == "termination_predictor":
        spec = em.EnvModelSpec(D, A, em.DEFAULT_HIDDEN, hidden)
        trainer = TerminationPredictorEnsembleTrainer(spec, [em.init_termination_predictor(spec, s) for s in seeds],
                                                      StepLoader(train), StepLoader(val), config, seeds,
                                                      loggers=loggers, bootstrap=oob is not None)
    else:
        raise ValueError(f"no batched ensemble trainer for model {config.model!r}")
    trainer.train()
    for cfg, name, params in zip(configs, names, trainer.params):
        _save(save_dir, name, cfg, params)
    if oob is not None:
        oob.extend(oob_row(k, s, trainer, trainer.last_oob[k], model=k) for k, s in enumerate(seeds))
    trainer.close()
    return save_dir


def train_one(config, name: str, oob=None):
    """One training run of config.model, saved under ``name``."""
    train, val, save_dir = _load_data(config)
    D, A = train["observations"].shape[-1], train["actions"].shape[-1]
    hidden = tuple(config.model_config.get("hidden_dims", em.DEFAULT_HIDDEN))
    logger = _CsvRunLogger(save_dir / f"{name}_log.csv")
    np.random.seed(config.seed)
    if config.model in ("baseline", "multistep"):
        spec, tp = _state_predictor_spec(config, D, A, hidden, save_dir)
        if config.model == "multistep":
            loaders = (MultistepLoader(train, config.sequence_length), MultistepLoader(val, config.sequence_length))
        else:
            loaders = (StepLoader(train), StepLoader(val))
        trainer = StatePredictorTrainer(spec, em.init_state_predictor(spec, config.seed), *loaders, config,
                                        logger=logger, tp_params=tp, bootstrap=oob is not None)
    elif config.model == "termination_predictor":
        spec = em.EnvModelSpec(D, A, em.DEFAULT_HIDDEN, hidden)
        trainer = TerminationPredictorTrainer(spec, em.init_termination_predictor(spec, config.seed),
                                              StepLoader(train), StepLoader(val), config, logger=logger,
                                              bootstrap=oob is not None)
    elif config.model == "initial_observation":
        io_spec = iobs.InitialObservationSpec(D, int(config.model_config.get("latent_dim", 4)), hidden)
        trainer = iobs.InitialObservationTrainer(io_spec, iobs.init_initial_observation(io_spec, config.seed),
                                                 InitialObservationLoader(train), InitialObservationLoader(val),
                                                 config, logger=logger)
        trainer.train()
        iobs.save_initial_observation_model(save_dir, io_spec, trainer.params)
        trainer.close()
        return save_dir
    else:
        raise ValueError(f"unknown model {config.model!r} (baseline, multistep, termination_predictor, "
                         "initial_observation)")
    trainer.train()
    _save(save_dir, name, config, trainer.params)
    if oob is not None:
        oob.append(oob_row(len(oob), config.seed, trainer, trainer.last_oob))
    trainer.close()
    return save_dir


if __name__ == "__main__":
    print(main())
