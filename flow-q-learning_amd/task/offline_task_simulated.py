"""Offline task evaluated in a learned world model (reference
task/offline_task_simulated.py:13-111), with the evaluation on the GPU.

Training data: a dict dataset (synthetic of the env's shape by default, or a
local OGBench ``.npz`` through task.offline_task_npz).  Evaluation: the
reference steps ``num_evaluation_envs`` copies of the state predictor and the
termination predictor from real-env resets, one Python-driven jit call per
step (evaluator/evaluation.py:75-114).  Here

* ``evaluate_members`` rolls every requested population member in ONE device
  launch (``Population.rollout`` -> ``fqlpop_rollout``) and returns the
  success rate per member (BASELINE config 5);
* ``reset`` / ``step`` keep the reference's per-step Task contract for the
  generic ``evaluate_agent`` loop, each step running the env model on the
  GPU (``fqlpop_envmodel_step``).

Initial observations: the reference resets MuJoCo envs (absent here); this
task draws episode starts of the training dataset, rows 0, 1000, 2000, ...
as utils/data_loader.py:14-19 (InitialObservationLoader) does, by default; with
``initial_observations="model"`` it decodes them from the trained initial-observation
VAE (envmodel/initial_observation.py; explicit ``initial_observation_model=(spec,
params)`` or ``initial_observation.pt`` + ``initial_observation_config.yaml`` under
``<save_directory>/<env_name>/env_models``), one seeded GPU launch per reset.

Env model source, in order: explicit ``env_model=(sp_tree, tp_tree)``; the
reference's files ``<save_directory>/<env_name>/env_models/{model}.pt`` +
``{model}_config.yaml`` and ``termination_predictor.*`` (utils/envmodel.py:10-49;
flax msgpack read by envmodel.flax_msgpack, yaml with SafeLoader); otherwise
a seeded synthetic model of the default shape.

Ensembles: ``env_models=[(sp_tree, tp_tree), ...]`` (or ``ensemble_size=K`` with
``save_directory``: the files ``{model}_ens<k>.pt`` written by ``train_env_model.py
--ensemble_size K``) scores every member under K models of one shape in one launch
(``Population.rollout_ensemble``).  ``ensemble_score`` picks the score that the
strategies see: the ``mean`` or the ``min`` of the per-model success rates, or the
success rate of ``mixed`` episodes that draw a model afresh at every step; the spread
over the models goes next to it (``success_std`` / ``success_min`` / ``success_max``).
``reset`` / ``step`` keep using model 0.
"""
from __future__ import annotations

from pathlib import Path
from typing import Literal

import numpy as np
import yaml

import envmodel as em
from task.offline_task_synthetic import env_shape, make_synthetic_dataset
from task.task import Task


def load_reference_env_model(save_directory: Path, env_name: str, model: str):
    """(sp_tree, tp_tree) from the reference's save layout (utils/envmodel.py:10-49)."""
    d = Path(save_directory) / env_name / "env_models"
    trees = []
    for name in (model, "termination_predictor"):
        cfg_path, pt_path = d / f"{name}_config.yaml", d / f"{name}.pt"
        if not cfg_path.exists() or not pt_path.exists():
            raise FileNotFoundError(f"env model {name} not found under {d}")
        with open(cfg_path) as f:
            yaml.load(f, Loader=yaml.SafeLoader)  # hidden dims are re-derived from the shapes
        tree = em.load_flax_msgpack(pt_path)
        trees.append(tree)
    return trees[0], trees[1]


ENSEMBLE_SCORES = ("mean", "min", "mixed")


def ensemble_model_names(directory: Path, model: str, ensemble_size: int):
    """[(state predictor name, termination predictor name)] of the K members saved by
    ``train_env_model.py --ensemble_size K`` under ``directory``: ``{model}_ens<k>`` with
    ``termination_predictor_ens<k>`` if all K of those exist, else the shared
    ``termination_predictor``.  FileNotFoundError names the first missing file."""
    d = Path(directory)
    own_tp = all((d / f"termination_predictor_ens{k}.pt").exists() for k in range(ensemble_size))
    names = [(f"{model}_ens{k}", f"termination_predictor_ens{k}" if own_tp else "termination_predictor")
             for k in range(ensemble_size)]
    for pair in names:
        for name in pair:
            if not (d / f"{name}.pt").exists():
                raise FileNotFoundError(f"env model ensemble member {name}.pt not found under {d}")
    return names


def load_env_model_ensemble(save_directory: Path, env_name: str, model: str, ensemble_size: int, members=None):
    """[(sp_tree, tp_tree)] * K from ``<save_directory>/<env_name>/env_models`` (ensemble_model_names);
    ``members``: the indices to load, in that order (``select_elites``), instead of all K."""
    d = Path(save_directory) / env_name / "env_models"
    names = ensemble_model_names(d, model, ensemble_size)
    if members is not None:
        names = [names[k] for k in members]
    return [(em.load_flax_msgpack(d / f"{sp}.pt"), em.load_flax_msgpack(d / f"{tp}.pt")) for sp, tp in names]


ELITE_LOSS = "next_observation_loss"  # the out-of-bag state loss of <model>_ens_oob.csv


def select_elites(directory: Path, model: str, ensemble_size: int, elites: int) -> list:
    """The ``elites`` of the K models that ``train_env_model.py --ensemble_size K --bootstrap``
    ranks best (PETS / MBPO): the indices with the lowest final out-of-bag state loss in
    ``<directory>/<model>_ens_oob.csv``, best first, ties to the lower index.  ValueError for
    ``elites`` outside 1..K or a CSV that does not list the K models; FileNotFoundError names a
    missing CSV."""
    import csv
    K, E = int(ensemble_size), int(elites)
    if not 1 <= E <= K:
        raise ValueError(f"--env_model_elites must be in 1..{K} (--env_model_ensemble), got {E}")
    path = Path(directory) / f"{model}_ens_oob.csv"
    if not path.exists():
        raise FileNotFoundError(f"{path} not found: train the ensemble with train_env_model.py --ensemble_size "
                                f"{K} --bootstrap")
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    loss = {int(r["model"]): float(r[ELITE_LOSS]) for r in rows if ELITE_LOSS in r}
    if sorted(loss) != list(range(K)):
        raise ValueError(f"{path} does not list the {ELITE_LOSS} of models 0..{K - 1}")
    return sorted(range(K), key=lambda k: (loss[k], k))[:E]


def ensemble_scores(per_model_success, per_model_length, score: str = "mean", mixed=None) -> dict:
    """One member's evaluation entry from its per-model success rates and mean episode
    lengths ([K] each): ``success`` is their mean, their minimum, or (``mixed``: a
    (success rate, mean length) pair) the mixed-mode rate; ``success_std`` (population
    std), ``success_min`` and ``success_max`` are over the K per-model rates.  Scalars only."""
    if score not in ENSEMBLE_SCORES:
        raise ValueError(f"ensemble_score must be one of {ENSEMBLE_SCORES}, got {score!r}")
    rates = [float(v) for v in per_model_success]
    lens = [float(v) for v in per_model_length]
    if score == "mixed":
        if mixed is None:
            raise ValueError("ensemble_score 'mixed' needs the mixed-mode result")
        success, length = float(mixed[0]), float(mixed[1])
    elif score == "min":
        k = int(np.argmin(rates))
        success, length = rates[k], lens[k]
    else:
        success, length = float(np.mean(rates)), float(np.mean(lens))
    return {"success": success, "episode_length": length, "success_std": float(np.std(rates)),
            "success_min": float(np.min(rates)), "success_max": float(np.max(rates))}


class OfflineTaskWithSimulatedEvaluations(Task):
    def __init__(self, env_name: str = "cube-single-play-singletask-task2-v0", model: str = "multistep",
                 save_directory: Path | None = None, dataset: dict | None = None, val_dataset: dict | None = None,
                 n_rows: int = 100_000, n_val_rows: int = 10_000, num_evaluation_envs: int = 50,
                 max_episode_steps: int = 1000, env_model=None, seed: int = 0,
                 initial_observations: Literal["dataset", "model"] = "dataset", initial_observation_model=None,
                 device: int = 0, env_models=None, ensemble_size: int = 0,
                 ensemble_score: Literal["mean", "min", "mixed"] = "mean"):
        if ensemble_score not in ENSEMBLE_SCORES:
            raise ValueError(f"ensemble_score must be one of {ENSEMBLE_SCORES}, got {ensemble_score!r}")
        if initial_observations not in ("dataset", "model"):
            raise ValueError(f"initial_observations must be 'dataset' or 'model', got {initial_observations!r}")
        self.env_name = env_name
        self.model = model
        self.max_episode_steps = int(max_episode_steps)
        self.num_envs = int(num_evaluation_envs)
        obs_dim, action_dim = env_shape(env_name)
        if dataset is None:
            dataset = make_synthetic_dataset(n_rows, obs_dim, action_dim, seed)
            val_dataset = make_synthetic_dataset(n_val_rows, obs_dim, action_dim, seed + 1)
        self.train_dataset = dataset
        self.val_dataset = val_dataset if val_dataset is not None else dataset
        self.obs_dim = self.train_dataset["observations"].shape[-1]
        self.action_dim = self.train_dataset["actions"].shape[-1]
        self.ensemble_score = ensemble_score
        if env_models is None and ensemble_size > 0:
            if save_directory is None:
                raise FileNotFoundError("ensemble_size needs save_directory with the trained ensemble "
                                        "(train_env_model.py --ensemble_size)")
            env_models = load_env_model_ensemble(save_directory, env_name, model, int(ensemble_size))
        self.env_models = None if env_models is None else [tuple(m) for m in env_models]
        if self.env_models is not None:
            if not self.env_models:
                raise ValueError("env_models is empty")
            if env_model is None:
                env_model = self.env_models[0]  # reset / step and the plain rollout: model 0
        if env_model is None and save_directory is not None:
            env_model = load_reference_env_model(save_directory, env_name, model)
        if env_model is None:
            spec = em.EnvModelSpec(self.obs_dim, self.action_dim)
            env_model = (em.init_state_predictor(spec, seed), em.init_termination_predictor(spec, seed + 1))
        self.sp_tree, self.tp_tree = env_model
        self.spec = em.spec_from_trees(self.sp_tree, self.tp_tree)
        if self.env_models is not None:
            for sp, tp in self.env_models:
                if em.spec_from_trees(sp, tp) != self.spec:
                    raise ValueError("the models of an ensemble must share one shape")
        self.initial_observations = self.train_dataset["observations"][::1000]
        self.initial_observation_source = initial_observations
        self._sampler = None
        if initial_observations == "model":
            from envmodel.initial_observation import InitialObservationSampler, load_initial_observation_model
            if initial_observation_model is None:
                if save_directory is None:
                    raise FileNotFoundError("initial_observations='model' needs initial_observation_model=(spec, "
                                            "params) or save_directory with a trained initial_observation model")
                initial_observation_model = load_initial_observation_model(
                    Path(save_directory) / env_name / "env_models")
            io_spec, io_params = initial_observation_model
            if io_spec.obs_dim != self.obs_dim:
                raise ValueError(f"initial-observation model has obs_dim {io_spec.obs_dim}, the task {self.obs_dim}")
            self._sampler = InitialObservationSampler(io_spec, io_params, device=device)
        self._population = None
        self.current_observations = None
        self.episode_steps = 0
        self.invalidate = []

    # ---------------------------------------------------------------- data
    def sample(self, dataset: Literal["train", "val"], batch_size: int):
        data = self.train_dataset if dataset == "train" else self.val_dataset
        idx = np.random.randint(data["observations"].shape[0], size=batch_size)
        return {k: v[idx] for k, v in data.items()}

    def device_datasets(self):
        keys = ("observations", "actions", "rewards", "masks", "next_observations")
        return {"train": {k: self.train_dataset[k] for k in keys},
                "val": {k: self.val_dataset[k] for k in keys}}

    # ---------------------------------------------------- device env model
    def attach(self, population) -> None:
        """Upload the env model into a population's handle (once per handle)."""
        if self._population is population:
            return
        population.set_env_model(em.flatten_state_predictor(self.spec, self.sp_tree),
                                 em.flatten_termination_predictor(self.spec, self.tp_tree),
                                 self.spec.sp_hidden, self.spec.tp_hidden)
        if self.env_models is not None:
            population.set_env_model_ensemble(
                [em.flatten_state_predictor(self.spec, sp) for sp, _ in self.env_models],
                [em.flatten_termination_predictor(self.spec, tp) for _, tp in self.env_models],
                self.spec.sp_hidden, self.spec.tp_hidden)
        self._population = population

    def reset_observations(self, seed: int | None = None) -> np.ndarray:
        if self._sampler is not None:
            # decoder(z), z ~ N(0, 1) keyed by the seed (no seed: a fresh one, as default_rng(None))
            s = int(np.random.SeedSequence().entropy & 0xFFFFFFFFFFFFFFFF) if seed is None else int(seed)
            return self._sampler.sample(self.num_envs, seed=s)
        rng = np.random.default_rng(seed)
        idx = rng.integers(0, self.initial_observations.shape[0], size=self.num_envs)
        return self.initial_observations[idx].astype(np.float32)

    def evaluate_members(self, population, members, seed: int = 0, record: bool = False) -> dict:
        """Success rate of each member in ``members`` (population slots): every
        member's episodes in one GPU launch.  Restores the active mask.  With
        ``record`` each member's entry also holds its ``transitions`` (the reference's
        evaluate_agent second result): (observations [max_steps, n_envs, obs], clipped
        actions [max_steps, n_envs, act]), 0 from an env's episode length on."""
        if self.env_models is not None and not record:
            return self._evaluate_members_ensemble(population, members, seed)
        self.attach(population)
        saved = population.active.copy()
        mask = np.zeros(population.n, dtype=bool)
        mask[list(members)] = True
        population.set_active(mask)
        try:
            res = population.rollout(self.reset_observations(seed), self.max_episode_steps, seed=seed, record=record)
        finally:
            population.set_active(saved)
        success, lengths = res[0], res[1]
        ids = [int(i) for i in np.nonzero(mask)[0]]
        out = {m: {"success": float(success[k].mean()), "episode_length": float(lengths[k].mean())}
               for k, m in enumerate(ids)}
        if record:
            for k, m in enumerate(ids):
                out[m]["transitions"] = (res[2][k], res[3][k])
        return out

    def _evaluate_members_ensemble(self, population, members, seed: int) -> dict:
        """evaluate_members under the ensemble: one per-model launch (and one mixed launch
        for ensemble_score 'mixed'), scalars per member (ensemble_scores)."""
        self.attach(population)
        saved = population.active.copy()
        mask = np.zeros(population.n, dtype=bool)
        mask[list(members)] = True
        population.set_active(mask)
        try:
            obs0 = self.reset_observations(seed)
            success, lengths = population.rollout_ensemble(obs0, self.max_episode_steps, seed=seed, mode="per_model")
            mixed = None
            if self.ensemble_score == "mixed":
                mixed = population.rollout_ensemble(obs0, self.max_episode_steps, seed=seed, mode="mixed")
        finally:
            population.set_active(saved)
        ids = [int(i) for i in np.nonzero(mask)[0]]
        return {m: ensemble_scores([success[k, j].mean() for j in range(success.shape[1])],
                                   [lengths[k, j].mean() for j in range(lengths.shape[1])], self.ensemble_score,
                                   None if mixed is None else (mixed[0][k].mean(), mixed[1][k].mean()))
                for k, m in enumerate(ids)}

    # ------------------------------------------- reference per-step contract
    def reset(self, seed: int | None = None):
        self.current_observations = self.reset_observations(seed)
        self.episode_steps = 0
        self.invalidate = [False] * self.num_envs
        return self.current_observations.copy(), [{} for _ in range(self.num_envs)]

    def step(self, actions):
        if self._population is None:
            raise RuntimeError("attach(population) first: the env model runs on the population's GPU")
        nxt, logits = self._population.envmodel_step(self.current_observations, np.clip(actions, -1, 1))
        terminations = logits > 0
        reward = np.where(terminations, 0, -1)
        self.current_observations = nxt
        self.episode_steps += 1
        truncations = np.full(terminations.shape, self.episode_steps >= self.max_episode_steps)
        infos = [{"success": bool(s)} for s in terminations]
        for i in range(self.num_envs):
            if self.invalidate[i]:
                infos[i]["invalid"] = True
            if terminations[i] or truncations[i]:
                self.invalidate[i] = True
        return nxt.copy(), reward, terminations, truncations, infos

    def close(self):
        self._population = None
        if self._sampler is not None:
            self._sampler.close()
            self._sampler = None
