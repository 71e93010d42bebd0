"""Population trainer (reference trainer/trainer.py:11-120).

Same surface and bookkeeping as the reference ``Trainer`` (candidates,
untrained/finished candidates, strategy updates, pruning, resumable
``state_dict``), but every evaluation round trains its candidates TOGETHER:
one HBM-resident population, one set of member-batched HIP launches per
update (the reference trains members one after the other).

Deliberate fix: the strategy is updated with the
candidate's ExperimentConfig, not the Experiment object (the reference passes
``self.experiments[config]`` at trainer/trainer.py:86, which breaks
SuccessiveHalving because ``sample()`` then returns Experiments).

Determinism across world sizes: candidates are visited in ``D.ordered`` order
(the reference iterates a set), and the evaluation of round r is seeded by
``D.eval_round_seed(seed, r)`` (world-model rollouts of the whole round) or
``D.member_eval_seed(seed, r, config)`` (per-experiment evaluation), never by the
global np.random stream.  So ``Trainer`` and ``DistributedTrainer`` at any world
size score every member identically and take the same decisions.
"""
from __future__ import annotations

import random
import time
from pathlib import Path

import numpy as np

from fqlpop import Population, PopulationConfig
from fqlpop import distributed as D
from hpo.strategy import HpoStrategy
from task.online_envs import online_envs_of
from task.task import Task
from trainer.config import ModelRolloutConfig, OnlineConfig, TrainerConfig
from trainer.experiment import Experiment, agent_config_for, train_population
from dataclasses import asdict

PBT_DISTRIBUTED_MSG = ("strategies that clone members (parent_of: PopulationBasedTraining) run on one GPU only: "
                       "cross-rank exploit is not implemented; run tune_alpha.py --strategy pbt without "
                       "torch.distributed.run (WORLD_SIZE = 1)")
MODEL_ROLLOUT_DISTRIBUTED_MSG = ("training on world-model branches (--model_rollout_branches) runs on one GPU only: "
                                 "a member's ring of synthetic transitions lives on its GPU and is not moved "
                                 "when pruning rebalances members between ranks; run tune_alpha.py without "
                                 "torch.distributed.run (WORLD_SIZE = 1)")
MODEL_ROLLOUT_TASK_MSG = ("training on world-model branches (--model_rollout_branches) needs a task that can attach "
                          "an env model to the population: OfflineTaskWithSimulatedEvaluations (--task simulated); "
                          "got {task}")
MODEL_ROLLOUT_ENSEMBLE_MSG = ("branches under the env-model ensemble (--model_rollout_ensemble) need a task with an "
                              "ensemble: OfflineTaskWithSimulatedEvaluations(env_models=... or ensemble_size=K) "
                              "(--env_model_ensemble K); this task has one env model")
ONLINE_ROLLOUT_MSG = ("an online phase (--online_steps) and training on world-model branches "
                      "(--model_rollout_branches) both write the members' rings: one ring, two writers; choose one")
ONLINE_CLONE_MSG = ("an online phase (--online_steps) does not run under strategies that clone members (parent_of: "
                    "PopulationBasedTraining): a clone's environments would not follow its parent's; use --strategy "
                    "identity or successive_halving")
ONLINE_DISTRIBUTED_MSG = ("an online phase (--online_steps) runs on one GPU only: a member's environments and ring "
                          "are not moved when pruning rebalances members between ranks; run tune_alpha.py without "
                          "torch.distributed.run (WORLD_SIZE = 1)")
LINEAGE_COLUMNS = ("round", "step", "child", "parent", "parent_alpha", "child_alpha", "parent_score")


def member_hparams_for(acfg) -> dict:
    """The per-member engine hyper-parameters of an AgentConfig (Population.set_member_hparams)."""
    return {"lr": float(acfg.lr), "discount": float(acfg.discount), "tau": float(acfg.tau)}


def collect_number(step: int, mr: ModelRolloutConfig) -> int:
    """Which collect of its group the one after update ``step`` (a multiple of ``mr.interval``,
    at least ``mr.warmup``) is, from 0: k - k0 with step = k * interval and k0 the first
    multiple that collects.  The running count of a group that trains in lock step."""
    first = max(1, -(-mr.warmup // mr.interval))
    return step // mr.interval - first


class Trainer:
    _clones = False  # (DistributedTrainer refuses cloning strategies)

    def __init__(self, task: Task, strategy: HpoStrategy, config: TrainerConfig, state_dict: dict | None = None,
                 device: int = 0, model_rollouts: ModelRolloutConfig | None = None,
                 online: OnlineConfig | None = None):
        self.task = task
        self.strategy = strategy
        self.config = config
        self.experiments = {}
        self.member_of = {}
        # offline-to-online fine-tuning: off (and nothing below differs) unless steps > 0
        self.online = online if online is not None else OnlineConfig()
        self.online_envs = None
        self.online_env_steps = int(state_dict.get("online", {}).get("env_steps", 0)) if state_dict else 0
        if self.online.enabled:  # refused before any GPU call
            self.online.validate()
            if model_rollouts is not None and model_rollouts.enabled:
                raise ValueError(ONLINE_ROLLOUT_MSG)
            if hasattr(strategy, "parent_of"):
                raise ValueError(ONLINE_CLONE_MSG)
            if not hasattr(task, "online_envs"):
                online_envs_of(task, 0, 0, 0)  # raises: the task offers no online environments
            if task.device_datasets() is None:
                raise ValueError("an online phase (--online_steps) needs a task whose dataset the population "
                                 "samples on the device (Task.device_datasets)")
        # training on world-model branches: off (and nothing below differs) unless branches > 0
        self.model_rollouts = model_rollouts if model_rollouts is not None else ModelRolloutConfig()
        self.collect_index = int(state_dict.get("collect_index", 0)) if state_dict else 0
        if self.model_rollouts.enabled:  # refused before any GPU call
            from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
            if not isinstance(task, OfflineTaskWithSimulatedEvaluations):
                raise ValueError(MODEL_ROLLOUT_TASK_MSG.format(task=type(task).__name__))
            self.model_rollouts.validate()
            if self.model_rollouts.ensemble and task.env_models is None:
                raise ValueError(MODEL_ROLLOUT_ENSEMBLE_MSG)
        # a strategy that exposes parent_of (PopulationBasedTraining) refills the slots of the
        # candidates it drops with clones of others; everything below keyed on _clones is new
        # ground, and Identity / SuccessiveHalving runs take none of it
        self._clones = hasattr(strategy, "parent_of")
        self.retired_experiments = list(state_dict.get("retired", [])) if state_dict else []
        self.lineage = list(state_dict.get("lineage", [])) if state_dict else []
        # strategy.sample() is called once on a fresh start (trainer/trainer.py:37-40 of the
        # reference): the same set sizes the population and becomes the candidates, so a
        # strategy whose sample() is stateful or random places the configs it returned
        sampled = None if state_dict else strategy.sample()
        initial = list(state_dict["experiments"]) if state_dict else list(sampled)
        self.population = self._make_population(initial, device)
        if self.online.enabled:
            self.online_envs = online_envs_of(task, self.population.n, self.online.envs,
                                              D.online_seed(config.seed))
            if state_dict is not None and "envs" in state_dict.get("online", {}):
                self.online_envs.load_state_dict(state_dict["online"]["envs"])
        if state_dict is not None:
            for cfg, exp_state in state_dict["experiments"].items():
                self.create_experiment(cfg, state_dict=exp_state)
            self.candidates = state_dict["candidates"]
            self.untrained_candidates = state_dict["untrained_candidates"]
            self.finished_candidates = state_dict["finished_candidates"]
            random.setstate(state_dict["random_rng_state"])
            np.random.set_state(state_dict["np_rng_state"])
            self.round_index = int(state_dict.get("round_index", 0))
        else:
            self.round_index = 0
            self.untrained_candidates = []
            self.finished_candidates = []
            self.candidates = sampled
            for cfg in self.candidates:
                self.create_experiment(cfg)

    # ----------------------------------------------------------- population
    def _make_population(self, configs, device):
        example = self.task.sample("train", 1)
        alphas, seeds, hparams = [], [], []
        for cfg in configs:
            acfg, _ = agent_config_for(self.config, cfg)
            alphas.append(acfg.alpha)
            seeds.append(acfg.seed if cfg.seed is None else cfg.seed)
            hparams.append(member_hparams_for(acfg))
        # the shared fields (widths, batch size, ...) come from the first config; lr, discount
        # and tau are per member, each from its own AgentConfig
        acfg, _ = agent_config_for(self.config, configs[0])
        pcfg = PopulationConfig.from_agent_config(asdict(acfg), example["observations"].shape[-1],
                                                  example["actions"].shape[-1])
        pop = Population(pcfg, alphas, seeds, device=device, hparams=hparams)
        dd = self.task.device_datasets()
        if dd is not None:
            pop.set_dataset(dd["train"], "train")
            pop.set_dataset(dd["val"], "val")
        self._free_slots = list(range(len(configs)))
        if self.model_rollouts.enabled:
            # the rings start empty: until a member's first collect its minibatches are offline
            # rows only.  On a resumed run each Experiment puts its member's ring back from its
            # state dict ("synth_ring"), so the run continues as if it had not stopped
            self.task.attach(pop)
            pop.synth_create(self.model_rollouts.buffer_rows)
            pop.set_real_ratio(self.model_rollouts.real_ratio)
        if self.online.enabled:
            # the rings start empty and real_ratio at 1: the offline updates draw offline rows
            # only.  A resumed run's Experiments put their rings back ("synth_ring")
            pop.synth_create(self.online.buffer_rows)
        return pop

    def _slot_for(self, cfg) -> int:
        if cfg in self.member_of:
            return self.member_of[cfg]
        if not self._free_slots:
            raise RuntimeError("population is full: every slot holds a candidate")
        slot = self._free_slots.pop(0)
        acfg, _ = agent_config_for(self.config, cfg)
        self.population.set_member(slot, acfg.alpha, acfg.seed if cfg.seed is None else cfg.seed, reinit=True)
        self.population.set_member_hparams(slot, **member_hparams_for(acfg))  # (set_member keeps the slot's)
        self.member_of[cfg] = slot
        return slot

    def create_experiment(self, experiment_config, **kwargs) -> Experiment:
        slot = self._slot_for(experiment_config)
        exp = Experiment(self.task, self.config, experiment_config, population=self.population, member=slot,
                         **kwargs)
        self.experiments[experiment_config] = exp
        return exp

    def state_dict(self) -> dict:
        sd = self._base_state_dict()
        if self._clones:
            # retired experiments are not under "experiments": a resumed trainer allocates
            # exactly len(candidates) slots
            sd["retired"] = list(self.retired_experiments)
            sd["lineage"] = list(self.lineage)
        if self.model_rollouts.enabled:
            sd["collect_index"] = self.collect_index
        if self.online.enabled:
            sd["online"] = {"env_steps": self.online_env_steps, "envs": self.online_envs.state_dict()}
        return sd

    def _base_state_dict(self) -> dict:
        return {
            "experiments": {cfg: exp.state_dict() for cfg, exp in self.experiments.items()},
            "candidates": self.candidates,
            "random_rng_state": random.getstate(),
            "np_rng_state": np.random.get_state(),
            "untrained_candidates": self.untrained_candidates,
            "finished_candidates": self.finished_candidates,
            "round_index": self.round_index,
        }

    # ---------------------------------------------------------------- train
    def _train_round(self, configs):
        """eval_interval updates of every config, in lock-step groups by step."""
        groups = {}
        for cfg in configs:
            exp = self.experiments[cfg]
            groups.setdefault(exp.current_step, []).append(exp)
        for step, exps in groups.items():
            n = min(self.config.eval_interval, self.config.steps - step)
            if exps[0].on_device and self.online.enabled and step + n > self.online_start:
                offline = max(0, self.online_start - step)
                train_population(exps, offline)
                self._train_online(exps, n - offline)
            elif exps[0].on_device and self.model_rollouts.enabled:
                self._train_with_rollouts(exps, n)
            elif exps[0].on_device:
                train_population(exps, n)
            else:
                for e in exps:
                    e.train(self.config.eval_interval)

    def _train_with_rollouts(self, exps, n: int) -> None:
        """``n`` updates of one lock-step group in chunks that end at the multiples of
        ``model_rollouts.interval``; after each such chunk, from ``warmup`` updates on, every
        member of the group rolls its branches into its ring (one ``Population.collect``,
        stream-ordered between the steps: no synchronisation).  The collect after the run's
        last update is skipped: nothing would train on it.

        A collect is seeded by the update it follows: the one after update k * interval is
        number k - k0 of its group, k0 the first multiple that collects.  While all candidates
        train in lock step that is the running ``collect_index``; a candidate that
        ``max_evaluations`` defers to a later round or invocation gets the seeds it would have
        had in lock step, so a run does not depend on how it was cut into invocations.
        ``collect_index`` still counts the collects done (it is saved with the state)."""
        mr = self.model_rollouts
        cur, target = exps[0].current_step, exps[0].current_step + n
        while cur < target:
            nxt = min(target, (cur // mr.interval + 1) * mr.interval)
            train_population(exps, nxt - cur)  # (leaves exactly this group active)
            cur = nxt
            if cur % mr.interval == 0 and cur >= mr.warmup and cur < self.config.steps:
                self.population.collect(mr.branches, mr.horizon,
                                        D.collect_seed(self.config.seed, collect_number(cur, mr)),
                                        ensemble=mr.ensemble, penalty=mr.penalty)
                self.collect_index += 1

    @property
    def online_start(self) -> int:
        """The update the online phase begins after: the last ``online.steps`` are online."""
        return max(0, self.config.steps - self.online.steps)

    def _train_online(self, exps, n: int) -> None:
        """``n`` online updates of one lock-step group.  Before every ``utd``-th update (counted
        from the start of the online phase) the group takes one environment step: one
        ``Population.act`` on the members' current observations (noise drawn on the device at
        t = the group's environment-step count, from 1, under ``D.online_seed``), one step of
        their environments, one ``synth_append_active`` of the observed transitions (masks =
        1 - terminated, the environment's reward) and the real_ratio for the rings' new
        size; then up to ``utd`` updates.  The environment-step count follows from the
        group's update count, so a run does not depend on how it was cut into invocations."""
        on, pop, envs = self.online, self.population, self.online_envs
        members = [e.agent.member for e in exps]
        if sorted(members) != members:
            exps = sorted(exps, key=lambda e: e.agent.member)
            members = [e.agent.member for e in exps]
        mask = [False] * pop.n
        for m in members:
            mask[m] = True
        n_offline = int(self.task.device_datasets()["train"]["observations"].shape[0])
        seed = D.online_seed(self.config.seed)
        cur, target = exps[0].current_step, exps[0].current_step + n
        # (a resumed run, or another group's turn: the ratio that belongs to these rings)
        pop.set_real_ratio(on.ratio(n_offline, int(pop.synth_rows_host[members[0]])))
        while cur < target:
            done = cur - self.online_start  # online updates so far
            if done % on.utd == 0:
                pop.set_active(mask)
                obs = envs.observations[members]
                actions = pop.act(obs, seed=seed, t=done // on.utd + 1)
                nxt, rew, term, _ = envs.step(actions, members)
                pop.synth_append_active({"observations": obs, "actions": actions, "rewards": rew,
                                         "masks": (1.0 - term).astype(np.float32), "next_observations": nxt})
                pop.set_real_ratio(on.ratio(n_offline, int(pop.synth_rows_host[members[0]])))
                self.online_env_steps += 1
            k = min(on.utd - done % on.utd, target - cur)
            train_population(exps, k)
            cur += k

    def _evaluate_round(self, configs) -> dict:
        """World-model tasks: every candidate of the round in one GPU rollout
        (slot -> eval info); other tasks evaluate per experiment."""
        if not hasattr(self.task, "evaluate_members"):
            return {}
        members = [self.member_of[cfg] for cfg in configs if cfg in self.member_of]
        if not members:
            return {}
        return self.task.evaluate_members(self.population, members,
                                          D.eval_round_seed(self.config.seed, self.round_index))

    def _score(self, cfg, round_eval: dict) -> float:
        """The candidate's evaluation of this round: the round's world-model result, or
        its own evaluation seeded by (run seed, round, candidate)."""
        info = round_eval.get(self.member_of.get(cfg))
        seed = None if info is not None else D.member_eval_seed(self.config.seed, self.round_index, cfg)
        return self.experiments[cfg].evaluate(info, seed=seed)

    def train(self, max_evaluations: int) -> None:
        while max_evaluations > 0:
            queue = list(self.untrained_candidates) if self.untrained_candidates else D.ordered(self.candidates)
            this_round, deferred = queue[:max_evaluations], queue[max_evaluations:]
            start = time.perf_counter()
            self._train_round(this_round)
            round_eval = self._evaluate_round(this_round)
            for cfg in this_round:
                exp = self.experiments[cfg]
                if exp.current_step == exp.steps and cfg not in self.finished_candidates:
                    exp.save_agent()
                    self.finished_candidates.append(cfg)
                self.strategy.update(cfg, self._score(cfg, round_eval))
                max_evaluations -= 1
            self.round_index += 1
            print(f"Elapsed time: {time.perf_counter() - start:.6f} seconds ({len(this_round)} candidates)")
            if deferred:
                self.untrained_candidates = deferred
                break
            self.untrained_candidates = []
            if all(cfg in self.finished_candidates for cfg in self.candidates):
                break
            new_candidates = self.strategy.sample()
            if self._clones:
                self._exploit(new_candidates)
            else:
                for cfg in new_candidates:
                    if cfg not in self.experiments:
                        self.create_experiment(cfg)
                for cfg in self.candidates:
                    if cfg not in new_candidates:
                        self.experiments[cfg].stop()
            self.candidates = new_candidates
        for exp in self.experiments.values():
            exp.stop()
        if self._clones:
            self._write_lineage()

    # ------------------------------------------------- exploit (strategies with parent_of)
    def _retire(self, cfg) -> None:
        """Stop a candidate the strategy dropped and give its slot back."""
        exp = self.experiments.pop(cfg)
        exp.stop()
        self.retired_experiments.append({"experiment_name": exp.experiment_name, "current_step": exp.current_step,
                                         "logger": exp.logger.state_dict()})
        self._free_slots.append(self.member_of.pop(cfg))

    def _exploit(self, new_candidates) -> None:
        """Candidates that dropped out free their slots; each new candidate with a parent
        takes a freed slot and the parent's complete training state, all of the round in ONE
        on-device ``clone_members`` call, and continues from the parent's step in lock-step
        with it."""
        for cfg in D.ordered(self.candidates):
            if cfg not in new_candidates:
                self._retire(cfg)
        pairs = []
        for cfg in D.ordered(new_candidates):
            if cfg in self.experiments:
                continue
            parent = self.strategy.parent_of.get(cfg)
            if parent not in self.experiments:
                self.create_experiment(cfg)  # no live parent: a fresh member
                continue
            if not self._free_slots:
                raise RuntimeError("population is full: every slot holds a candidate")
            pairs.append((cfg, parent, self._free_slots.pop(0)))
        if not pairs:
            return
        alphas, seeds, hparams = [], [], []
        for cfg, _, _ in pairs:
            acfg, _ = agent_config_for(self.config, cfg)
            alphas.append(acfg.alpha)
            seeds.append(acfg.seed if cfg.seed is None else cfg.seed)
            hparams.append(member_hparams_for(acfg))
        # the clone hands the child its parent's lr, discount and tau; its own follow
        self.population.clone_members([self.member_of[p] for _, p, _ in pairs], [s for _, _, s in pairs],
                                      alphas=alphas, seeds=seeds, hparams=hparams)
        self.population.sync()
        rows = {row["child"]: row for row in getattr(self.strategy, "lineage", [])}
        for cfg, parent, slot in pairs:
            pexp = self.experiments[parent]
            self.member_of[cfg] = slot
            exp = Experiment(self.task, self.config, cfg, population=self.population, member=slot,
                             start_step=pexp.current_step)
            self.experiments[cfg] = exp
            row = rows.get(cfg, {})
            self.lineage.append({"round": row.get("round", self.round_index), "step": pexp.current_step,
                                 "child": exp.experiment_name, "parent": pexp.experiment_name,
                                 "parent_alpha": parent.alpha, "child_alpha": cfg.alpha,
                                 "parent_score": row.get("parent_score", "")})
            for k in self._extra_lineage_columns():
                self.lineage[-1][k] = row.get(k, "")

    def _extra_lineage_columns(self) -> tuple:
        """parent_<f> / child_<f> of the fields beyond alpha that the strategy explores."""
        extra = [f for f in getattr(self.strategy, "explore", ()) if f != "alpha"]
        return tuple(f"{side}_{f}" for f in extra for side in ("parent", "child"))

    def _write_lineage(self) -> None:
        path = Path(self.config.save_directory) / self.config.env_name / "pbt_lineage.csv"
        path.parent.mkdir(parents=True, exist_ok=True)
        columns = LINEAGE_COLUMNS + self._extra_lineage_columns()
        with open(path, "w") as f:
            f.write(",".join(columns) + "\n")
            for row in self.lineage:
                f.write(",".join(str(row.get(k, "")) for k in columns) + "\n")
