"""GPU tests of population-based training end to end: Trainer with PopulationBasedTraining
(on-device clones into freed slots, lock-step continuation, lineage), the tune_alpha.py
driver with --strategy pbt (run and resume), and the single-GPU restriction.  The per-layer
config of test_gpu_surface.py (hidden (64,) x 4, B = 64), OfflineTaskSynthetic, tmp dirs."""
import csv
import pickle

import numpy as np
import pytest

from oracle import fql_oracle as O

pytestmark = pytest.mark.gpu
ENV = "cube-single-play-singletask-task2-v0"
SMALL = "(64, 64, 64, 64)"


def _trainer_config(tmp_path, steps=40, eval_interval=10, log_interval=5):
    from trainer.config import AgentConfig, TrainerConfig
    return TrainerConfig(steps=steps, eval_interval=eval_interval, log_interval=log_interval,
                         save_directory=tmp_path, env_name=ENV,
                         agent=AgentConfig(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4,
                                           batch_size=64))


def _configs():
    from trainer.config import ExperimentConfig
    return [ExperimentConfig(seed=s, alpha=a) for a, s in [(3.0, 1), (30.0, 2), (300.0, 3), (1000.0, 4)]]


def _task():
    from task.offline_task_synthetic import OfflineTaskSynthetic
    return OfflineTaskSynthetic(n_rows=20_000, n_val_rows=2_000, num_evaluation_envs=4, max_episode_steps=8)


def _recording_strategy(configs):
    from hpo.pbt import PopulationBasedTraining

    class Recording(PopulationBasedTraining):
        sizes = []

        def sample(self):
            out = super().sample()
            self.sizes.append(len(out))
            return out
    return Recording(set(configs), total_evaluations=0, truncation=0.25, seed=1)


def test_trainer_keeps_the_population_full(tmp_path):
    from trainer.trainer import Trainer
    cfg = _trainer_config(tmp_path)
    configs = _configs()
    strategy = _recording_strategy(configs)
    trainer = Trainer(_task(), strategy, cfg)
    trainer.train(max_evaluations=100)
    assert strategy.sizes and all(n == 4 for n in strategy.sizes)
    assert len(trainer.candidates) == 4 and trainer.population.n == 4
    assert len(trainer.experiments) == 4 and sorted(trainer.member_of.values()) == [0, 1, 2, 3]
    n_clones = len(strategy.lineage)
    assert n_clones >= 1 and len(trainer.retired_experiments) == n_clones
    root = tmp_path / ENV
    for c in trainer.candidates:
        exp = trainer.experiments[c]
        assert exp.current_step == cfg.steps and c in trainer.finished_candidates
        assert (root / exp.experiment_name / "params.pkl").exists()
    with open(root / "pbt_lineage.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == n_clones
    assert list(rows[0]) == ["round", "step", "child", "parent", "parent_alpha", "child_alpha", "parent_score"]
    names = set()
    for row in rows:
        assert (root / row["child"]).is_dir() and (root / row["parent"]).is_dir()
        assert row["child"] != row["parent"] and row["child"] not in names
        names.add(row["child"])
        birth = int(row["step"])
        assert 0 < birth < cfg.steps and birth % cfg.eval_interval == 0
        assert float(row["child_alpha"]) in (float(row["parent_alpha"]) * 0.8, float(row["parent_alpha"]) * 1.25)
        with open(root / row["child"] / "train.csv") as f:
            train_rows = list(csv.DictReader(f))
        # a child logs from its birth step on (a child that was itself replaced before its
        # first log_interval has no row)
        assert all(int(r["step"]) > birth for r in train_rows)
        if train_rows:
            assert int(train_rows[0]["step"]) == birth + cfg.log_interval
    # every retired experiment left the trainer's live set, and its name is not a live one
    live = {e.experiment_name for e in trainer.experiments.values()}
    assert all(r["experiment_name"] not in live for r in trainer.retired_experiments)
    sd = trainer.state_dict()
    assert len(sd["experiments"]) == 4 and len(sd["retired"]) == n_clones


def test_child_equals_parent_at_the_clone(tmp_path):
    from fql.utils.serialization import params_of
    from trainer.trainer import Trainer
    cfg = _trainer_config(tmp_path, steps=20, eval_interval=10, log_interval=5)
    strategy = _recording_strategy(_configs())
    seen = []

    class Checking(Trainer):
        def _exploit(self, new_candidates):
            known = set(self.experiments)
            super()._exploit(new_candidates)
            for c in set(self.experiments) - known:
                parent = self.strategy.parent_of[c]
                child_exp, parent_exp = self.experiments[c], self.experiments[parent]
                a, b = (params_of(e.agent.to_state_dict()) for e in (child_exp, parent_exp))
                for net in O.NETS:
                    for leaf in a[net]:
                        assert np.array_equal(a[net][leaf].view(np.uint32), b[net][leaf].view(np.uint32)), (net, leaf)
                assert child_exp.agent.step == parent_exp.agent.step == parent_exp.current_step
                assert child_exp.current_step == parent_exp.current_step
                assert child_exp.experiment_name != parent_exp.experiment_name
                m = child_exp.agent.member
                assert float(self.population.alphas[m]) == np.float32(c.alpha) and int(self.population.seeds[m]) == c.seed
                seen.append(c)
    trainer = Checking(_task(), strategy, cfg)
    trainer.train(max_evaluations=100)
    assert len(seen) == 1 and seen[0] in trainer.candidates


def test_tune_alpha_pbt_run_and_resume(tmp_path, monkeypatch):
    import tune_alpha
    from trainer.trainer import Trainer
    made = []

    class Recording(Trainer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(tune_alpha, "Trainer", Recording)
    args = [f"--save_directory={tmp_path}", "--steps=20", "--eval_interval=10", "--log_interval=10",
            f"--agent.actor_hidden_dims={SMALL}", f"--agent.value_hidden_dims={SMALL}",
            "--agent.batch_size=64", "--agent.layer_norm", "--eval_episodes=4", "--synthetic_rows=5000",
            "--number_of_alphas=4", "--number_of_seeds=1", "--max_evaluations=100", "--strategy=pbt",
            "--pbt_alpha_min=1.0", "--pbt_alpha_max=2000.0"]
    tune_alpha.main(args)
    ckpt = tmp_path / ENV / "checkpoint.pkl"
    with open(ckpt, "rb") as f:
        state = pickle.load(f)
    assert len(state["trainer"]["experiments"]) == 4
    assert len(state["trainer"]["retired"]) == 1 and len(state["strategy"]["lineage"]) == 1
    assert {"experiment_name", "current_step", "logger"} <= set(state["trainer"]["retired"][0])
    assert all(e["current_step"] == 20 for e in state["trainer"]["experiments"].values())
    tune_alpha.main(args)  # resume
    assert len(made) == 2
    resumed = made[1]
    assert resumed.population.n == 4 and len(resumed.experiments) == 4
    assert len(resumed.retired_experiments) == 1
    assert set(resumed.candidates) == set(state["trainer"]["candidates"])
    with open(ckpt, "rb") as f:
        again = pickle.load(f)
    assert len(again["trainer"]["experiments"]) == 4 and len(again["trainer"]["retired"]) == 1
    assert len((tmp_path / ENV / "pbt_lineage.csv").read_text().strip().splitlines()) == 2


def test_pbt_is_single_gpu_only(tmp_path, monkeypatch):
    import tune_alpha
    from hpo.pbt import PopulationBasedTraining
    from trainer.distributed_trainer import DistributedTrainer
    strategy = PopulationBasedTraining(set(_configs()), total_evaluations=0)
    with pytest.raises(NotImplementedError, match="one GPU only"):
        DistributedTrainer(None, strategy, _trainer_config(tmp_path))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU only"):
        tune_alpha.main([f"--save_directory={tmp_path}", "--strategy=pbt", "--number_of_alphas=4"])
    assert not (tmp_path / ENV).exists()
