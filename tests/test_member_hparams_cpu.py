"""CPU side of per-member lr, discount and tau: ExperimentConfig's new fields, the total order
and the evaluation seeds, PopulationBasedTraining's ``explore``, the tune_alpha.py grid, and
the conditions of the trained-like states tests/test_gpu_member_hparams.py starts from.

Everything an old-style config (no lr / discount / tau) gives is compared with LITERALS
recorded from the code before these fields existed, never with a call into the new code."""
import hashlib
import itertools
import json
import os
import pickle
import random

import numpy as np
import pytest

from _helpers import check_member_conditions, trained_member
from member_hparams_cases import ALL_MIXED_SPECS, HPS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cfg(**kw):
    from trainer.config import ExperimentConfig
    return ExperimentConfig(**kw)


OLD = (dict(seed=7, alpha=3.0), dict(seed=None, alpha=54.77), dict(seed=9999, alpha=None), dict())


# ------------------------------------------------------------ ExperimentConfig
def test_experiment_config_defaults_and_hashing():
    from dataclasses import fields
    from trainer.config import ExperimentConfig
    assert [f.name for f in fields(ExperimentConfig)] == ["seed", "alpha", "lr", "discount", "tau"]
    c = ExperimentConfig()
    assert (c.seed, c.alpha, c.lr, c.discount, c.tau) == (None,) * 5
    assert ExperimentConfig(7, 3.0) == ExperimentConfig(seed=7, alpha=3.0, lr=None, discount=None, tau=None)
    a, b = ExperimentConfig(seed=7, alpha=3.0, lr=1e-4), ExperimentConfig(seed=7, alpha=3.0, lr=1e-3)
    assert a != b and a != ExperimentConfig(seed=7, alpha=3.0) and len({a, b, ExperimentConfig(seed=7, alpha=3.0)}) == 3
    assert hash(a) == hash(ExperimentConfig(seed=7, alpha=3.0, lr=1e-4)) and {a: 1}[ExperimentConfig(7, 3.0, 1e-4)] == 1
    with pytest.raises(Exception):
        a.lr = 2.0   # frozen


def test_old_pickles_load():
    """A config pickled before the fields existed has only seed and alpha in its state."""
    from trainer.config import ExperimentConfig
    old = object.__new__(ExperimentConfig)
    object.__setattr__(old, "seed", 7)
    object.__setattr__(old, "alpha", 3.0)
    assert set(vars(old)) == {"seed", "alpha"}
    got = pickle.loads(pickle.dumps(old))
    assert got == ExperimentConfig(seed=7, alpha=3.0) and hash(got) == hash(ExperimentConfig(seed=7, alpha=3.0))
    assert (got.lr, got.discount, got.tau) == (None, None, None)
    new = ExperimentConfig(seed=7, alpha=3.0, tau=0.01)
    assert pickle.loads(pickle.dumps(new)) == new


def test_experiment_names_and_agent_configs():
    from trainer.config import TrainerConfig
    from trainer.experiment import agent_config_for
    names = ["_".join(f"{f}_{v}" for f, v in agent_config_for(TrainerConfig(), _cfg(**kw))[1]) for kw in OLD]
    assert names == ["seed_7_alpha_3.0", "alpha_54.77", "seed_9999", ""]   # recorded before the change
    acfg, tuned = agent_config_for(TrainerConfig(), _cfg(seed=7, alpha=3.0, lr=1e-3, tau=0.05))
    assert tuned == [("seed", 7), ("alpha", 3.0), ("lr", 1e-3), ("tau", 0.05)]
    assert (acfg.lr, acfg.discount, acfg.tau, acfg.alpha) == (1e-3, 0.99, 0.05, 3.0)
    from trainer.trainer import member_hparams_for
    assert member_hparams_for(acfg) == {"lr": 1e-3, "discount": 0.99, "tau": 0.05}


# ------------------------------------------------------- order and eval seeds
def test_config_key_is_a_total_order():
    from fqlpop.distributed import config_key, ordered
    vals = {"alpha": (None, 3.0), "seed": (None, 1), "lr": (None, 1e-4, 1e-3), "discount": (None, 0.9),
            "tau": (None, 0.005, 0.05)}
    cfgs = [_cfg(**dict(zip(vals, v))) for v in itertools.product(*vals.values())]
    keys = [config_key(c) for c in cfgs]
    assert len(set(keys)) == len(cfgs)           # distinct configs never tie
    rng = random.Random(0)
    want = ordered(cfgs)
    for _ in range(3):
        shuffled = cfgs[:]
        rng.shuffle(shuffled)
        assert ordered(shuffled) == want
    # alpha, then seed, then lr, discount, tau; None first
    assert ordered([_cfg(alpha=3.0, lr=1e-3), _cfg(alpha=3.0, lr=1e-4), _cfg(alpha=3.0), _cfg(alpha=1.0, tau=0.5)]) == [
        _cfg(alpha=1.0, tau=0.5), _cfg(alpha=3.0), _cfg(alpha=3.0, lr=1e-4), _cfg(alpha=3.0, lr=1e-3)]
    assert ordered([_cfg(seed=2, alpha=3.0), _cfg(seed=1, alpha=3.0, lr=1.0)])[0] == _cfg(seed=1, alpha=3.0, lr=1.0)
    # old-style configs: the first two components are the key of before (recorded)
    assert [repr(config_key(_cfg(**kw))[:2]) for kw in OLD] == [
        "((1, 3.0), (1, 7.0))", "((1, 54.77), (0, 0.0))", "((0, 0.0), (1, 9999.0))", "((0, 0.0), (0, 0.0))"]
    assert all(config_key(_cfg(**kw))[2:] == ((0, 0.0),) * 3 for kw in OLD)


def test_member_eval_seed_of_old_configs_is_unchanged():
    from fqlpop.distributed import member_eval_seed
    got = [member_eval_seed(5, r, _cfg(**kw)) for r in (0, 3) for kw in OLD]
    assert got == [970236010, 1170973600, 1063797594, 57824865,
                   1894254694, 1027481163, 1799437688, 781949438]   # recorded before the change
    base = member_eval_seed(5, 0, _cfg(seed=7, alpha=3.0))
    seen = {base}
    for kw in (dict(lr=1e-4), dict(lr=1e-3), dict(discount=1e-4), dict(tau=1e-4), dict(lr=1e-4, tau=1e-4)):
        s = member_eval_seed(5, 0, _cfg(seed=7, alpha=3.0, **kw))
        assert s not in seen and 0 <= s < 2**31 - 1
        seen.add(s)


# ------------------------------------------------------------------------ PBT
def _pbt_trace(**kw):
    from fqlpop import distributed as D
    from hpo.pbt import PopulationBasedTraining
    extra = kw.pop("member_fields", {})
    pop = [_cfg(seed=100 + i, alpha=float(a), **extra)
           for i, a in enumerate([3.0, 10.0, 30.0, 100.0, 300.0, 1000.0, 5.0, 50.0])]
    s = PopulationBasedTraining(pop, total_evaluations=100, ready_interval=1, truncation=0.25, seed=3, **kw)
    for r in range(3):
        for c in D.ordered(s.sample()):
            s.update(c, ((c.seed * 7 + r * 13) % 11) / 11.0 + c.alpha * 1e-4)
    return s, D.ordered(s.sample())


# (round, child alpha, child seed, parent alpha, parent seed, parent score) of the six clones of
# _pbt_trace() and the final population, recorded before ``explore`` existed
OLD_LINEAGE = [(0, 800.0, 6061, 1000.0, 105, 0.9181818181818182), (0, 24.0, 9922, 30.0, 102, 0.9120909090909091),
               (1, 3.75, 4249, 3.0, 100, 0.8184818181818182), (1, 2.4000000000000004, 7704, 3.0, 100, 0.8184818181818182),
               (2, 3.0000000000000004, 2467, 2.4000000000000004, 7704, 0.9093309090909091),
               (2, 80.0, 8571, 100.0, 103, 0.9190909090909091)]
OLD_FINAL = [(2.4000000000000004, 7704), (3.0000000000000004, 2467), (5.0, 106), (10.0, 101), (24.0, 9922),
             (80.0, 8571), (100.0, 103), (800.0, 6061)]
OLD_FINAL_BOUNDED = [(4.0, 7704), (5.0, 106), (5.0, 2467), (10.0, 101), (24.0, 9922), (80.0, 8571), (100.0, 103),
                     (500.0, 6061)]
OLD_RNG = "c8b1ab930cf6b11db1a77965ce108500fb3f2ba364c00ad919ec2e6705921a76"
OLD_ROW_KEYS = ["child", "child_alpha", "parent", "parent_alpha", "parent_score", "round"]
OLD_STATE_KEYS = ["candidate_scores", "exploit_rounds", "last_exploit", "lineage", "parent_of",
                  "performed_evaluations", "population", "rng_state"]


def test_pbt_default_explore_reproduces_the_recorded_trace():
    s, final = _pbt_trace()
    assert [(c.alpha, c.seed) for c in final] == OLD_FINAL
    assert all((c.lr, c.discount, c.tau) == (None, None, None) for c in final)
    rows = [(r["round"], r["child"].alpha, r["child"].seed, r["parent"].alpha, r["parent"].seed, r["parent_score"])
            for r in s.lineage]
    assert rows == OLD_LINEAGE
    assert all(sorted(r) == OLD_ROW_KEYS for r in s.lineage)
    assert all(r["parent_alpha"] == r["parent"].alpha and r["child_alpha"] == r["child"].alpha for r in s.lineage)
    assert hashlib.sha256(repr(s.rng.getstate()).encode()).hexdigest() == OLD_RNG
    assert sorted(s.state_dict()) == OLD_STATE_KEYS
    s, final = _pbt_trace(alpha_bounds=(4.0, 500.0))
    assert [(c.alpha, c.seed) for c in final] == OLD_FINAL_BOUNDED
    assert hashlib.sha256(repr(s.rng.getstate()).encode()).hexdigest() == OLD_RNG
    # bounds["alpha"] is alpha_bounds
    assert [(c.alpha, c.seed) for c in _pbt_trace(bounds={"alpha": (4.0, 500.0)})[1]] == OLD_FINAL_BOUNDED


def test_pbt_explores_every_field_deterministically_within_bounds():
    from hpo.pbt import PopulationBasedTraining
    base = {"lr": 3e-4, "discount": 0.99, "tau": 0.005}
    kw = dict(explore=("tau", "alpha", "discount", "lr"), base=base,
              bounds={"lr": (2.5e-4, 3.5e-4), "tau": (None, 0.006), "discount": (0.98, None)})
    s, final = _pbt_trace(**kw)
    s2, final2 = _pbt_trace(**kw)
    assert final == final2 and s.lineage == s2.lineage and s.rng.getstate() == s2.rng.getstate()
    assert s.explore == ("alpha", "lr", "discount", "tau")      # the fixed order, whatever was passed
    assert len(s.lineage) == 6
    f = (0.8, 1.25)
    for row in s.lineage:
        child, parent = row["child"], row["parent"]
        assert sorted(row) == sorted(OLD_ROW_KEYS + [f"{side}_{k}" for k in base for side in ("parent", "child")])
        pv = {k: base[k] if getattr(parent, k) is None else getattr(parent, k) for k in base}
        assert all(row[f"parent_{k}"] == pv[k] and row[f"child_{k}"] == getattr(child, k) for k in base)
        assert child.alpha in [parent.alpha * x for x in f]
        assert child.lr in [min(3.5e-4, max(2.5e-4, pv["lr"] * x)) for x in f]
        assert child.tau in [min(0.006, pv["tau"] * x) for x in f]
        # discount moves through 1 - discount: the horizon 1 / (1 - discount) scales by 1 / factor
        assert child.discount in [max(0.98, 1.0 - (1.0 - pv["discount"]) * x) for x in f]
        assert 2.5e-4 <= child.lr <= 3.5e-4 and child.tau <= 0.006 and 0.98 <= child.discount < 1.0
    first = s.lineage[0]["child"]
    assert first.discount in (1.0 - (1.0 - 0.99) * 0.8, 1.0 - (1.0 - 0.99) * 1.25) and first.discount != 0.99 * 0.8
    # the engine's ranges hold without explicit bounds
    s3, _ = _pbt_trace(explore=("discount", "tau"), perturb_factors=(300.0,), base=base)
    assert all(r["child"].discount == 0.0 and r["child"].tau == 1.0 and r["child"].alpha == r["parent"].alpha
               for r in s3.lineage)
    # a field that is not explored is the parent's
    s4, _ = _pbt_trace(explore=("lr",), base=base, member_fields={"tau": 0.02})
    assert all(r["child"].tau == 0.02 and r["child"].alpha == r["parent"].alpha and r["child"].discount is None
               for r in s4.lineage)
    assert all(sorted(r) == sorted(OLD_ROW_KEYS + ["parent_lr", "child_lr"]) for r in s4.lineage)
    with pytest.raises(ValueError):
        PopulationBasedTraining([_cfg(seed=1, alpha=3.0)], 10, explore=("lr",))       # no default for lr
    with pytest.raises(ValueError):
        PopulationBasedTraining([_cfg(seed=1, alpha=3.0)], 10, explore=("batch_size",))
    PopulationBasedTraining([_cfg(seed=1, alpha=3.0, lr=1e-3)], 10, explore=("lr",))  # every member has one
    with pytest.raises(ValueError):   # two different bounds for alpha
        PopulationBasedTraining([_cfg(seed=1, alpha=3.0)], 10, alpha_bounds=(1.0, 9.0), bounds={"alpha": (2.0, 9.0)})
    both = PopulationBasedTraining([_cfg(seed=1, alpha=3.0)], 10, alpha_bounds=(1.0, 9.0), bounds={"alpha": (1.0, 9.0)})
    assert both.alpha_bounds == both.bounds["alpha"] == (1.0, 9.0)


def test_pbt_state_dict_round_trip_with_explore():
    from hpo.pbt import PopulationBasedTraining
    base = {"lr": 3e-4, "discount": 0.99, "tau": 0.005}
    s, final = _pbt_trace(explore=("alpha", "lr"), base=base)
    sd = pickle.loads(pickle.dumps(s.state_dict()))
    assert sorted(sd) == OLD_STATE_KEYS
    r = PopulationBasedTraining(final, 100, truncation=0.25, seed=99, state_dict=sd, explore=("alpha", "lr"), base=base)
    assert r.lineage == s.lineage and r.rng.getstate() == s.rng.getstate() and r.population == s.population


# ----------------------------------------------------------------- tune_alpha
class _FakeTrainer:
    made = []

    def __init__(self, task, strategy, config, state_dict=None, model_rollouts=None):
        self.strategy = strategy
        _FakeTrainer.made.append(self)

    def train(self, max_evaluations):
        pass

    def state_dict(self):
        return None


def _grid_of(monkeypatch, tmp_path, *argv):
    import tune_alpha
    _FakeTrainer.made = []
    monkeypatch.setattr(tune_alpha, "Trainer", _FakeTrainer)
    monkeypatch.setattr(tune_alpha, "make_task", lambda args, config: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    tune_alpha.main([f"--save_directory={tmp_path}", *argv])
    return list(_FakeTrainer.made[0].strategy.sample())


def test_tune_alpha_grid_and_seeds_without_the_new_flags(monkeypatch, tmp_path):
    ref = json.load(open(os.path.join(GOLDEN, "reference_seeds.json")))
    got = _grid_of(monkeypatch, tmp_path, "--number_of_alphas=4", "--number_of_seeds=2")
    seeds = ref["random_sample_seed0"]["2"]
    random.seed(0)
    assert seeds == random.sample(range(10000), 2)
    alphas = np.logspace(np.log10(3), np.log10(1000), num=4).tolist()
    assert got == [_cfg(seed=s, alpha=a) for a in alphas for s in seeds]      # alpha-major, as before
    assert all(vars(c) == {"seed": c.seed, "alpha": c.alpha, "lr": None, "discount": None, "tau": None} for c in got)


def test_tune_alpha_grid_with_the_new_flags(monkeypatch, tmp_path):
    import tune_alpha
    got = _grid_of(monkeypatch, tmp_path, "--number_of_alphas=2", "--number_of_seeds=2", "--lrs", "1e-4", "1e-3",
                   "--discounts", "0.99", "0.995", "--taus", "0.01")
    random.seed(0)
    seeds = random.sample(range(10000), 2)
    alphas = np.logspace(np.log10(3), np.log10(1000), num=2).tolist()
    want = [_cfg(seed=s, alpha=a, lr=lr, discount=d, tau=0.01)
            for a in alphas for s in seeds for lr in (1e-4, 1e-3) for d in (0.99, 0.995)]
    assert got == want and len(set(got)) == 16
    # --job_id indexes the same list
    seen = []

    class FakeExperiment:
        def __init__(self, task, config, cfg):
            seen.append(cfg)

        def train(self, n):
            return True

        def save_agent(self, checkpoint=False):
            pass

        def stop(self):
            pass
    monkeypatch.setattr(tune_alpha, "Experiment", FakeExperiment)
    tune_alpha.main([f"--save_directory={tmp_path}", "--number_of_alphas=2", "--number_of_seeds=2", "--lrs", "1e-4",
                     "1e-3", "--discounts", "0.99", "0.995", "--taus", "0.01", "--single_experiment", "--job_id=5"])
    tune_alpha.main([f"--save_directory={tmp_path}", "--number_of_alphas=2", "--number_of_seeds=2",
                     "--single_experiment", "--job_id=3"])
    assert seen == [want[5], _cfg(seed=seeds[1], alpha=alphas[1])]


def test_tune_alpha_pbt_flags_reach_the_strategy(monkeypatch, tmp_path):
    _grid_of(monkeypatch, tmp_path, "--number_of_alphas=4", "--strategy=pbt", "--pbt_explore", "lr", "tau",
             "--pbt_lr_min=1e-5", "--pbt_tau_max=0.1", "--agent.lr=1e-3")
    s = _FakeTrainer.made[0].strategy
    assert s.explore == ("lr", "tau") and s.base == {"lr": 1e-3, "discount": 0.99, "tau": 0.005}
    assert s.bounds["lr"] == (1e-5, None) and s.bounds["tau"] == (None, 0.1) and s.bounds["discount"] == (0.0, 1.0)
    _grid_of(monkeypatch, tmp_path, "--number_of_alphas=4", "--strategy=pbt")
    assert _FakeTrainer.made[0].strategy.explore == ("alpha",)


# ------------------------------------------- the GPU file's trained-like states
@pytest.mark.parametrize("spec", ALL_MIXED_SPECS, ids=lambda s: f"h{s.H}_seed{s.seed}")
def test_mixed_specs_meet_the_member_conditions(spec):
    """As tests/test_oracle.py for ALL_TRAINED_SPECS: the float64 oracle alone, under the
    member's own lr, discount and tau, meets every clamp condition in every step."""
    tm = trained_member(spec)
    hp = dict(spec.kw)
    assert hp in list(HPS) and (tm.cfg.lr, tm.cfg.discount, tm.cfg.tau) == (hp["lr"], hp["discount"], hp["tau"])
    check_member_conditions(tm)
