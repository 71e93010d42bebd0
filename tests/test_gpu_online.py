"""The online phase: ``Population.synth_append_active`` against per-member appends, and
``Trainer``'s act -> env step -> append -> update loop on the toy reach environments
(H = 64, B = 64, 3 members, 4 envs, rings of 64 rows).
"""
from __future__ import annotations

import pickle

import numpy as np
import pytest

import act_np as N
import synth_np as S
from oracle import fql_oracle as O

pytestmark = pytest.mark.gpu

H, B, D, A = 64, 64, 28, 5
MEMBERS, ENVS, CAP = 3, 4, 64
ENV = "cube-single-play-singletask-task2-v0"
SMALL = "(64,64,64,64)"


def _pop():
    from fqlpop import Population, PopulationConfig
    pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * 4, batch_size=B),
                     [3.0, 30.0, 300.0], [1, 2, 3])
    cfg = O.OracleConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * 4, batch_size=B)
    for i in range(MEMBERS):
        pop.set_params(i, O.cast_tree(O.init_params(cfg, 40 + i), np.float32))
    pop.synth_create(CAP)
    return pop


def _rows(rng, nz, n):
    return {"observations": rng.standard_normal((nz, n, D)).astype(np.float32),
            "actions": rng.uniform(-1, 1, (nz, n, A)).astype(np.float32),
            "rewards": rng.uniform(-1, 0, (nz, n)).astype(np.float32),
            "masks": (rng.uniform(size=(nz, n)) < 0.9).astype(np.float32),
            "next_observations": rng.standard_normal((nz, n, D)).astype(np.float32)}


def _assert_rings_equal(a, b, tag):
    for m in range(MEMBERS):
        assert a.synth_info(m) == b.synth_info(m), f"{tag}: member {m} counters"
        ra, rb = a.synth_read(m), b.synth_read(m)
        for k in S.FIELDS:
            assert ra[k].tobytes() == rb[k].tobytes(), f"{tag}: member {m} {k}"


def test_append_active_equals_member_appends():
    """One call for the active members against one ``synth_append`` each on a twin: rings and
    counters byte-equal, through a wrap past the capacity and with a member inactive."""
    one, each = _pop(), _pop()
    rng = np.random.default_rng(3)
    # 24 + 24 + 24 rows wrap a 64-row ring; then the middle member sits out; then all again
    for step, (active, n) in enumerate([([0, 1, 2], 24), ([0, 1, 2], 24), ([0, 1, 2], 24), ([0, 2], 40),
                                        ([0, 1, 2], 7), ([1], CAP)]):
        mask = [m in active for m in range(MEMBERS)]
        one.set_active(mask)
        each.set_active(mask)
        rows = _rows(rng, len(active), n)
        one.synth_append_active(rows)
        for z, m in enumerate(active):
            each.synth_append(m, {k: v[z] for k, v in rows.items()})
        _assert_rings_equal(one, each, f"call {step}")
        assert list(one.synth_rows_host) == [one.synth_info(m)["rows"] for m in range(MEMBERS)]
    assert one.synth_info(1)["appended"] == 24 * 3 + 7 + CAP and one.synth_info(0)["appended"] == 24 * 3 + 40 + 7
    one.close()
    each.close()


def _trainer_config(tmp_path, steps=12, eval_interval=12):
    from trainer.config import AgentConfig, TrainerConfig
    return TrainerConfig(steps=steps, eval_interval=eval_interval, log_interval=6, save_directory=tmp_path, env_name=ENV,
                         agent=AgentConfig(actor_hidden_dims=(H,) * 4, value_hidden_dims=(H,) * 4, batch_size=B))


def _task():
    from task.offline_task_synthetic import OfflineTaskSynthetic
    return OfflineTaskSynthetic(n_rows=5_000, n_val_rows=1_000, num_evaluation_envs=4, max_episode_steps=8)


def _configs():
    from trainer.config import ExperimentConfig
    return [ExperimentConfig(seed=s, alpha=a) for a, s in [(3.0, 1), (30.0, 2), (300.0, 3)]]


def _online(steps=12):
    from trainer.config import OnlineConfig
    return OnlineConfig(steps=steps, envs=ENVS, utd=1, buffer_rows=CAP)


def _run_identity(tmp_path):
    from hpo.identity import Identity
    from trainer.trainer import Trainer
    trainer = Trainer(_task(), Identity(population=_configs(), total_evaluations=0), _trainer_config(tmp_path),
                      online=_online())
    trainer.train(max_evaluations=100)
    return trainer


def _member_state(pop, m):
    from fqlpop._lib import STATE_ADAM_M, STATE_ADAM_V, STATE_PARAMS
    return [pop.get_flat(m, w).tobytes() for w in (STATE_PARAMS, STATE_ADAM_M, STATE_ADAM_V)]


def test_online_loop_fills_the_rings_with_the_envs_transitions(tmp_path):
    from fqlpop import distributed as Dist
    first = _run_identity(tmp_path / "a")
    pop = first.population
    task = _task()
    envs = task.online_envs(MEMBERS, ENVS, Dist.online_seed(0))
    rings = [pop.synth_read(m) for m in range(MEMBERS)]
    for m in range(MEMBERS):
        assert pop.synth_info(m) == {"rows": 12 * ENVS, "head": 12 * ENVS, "appended": 12 * ENVS}
        assert pop.get_count(m) == 12
    n_term = 0
    for t in range(12):  # a host copy of the environments, stepped with the rings' stored actions
        sl = slice(t * ENVS, (t + 1) * ENVS)
        obs = envs.observations
        act = np.stack([rings[m]["actions"][sl] for m in range(MEMBERS)])
        assert np.all(np.abs(act) <= 1.0)
        nxt, rew, term, _ = envs.step(act)
        for m in range(MEMBERS):
            r = rings[m]
            assert np.array_equal(r["observations"][sl], obs[m]), f"member {m} step {t}: observations"
            assert np.array_equal(r["next_observations"][sl], nxt[m]), f"member {m} step {t}: next observations"
            assert np.array_equal(r["rewards"][sl], rew[m]) and np.array_equal(r["masks"][sl], 1.0 - term[m])
            want = N.reach_step(obs[m], act[m], A)   # the dynamics, restated
            assert np.array_equal(want[0], nxt[m]) and np.array_equal(want[1], rew[m])
        n_term += int(term.sum())
    print(f"terminated transitions: {n_term} of {12 * ENVS * MEMBERS}; truncations reset after 8 steps")
    assert first.online_env_steps == 12
    # the stored actions are act's: the last step's, from the final parameters' predecessor, cannot be
    # re-run, but two identical runs agree byte for byte
    second = _run_identity(tmp_path / "b")
    for m in range(MEMBERS):
        again = second.population.synth_read(m)
        for k in S.FIELDS:
            assert again[k].tobytes() == rings[m][k].tobytes(), f"member {m} {k} differs between identical runs"
        assert _member_state(second.population, m) == _member_state(pop, m)
    first.population.close()
    second.population.close()


def test_online_actions_are_acts(tmp_path):
    """The first environment step runs on the initial parameters: its stored actions are
    ``act`` on the reset observations at (online seed, t = 1) of a population at that state."""
    from fqlpop import distributed as Dist
    from hpo.identity import Identity
    from trainer.trainer import Trainer
    trainer = Trainer(_task(), Identity(population=_configs(), total_evaluations=0), _trainer_config(tmp_path),
                      online=_online())
    pop = trainer.population
    seed = Dist.online_seed(0)
    obs = trainer.online_envs.observations
    want = pop.act(obs, seed=seed, t=1)
    trainer.train(max_evaluations=100)
    for m in range(MEMBERS):
        assert np.array_equal(pop.synth_read(m)["actions"][:ENVS], want[m])
    pop.close()


def _tune_alpha_args(save, max_evaluations):
    return [f"--save_directory={save}", "--steps=8", "--eval_interval=4", "--log_interval=4",
            f"--agent.actor_hidden_dims={SMALL}", f"--agent.value_hidden_dims={SMALL}", "--agent.batch_size=64",
            "--agent.layer_norm", "--eval_episodes=4", "--synthetic_rows=5000", "--number_of_alphas=3",
            "--number_of_seeds=1", f"--max_evaluations={max_evaluations}", "--online_steps=6", f"--online_envs={ENVS}",
            f"--online_buffer_rows={CAP}"]


def test_online_resume_is_bitwise(tmp_path, monkeypatch):
    """Two rounds in one invocation against one round, a checkpoint, and one more round."""
    import tune_alpha
    from trainer.trainer import Trainer
    made = []

    class Recording(Trainer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(tune_alpha, "Trainer", Recording)
    tune_alpha.main(_tune_alpha_args(tmp_path / "once", 6))
    tune_alpha.main(_tune_alpha_args(tmp_path / "twice", 3))
    with open(tmp_path / "twice" / ENV / "checkpoint.pkl", "rb") as f:
        state = pickle.load(f)
    assert state["trainer"]["online"]["env_steps"] == 2   # updates 3 and 4 of the first round are online
    tune_alpha.main(_tune_alpha_args(tmp_path / "twice", 3))
    once, resumed = made[0], made[2]
    assert resumed.online_env_steps == 6 and once.online_env_steps == 6
    for cfg in once.candidates:
        a, b = once.member_of[cfg], resumed.member_of[cfg]
        assert once.population.get_count(a) == resumed.population.get_count(b) == 8
        assert _member_state(once.population, a) == _member_state(resumed.population, b), cfg
        assert once.population.synth_info(a) == resumed.population.synth_info(b) == {
            "rows": 6 * ENVS, "head": 6 * ENVS, "appended": 6 * ENVS}
        ra, rb = once.population.synth_read(a), resumed.population.synth_read(b)
        for k in S.FIELDS:
            assert ra[k].tobytes() == rb[k].tobytes(), (cfg, k)
    for t in made:
        t.population.close()


def test_online_with_successive_halving_prunes(tmp_path):
    """A pruned member is simply not active: its ring and update count stop where it left, the
    others go on."""
    from hpo.successive_halving import SuccessiveHalving
    from trainer.trainer import Trainer
    cfg = _trainer_config(tmp_path, steps=16, eval_interval=4)
    # milestones after 2 and 3 evaluations per candidate: 3 -> 2 -> 1 members
    strategy = SuccessiveHalving(set(_configs()), total_evaluations=4, fraction=1.0 / 3.0, history_length=1)
    assert sorted(strategy.halving_milestones) == [2, 3]
    trainer = Trainer(_task(), strategy, cfg, online=_online(steps=12))
    pop = trainer.population
    frozen = {}   # pruned config -> its member's state and ring when the strategy dropped it
    sample = strategy.sample

    def recording_sample():
        kept = sample()
        for c, m in trainer.member_of.items():
            if c in kept:
                frozen.pop(c, None)   # (halving may bring a candidate back)
            elif c not in frozen:
                frozen[c] = (pop.get_count(m), _member_state(pop, m), pop.synth_info(m), pop.synth_read(m))
        return kept
    strategy.sample = recording_sample
    trainer.train(max_evaluations=100)
    assert len(trainer.candidates) == 1 and len(frozen) == 2
    for c, (count, state, info, ring) in frozen.items():
        m = trainer.member_of[c]
        assert 8 <= count < 16 and pop.get_count(m) == count
        assert _member_state(pop, m) == state and pop.synth_info(m) == info
        now = pop.synth_read(m)
        assert all(now[k].tobytes() == ring[k].tobytes() for k in S.FIELDS)
    for m in range(MEMBERS):
        assert pop.synth_info(m)["appended"] == (pop.get_count(m) - 4) * ENVS   # the first 4 updates are offline
    (winner,) = trainer.candidates
    assert pop.get_count(trainer.member_of[winner]) == 16
    pop.close()
