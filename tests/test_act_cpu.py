"""CPU side of the online phase: the probes tests/test_gpu_act.py compares on, the device
noise's power to tell members and steps apart, OnlineConfig, the refusals, the flags, the toy
environments and the "auto" real_ratio.  No GPU.
"""
from __future__ import annotations

import pickle

import numpy as np
import pytest

import act_np as N
from _helpers import check_clamp_conditions


@pytest.mark.parametrize("key", sorted(N.PROBE_SEEDS), ids=lambda k: f"{k[0]}-{k[1]}")
def test_probes_meet_the_clamp_conditions(key):
    """For every (member, n_envs) the GPU test compares on, the oracle's raw actions lie
    15-85 % outside [-1, 1] and none within 1e-4 of +-1: both clamp branches are exercised and
    no clamp decision can differ between float32 and float64."""
    group, member = key
    obs, noise = N.probe(group, member)
    raw = N.raw_actions(N.GROUPS[group][member], obs, noise)
    assert raw.shape == (N.ROWS, N.GROUPS[group][member].A)
    for n in N.N_ENVS:
        check_clamp_conditions(raw[:n], f"{group}[{member}] first {n} rows")


@pytest.mark.parametrize("A", (5, 8))
def test_device_noise_tells_members_and_steps_apart(A):
    """A draw under another member's key, or at t + 1, is more than 0.1 away from the wanted
    one in over half of the entries: the GPU test's 1e-3 bound on z discriminates."""
    seed, t, n_envs = 1234, 3, 17
    want = N.device_noise(seed, 11, 4.0, n_envs, t, A)
    assert want.shape == (n_envs, A)
    other_member = N.device_noise(seed, 12, 40.0, n_envs, t, A)
    next_step = N.device_noise(seed, 11, 4.0, n_envs, t + 1, A)
    other_seed = N.device_noise(seed + 1, 11, 4.0, n_envs, t, A)
    for name, z in (("member", other_member), ("t + 1", next_step), ("seed", other_seed)):
        assert (np.abs(z - want) > 0.1).mean() > 0.5, name


def test_online_config_validate():
    from trainer.config import OnlineConfig
    off = OnlineConfig()
    assert not off.enabled
    OnlineConfig(envs=0).validate()   # off: nothing is checked
    on = OnlineConfig(steps=10, envs=4, utd=2, buffer_rows=64)
    assert on.enabled
    on.validate()
    OnlineConfig(steps=10, real_ratio=0.25).validate()
    for bad in (dict(envs=0), dict(utd=0), dict(envs=65, buffer_rows=64), dict(real_ratio=1.5),
                dict(real_ratio=-0.1), dict(real_ratio="half")):
        with pytest.raises(ValueError):
            OnlineConfig(steps=10, **bad).validate()


def test_real_ratio_auto():
    """n_offline / (n_offline + ring rows): a uniform draw over dataset and online rows."""
    from trainer.config import OnlineConfig
    auto = OnlineConfig(steps=1)
    assert auto.real_ratio == "auto"
    assert auto.ratio(1000, 0) == 1.0
    assert auto.ratio(1000, 1000) == 0.5
    assert auto.ratio(300, 100) == pytest.approx(0.75)
    assert OnlineConfig(steps=1, real_ratio=0.3).ratio(1000, 5) == pytest.approx(0.3)


def test_flags_default_to_off():
    import tune_alpha
    from argparser import build_online_config_from_args
    args = tune_alpha.build_parser().parse_args([])
    cfg = build_online_config_from_args(args)
    assert not cfg.enabled and cfg.real_ratio == "auto" and (cfg.envs, cfg.utd, cfg.buffer_rows) == (8, 1, 100_000)
    args = tune_alpha.build_parser().parse_args(["--online_steps=50", "--online_envs=16", "--online_utd=4",
                                                 "--online_buffer_rows=4096", "--online_real_ratio=0.5"])
    cfg = build_online_config_from_args(args)
    assert cfg.enabled and (cfg.steps, cfg.envs, cfg.utd, cfg.buffer_rows, cfg.real_ratio) == (50, 16, 4, 4096, 0.5)
    cfg.validate()


class _NoPopulationTrainerMixin:
    """Trainer whose population must never be built: the refusals come first."""

    def _make_population(self, configs, device):
        raise AssertionError("a population was built before the refusal")


def _trainer_args(tmp_path):
    from hpo.identity import Identity
    from task.offline_task_synthetic import OfflineTaskSynthetic
    from trainer.config import ExperimentConfig, TrainerConfig
    task = OfflineTaskSynthetic(n_rows=100, n_val_rows=100, num_evaluation_envs=2, max_episode_steps=4)
    configs = [ExperimentConfig(seed=1, alpha=3.0), ExperimentConfig(seed=2, alpha=30.0)]
    return task, Identity(population=configs, total_evaluations=0), TrainerConfig(steps=10, save_directory=tmp_path)


def test_refusals_come_before_any_population(tmp_path, monkeypatch):
    import tune_alpha
    from hpo.pbt import PopulationBasedTraining
    from trainer.config import ModelRolloutConfig, OnlineConfig
    from trainer.distributed_trainer import DistributedTrainer
    from trainer.trainer import (ONLINE_CLONE_MSG, ONLINE_DISTRIBUTED_MSG, ONLINE_ROLLOUT_MSG, Trainer)

    class T(_NoPopulationTrainerMixin, Trainer):
        pass
    task, strategy, cfg = _trainer_args(tmp_path)
    online = OnlineConfig(steps=5, envs=2, buffer_rows=16)
    with pytest.raises(ValueError, match="one ring, two writers"):
        T(task, strategy, cfg, model_rollouts=ModelRolloutConfig(branches=4), online=online)
    pbt = PopulationBasedTraining(population=set(strategy.population), total_evaluations=10, seed=0)
    with pytest.raises(ValueError, match="clone members"):
        T(task, pbt, cfg, online=online)
    with pytest.raises(NotImplementedError, match="one GPU only"):
        DistributedTrainer(task, strategy, cfg, online=online)
    assert len({ONLINE_CLONE_MSG, ONLINE_DISTRIBUTED_MSG, ONLINE_ROLLOUT_MSG}) == 3

    class NoEnvs:   # a task without online_envs
        pass
    with pytest.raises(ValueError, match="NoEnvs offers no online environments"):
        T(NoEnvs(), strategy, cfg, online=online)
    with pytest.raises(ValueError, match="online_envs >= 1"):
        T(task, strategy, cfg, online=OnlineConfig(steps=5, envs=0))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU only"):
        tune_alpha.main([f"--save_directory={tmp_path}", "--online_steps=5"])
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit, match="drop --single_experiment"):
        tune_alpha.main([f"--save_directory={tmp_path}", "--online_steps=5", "--single_experiment"])


def _envs(seed=7, members=3, n_envs=4):
    from task.offline_task_synthetic import OfflineTaskSynthetic
    task = OfflineTaskSynthetic(n_rows=10, n_val_rows=10, num_evaluation_envs=2, max_episode_steps=5)
    return task.online_envs(members, n_envs, seed)


def test_reach_envs_contract_and_determinism():
    from task.online_envs import OnlineEnvs
    a, b = _envs(), _envs()
    assert isinstance(a, OnlineEnvs)
    assert a.observations.shape == (3, 4, 28) and a.observations.dtype == np.float32
    assert np.array_equal(a.observations, b.observations)
    assert not np.array_equal(a.observations[0], a.observations[1])   # members' envs are independent
    rng = np.random.default_rng(0)
    finished = 0
    for t in range(12):
        act = rng.uniform(-1, 1, (3, 4, 5)).astype(np.float32)
        obs = a.observations
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)
        nxt, rew, term, trunc = ra
        for m in range(3):
            want = N.reach_step(obs[m], act[m], 5)
            assert np.array_equal(want[0], nxt[m]) and np.array_equal(want[1], rew[m]) and np.array_equal(want[2], term[m])
        done = term | trunc
        finished += int(done.sum())
        # next_obs is the pre-reset observation; the current one is post-reset where an env finished
        assert np.array_equal(a.observations[~done], nxt[~done])
        if done.any():
            assert not np.any(np.all(a.observations[done] == nxt[done], axis=-1))
    assert finished >= 3 * 4 * 2   # (truncation after 5 steps)
    assert np.array_equal(a.reset(7), _envs().observations)


def test_reach_envs_terminate_on_success():
    """Actions that drive the reach coordinates to 0 succeed: terminated, reward 0, the next
    observation is the reached one and the environment starts afresh."""
    envs = _envs()
    seen = 0
    for t in range(5):
        obs = envs.observations
        nxt, rew, term, trunc = envs.step(np.clip(-3.0 * obs[:, :, :5], -1, 1))
        assert np.array_equal(rew, np.where(term, 0.0, -1.0).astype(np.float32))
        norm = np.linalg.norm(nxt[:, :, :5], axis=-1)
        assert np.array_equal(term, norm < np.float32(0.25 * np.sqrt(5)))
        seen += int(term.sum())
        assert not np.any(np.all(envs.observations[term] == nxt[term], axis=-1))
    assert seen >= 12   # every environment gets there within a few steps


def test_reach_envs_member_stream_depends_on_seed_and_slot_only():
    """Stepping a subset leaves the others where they were, and a member's observations are
    those it has when every member steps."""
    every, some = _envs(), _envs()
    rng = np.random.default_rng(1)
    for t in range(11):
        act = rng.uniform(-1, 1, (3, 4, 5)).astype(np.float32)
        full = every.step(act)
        part = some.step(act[[0, 2]], members=[0, 2])
        for x, y in zip(full, part):
            assert np.array_equal(x[[0, 2]], y)
    assert np.array_equal(every.observations[[0, 2]], some.observations[[0, 2]])
    assert np.array_equal(some.observations[1], _envs().observations[1])
    assert not np.array_equal(_envs(seed=8).observations, _envs(seed=7).observations)


def test_reach_envs_state_dict_round_trip():
    a = _envs()
    rng = np.random.default_rng(2)
    acts = rng.uniform(-1, 1, (9, 3, 4, 5)).astype(np.float32)
    for t in range(4):
        a.step(acts[t])
    state = pickle.loads(pickle.dumps(a.state_dict()))
    b = _envs(seed=99)
    b.load_state_dict(state)
    assert np.array_equal(a.observations, b.observations)
    for t in range(4, 9):   # through truncations: the restored generators continue the streams
        for x, y in zip(a.step(acts[t]), b.step(acts[t])):
            assert np.array_equal(x, y)
    assert np.array_equal(a.observations, b.observations)
    with pytest.raises(ValueError, match="saved as"):
        _envs(members=2).load_state_dict(state)


def test_act_stage_under_sanitizers(tmp_path):
    """csrc/popmem.h's PopActStage on the host (tests/cpp/actstage_test.cpp, a stand-alone child
    process under AddressSanitizer and UBSan): layout, growth, a failed growth, no leak."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "actstage_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(root, "tests", "cpp", "actstage_test.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failed checks, 0 live allocations" in run.stdout and "0 double frees" in run.stdout, run.stdout


def test_population_act_and_append_validate_shapes():
    """The Python wrappers refuse wrong shapes before the library is called."""
    from fqlpop import Population, PopulationConfig

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"library call {name}")
    pop = object.__new__(Population)
    pop.cfg, pop.n, pop.lib, pop._h = PopulationConfig(obs_dim=28, action_dim=5), 2, NoCalls(), None
    pop.active = np.array([True, True])
    pop.synth_capacity = 16
    with pytest.raises(ValueError, match="observations must have shape"):
        pop.act(np.zeros((1, 4, 28), np.float32))
    with pytest.raises(ValueError, match="noise must have shape"):
        pop.act(np.zeros((2, 4, 28), np.float32), noise=np.zeros((2, 4, 4), np.float32))
    rows = {"observations": np.zeros((2, 3, 28), np.float32), "actions": np.zeros((2, 3, 5), np.float32),
            "rewards": np.zeros((2, 3), np.float32), "masks": np.zeros((2, 3), np.float32),
            "next_observations": np.zeros((2, 3, 28), np.float32)}
    with pytest.raises(ValueError, match="need the fields"):
        pop.synth_append_active({k: v for k, v in rows.items() if k != "masks"})
    with pytest.raises(ValueError, match="must be float32"):
        pop.synth_append_active({**rows, "rewards": rows["rewards"].astype(np.float64)})
    with pytest.raises(ValueError, match="must have shape"):
        pop.synth_append_active({**rows, "actions": np.zeros((2, 4, 5), np.float32)})
    with pytest.raises(ValueError, match="must have shape"):
        pop.synth_append_active({k: v[:1] for k, v in rows.items()})
    pop._h = None
