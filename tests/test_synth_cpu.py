"""CPU tests of training on world-model branches: the host restatement the GPU tests compare
with (tests/synth_np.py) is self-consistent, the collect seed, the flags, and the refusals
that need no GPU."""
import numpy as np
import pytest

import synth_np as S
from philox_np import draw, philox4x32_10, sample_key

D, A = 3, 2


def _rollout(rng, E=7, T=4):
    """A made-up recorded rollout in fqlpop_rollout_record's layout: lengths in 1..T, entries
    from an env's length on are 0."""
    length = rng.integers(1, T + 1, E)
    length[0], length[1] = T, 1
    success = (rng.uniform(size=E) < 0.5).astype(np.float32)
    success[0] = 0.0  # a truncation
    tobs = rng.standard_normal((T, E, D)).astype(np.float32)
    tact = rng.uniform(-1, 1, (T, E, A)).astype(np.float32)
    for e in range(E):
        tobs[length[e]:, e] = 0
        tact[length[e]:, e] = 0
    return success, length.astype(np.float32), rng.standard_normal((E, D)).astype(np.float32), tobs, tact


def test_transitions_order_and_fields():
    rng = np.random.default_rng(0)
    success, length, oobs, tobs, tact = _rollout(rng)
    tr = S.transitions(success, length, oobs, tobs, tact)
    n = int(length.sum())
    assert all(tr[k].shape[0] == n for k in S.FIELDS)
    order = [(t, e) for t in range(tobs.shape[0]) for e in range(tobs.shape[1]) if t < length[e]]
    assert order == sorted(order) and len(order) == n
    for i, (t, e) in enumerate(order):
        np.testing.assert_array_equal(tr["observations"][i], tobs[t, e])
        np.testing.assert_array_equal(tr["actions"][i], tact[t, e])
        last = t + 1 == length[e]
        np.testing.assert_array_equal(tr["next_observations"][i], oobs[e] if last else tobs[t + 1, e])
        terminal = last and success[e] == 1
        assert tr["rewards"][i] == (0.0 if terminal else -1.0) and tr["masks"][i] == (0.0 if terminal else 1.0)
    # env 0 ran to the horizon without terminating: its last transition is no terminal
    i0 = order.index((tobs.shape[0] - 1, 0))
    assert tr["masks"][i0] == 1.0 and tr["rewards"][i0] == -1.0


def test_host_ring_fill_and_wrap():
    rng = np.random.default_rng(1)
    ring = S.HostRing(20, D, A)
    log = []
    for _ in range(4):
        tr = S.transitions(*_rollout(rng))
        ring.append(tr)
        log.append(tr)
        total = sum(t["rewards"].shape[0] for t in log)
        assert ring.info() == {"rows": min(20, total), "head": total % 20, "appended": total}
    flat = {k: np.concatenate([t[k] for t in log]) for k in S.FIELDS}
    total = flat["rewards"].shape[0]
    assert total > 40  # wrapped at least twice
    for p in range(20):  # position p holds the latest transition i with i % 20 == p
        i = max(j for j in range(total) if j % 20 == p)
        for k in S.FIELDS:
            np.testing.assert_array_equal(ring.data[k][p], flat[k][i])
    with pytest.raises(ValueError):
        S.HostRing(3, D, A).append(log[0])


def test_mixed_draw_reduces_to_its_two_ends():
    key, B, N, rows = sample_key(7, 30.0), 256, 100_003, 977
    off_idx, noise = draw(key, 5, B, N, A)
    fr, idx, nz = S.mixed_draw(key, 5, B, N, rows, 1.0, A)
    assert not fr.any()
    np.testing.assert_array_equal(idx, off_idx)
    for k in noise:
        np.testing.assert_array_equal(nz[k], noise[k])
    fr, idx, _ = S.mixed_draw(key, 5, B, N, rows, 0.0, A)
    assert fr.all() and idx.max() < rows
    b = np.arange(B, dtype=np.uint32)
    ctr = np.stack([b, np.full(B, 5, np.uint32), np.full(B, 0x51A7, np.uint32), np.zeros(B, np.uint32)], -1)
    w0 = philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))[:, 0].astype(np.uint64)
    np.testing.assert_array_equal(idx, ((w0 * np.uint64(rows)) >> np.uint64(32)).astype(np.int64))
    fr, idx, _ = S.mixed_draw(key, 5, B, N, 0, 0.0, A)        # an empty ring: offline rows
    assert not fr.any()
    np.testing.assert_array_equal(idx, off_idx)
    fr, _, _ = S.mixed_draw(key, 5, B, N, rows, 0.5, A)
    assert 0.35 < fr.mean() < 0.65
    # the source choice does not move the row word: offline rows keep draw()'s index
    np.testing.assert_array_equal(S.mixed_draw(key, 5, B, N, rows, 0.5, A)[1][~fr], off_idx[~fr])


def test_mixed_batch_takes_rows_from_both_sources():
    rng = np.random.default_rng(2)
    off = {k: rng.standard_normal((50,) + s).astype(np.float32)
           for k, s in zip(S.FIELDS, [(D,), (A,), (), (), (D,)])}
    ring = {k: 100 + v[:9] for k, v in off.items()}
    fr = np.array([True, False, True, False])
    idx = np.array([8, 49, 0, 3])
    got = S.mixed_batch(off, ring, fr, idx)
    for k in S.FIELDS:
        np.testing.assert_array_equal(got[k][0], ring[k][8])
        np.testing.assert_array_equal(got[k][1], off[k][49])
        np.testing.assert_array_equal(got[k][2], ring[k][0])
        np.testing.assert_array_equal(got[k][3], off[k][3])


def test_start_rows_in_range_and_seeded():
    a, b = S.start_rows(21, 512, 2003), S.start_rows(22, 512, 2003)
    assert a.min() >= 0 and a.max() < 2003 and not np.array_equal(a, b)
    np.testing.assert_array_equal(a, S.start_rows(21, 512, 2003))
    np.testing.assert_array_equal(a[:20], S.start_rows(21, 20, 2003))  # per branch: no dependence on the count


def test_collect_seed_is_deterministic_and_distinct():
    from fqlpop.distributed import collect_seed, eval_round_seed
    seeds = [collect_seed(3, i) for i in range(200)]
    assert seeds == [collect_seed(3, i) for i in range(200)]
    assert len(set(seeds)) == 200 and all(0 <= s < 2**31 - 1 for s in seeds)
    assert collect_seed(4, 0) != collect_seed(3, 0)
    assert collect_seed(3, 5) != eval_round_seed(3, 5)


def test_flags_parse_with_inert_defaults():
    from argparser import build_config_from_args, build_model_rollout_config_from_args, get_argparser
    from trainer.config import ModelRolloutConfig
    import tune_alpha
    args = get_argparser().parse_args([])
    mr = build_model_rollout_config_from_args(args)
    assert mr == ModelRolloutConfig() and not mr.enabled and mr.branches == 0
    # the trainer config is what it was without the flags (the golden argparser test holds it
    # to the reference's)
    flagged = get_argparser().parse_args(["--model_rollout_branches=64", "--model_rollout_horizon=3",
                                          "--model_rollout_interval=500", "--model_rollout_warmup=2000",
                                          "--model_real_ratio=0.25", "--model_buffer_rows=4096"])
    assert build_config_from_args(flagged) == build_config_from_args(args)
    mr = build_model_rollout_config_from_args(flagged)
    assert (mr.branches, mr.horizon, mr.interval, mr.warmup, mr.real_ratio, mr.buffer_rows) == (64, 3, 500, 2000, 0.25,
                                                                                                4096)
    assert mr.enabled
    mr.validate()
    assert build_model_rollout_config_from_args(tune_alpha.build_parser().parse_args([])) == ModelRolloutConfig()
    for bad in (dict(branches=8, horizon=0), dict(branches=8, real_ratio=1.5), dict(branches=100, horizon=5,
                                                                                   buffer_rows=499)):
        with pytest.raises(ValueError):
            ModelRolloutConfig(**bad).validate()
    ModelRolloutConfig(horizon=0).validate()  # off: nothing to check


def _configs():
    from trainer.config import ExperimentConfig
    return [ExperimentConfig(seed=1, alpha=3.0), ExperimentConfig(seed=2, alpha=30.0)]


def test_trainer_refuses_a_task_without_env_model(tmp_path):
    from hpo.identity import Identity
    from task.offline_task_synthetic import OfflineTaskSynthetic
    from trainer.config import ModelRolloutConfig, TrainerConfig
    from trainer.trainer import Trainer
    task = OfflineTaskSynthetic(n_rows=500, n_val_rows=100, num_evaluation_envs=2, max_episode_steps=4)
    with pytest.raises(ValueError, match="OfflineTaskWithSimulatedEvaluations"):
        Trainer(task, Identity(population=_configs(), total_evaluations=0), TrainerConfig(save_directory=tmp_path),
                model_rollouts=ModelRolloutConfig(branches=8))
    assert not list(tmp_path.iterdir())  # refused before anything was created


def test_distributed_trainer_refuses_model_rollouts(tmp_path, monkeypatch):
    import tune_alpha
    from hpo.identity import Identity
    from trainer.config import ModelRolloutConfig, TrainerConfig
    from trainer.distributed_trainer import DistributedTrainer
    with pytest.raises(NotImplementedError, match="one GPU only"):
        DistributedTrainer(None, Identity(population=_configs(), total_evaluations=0),
                           TrainerConfig(save_directory=tmp_path), model_rollouts=ModelRolloutConfig(branches=8))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU only"):
        tune_alpha.main([f"--save_directory={tmp_path}", "--task=simulated", "--model_rollout_branches=8"])
    assert not list(tmp_path.iterdir())
