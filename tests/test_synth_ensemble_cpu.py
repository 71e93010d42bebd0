"""CPU tests of branching under the world-model ensemble: the new flags and config fields,
the refusals that need no GPU, and the float64 restatement of the ensemble's disagreement
(tests/synth_ens_np.py) that the GPU tests compare with."""
import numpy as np
import pytest

import synth_ens_np as SE


def test_flags_parse_with_inert_defaults():
    from argparser import build_config_from_args, build_model_rollout_config_from_args, get_argparser
    from trainer.config import ModelRolloutConfig
    import tune_alpha
    args = get_argparser().parse_args([])
    assert args.model_rollout_ensemble is False and args.model_rollout_penalty == 0.0
    mr = build_model_rollout_config_from_args(args)
    assert mr == ModelRolloutConfig() and mr.ensemble is False and mr.penalty == 0.0 and not mr.enabled
    flagged = get_argparser().parse_args(["--model_rollout_branches=64", "--model_rollout_ensemble",
                                          "--model_rollout_penalty=1.5"])
    assert build_config_from_args(flagged) == build_config_from_args(args)
    mr = build_model_rollout_config_from_args(flagged)
    assert mr.enabled and mr.ensemble is True and mr.penalty == 1.5
    mr.validate()
    assert build_model_rollout_config_from_args(tune_alpha.build_parser().parse_args([])) == ModelRolloutConfig()
    # a namespace without the flags: the inert defaults
    import argparse
    assert build_model_rollout_config_from_args(argparse.Namespace()) == ModelRolloutConfig()


def test_validate_refuses_a_bad_penalty():
    from trainer.config import ModelRolloutConfig
    ModelRolloutConfig(branches=8, ensemble=True, penalty=0.0).validate()
    ModelRolloutConfig(branches=8, ensemble=True, penalty=2.0).validate()
    ModelRolloutConfig(branches=8, ensemble=True).validate()
    for bad in (dict(ensemble=True, penalty=-0.5), dict(ensemble=True, penalty=float("nan")),
                dict(ensemble=True, penalty=float("inf")), dict(ensemble=False, penalty=1.0)):
        with pytest.raises(ValueError, match="model_rollout_penalty"):
            ModelRolloutConfig(branches=8, **bad).validate()


def test_trainer_refuses_ensemble_branches_without_an_ensemble(tmp_path):
    from hpo.identity import Identity
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    from trainer.config import ExperimentConfig, ModelRolloutConfig, TrainerConfig
    from trainer.trainer import MODEL_ROLLOUT_ENSEMBLE_MSG, Trainer
    task = OfflineTaskWithSimulatedEvaluations(n_rows=500, n_val_rows=100, num_evaluation_envs=2, max_episode_steps=4)
    assert task.env_models is None
    configs = [ExperimentConfig(seed=1, alpha=3.0), ExperimentConfig(seed=2, alpha=30.0)]
    with pytest.raises(ValueError) as err:
        Trainer(task, Identity(population=configs, total_evaluations=0), TrainerConfig(save_directory=tmp_path),
                model_rollouts=ModelRolloutConfig(branches=8, ensemble=True, penalty=1.0))
    assert str(err.value) == MODEL_ROLLOUT_ENSEMBLE_MSG and "--env_model_ensemble" in MODEL_ROLLOUT_ENSEMBLE_MSG
    assert not list(tmp_path.iterdir())  # refused before anything was created


def test_distributed_trainer_still_refuses_model_rollouts(tmp_path):
    from hpo.identity import Identity
    from trainer.config import ExperimentConfig, ModelRolloutConfig, TrainerConfig
    from trainer.distributed_trainer import DistributedTrainer
    configs = [ExperimentConfig(seed=1, alpha=3.0)]
    with pytest.raises(NotImplementedError, match="one GPU only"):
        DistributedTrainer(None, Identity(population=configs, total_evaluations=0),
                           TrainerConfig(save_directory=tmp_path),
                           model_rollouts=ModelRolloutConfig(branches=8, ensemble=True, penalty=1.0))


def test_disagreement_is_zero_for_identical_predictions():
    rng = np.random.default_rng(0)
    p = rng.standard_normal((1, 9, 28))
    for K in (1, 3, 5):
        u = SE.disagreement(np.repeat(p, K, axis=0))
        assert u.shape == (9,) and (u == 0.0).all()


def test_disagreement_is_the_norm_of_the_per_coordinate_std():
    rng = np.random.default_rng(1)
    for K, shape in ((2, (7,)), (3, (4, 5)), (5, (11,)), (16, (3,))):
        p = 3.0 + rng.standard_normal((K,) + shape + (28,))
        want = np.linalg.norm(np.std(p, axis=0), axis=-1)
        got = SE.disagreement(p)
        assert got.shape == shape
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # nearly equal predictions: the differences from model 0 keep the small spread that
    # E[x^2] - E[x]^2 on the raw values would lose
    base = 100.0 + rng.standard_normal((1, 6, 28))
    p = base + 1e-7 * rng.standard_normal((3, 6, 28))
    np.testing.assert_allclose(SE.disagreement(p), np.linalg.norm(np.std(p - base, axis=0), axis=-1), rtol=1e-6)


def test_penalised_transitions_lower_only_the_rewards():
    import synth_np as S
    rng = np.random.default_rng(2)
    E, T, D, A = 6, 4, 3, 2
    length = np.array([4, 1, 2, 4, 3, 4], np.float32)
    success = np.array([0, 1, 0, 1, 1, 0], np.float32)
    tobs = rng.standard_normal((T, E, D)).astype(np.float32)
    tact = rng.uniform(-1, 1, (T, E, A)).astype(np.float32)
    unc = rng.uniform(0.5, 2.0, (T, E)).astype(np.float32)
    tr = S.transitions(success, length, rng.standard_normal((E, D)).astype(np.float32), tobs, tact)
    pen = SE.penalised(tr, length, unc, 0.5)
    for k in S.FIELDS:
        if k != "rewards":
            np.testing.assert_array_equal(pen[k], tr[k])
    order = [(t, e) for t in range(T) for e in range(E) if t < length[e]]
    want = np.array([tr["rewards"][i] - np.float32(0.5) * unc[t, e] for i, (t, e) in enumerate(order)], np.float32)
    np.testing.assert_array_equal(pen["rewards"], want)
    assert (pen["rewards"] < tr["rewards"]).all() and (pen["rewards"] < -1).any()
    np.testing.assert_array_equal(SE.penalised(tr, length, unc, 0.0)["rewards"], tr["rewards"])
