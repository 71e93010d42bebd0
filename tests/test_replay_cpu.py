"""CPU tests of the env-model evaluator's host side (evaluator/env_model_evaluator.py):
the per-step statistics over ragged episodes and the episode windows cut from a dataset."""
import numpy as np
import pytest

from evaluator.env_model_evaluator import episodes_from_dataset, summarise

NAN = float("nan")


def _ragged():
    # 4 episodes, T = 4, lengths 4, 2, 1, 3
    lengths = np.array([4, 2, 1, 3])
    mse = np.array([[1.0, 2.0, 3.0, 4.0],
                    [3.0, 6.0, 99., 99.],
                    [5.0, 99., 99., 99.],
                    [7.0, 4.0, 9.0, 99.]])
    mae = np.sqrt(mse)
    #               t0     t1     t2    t3
    logits = np.array([[-1.0, -1.0, 2.0, -3.0],
                       [-1.0, 0.5, 9.0, 9.0],    # beyond length 2: ignored
                       [-2.0, 9.0, 9.0, 9.0],    # never positive inside its length
                       [-1.0, 3.0, -1.0, 9.0]])
    masks = np.array([[1.0, 1.0, 0.0, 0.0],
                      [1.0, 1.0, 0.0, 0.0],      # recorded termination beyond length 2: ignored
                      [1.0, 0.0, 0.0, 0.0],
                      [1.0, 0.0, 0.0, 1.0]])
    return mse, mae, logits, masks, lengths


def test_summarise_ragged_statistics():
    mse, mae, logits, masks, lengths = _ragged()
    r = summarise(mse, mae, logits, masks, lengths)
    np.testing.assert_array_equal(r["n_valid"], [4, 3, 2, 1])
    np.testing.assert_allclose(r["mse_mean"], [4.0, 4.0, 6.0, 4.0])
    np.testing.assert_array_equal(r["mse_min"], [1.0, 2.0, 3.0, 4.0])
    np.testing.assert_array_equal(r["mse_max"], [7.0, 6.0, 9.0, 4.0])
    np.testing.assert_allclose(r["mae_mean"], [np.sqrt([1, 3, 5, 7]).mean(), np.sqrt([2, 6, 4]).mean(),
                                               np.sqrt([3, 9]).mean(), 2.0])
    np.testing.assert_allclose(r["mae_min"], np.sqrt([1.0, 2.0, 3.0, 4.0]))
    np.testing.assert_allclose(r["mae_max"], np.sqrt([7.0, 6.0, 9.0, 4.0]))
    # episodes 0 (t2), 1 (t1), 3 (t1) have a positive logit inside their length; episode 2 does not
    assert r["real2sim_success"] == 0.75
    # mask == 0 inside the length: episodes 0 (t2) and 3 (t1)
    assert r["recorded_success"] == 0.5


def test_summarise_termination_metrics_per_step():
    mse, mae, logits, masks, lengths = _ragged()
    r = summarise(mse, mae, logits, masks, lengths)
    # t0: no positive predicted or recorded among 4 valid -> accuracy 1, precision and recall undefined
    # t1: valid eps 0, 1, 3: predicted (F, T, T), recorded (F, F, T) -> acc 2/3, precision 1/2, recall 1
    # t2: valid eps 0, 3: predicted (T, F), recorded (T, T) -> acc 1/2, precision 1, recall 1/2
    # t3: valid ep 0: predicted F, recorded T -> acc 0, precision undefined, recall 0
    np.testing.assert_allclose(r["accuracy"], [1.0, 2 / 3, 0.5, 0.0])
    np.testing.assert_allclose(r["precision"], [NAN, 0.5, 1.0, NAN])
    np.testing.assert_allclose(r["recall"], [NAN, 1.0, 0.5, 0.0])


def test_summarise_step_without_valid_episode():
    mse = np.ones((2, 3))
    r = summarise(mse, mse, -np.ones((2, 3)), np.ones((2, 3)), [2, 1])
    np.testing.assert_array_equal(r["n_valid"], [2, 1, 0])
    assert np.isnan(r["mse_mean"][2]) and np.isnan(r["mse_min"][2]) and np.isnan(r["mae_max"][2])
    assert np.isnan(r["accuracy"][2])
    assert r["real2sim_success"] == 0.0 and r["recorded_success"] == 0.0


def _dataset(n_eps, L, D=3, A=2):
    rows = n_eps * L
    obs = np.arange(rows * D, dtype=np.float32).reshape(rows, D)
    return {"observations": obs, "next_observations": obs + 0.5,
            "actions": -np.arange(rows * A, dtype=np.float32).reshape(rows, A),
            "masks": (np.arange(rows) % L != L - 1).astype(np.float32)}


def test_episodes_window_and_lengths():
    L = 10
    ds = _dataset(6, L)
    ep = episodes_from_dataset(ds, 4, horizon=4, episode_length=L, start=3, seed=1)
    ids = ep["episodes"]
    assert len(set(ids.tolist())) == 4 and ids.min() >= 0 and ids.max() < 6  # without replacement
    assert ep["actions"].shape == (4, 4, 2) and ep["next_obs"].shape == (4, 4, 3) and ep["masks"].shape == (4, 4)
    np.testing.assert_array_equal(ep["lengths"], [4] * 4)
    for k, e in enumerate(ids):
        rows = e * L + np.arange(3, 7)
        np.testing.assert_array_equal(ep["init_obs"][k], ds["observations"][rows[0]])
        np.testing.assert_array_equal(ep["anchor_obs"][k], ds["observations"][rows])
        np.testing.assert_array_equal(ep["next_obs"][k], ds["next_observations"][rows])
        np.testing.assert_array_equal(ep["actions"][k], ds["actions"][rows])
        np.testing.assert_array_equal(ep["masks"][k], ds["masks"][rows])


def test_episodes_window_clipped_to_episode():
    L = 10
    ds = _dataset(3, L)
    ep = episodes_from_dataset(ds, 3, horizon=100, episode_length=L, start=7, seed=0)
    assert ep["actions"].shape == (3, 3, 2)           # rows 7, 8, 9 only: never into the next episode
    np.testing.assert_array_equal(ep["lengths"], [3, 3, 3])
    np.testing.assert_array_equal(ep["masks"], [[1, 1, 0]] * 3)
    full = episodes_from_dataset(ds, 3, horizon=L, episode_length=L)
    assert full["actions"].shape == (3, L, 2)
    assert sorted(full["episodes"].tolist()) == [0, 1, 2]


def test_episodes_deterministic_per_seed():
    ds = _dataset(40, 5)
    a = episodes_from_dataset(ds, 10, 5, episode_length=5, seed=3)
    b = episodes_from_dataset(ds, 10, 5, episode_length=5, seed=3)
    c = episodes_from_dataset(ds, 10, 5, episode_length=5, seed=4)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert not np.array_equal(a["episodes"], c["episodes"])


def test_episodes_refuse_bad_requests():
    ds = _dataset(3, 10)
    with pytest.raises(ValueError, match="whole number"):
        episodes_from_dataset(ds, 2, 5, episode_length=7)
    with pytest.raises(ValueError, match="n_episodes"):
        episodes_from_dataset(ds, 4, 5, episode_length=10)
    with pytest.raises(ValueError, match="window"):
        episodes_from_dataset(ds, 2, 5, episode_length=10, start=10)
