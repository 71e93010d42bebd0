"""How fast does a learned env model drift from recorded trajectories?

The reference's evaluator/env_model_evaluator.py:13-77 records an agent's transitions in
the real environment, replays the recorded actions through the env model ("real2sim",
generate_actor_fn) and reports the per-step MSE / MAE between the two trajectories as
mean, min and max over episodes (get_stats, lines 58-77), with the real2sim success rate.

Here the recorded trajectories are the dataset's episodes (real-environment transitions;
MuJoCo is absent) and the replay is ONE device launch over all episodes
(``Population.envmodel_replay`` -> ``fqlpop_envmodel_replay``).  ``anchor_every`` resets
the state to the recorded one every k steps: 0 is the reference's fully open-loop replay,
1 the teacher-forced one-step error, k the error at horizon k.  No plotting.
"""
from __future__ import annotations

import csv
from pathlib import Path

import numpy as np

CSV_COLUMNS = ("n_valid", "mse_mean", "mse_min", "mse_max", "mae_mean", "mae_min", "mae_max",
               "accuracy", "precision", "recall")


def episodes_from_dataset(dataset: dict, n_episodes: int, horizon: int, episode_length: int = 1000, start: int = 0,
                          seed: int = 0) -> dict:
    """``n_episodes`` recorded episodes (drawn without replacement, seeded) cut to the
    window [start, start + horizon) clipped to the episode.  Episodes are consecutive
    ``episode_length``-row blocks of the dataset (utils/data_loader.py:14-39).

    Returns init_obs [n, obs], actions [n, T, act], next_obs / anchor_obs [n, T, obs]
    (recorded observation after / before step t), masks [n, T], lengths [n] and the drawn
    ``episodes``."""
    rows = len(dataset["observations"])
    if rows == 0 or rows % episode_length:
        raise ValueError(f"{rows} rows is not a whole number of {episode_length}-step episodes")
    total = rows // episode_length
    if not 1 <= n_episodes <= total:
        raise ValueError(f"n_episodes must be in 1..{total}, got {n_episodes}")
    if horizon <= 0 or not 0 <= start < episode_length:
        raise ValueError(f"empty window: start {start}, horizon {horizon}, episode_length {episode_length}")
    end = min(start + horizon, episode_length)
    ep = np.random.default_rng(seed).choice(total, size=n_episodes, replace=False)
    idx = ep[:, None] * episode_length + np.arange(start, end)[None, :]
    obs = np.asarray(dataset["observations"], np.float32)[idx]
    masks = np.asarray(dataset["masks"], np.float32).reshape(-1)[idx] if "masks" in dataset \
        else np.ones(idx.shape, np.float32)
    return {"init_obs": np.ascontiguousarray(obs[:, 0]),
            "actions": np.asarray(dataset["actions"], np.float32)[idx],
            "next_obs": np.asarray(dataset["next_observations"], np.float32)[idx],
            "anchor_obs": obs,
            "masks": masks,
            "lengths": np.full(n_episodes, end - start, np.int32),
            "episodes": ep}


def _ratio(num, den):
    return np.where(den > 0, num / np.maximum(den, 1), np.nan)


def summarise(mse, mae, logits, masks, lengths) -> dict:
    """Per-step statistics of a replay ([n, T] arrays, lengths [n]) over the episodes still
    valid at step t (t < lengths): the reference's get_stats (mean / min / max of MSE and
    MAE), ``n_valid``, and the termination predictor's per-step accuracy / precision /
    recall of ``logit > 0`` against the recorded ``mask == 0`` (NaN where undefined: no
    valid episode, no predicted positive, no recorded positive).  Scalars:
    ``real2sim_success`` (share of episodes with a logit > 0 inside their length) and
    ``recorded_success`` (share with a mask == 0 inside it)."""
    mse, mae, logits, masks = (np.asarray(a, np.float64) for a in (mse, mae, logits, masks))
    n, T = mse.shape
    valid = np.arange(T)[None, :] < np.asarray(lengths).reshape(n, 1)
    n_valid = valid.sum(axis=0)
    out = {"n_valid": n_valid}
    for name, a in (("mse", mse), ("mae", mae)):
        out[f"{name}_mean"] = _ratio(np.where(valid, a, 0.0).sum(axis=0), n_valid)
        out[f"{name}_min"] = np.where(n_valid > 0, np.where(valid, a, np.inf).min(axis=0), np.nan)
        out[f"{name}_max"] = np.where(n_valid > 0, np.where(valid, a, -np.inf).max(axis=0), np.nan)
    pred = (logits > 0) & valid
    true = (masks == 0) & valid
    tp = (pred & true).sum(axis=0)
    out["accuracy"] = _ratio(((pred == true) & valid).sum(axis=0), n_valid)
    out["precision"] = _ratio(tp, pred.sum(axis=0))
    out["recall"] = _ratio(tp, true.sum(axis=0))
    out["real2sim_success"] = float(pred.any(axis=1).mean())
    out["recorded_success"] = float(true.any(axis=1).mean())
    return out


class EnvModelEvaluator:
    """Replay recorded episodes of ``dataset`` through the env model uploaded into
    ``population`` (``Population.set_env_model``)."""

    def __init__(self, dataset: dict, population, episode_length: int = 1000):
        self.dataset = dataset
        self.population = population
        self.episode_length = episode_length
        self.result = None

    def evaluate(self, horizon: int, n_episodes: int = 50, anchor_every: int = 0, seed: int = 0,
                 initial_observations: np.ndarray | None = None) -> dict:
        """``initial_observations`` [n_episodes][obs] (generated starts, e.g. an
        ``InitialObservationSampler``'s) replace the recorded first observations: the
        recorded actions are then replayed open loop from starts the recording never saw,
        so the termination statistics stay meaningful and the MSE / MAE columns measure
        the distance to the recorded episode, not a model error."""
        ep = episodes_from_dataset(self.dataset, n_episodes, horizon, self.episode_length, seed=seed)
        if initial_observations is not None:
            init = np.ascontiguousarray(np.asarray(initial_observations, np.float32))
            if init.shape != ep["init_obs"].shape:
                raise ValueError(f"initial_observations have shape {init.shape}, expected {ep['init_obs'].shape}")
            ep["init_obs"] = init
        r = self.population.envmodel_replay(ep["init_obs"], ep["actions"], next_obs=ep["next_obs"],
                                            anchor_obs=ep["anchor_obs"], lengths=ep["lengths"],
                                            anchor_every=anchor_every)
        self.result = summarise(r["mse"], r["mae"], r["logits"], ep["masks"], ep["lengths"])
        return self.result

    def write_csv(self, path) -> Path:
        """One row per step: step and CSV_COLUMNS."""
        if self.result is None:
            raise RuntimeError("evaluate() first")
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        with open(path, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(("step",) + CSV_COLUMNS)
            for t in range(len(self.result["n_valid"])):
                wr.writerow([t] + [repr(self.result[k][t].item()) for k in CSV_COLUMNS])
        return path
