"""NumPy restatement of branching under the world-model ensemble (test infrastructure, not a
test module): the ensemble's disagreement ``u`` that ``fqlpop_rollout_ensemble_record``
writes to out_traj_unc, the float64 mixed rollout with its per-step traces, and what
``fqlpop_synth_collect_ensemble`` appends with a penalty (include/fqlpop.h).

* u: with s'_k model k's next observation from one (s, a), r_k = s'_k - s'_0,
  Q = sum_k |r_k|^2, m = sum_k r_k: u = sqrt(max(0, Q / K - |m|^2 / K^2)), the norm of the
  per-coordinate (population) standard deviation of the K predictions;
* mixed rollout: tests/test_gpu_ensemble._mixed_oracle, also returning the (s, a) of every
  step an env ran (0 elsewhere, as the device's traces);
* penalised transitions: tests/synth_np.transitions with r - penalty * u(t, e).
"""
from __future__ import annotations

import numpy as np

import synth_np as S
from oracle import envmodel_oracle as EO
from oracle import fql_oracle as O


def disagreement(preds) -> np.ndarray:
    """preds [K, ..., D] (the K models' next observations) -> u [...] in float64."""
    p = np.asarray(preds, np.float64)
    K = p.shape[0]
    r = p - p[0]
    Q = (r * r).sum(-1).sum(0)
    m = r.sum(0)
    return np.sqrt(np.maximum(0.0, Q / K - (m * m).sum(-1) / (K * K)))


def predictions(models, obs, act) -> np.ndarray:
    """[K, n, D]: every model's float64 next observation from (obs [n, D], act [n, A])."""
    obs, act = np.asarray(obs, np.float64), np.asarray(act, np.float64)
    return np.stack([EO.state_predictor(sp, obs, act) for sp, _ in models])


def mixed_oracle_traces(cfg, params, models, obs0, noise, choice, steps):
    """One member in float64, as _mixed_oracle: env e steps under models[choice[t - 1, e]] at
    step t; a done env keeps its observation.  Returns (success, length, final obs, min
    |logit| over every live env and step, traj_obs [steps, n, D], traj_act [steps, n, A])."""
    obs = np.asarray(obs0, np.float64)
    n = obs.shape[0]
    done = np.zeros(n, bool)
    success, length = np.zeros(n), np.zeros(n)
    margin = np.inf
    tobs = np.zeros((steps, n, obs.shape[1]))
    tact = None
    for t in range(1, steps + 1):
        a = O.sample_actions(cfg, params, obs, np.asarray(noise[t - 1], np.float64))
        if tact is None:
            tact = np.zeros((steps, n, a.shape[1]))
        live = ~done
        tobs[t - 1][live] = obs[live]
        tact[t - 1][live] = a[live]
        nxt, logit = np.zeros_like(obs), np.zeros(n)
        for k, (sp, tp) in enumerate(models):
            m = choice[t - 1] == k
            if m.any():
                nxt[m] = EO.state_predictor(sp, obs[m], a[m])
                logit[m] = EO.termination_predictor(tp, nxt[m])
        margin = min(margin, float(np.abs(logit[live]).min()))
        term = logit > 0
        new = live & (term | (t >= steps))
        success[live & term] = 1.0
        length[new] = t
        obs = np.where(live[:, None], nxt, obs)
        done |= new
        if done.all():
            break
    return success, length, obs, margin, tobs, tact


def penalised(tr: dict, length, traj_unc, penalty: float) -> dict:
    """The transitions ``tr`` (synth_np.transitions of one member's recorded rollout) with the
    reward of step (t, e) lowered by penalty * traj_unc[t, e], in float32 as the device:
    base - penalty * u (the device may fuse the multiply and the subtraction: one rounding)."""
    length = np.asarray(length).astype(np.int64)
    T, E = traj_unc.shape
    u = np.asarray([traj_unc[t, e] for t in range(T) for e in range(E) if t < length[e]], np.float32)
    out = dict(tr)
    out["rewards"] = (tr["rewards"].astype(np.float32) - np.float32(penalty) * u).astype(np.float32)
    return out

