"""Float64 restatement of ``Population.act`` and of the toy online environments (test
infrastructure, not a test module).

* actions: ``oracle.fql_oracle.sample_actions`` per member on the z the call used, injected
  or ``synth_np.rollout_noise`` at step t under the member's sampler key;
* probes: per trained-like member (``_helpers.TRAINED``) observations and noise whose raw
  (unclipped) oracle actions meet ``_helpers.check_clamp_conditions`` on their first 1, 17 and
  50 rows -- PROBE_SEEDS is chosen on the CPU from the float64 oracle alone
  (tests/test_act_cpu.py asserts it);
* ``reach_step``: one step of the toy reach dynamics (task.online_envs.ReachEnvs) on one
  member's rows, in the environment's own float32 expressions.
"""
from __future__ import annotations

import numpy as np

import synth_np as S
from _helpers import TRAINED, trained_member
from oracle import fql_oracle as O
from philox_np import sample_key

N_ENVS = (1, 17, 50)   # a partial tile, one past a tile boundary, the workload's count
ROWS = max(N_ENVS)

# the populations tests/test_gpu_act.py builds: name -> the trained-like members, in slot order
GROUPS = {
    "h64": TRAINED["h64"][0:2],              # K0 = 33: an odd tail
    "h128": TRAINED["h128_no_ln"][0:1],
    "h1024": TRAINED["h1024"][0:1],          # the LDS extreme
    "h512": TRAINED["h512"][0:3],            # (the third member: the slot-indirection test)
    "h512_d27": TRAINED["h512_d27"][0:1],    # K0 = 32: an exact multiple of 4
    "h512_d42": TRAINED["h512_d42"][0:1],    # K0 = 50: two passes, A = 8
}
PARITY_GROUPS = ("h64", "h128", "h1024", "h512", "h512_d27", "h512_d42")

# probe seed per (group, member): the smallest for which the oracle's raw actions meet the clamp
# conditions on the first 1, 17 and 50 rows
PROBE_SEEDS = {
    ("h64", 0): 0, ("h64", 1): 0, ("h128", 0): 0, ("h1024", 0): 0,
    ("h512", 0): 0, ("h512", 1): 0, ("h512", 2): 0, ("h512_d27", 0): 0, ("h512_d42", 0): 0,
}


def probe(group: str, member: int, seed: int | None = None):
    """(observations [ROWS, D], noise [ROWS, A]) in float32 for ``GROUPS[group][member]``."""
    spec = GROUPS[group][member]
    seed = PROBE_SEEDS[(group, member)] if seed is None else seed
    rng = np.random.default_rng([spec.seed, 3, seed])
    return (rng.standard_normal((ROWS, spec.D)).astype(np.float32),
            rng.standard_normal((ROWS, spec.A)).astype(np.float32))


def raw_actions(spec, obs, noise):
    """The one-step actor's outputs before the clamp, float64 [n, A], for a trained-like member."""
    tm = trained_member(spec)
    return O.sample_actions(tm.cfg, tm.params, np.asarray(obs, np.float64), np.asarray(noise, np.float64), clip=False)


def group_inputs(group: str, n_envs: int, members=None):
    """(obs [z, n_envs, D], noise [z, n_envs, A], raw [z, n_envs, A]) of a group's members."""
    members = range(len(GROUPS[group])) if members is None else members
    obs, noise, raw = [], [], []
    for m in members:
        o, z = probe(group, m)
        obs.append(o[:n_envs])
        noise.append(z[:n_envs])
        raw.append(raw_actions(GROUPS[group][m], o[:n_envs], z[:n_envs]))
    return np.stack(obs), np.stack(noise), np.stack(raw)


def device_noise(seed: int, pop_seed: int, alpha: float, n_envs: int, t: int, A: int) -> np.ndarray:
    """The z ``act(noise=None, seed, t)`` draws for one member, float64 [n_envs, A]."""
    return S.rollout_noise(int(seed), sample_key(int(pop_seed), float(alpha)), n_envs, t, A)[t - 1]


def reach_step(obs, actions, A: int):
    """(next_obs, rewards, terminated) of one toy reach step from float32 rows ``obs``."""
    s = np.array(obs, dtype=np.float32)
    a = np.clip(np.asarray(actions, np.float32), -1, 1)
    s[:, :A] = np.float32(0.9) * s[:, :A] + np.float32(0.3) * a
    success = np.linalg.norm(s[:, :A], axis=1) < np.float32(0.25 * np.sqrt(A))
    return s, np.where(success, 0.0, -1.0).astype(np.float32), success
