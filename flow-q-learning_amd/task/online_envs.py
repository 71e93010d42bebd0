"""Environments for an online phase (trainer.config.OnlineConfig): every population member
acts in ``n_envs`` environments of its own, all members stepped by one call.

A task that can offer them has ``online_envs(n_members, n_envs, seed) -> OnlineEnvs``;
``online_envs_of`` raises for a task that cannot.  ``ReachEnvs`` is the toy reach dynamics
of ``OfflineTaskSynthetic.step``, vectorised over members x envs.
"""
from __future__ import annotations

from typing import Protocol, runtime_checkable

import numpy as np


@runtime_checkable
class OnlineEnvs(Protocol):
    def reset(self, seed: int) -> np.ndarray:
        """Reset every environment; returns observations [n_members, n_envs, obs_dim]."""

    def step(self, actions, members=None):
        """Step the environments of ``members`` (slots; None: all) under actions
        [len(members), n_envs, action_dim].  Returns (next_obs, rewards, terminated,
        truncated), each with leading axes [len(members), n_envs]; ``next_obs`` is the
        observation the step led to, before any reset.  A finished environment resets itself
        from the environments' own seeded generator."""

    @property
    def observations(self) -> np.ndarray:
        """The current observations [n_members, n_envs, obs_dim]: post-reset where an
        environment finished."""

    def state_dict(self) -> dict:
        """Everything a resumed run needs to continue bit for bit."""

    def load_state_dict(self, state: dict) -> None:
        """Put ``state_dict``'s result back."""


def online_envs_of(task, n_members: int, n_envs: int, seed: int) -> OnlineEnvs:
    make = getattr(task, "online_envs", None)
    if make is None:
        raise ValueError(f"{type(task).__name__} offers no online environments (--online_steps needs a task with "
                         "online_envs: --task synthetic)")
    return make(n_members, n_envs, seed)


class ReachEnvs:
    """The toy reaching task: the first ``action_dim`` coordinates follow 0.9 x + 0.3 a, an
    episode succeeds (terminates, reward 0; else -1) once their norm is below
    0.25 sqrt(action_dim) and is truncated after ``max_episode_steps``.  Member ``m`` draws
    its starts from its own generator seeded by (seed, m): its stream depends on nothing
    else, whichever other members step."""

    def __init__(self, n_members: int, n_envs: int, obs_dim: int, action_dim: int, max_episode_steps: int,
                 seed: int = 0):
        self.n_members, self.n_envs = int(n_members), int(n_envs)
        self.obs_dim, self.action_dim = int(obs_dim), int(action_dim)
        self.max_episode_steps = int(max_episode_steps)
        self.reset(seed)

    def reset(self, seed: int) -> np.ndarray:
        self.seed = int(seed)
        self._rngs = [np.random.default_rng([self.seed & 0xFFFFFFFF, m, 0x5E15]) for m in range(self.n_members)]
        self._state = np.stack([r.standard_normal((self.n_envs, self.obs_dim)).astype(np.float32)
                                for r in self._rngs])
        self._t = np.zeros((self.n_members, self.n_envs), dtype=np.int64)
        return self._state.copy()

    @property
    def observations(self) -> np.ndarray:
        return self._state.copy()

    def step(self, actions, members=None):
        members = list(range(self.n_members)) if members is None else [int(m) for m in members]
        A = self.action_dim
        actions = np.clip(np.asarray(actions, np.float32), -1, 1)
        if actions.shape != (len(members), self.n_envs, A):
            raise ValueError(f"actions must have shape {(len(members), self.n_envs, A)}, got {actions.shape}")
        nxt = np.zeros((len(members), self.n_envs, self.obs_dim), np.float32)
        rew = np.zeros((len(members), self.n_envs), np.float32)
        term = np.zeros((len(members), self.n_envs), bool)
        trunc = np.zeros((len(members), self.n_envs), bool)
        for z, m in enumerate(members):
            s = self._state[m]
            s[:, :A] = np.float32(0.9) * s[:, :A] + np.float32(0.3) * actions[z]
            self._t[m] += 1
            dist = np.linalg.norm(s[:, :A], axis=1)
            success = dist < np.float32(0.25 * np.sqrt(A))
            term[z] = success
            trunc[z] = self._t[m] >= self.max_episode_steps
            rew[z] = np.where(success, 0.0, -1.0)
            nxt[z] = s
            for e in np.nonzero(term[z] | trunc[z])[0]:  # in env order: one generator per member
                s[e] = self._rngs[m].standard_normal(self.obs_dim).astype(np.float32)
                self._t[m, e] = 0
        return nxt, rew, term, trunc

    def state_dict(self) -> dict:
        return {"seed": self.seed, "state": self._state.copy(), "t": self._t.copy(),
                "rng": [r.bit_generator.state for r in self._rngs],
                "shape": (self.n_members, self.n_envs, self.obs_dim, self.action_dim, self.max_episode_steps)}

    def load_state_dict(self, state: dict) -> None:
        shape = (self.n_members, self.n_envs, self.obs_dim, self.action_dim, self.max_episode_steps)
        if tuple(state["shape"]) != shape:
            raise ValueError(f"the environments were saved as {tuple(state['shape'])}, these are {shape}")
        self.seed = int(state["seed"])
        self._state = np.array(state["state"], dtype=np.float32)
        self._t = np.array(state["t"], dtype=np.int64)
        for r, st in zip(self._rngs, state["rng"]):
            r.bit_generator.state = st
