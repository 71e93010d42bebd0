"""NumPy restatement of training on world-model branches (test infrastructure, not a test
module): what ``fqlpop_synth_collect`` appends to a member's ring, given the recorded
rollout it is defined by, and the mixed training draw of ``sample_ring_kernel``
(include/fqlpop.h, "Training on world-model branches"; csrc/kernels.hip).

* start rows: branch e starts at training row (w0 * n_rows) >> 32, w0 the first word of
  Philox4x32-10 at counter (e, 0, 0x5E13, 0) under the key of the call seed alone;
* transitions: step t < len_e of branch e is (s_t, a_t, r, m, s_{t+1}) with s_{t+1} the next
  recorded observation (the rollout's out_obs after the branch's last step), r = 0, m = 0
  where that step terminated and r = -1, m = 1 elsewhere, a truncation at the horizon
  included; a call's transitions are ordered by (t, e);
* ring: transition i of a call goes to position (head + i) mod capacity;
* mixed draw: row b at update count c reads the block of ``philox_np.draw`` (counter
  (b, c, salt, 0)); with u = (w2 >> 8) * 2^-24 it is the offline row (w0 * n_rows) >> 32 if
  u < rho (float32) or the ring is empty, else ring position (w0 * rows) >> 32.
"""
from __future__ import annotations

import numpy as np

from philox_np import SALT_TRAIN, draw, philox4x32_10

SALT_START = 0x5E13
SALT_ROLLOUT_NOISE = 0x5E11
FIELDS = ("observations", "actions", "rewards", "masks", "next_observations")
_M64 = (1 << 64) - 1


def start_rows(seed: int, n_branches: int, n_rows: int) -> np.ndarray:
    e = np.arange(n_branches, dtype=np.uint32)
    ctr = np.stack([e, np.zeros_like(e), np.full_like(e, SALT_START), np.zeros_like(e)], -1)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return ((w[:, 0].astype(np.uint64) * np.uint64(n_rows)) >> np.uint64(32)).astype(np.int64)


def rollout_noise(seed: int, member_key: int, n_envs: int, steps: int, A: int) -> np.ndarray:
    """The rollout kernels' device noise [steps][n_envs][A] in float64 (rollout_kernel: key =
    seed ^ member_key * golden, counter (env, t, 0x5E11, q), Box-Muller pair q -> actions 2q,
    2q + 1).  The device computes it in float32: close, not bitwise."""
    key = (seed ^ ((member_key * 0x9E3779B97F4A7C15) & _M64)) & _M64
    k = (key & 0xFFFFFFFF, key >> 32)
    out = np.zeros((steps, n_envs, A))
    e = np.arange(n_envs, dtype=np.uint32)
    for t in range(1, steps + 1):
        for q in range((A + 1) // 2):
            ctr = np.stack([e, np.full_like(e, t), np.full_like(e, SALT_ROLLOUT_NOISE), np.full_like(e, q)], -1)
            w = philox4x32_10(ctr, k)
            r = np.sqrt(-2.0 * np.log(((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0))
            ang = 2.0 * np.pi * (w[:, 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
            out[t - 1, :, 2 * q] = r * np.cos(ang)
            if 2 * q + 1 < A:
                out[t - 1, :, 2 * q + 1] = r * np.sin(ang)
    return out


def transitions(success, length, out_obs, traj_obs, traj_act) -> dict:
    """One member's recorded rollout (success [E], length [E], out_obs [E, D], traj_obs
    [T, E, D], traj_act [T, E, A]) as the transitions a collect appends, in (t, e) order."""
    length = np.asarray(length).astype(np.int64)
    T, E = traj_obs.shape[:2]
    rows = {k: [] for k in FIELDS}
    for t in range(T):
        for e in range(E):
            if t >= length[e]:
                continue
            last = t + 1 >= length[e]
            term = last and success[e] > 0.5
            rows["observations"].append(traj_obs[t, e])
            rows["actions"].append(traj_act[t, e])
            rows["rewards"].append(0.0 if term else -1.0)
            rows["masks"].append(0.0 if term else 1.0)
            rows["next_observations"].append(out_obs[e] if last else traj_obs[t + 1, e])
    D, A = traj_obs.shape[2], traj_act.shape[2]
    shape = {"observations": (0, D), "actions": (0, A), "rewards": (0,), "masks": (0,), "next_observations": (0, D)}
    return {k: np.asarray(v, np.float32).reshape((len(v),) + shape[k][1:]) for k, v in rows.items()}


class HostRing:
    """One member's ring on the host: the same positions and counters."""

    def __init__(self, capacity: int, D: int, A: int):
        self.capacity = int(capacity)
        self.data = {"observations": np.zeros((capacity, D), np.float32), "actions": np.zeros((capacity, A), np.float32),
                     "rewards": np.zeros(capacity, np.float32), "masks": np.zeros(capacity, np.float32),
                     "next_observations": np.zeros((capacity, D), np.float32)}
        self.rows = self.head = self.appended = 0

    def append(self, tr: dict) -> None:
        n = tr["rewards"].shape[0]
        if n > self.capacity:
            raise ValueError("a call's transitions exceed the capacity")
        pos = (self.head + np.arange(n)) % self.capacity
        for k in FIELDS:
            self.data[k][pos] = tr[k]
        self.head = (self.head + n) % self.capacity
        self.rows = min(self.capacity, self.rows + n)
        self.appended += n

    def info(self) -> dict:
        return {"rows": self.rows, "head": self.head, "appended": self.appended}

    def valid(self) -> dict:
        return {k: v[:self.rows] for k, v in self.data.items()}


def mixed_draw(key: int, count: int, B: int, n_rows: int, ring_rows: int, rho: float, A: int,
               salt: int = SALT_TRAIN):
    """(from_ring [B] bool, idx [B] int64, noise) of one member's training draw: idx indexes
    the ring (physical positions) where from_ring, else the offline rows.  The flow time and
    the noises are ``philox_np.draw``'s, whatever the source."""
    off_idx, noise = draw(key, count, B, n_rows, A, salt)
    b = np.arange(B, dtype=np.uint32)
    ctr = np.stack([b, np.full(B, count, np.uint32), np.full(B, salt, np.uint32), np.zeros(B, np.uint32)], -1)
    w = philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))
    u = ((w[:, 2] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)
    from_ring = ~(u < np.float32(rho)) & (ring_rows > 0)
    ring_idx = ((w[:, 0].astype(np.uint64) * np.uint64(max(ring_rows, 1))) >> np.uint64(32)).astype(np.int64)
    return from_ring, np.where(from_ring, ring_idx, off_idx), noise


def mixed_batch(offline: dict, ring: dict, from_ring, idx) -> dict:
    """The minibatch of a mixed draw from the offline dataset dict and a ring's valid rows."""
    out = {}
    for k in FIELDS:
        a = np.asarray(offline[k])[np.where(from_ring, 0, idx)]
        if from_ring.any():
            a = a.copy()
            a[from_ring] = np.asarray(ring[k])[idx[from_ring]]
        out[k] = a
    return out
