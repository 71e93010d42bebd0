"""NumPy restatement of the env-model trainers' device draws (test infrastructure, not a test
module): the minibatch rows of ``em_grad_kernel``, the episode windows of ``em_seq_grad_kernel``
and ``em_sweep_kernel``, the bootstrap tables and out-of-bag lists of
``fqlpop_emtrain_set_bootstrap`` and the out-of-bag batches of ``fqlpop_emtrain_eval_oob``
(flow-q-learning_amd/csrc/emtrain.hip, ``em_unit`` and the bootstrap set-up kernels), built on
``philox_np.philox4x32_10``.  Every draw is keyed by the model's seed: (lo32, hi32).

* batch position p at update count s: counter (p, s, SALT_ROW | SALT_EP, 0), index
  u = (x1 << 32 | x0) mod n_units; the unit is u, or ``table[u]`` under a bootstrap table;
  the multistep window starts at x2 mod (ep_len - T) inside the unit (an episode)
* ``table[i]``: counter (lo32 i, hi32 i, SALT_BOOT, 0), (x1 << 32 | x0) mod n_units
* out-of-bag batch j of a call with ``draw``: counter (p, j, SALT_OOB, lo32 draw), unit
  ``oob[(x1 << 32 | x0) mod len(oob)]``
"""
from __future__ import annotations

import numpy as np

from philox_np import philox4x32_10

SALT_ROW, SALT_EP, SALT_BOOT, SALT_OOB = 0xE7, 0xE5, 0xB7, 0xB5


def _key(seed: int):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _words(seed, c0, c1, c2, c3):
    """Philox words [n][4] (uint64 holding uint32 values) of n counters; scalars broadcast."""
    n = len(c0)
    ctr = np.stack([np.asarray(c0, np.uint64) & np.uint64(0xFFFFFFFF)] +
                   [np.full(n, int(c) & 0xFFFFFFFF, np.uint64) if np.isscalar(c)
                    else np.asarray(c, np.uint64) & np.uint64(0xFFFFFFFF) for c in (c1, c2, c3)], -1)
    return philox4x32_10(ctr, _key(seed)).astype(np.uint64)


def _mod64(w, n: int) -> np.ndarray:
    """(x1 << 32 | x0) mod n as int64 (n < 2^63)."""
    v = (w[:, 1] << np.uint64(32)) | w[:, 0]
    return (v % np.uint64(n)).astype(np.int64)


def train_rows(seed: int, step: int, B: int, n_rows: int, table=None) -> np.ndarray:
    """Dataset rows [B] of the state / termination trainer's batch at update count ``step``."""
    u = _mod64(_words(seed, np.arange(B), step, SALT_ROW, 0), n_rows)
    return u if table is None else np.asarray(table, np.int64)[u]


def train_windows(seed: int, step: int, B: int, n_rows: int, ep_len: int, T: int, table=None) -> np.ndarray:
    """First dataset row [B] of each multistep window (rows base .. base + T - 1)."""
    w = _words(seed, np.arange(B), step, SALT_EP, 0)
    ep = _mod64(w, n_rows // ep_len)
    if table is not None:
        ep = np.asarray(table, np.int64)[ep]
    return ep * ep_len + (w[:, 2] % np.uint64(ep_len - T)).astype(np.int64)


def bootstrap_table(seed: int, n_units: int) -> np.ndarray:
    """The device-drawn resample [n_units] of the model with ``seed``."""
    i = np.arange(n_units, dtype=np.uint64)
    return _mod64(_words(seed, i, i >> np.uint64(32), SALT_BOOT, 0), n_units)


def oob_list(table, n_units: int) -> np.ndarray:
    """The units that do not occur in ``table``, ascending."""
    seen = np.zeros(n_units, bool)
    seen[np.asarray(table, np.int64)] = True
    return np.flatnonzero(~seen).astype(np.int64)


def oob_units(seed: int, j: int, draw: int, B: int, oob, ep_len: int | None = None, T: int | None = None):
    """Units [B] of out-of-bag batch ``j`` of an ``eval_oob(.., draw)`` call.  With ``ep_len`` and
    ``T`` (multistep) the units are episodes and the result is each window's first dataset row."""
    oob = np.asarray(oob, np.int64)
    w = _words(seed, np.arange(B), j, SALT_OOB, int(draw) & 0xFFFFFFFF)
    unit = oob[_mod64(w, len(oob))]
    if ep_len is None:
        return unit
    return unit * ep_len + (w[:, 2] % np.uint64(ep_len - T)).astype(np.int64)
