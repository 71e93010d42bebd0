"""NumPy restatement of the initial-observation VAE (test infrastructure, not a test module).

The model and loss of the reference's envmodel/initial_observation.py:8-78 in float64 with
hand-written backward passes, the optimiser of its other env-model trainers
(optax.adam over optax.cosine_decay_schedule), and the host restatement of the random
draws of ``em_vae_grad_kernel`` / ``em_vae_decode_kernel`` (flow-q-learning_amd/csrc/
emtrain.hip, VAE section), built on ``philox_np.philox4x32_10``.

Trees are ``{"encoder": {"Dense_i": {"kernel", "bias"}}, "decoder": {...}}``; with n hidden
layers the encoder's ``Dense_n`` is the mu head and ``Dense_{n+1}`` the logvar head.
"""
from __future__ import annotations

import math

import numpy as np

from philox_np import philox4x32_10

SALT_ROW, SALT_EPS, SALT_Z = 0xE7, 0x1E5, 0x5A3


def f64(tree):
    return {m: {l: {k: np.asarray(v, np.float64) for k, v in d.items()} for l, d in ls.items()}
            for m, ls in tree.items()}


def zeros_like(tree):
    return {m: {l: {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in d.items()} for l, d in ls.items()}
            for m, ls in tree.items()}


def _W(t, i):
    return t[f"Dense_{i}"]["kernel"]


def _b(t, i):
    return t[f"Dense_{i}"]["bias"]


def decode(dec, z, pre=None):
    """decoder(z); ``pre`` collects the hidden pre-activations."""
    n = len(dec) - 1
    ins = []
    h = np.asarray(z, np.float64)
    for i in range(n):
        ins.append(h)
        u = h @ _W(dec, i) + _b(dec, i)
        if pre is not None:
            pre.append(u)
        h = np.maximum(u, 0.0)
    ins.append(h)
    return h @ _W(dec, n) + _b(dec, n), ins


def vae_step(tree, x, eps, w, pre=None):
    """(loss, logs, grads) of vae_loss at float64; grads has the tree's structure."""
    enc, dec = tree["encoder"], tree["decoder"]
    n = len(dec) - 1
    x = np.asarray(x, np.float64)
    eps = np.asarray(eps, np.float64)
    B, D = x.shape
    e_in, h = [], x
    for i in range(n):
        e_in.append(h)
        u = h @ _W(enc, i) + _b(enc, i)
        if pre is not None:
            pre.append(u)
        h = np.maximum(u, 0.0)
    mu = h @ _W(enc, n) + _b(enc, n)
    lv = h @ _W(enc, n + 1) + _b(enc, n + 1)
    L = mu.shape[1]
    std = np.exp(0.5 * lv)
    z = mu + eps * std
    xhat, d_in = decode(dec, z, pre)
    rec = np.mean((x - xhat) ** 2)
    kl = -0.5 * np.mean(1 + lv - mu ** 2 - np.exp(lv))
    loss = (w * rec + kl) / (w + 1)
    logs = {"reconstruction_loss": float(rec), "kl": float(kl), "loss": float(loss)}

    g = {"encoder": {}, "decoder": {}}
    gy = (w / (w + 1)) * 2.0 * (xhat - x) / (B * D)
    for i in range(n, -1, -1):
        g["decoder"][f"Dense_{i}"] = {"kernel": d_in[i].T @ gy, "bias": gy.sum(0)}
        gy = gy @ _W(dec, i).T
        if i > 0:
            gy = gy * (d_in[i] > 0)
    dz = gy
    gmu = dz + mu / (B * L) / (w + 1)
    glv = dz * eps * 0.5 * std - 0.5 * (1 - np.exp(lv)) / (B * L) / (w + 1)
    g["encoder"][f"Dense_{n}"] = {"kernel": h.T @ gmu, "bias": gmu.sum(0)}
    g["encoder"][f"Dense_{n + 1}"] = {"kernel": h.T @ glv, "bias": glv.sum(0)}
    gy = (gmu @ _W(enc, n).T + glv @ _W(enc, n + 1).T) * (h > 0)
    for i in range(n - 1, -1, -1):
        g["encoder"][f"Dense_{i}"] = {"kernel": e_in[i].T @ gy, "bias": gy.sum(0)}
        if i > 0:
            gy = (gy @ _W(enc, i).T) * (e_in[i] > 0)
    return float(loss), logs, g


def relu_margin(tree, x, eps, w) -> float:
    """Smallest |pre-activation| of any hidden ReLU in the float64 forward."""
    pre = []
    vae_step(tree, x, eps, w, pre)
    return min(float(np.abs(u).min()) for u in pre)


def cosine_lr(init_lr: float, decay_steps: int, count: int) -> float:
    c = min(count, decay_steps)
    return init_lr * 0.5 * (1.0 + math.cos(math.pi * c / decay_steps))


def adam_update(tree, grads, m, v, count: int, lr: float):
    """optax.adam; count = updates done so far."""
    t = count + 1
    nt, nm, nv = {}, {}, {}
    for mod in tree:
        nt[mod], nm[mod], nv[mod] = {}, {}, {}
        for layer in tree[mod]:
            nt[mod][layer], nm[mod][layer], nv[mod][layer] = {}, {}, {}
            for leaf in tree[mod][layer]:
                g = grads[mod][layer][leaf]
                mm = 0.9 * m[mod][layer][leaf] + 0.1 * g
                vv = 0.999 * v[mod][layer][leaf] + 0.001 * g * g
                step = lr * (mm / (1 - 0.9 ** t)) / (np.sqrt(vv / (1 - 0.999 ** t)) + 1e-8)
                nt[mod][layer][leaf] = tree[mod][layer][leaf] - step
                nm[mod][layer][leaf], nv[mod][layer][leaf] = mm, vv
    return nt, nm, nv


# ------------------------------------------------------------ device draws
def _key(seed: int):
    return (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def _normal(words):
    """Box-Muller of a counter's words 0 and 1 (emtrain.hip nrand)."""
    u1 = ((words[..., 0] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (words[..., 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _grid(n, L, c2, salt):
    pos, j = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(L, dtype=np.uint32), indexing="ij")
    return np.stack([pos, j, np.full_like(pos, c2), np.full_like(pos, salt)], -1)


def device_eps(seed: int, step: int, B: int, L: int) -> np.ndarray:
    """eps [B][L] of the update at count ``step``: counter (batch position, latent index, step, salt)."""
    return _normal(philox4x32_10(_grid(B, L, step, SALT_EPS), _key(seed)))


def device_z(seed: int, n: int, L: int) -> np.ndarray:
    """z [n][L] of fqlpop_initobs_sample(seed, z = NULL): counter (row, latent index, 0, salt)."""
    return _normal(philox4x32_10(_grid(n, L, 0, SALT_Z), _key(seed)))


def device_rows(seed: int, step: int, B: int, n_rows: int) -> np.ndarray:
    """Dataset rows of the update at count ``step``: counter (batch position, step, salt, 0)."""
    b = np.arange(B, dtype=np.uint32)
    ctr = np.stack([b, np.full(B, step, np.uint32), np.full(B, SALT_ROW, np.uint32), np.zeros(B, np.uint32)], -1)
    w = philox4x32_10(ctr, _key(seed)).astype(np.uint64)
    return (((w[:, 1] << np.uint64(32)) | w[:, 0]) % np.uint64(n_rows)).astype(np.int64)
