"""Initial-observation VAE on the GPU: the reference's ``InitialObservationEnvModel``
and ``vae_loss`` (envmodel/initial_observation.py:8-78), trained and sampled through
``fqlpop_initobs_*`` (include/fqlpop.h).

* encoder: ``relu(Dense(h))`` per hidden dim, then ``mu`` and ``logvar`` heads from the
  last hidden activation (flax names ``encoder/Dense_0 .. Dense_{n-1}``, ``Dense_n`` =
  mu, ``Dense_{n+1}`` = logvar);
* decoder: ``relu(Dense(h))`` per reversed hidden dim, then ``Dense(obs_dim)``
  (``decoder/Dense_0 .. Dense_n``);
* loss ``(w rec + kl) / (w + 1)``; logs ``reconstruction_loss``, ``kl``, ``loss``.

The reference ships the model, its loss and its loader but no trainer; the trainer here
has the surface and the optimiser (cosine-decayed Adam) of its other env-model trainers.
The saved files are the ones distribution_visualizer.py:62-99 reads:
``initial_observation.pt`` (flax msgpack of ``{"params": {"encoder", "decoder"}}``) and
``initial_observation_config.yaml`` (``hidden_dims``, ``latent_dim``).

Flat vectors are flax path-sorted: every ``decoder/...`` leaf before ``encoder/...``,
``Dense_i/bias`` before ``Dense_i/kernel``, i ascending.  ``num_hidden`` is limited to
1..6 so that no index reaches 10 and the string sort stays numeric.  There is no CPU
path: a missing libfqlpop.so raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import yaml

from envmodel import _dense_stack
from envmodel.flax_msgpack import load_flax_msgpack, msgpack_serialize

LOG_KEYS = ("reconstruction_loss", "kl", "loss")
MODEL_NAME = "initial_observation"


@dataclass
class InitialObservationSpec:
    obs_dim: int
    latent_dim: int = 4
    hidden_dims: tuple = field(default=(128,))

    def __post_init__(self):
        self.hidden_dims = tuple(int(h) for h in self.hidden_dims)
        if not 1 <= len(self.hidden_dims) <= 6:
            raise ValueError("hidden_dims must hold 1..6 widths")

    def encoder_dims(self):
        """Trunk only: the two heads map hidden_dims[-1] -> latent_dim."""
        return [self.obs_dim, *self.hidden_dims]

    def decoder_dims(self):
        return [self.latent_dim, *self.hidden_dims[::-1], self.obs_dim]


def init_initial_observation(spec: InitialObservationSpec, seed: int = 0) -> dict:
    """flax-default initialisers (lecun-normal kernels, zero biases), as envmodel._dense_stack."""
    rng = np.random.default_rng(seed)
    n = len(spec.hidden_dims)
    enc = _dense_stack(spec.encoder_dims() + [spec.latent_dim], rng, 1.0)  # trunk + mu
    enc[f"Dense_{n + 1}"] = _dense_stack([spec.hidden_dims[-1], spec.latent_dim], rng, 1.0)["Dense_0"]
    return {"encoder": enc, "decoder": _dense_stack(spec.decoder_dims(), rng, 1.0)}


def leaf_names(spec: InitialObservationSpec):
    """(module, layer, leaf) of the flat vector, in flax's path-sorted order."""
    n = len(spec.hidden_dims)
    names = [("decoder", f"Dense_{i}", leaf) for i in range(n + 1) for leaf in ("bias", "kernel")]
    names += [("encoder", f"Dense_{i}", leaf) for i in range(n + 2) for leaf in ("bias", "kernel")]
    assert names == sorted(names)
    return names


def leaf_shapes(spec: InitialObservationSpec):
    n, d = len(spec.hidden_dims), spec.decoder_dims()
    e = spec.encoder_dims()
    shapes = []
    for mod, layer, leaf in leaf_names(spec):
        i = int(layer.split("_")[1])
        if mod == "decoder":
            k, o = d[i], d[i + 1]
        else:
            k, o = (e[i], e[i + 1]) if i < n else (e[n], spec.latent_dim)
        shapes.append((k, o) if leaf == "kernel" else (o,))
    return shapes


def _unwrap(tree: dict) -> dict:
    return tree["params"] if "params" in tree else tree


def flatten(spec: InitialObservationSpec, tree: dict) -> np.ndarray:
    t = _unwrap(tree)
    parts = []
    for (mod, layer, leaf), shp in zip(leaf_names(spec), leaf_shapes(spec)):
        a = np.asarray(t[mod][layer][leaf], np.float32)
        if a.shape != shp:
            raise ValueError(f"{mod}/{layer}/{leaf}: shape {a.shape}, expected {shp}")
        parts.append(a.reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def unflatten(spec: InitialObservationSpec, flat: np.ndarray) -> dict:
    tree, o = {"encoder": {}, "decoder": {}}, 0
    for (mod, layer, leaf), shp in zip(leaf_names(spec), leaf_shapes(spec)):
        n = int(np.prod(shp))
        tree[mod].setdefault(layer, {})[leaf] = np.asarray(flat[o:o + n]).reshape(shp).copy()
        o += n
    if o != len(flat):
        raise ValueError(f"flat vector has {len(flat)} values, the spec {o}")
    return tree


def spec_from_tree(tree: dict) -> InitialObservationSpec:
    """Shapes of a loaded checkpoint (the decoder alone fixes them)."""
    dec = _unwrap(tree)["decoder"]
    k = [np.asarray(dec[f"Dense_{i}"]["kernel"]).shape for i in range(len(dec))]
    return InitialObservationSpec(k[-1][1], k[0][0], tuple(s[1] for s in k[:-1])[::-1])


def save_initial_observation_model(save_dir, spec: InitialObservationSpec, params: dict) -> None:
    """The two files distribution_visualizer.py:62-99 reads."""
    d = Path(save_dir)
    d.mkdir(parents=True, exist_ok=True)
    t = _unwrap(params)
    with open(d / f"{MODEL_NAME}_config.yaml", "w") as f:
        yaml.safe_dump({"hidden_dims": list(spec.hidden_dims), "latent_dim": int(spec.latent_dim)}, f)
    with open(d / f"{MODEL_NAME}.pt", "wb") as f:
        f.write(msgpack_serialize({"params": {"encoder": t["encoder"], "decoder": t["decoder"]}}))


def load_initial_observation_model(save_dir):
    """(spec, params tree) from ``save_dir``; FileNotFoundError if either file is missing."""
    d = Path(save_dir)
    cfg_path, pt_path = d / f"{MODEL_NAME}_config.yaml", d / f"{MODEL_NAME}.pt"
    if not cfg_path.exists() or not pt_path.exists():
        raise FileNotFoundError(f"initial-observation model not found under {d}")
    with open(cfg_path) as f:
        cfg = yaml.load(f, Loader=yaml.SafeLoader)
    params = _unwrap(load_flax_msgpack(pt_path))
    spec = spec_from_tree(params)
    if list(spec.hidden_dims) != [int(h) for h in cfg["hidden_dims"]] or spec.latent_dim != int(cfg["latent_dim"]):
        raise ValueError(f"{cfg_path} ({cfg}) does not describe the parameters in {pt_path}")
    return spec, params


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


class _Handle:
    """fqlpop_initobs_t with its configuration."""

    def __init__(self, spec, flat, batch_size, steps, init_lr, reconstruction_weight, seed, device):
        from fqlpop._lib import InitObsConfig, check, fptr, load_library
        self.lib, self.check, self.fptr = load_library(), check, fptr
        c = InitObsConfig()
        c.obs_dim, c.latent_dim, c.num_hidden = int(spec.obs_dim), int(spec.latent_dim), len(spec.hidden_dims)
        for i, h in enumerate(spec.hidden_dims):
            c.hidden_dims[i] = int(h)
        c.batch_size, c.steps = int(batch_size), int(steps)
        c.init_lr, c.reconstruction_weight = float(init_lr), float(reconstruction_weight)
        c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg = c
        n = ctypes.c_int64()
        check(self.lib.fqlpop_initobs_param_count(ctypes.byref(c), ctypes.byref(n)))
        flat = _f32(flat)
        if n.value != flat.size:
            raise ValueError(f"parameter count {flat.size} != {n.value}")
        self.n_params = n.value
        h = ctypes.c_void_p()
        check(self.lib.fqlpop_initobs_create(ctypes.byref(c), fptr(flat), flat.size, int(device), ctypes.byref(h)))
        self.h = h

    def sample(self, n: int, seed: int, z=None) -> np.ndarray:
        n = int(n)
        out = np.zeros((max(n, 0), self.cfg.obs_dim), np.float32)
        zp = None
        if z is not None:
            z = _f32(z)
            if z.shape != (n, self.cfg.latent_dim):
                raise ValueError(f"z has shape {z.shape}, expected {(n, self.cfg.latent_dim)}")
            zp = self.fptr(z)
        self.check(self.lib.fqlpop_initobs_sample(self.h, n, int(seed) & 0xFFFFFFFFFFFFFFFF, zp, self.fptr(out)))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.fqlpop_initobs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class InitialObservationTrainer:
    """The surface of the other env-model trainers (envmodel/trainer.py) for the VAE.
    ``config`` is an ``EnvModelTrainerConfig``: ``model_config`` may carry ``hidden_dims``
    and ``latent_dim`` but the shapes that count are ``spec``'s."""

    def __init__(self, spec: InitialObservationSpec, params: dict, train_loader, val_loader, config, logger=None,
                 device: int = 0):
        self.spec, self.config, self.logger = spec, config, logger
        self.train_loader, self.val_loader = train_loader, val_loader
        self._hd = _Handle(spec, flatten(spec, params), config.batch_size, config.steps, config.init_learning_rate,
                           config.reconstruction_weight, config.seed, device)
        self._lib, self._check, self._fptr, self._h = self._hd.lib, self._hd.check, self._hd.fptr, self._hd.h
        self.n_params = self._hd.n_params
        self._val_rng = np.random.default_rng(int(config.seed) + 1)
        ds = getattr(train_loader, "dataset", None) if train_loader is not None else None
        self._device_sampling = isinstance(ds, dict) and "observations" in ds
        if self._device_sampling:
            obs = _f32(ds["observations"]).reshape(-1, spec.obs_dim)
            self._check(self._lib.fqlpop_initobs_set_dataset(self._h, self._fptr(obs), len(obs)))

    def _obs(self, batch) -> np.ndarray:
        obs = _f32(batch["observations"] if isinstance(batch, dict) else batch)
        want = (self.config.batch_size, self.spec.obs_dim)
        if obs.shape != want:
            raise ValueError(f"batch observations have shape {obs.shape}, expected {want}")
        return obs

    def _eps(self, eps) -> np.ndarray:
        eps = _f32(eps)
        want = (self.config.batch_size, self.spec.latent_dim)
        if eps.shape != want:
            raise ValueError(f"eps has shape {eps.shape}, expected {want}")
        return eps

    def train_step(self, state=None, batch=None, eps=None):
        """One update on a host batch; ``eps`` None draws the step's noise on the device."""
        obs = self._obs(batch)
        e = self._eps(eps) if eps is not None else None
        self._check(self._lib.fqlpop_initobs_step_injected(self._h, self._fptr(obs),
                                                           self._fptr(e) if e is not None else None))
        return self, self.read_logs()

    def eval_step(self, state=None, batch=None, eps=None) -> dict:
        """Logs of the current parameters, no update; ``eps`` None draws it from the
        trainer's validation generator on the host."""
        obs = self._obs(batch)
        e = self._eps(eps if eps is not None else self._val_rng.standard_normal((len(obs), self.spec.latent_dim)))
        out = np.zeros(4, np.float32)
        self._check(self._lib.fqlpop_initobs_eval(self._h, self._fptr(obs), self._fptr(e), self._fptr(out)))
        return {k: float(out[i]) for i, k in enumerate(LOG_KEYS)}

    def steps(self, n: int):
        """n updates on device-sampled rows and noise (asynchronous)."""
        self._check(self._lib.fqlpop_initobs_step(self._h, int(n)))

    def read_logs(self) -> dict:
        out = np.zeros(4, np.float32)
        self._check(self._lib.fqlpop_initobs_read_logs(self._h, self._fptr(out)))
        return {k: float(out[i]) for i, k in enumerate(LOG_KEYS)}

    def learning_rate(self, step: int) -> float:
        c = min(step, self.config.steps)
        return self.config.init_learning_rate * 0.5 * (1.0 + np.cos(np.pi * c / self.config.steps))

    def sync(self):
        self._check(self._lib.fqlpop_initobs_sync(self._h))

    @property
    def count(self) -> int:
        c = ctypes.c_int64()
        self._check(self._lib.fqlpop_initobs_get_count(self._h, ctypes.byref(c)))
        return c.value

    def flat(self, which: int = 0) -> np.ndarray:
        out = np.zeros(self.n_params, np.float32)
        self._check(self._lib.fqlpop_initobs_get_params(self._h, int(which), self._fptr(out), self.n_params))
        return out

    @property
    def params(self) -> dict:
        return unflatten(self.spec, self.flat(0))

    def sample(self, n: int, seed: int = 0, z=None) -> np.ndarray:
        """Decoded samples of the current parameters."""
        return self._hd.sample(n, seed, z)

    def _val(self, step: int):
        if self.val_loader is None:
            return
        logs = [self.eval_step(None, self.val_loader.sample(self.config.batch_size))
                for _ in range(self.config.val_batches)]
        if self.logger:
            for k in logs[0]:
                self.logger.log({f"val/{k}": float(np.mean([lg[k] for lg in logs]))}, step=step)

    def train(self) -> None:
        """The loop of the other trainers: val every 100 steps, one update per step, a final val pass."""
        for step in range(self.config.steps):
            if step % 100 == 0:
                self._val(step)
            if self._device_sampling:
                self.steps(1)
                logs = self.read_logs() if self.logger else None
            else:
                _, logs = self.train_step(None, self.train_loader.sample(self.config.batch_size))
            if self.logger:
                self.logger.log({"train/learning_rate": self.learning_rate(step),
                                 **{f"train/{k}": v for k, v in logs.items()}}, step=step)
        self._val(self.config.steps - 1)

    def close(self):
        self._hd.close()
        self._h = None


class InitialObservationSampler:
    """decoder(z), z ~ N(0, 1): what distribution_visualizer.py:92-99 does with the saved
    decoder.  ``params`` needs the decoder only (a missing encoder is zero-filled: the
    handle holds the whole model)."""

    def __init__(self, spec: InitialObservationSpec, params: dict, device: int = 0):
        self.spec = spec
        t = dict(_unwrap(params))
        if "encoder" not in t:
            zero = unflatten(spec, np.zeros(sum(int(np.prod(s)) for s in leaf_shapes(spec)), np.float32))
            t["encoder"] = zero["encoder"]
        self._hd = _Handle(spec, flatten(spec, t), 16, 1, 0.0, 1.0, 0, device)

    def sample(self, n: int, seed: int = 0, z=None) -> np.ndarray:
        """[n][obs_dim]; ``z`` [n][latent_dim] given, or drawn on the device from ``seed``."""
        return self._hd.sample(n, seed, z)

    def close(self):
        self._hd.close()
