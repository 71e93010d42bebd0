"""Env-model trainers on the GPU.

Same surface as the reference's ``StatePredictorTrainer``
(envmodel/state_predictor_trainer.py:22-170) and ``TerminationPredictorTrainer``
(envmodel/termination_predictor_trainer.py:21-171): ``train_step(state, batch)``,
``eval_step(state, batch)``, ``train()``, the cosine-decayed Adam of their
``__init__``, val logs every 100 steps over ``val_batches`` batches.  The step
itself is ``fqlpop_emtrain_*`` (include/fqlpop.h): one fused HIP launch for
forward + loss + backward of the 16-row blocks and one for the Adam update.
There is no CPU path: a missing libfqlpop.so raises.

``StatePredictorEnsembleTrainer`` / ``TerminationPredictorEnsembleTrainer`` train K models
that differ only in seed behind one handle (``fqlpop_emtrain_create_ensemble``): the same
launches with a model axis, model k bitwise the single trainer of seed k [no reference
counterpart: the reference loops over its trainer].

``bootstrap=True`` on any of the four trainers (PETS / MBPO / MOPO) gives every model its own
resample of the dataset's units -- rows, or episodes of the multistep model -- drawn on the
device from the model's seed (``fqlpop_emtrain_set_bootstrap``): ``bootstrap_table(k)`` and
``oob_rows(k)`` read it back, ``eval_oob(n_batches, draw)`` evaluates each model on the units
its resample missed without an upload, and ``train()`` logs that under ``oob/`` at every
validation interval (``draw`` = the step count).

Differences to the reference, by necessity:

* models are specified by ``EnvModelSpec`` + a parameter tree (flax is absent);
  the tree and flat-vector order are flax's (``envmodel.sp_leaf_names``);
* ``train()`` samples minibatches on the device from the loader's dataset
  (uniform with replacement, like ``Dataset.sample``) instead of the global
  numpy stream, when the loader exposes ``dataset``; otherwise it uploads
  ``loader.sample(B)`` every step;
* the dropout mask of the termination trainer is one fixed mask, as in the
  reference (it passes the same ``self.rng`` every step), but drawn by Philox.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import envmodel as em

DEFAULT_FOCAL_ALPHA, DEFAULT_FOCAL_GAMMA, DEFAULT_DROPOUT = 0.25, 2.0, 0.1
SP_LOG_KEYS = ("loss", "next_observation_loss", "termination_loss", "true_termination_loss",
               "false_termination_loss")
TP_TRAIN_LOG_KEYS = ("loss", "true_loss", "false_loss")
TP_EVAL_LOG_KEYS = ("loss", "true_loss", "false_loss", "accuracy", "precision", "recall")
MULTISTEP_EPISODE_LENGTH = 1000  # utils/data_loader.py:30 reshapes the dataset into 1000-step episodes


@dataclass
class EnvModelTrainerConfig:
    """envmodel/config.py:5-20 (TrainerConfig)."""
    seed: int = 0
    steps: int = 2000
    env_name: str = "cube-single-play-singletask-task2-v0"
    model: str = "baseline"
    true_termination_weight: float = 30.0
    termination_weight: float = 1.0
    reconstruction_weight: float = 1.0
    model_config: dict = field(default_factory=dict)
    init_learning_rate: float = 1e-3
    batch_size: int = 256
    sequence_length: int = 256
    val_batches: int = 20
    data_directory: Path = Path("data/")
    save_directory: Path = Path("exp/")


def unflatten(names, shapes, flat: np.ndarray) -> dict:
    tree, o = {}, 0
    for (mod, leaf), shp in zip(names, shapes):
        n = int(np.prod(shp))
        tree.setdefault(mod, {})[leaf] = flat[o:o + n].reshape(shp).copy()
        o += n
    return tree


def _leaf_shapes(names, dims, ln_dim=None):
    shapes = []
    for mod, leaf in names:
        if mod.startswith("Dense_"):
            i = int(mod.split("_")[1])
            shapes.append((dims[i], dims[i + 1]) if leaf == "kernel" else (dims[i + 1],))
        else:
            shapes.append((ln_dim,))
    return shapes


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


class _GpuEnvModelTrainer:
    kind = None

    def __init__(self, spec: em.EnvModelSpec, params: dict, train_loader, val_loader, config: EnvModelTrainerConfig,
                 logger=None, device: int = 0, tp_params: dict | None = None, focal_alpha=DEFAULT_FOCAL_ALPHA,
                 focal_gamma=DEFAULT_FOCAL_GAMMA, dropout_rate=DEFAULT_DROPOUT, bootstrap=False):
        self.bootstrap = bool(bootstrap)
        flat = self._setup(spec, [params], train_loader, val_loader, config, focal_alpha, focal_gamma, dropout_rate)
        self.logger = logger
        h = ctypes.c_void_p()
        self._check(self._lib.fqlpop_emtrain_create(ctypes.byref(self._cfg), self._fptr(flat), flat.size, int(device),
                                                    ctypes.byref(h)))
        self._h = h
        self._finish_setup(tp_params)

    # ------------------------------------------------------------- plumbing
    def _setup(self, spec, params_list, train_loader, val_loader, config, focal_alpha, focal_gamma, dropout_rate):
        """The C config (self._cfg), the leaf layout, and the flat [len(params_list)][P] parameters."""
        from fqlpop._lib import EM_MULTISTEP, EmTrainConfig, check, fptr, load_library
        self._lib, self._check, self._fptr = load_library(), check, fptr
        self.spec, self.config = spec, config
        self.train_loader, self.val_loader = train_loader, val_loader
        # the multistep model (train_env_model.py:46-66) trains the same cell through a scan
        self._ms = self.kind == 0 and getattr(config, "model", "baseline") == "multistep"
        self._T = int(config.sequence_length) if self._ms else 1
        c = EmTrainConfig()
        c.kind = EM_MULTISTEP if self._ms else self.kind
        c.sequence_length = self._T
        c.episode_length = int(getattr(train_loader, "episode_length", MULTISTEP_EPISODE_LENGTH)) if self._ms else 0
        c.obs_dim, c.action_dim = spec.obs_dim, spec.action_dim
        hid = spec.sp_hidden if self.kind == 0 else spec.tp_hidden
        c.num_hidden = len(hid)
        for i, hdim in enumerate(hid):
            c.hidden_dims[i] = int(hdim)
        c.batch_size, c.steps = int(config.batch_size), int(config.steps)
        c.init_lr = float(config.init_learning_rate)
        c.termination_weight = float(config.termination_weight) if self.kind == 0 else 0.0
        c.true_termination_weight = float(config.true_termination_weight)
        c.focal_alpha, c.focal_gamma, c.dropout_rate = float(focal_alpha), float(focal_gamma), float(dropout_rate)
        c.seed = int(config.seed) & 0xFFFFFFFFFFFFFFFF
        c.tp_num_hidden = len(spec.tp_hidden)
        for i, hdim in enumerate(spec.tp_hidden):
            c.tp_hidden_dims[i] = int(hdim)
        self._cfg = c
        if self.kind == 0:
            self._names = em.sp_leaf_names(spec)
            self._shapes = _leaf_shapes(self._names, spec.sp_dims(), spec.obs_dim + spec.action_dim)
            flats = [em.flatten_state_predictor(spec, p) for p in params_list]
        else:
            self._names = em.tp_leaf_names(spec)
            self._shapes = _leaf_shapes(self._names, spec.tp_dims())
            flats = [em.flatten_termination_predictor(spec, p) for p in params_list]
        n = ctypes.c_int64()
        check(self._lib.fqlpop_emtrain_param_count(ctypes.byref(c), ctypes.byref(n)))
        for flat in flats:
            if n.value != flat.size:
                raise ValueError(f"parameter count {flat.size} != {n.value}")
        self.n_params = n.value
        return _f32(np.concatenate([np.asarray(f, np.float32).reshape(-1) for f in flats]))

    def _finish_setup(self, tp_params):
        """The shared frozen termination predictor and the device-resident dataset."""
        if self.kind == 0 and self._cfg.termination_weight > 0:
            if tp_params is None:
                raise ValueError("termination_weight > 0 needs the trained termination predictor (tp_params)")
            tflat = _f32(em.flatten_termination_predictor(self.spec, tp_params))
            self._check(self._lib.fqlpop_emtrain_set_frozen_termination(self._h, self._fptr(tflat), tflat.size))
        ds = getattr(self.train_loader, "dataset", None) if self.train_loader is not None else None
        self._device_sampling = isinstance(ds, dict) and "observations" in ds
        if self._device_sampling:
            self._set_dataset(ds)
        if getattr(self, "bootstrap", False):
            if not self._device_sampling:
                raise ValueError("bootstrap needs device sampling: a loader exposing its dataset dict")
            self.set_bootstrap(True)

    def _set_dataset(self, ds: dict):
        # rows (a multistep loader holds [episodes][episode_length][..]: flattened back to rows)
        D, A = self.spec.obs_dim, self.spec.action_dim
        obs = _f32(ds["observations"]).reshape(-1, D)
        act = _f32(ds["actions"]).reshape(-1, A) if "actions" in ds else np.zeros((len(obs), A), np.float32)
        arrs = [obs, np.ascontiguousarray(act), _f32(ds["rewards"]).reshape(-1),
                _f32(ds["next_observations"]).reshape(-1, D)]
        self._check(self._lib.fqlpop_emtrain_set_dataset(self._h, *[self._fptr(a) for a in arrs], len(arrs[0])))

    # ------------------------------------------------------------ bootstrap
    _n_models = 1

    @property
    def n_units(self) -> int:
        """Units the device draw resamples: dataset rows, or episodes of the multistep model."""
        ds = self.train_loader.dataset["observations"]
        n = int(np.prod(np.shape(ds)[:-1]))
        return n // self._cfg.episode_length if self._ms else n

    def set_bootstrap(self, enable: bool = True, table=None):
        """Draw every model's resample and out-of-bag list on the device (fqlpop_emtrain_set_bootstrap),
        install the caller's ``table`` [K][n_units] instead, or drop them (``enable=False``)."""
        if table is not None:
            t = np.ascontiguousarray(np.asarray(table, np.int64))
            self._check(self._lib.fqlpop_emtrain_set_bootstrap_table(
                self._h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), t.size))
        else:
            self._check(self._lib.fqlpop_emtrain_set_bootstrap(self._h, 1 if enable else 0))
        self.bootstrap = bool(enable) or table is not None

    def _get_bootstrap(self, k: int):
        n = self.n_units
        i64 = ctypes.POINTER(ctypes.c_int64)
        table, oob, n_oob = np.zeros(n, np.int64), np.zeros(n, np.int64), ctypes.c_int64()
        self._check(self._lib.fqlpop_emtrain_get_bootstrap(self._h, int(k), table.ctypes.data_as(i64), n,
                                                           oob.ctypes.data_as(i64), n, ctypes.byref(n_oob)))
        return table, oob[:n_oob.value].copy()

    def bootstrap_table(self, k: int = 0) -> np.ndarray:
        """Model k's resample [n_units]: a device-sampled step trains on unit table[u]."""
        return self._get_bootstrap(k)[0]

    def oob_rows(self, k: int = 0) -> np.ndarray:
        """The units model k's resample misses (its out-of-bag set), ascending."""
        return self._get_bootstrap(k)[1]

    def _eval_oob_raw(self, n_batches: int, draw: int) -> np.ndarray:
        out = np.zeros((self._n_models, 8), np.float32)
        self._check(self._lib.fqlpop_emtrain_eval_oob(self._h, int(n_batches), int(draw) & 0xFFFFFFFFFFFFFFFF,
                                                      self._fptr(out)))
        return out

    def eval_oob(self, n_batches: int, draw: int):
        """eval_step averaged over n_batches out-of-bag batches drawn on the device (no upload, one
        synchronisation): a log dict (K of them on an ensemble trainer)."""
        out = self._eval_oob_raw(n_batches, draw)
        logs = [self._logs(out[k], self._eval_keys()) for k in range(self._n_models)]
        return logs if isinstance(self, _GpuEnvModelEnsembleTrainer) else logs[0]

    def _batch_ptrs(self, batch: dict):
        B = self.config.batch_size
        arrs = [_f32(batch["observations"]),
                _f32(batch.get("actions", np.zeros(np.shape(batch["observations"])[:-1] + (self.spec.action_dim,)))),
                _f32(batch["rewards"]), _f32(batch["next_observations"])]
        if arrs[0].shape[0] != B:
            raise ValueError(f"batch has {arrs[0].shape[0]} rows, batch_size is {B}")
        if self._ms and (arrs[0].ndim != 3 or arrs[0].shape[1] != self._T):
            raise ValueError(f"multistep batches are [B, {self._T}, ..], got {arrs[0].shape}")
        return arrs

    def _logs(self, v: np.ndarray, keys) -> dict:
        return {k: float(v[i]) for i, k in enumerate(keys)}

    # --------------------------------------------------------- reference API
    def train_step(self, state=None, batch: dict | None = None, keep_mask: np.ndarray | None = None):
        """One update on a host batch; returns (state, logs) like the reference's jitted step."""
        arrs = self._batch_ptrs(batch)
        km = None
        if keep_mask is not None:
            km = np.ascontiguousarray(np.asarray(keep_mask, np.uint8))
        self._check(self._lib.fqlpop_emtrain_step_injected(
            self._h, *[self._fptr(a) for a in arrs],
            km.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if km is not None else None))
        return self, self.read_logs()

    def eval_step(self, state=None, batch: dict | None = None) -> dict:
        arrs = self._batch_ptrs(batch)
        out = np.zeros(8, np.float32)
        self._check(self._lib.fqlpop_emtrain_eval(self._h, *[self._fptr(a) for a in arrs], self._fptr(out)))
        return self._logs(out, self._eval_keys())

    def steps(self, n: int):
        """n updates on device-sampled batches (asynchronous)."""
        if not self._device_sampling:
            raise RuntimeError("device sampling needs a loader exposing its dataset dict")
        self._check(self._lib.fqlpop_emtrain_step(self._h, int(n)))

    def read_logs(self) -> dict:
        out = np.zeros(8, np.float32)
        self._check(self._lib.fqlpop_emtrain_read_logs(self._h, self._fptr(out)))
        return self._logs(out, self._train_keys())

    def learning_rate(self, step: int) -> float:
        """optax.cosine_decay_schedule(init_learning_rate, steps)(step)."""
        c = min(step, self.config.steps)
        return self.config.init_learning_rate * 0.5 * (1.0 + np.cos(np.pi * c / self.config.steps))

    def sync(self):
        self._check(self._lib.fqlpop_emtrain_sync(self._h))

    @property
    def count(self) -> int:
        c = ctypes.c_int64()
        self._check(self._lib.fqlpop_emtrain_get_count(self._h, ctypes.byref(c)))
        return c.value

    @property
    def plan(self) -> dict:
        """The launch plan chosen at creation: ``sweep`` (the multistep step runs em_sweep_kernel +
        em_seq_dw_kernel, not em_seq_grad_kernel), ``tchunks`` (T chunks of its dW GEMM) and
        ``blocks`` (16-row blocks per model)."""
        v = [ctypes.c_int() for _ in range(3)]
        self._check(self._lib.fqlpop_emtrain_get_plan(self._h, *[ctypes.byref(x) for x in v]))
        return {"sweep": bool(v[0].value), "tchunks": v[1].value, "blocks": v[2].value}

    def flat(self, which: int = 0) -> np.ndarray:
        out = np.zeros(self.n_params, np.float32)
        self._check(self._lib.fqlpop_emtrain_get_params(self._h, int(which), self._fptr(out), self.n_params))
        return out

    @property
    def params(self) -> dict:
        return unflatten(self._names, self._shapes, self.flat(0))

    def _val(self, step: int):
        if self.val_loader is None:
            return self._oob(step)
        logs = [self.eval_step(None, self.val_loader.sample(self.config.batch_size))
                for _ in range(self.config.val_batches)]
        if self.logger:
            for k in logs[0]:
                self.logger.log({f"val/{k}": float(np.mean([lg[k] for lg in logs]))}, step=step)
        self._oob(step)

    def _oob(self, step: int):
        """Out-of-bag logs at a validation interval (bootstrap on): draw = the step count."""
        if not self.bootstrap:
            return
        self.last_oob = self.eval_oob(self.config.val_batches, self.count)
        if self.logger:
            self.logger.log({f"oob/{k}": v for k, v in self.last_oob.items()}, step=step)

    def train(self) -> None:
        """The reference loop (state_predictor_trainer.py:119-170): val every 100
        steps, one update per step, a final val pass."""
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
        # the reference logs the final pass at the last loop index (step = steps - 1,
        # state_predictor_trainer.py:160-175), so the val curves line up when overlaid
        self._val(self.config.steps - 1)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fqlpop_emtrain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StatePredictorTrainer(_GpuEnvModelTrainer):
    """envmodel/state_predictor_trainer.py:22-170: the baseline model, or the multistep
    model (envmodel/multistep.py) when ``config.model == "multistep"`` -- then batches
    are [B, sequence_length, ..] windows and ``params`` is the scanned cell's tree."""
    kind = 0

    def _train_keys(self):
        return SP_LOG_KEYS if self._cfg.termination_weight > 0 else SP_LOG_KEYS[:2]

    _eval_keys = _train_keys


class TerminationPredictorTrainer(_GpuEnvModelTrainer):
    """envmodel/termination_predictor_trainer.py:21-171 (focal loss, dropout)."""
    kind = 1

    def _train_keys(self):
        return TP_TRAIN_LOG_KEYS

    def _eval_keys(self):
        return TP_EVAL_LOG_KEYS


class _GpuEnvModelEnsembleTrainer(_GpuEnvModelTrainer):
    """K models of one kind behind one handle (fqlpop_emtrain_create_ensemble): every train
    step is one launch chain for all K.  The models share the spec, the config (schedule, step
    count, batch size), the dataset and the frozen termination predictor; model k has its own
    initial tree, seed (minibatch draw, dropout mask), logger and val sampling stream.  Model
    k is bitwise the single trainer built with ``config.seed = seeds[k]`` and
    ``params_list[k]``."""

    def __init__(self, spec: em.EnvModelSpec, params_list, train_loader, val_loader, config: EnvModelTrainerConfig,
                 seeds, loggers=None, device: int = 0, tp_params: dict | None = None, val_rngs=None,
                 focal_alpha=DEFAULT_FOCAL_ALPHA, focal_gamma=DEFAULT_FOCAL_GAMMA, dropout_rate=DEFAULT_DROPOUT,
                 bootstrap=False):
        self.bootstrap = bool(bootstrap)
        self.K = len(params_list)
        self.seeds = [int(s) for s in seeds]
        if len(self.seeds) != self.K:
            raise ValueError(f"{self.K} parameter trees but {len(self.seeds)} seeds")
        self.loggers = list(loggers) if loggers is not None else None
        if self.loggers is not None and len(self.loggers) != self.K:
            raise ValueError(f"{self.K} models but {len(self.loggers)} loggers")
        # per-model val sampling: model k's host batches come from its own stream (the sequential
        # runs draw them from the global stream after np.random.seed(seed_k): the same draws)
        self.val_rngs = list(val_rngs) if val_rngs is not None else [np.random.RandomState(s) for s in self.seeds]
        if len(self.val_rngs) != self.K:
            raise ValueError(f"{self.K} models but {len(self.val_rngs)} val streams")
        flat = self._setup(spec, list(params_list), train_loader, val_loader, config, focal_alpha, focal_gamma,
                           dropout_rate)
        sd = (ctypes.c_uint64 * self.K)(*[s & 0xFFFFFFFFFFFFFFFF for s in self.seeds])
        h = ctypes.c_void_p()
        self._check(self._lib.fqlpop_emtrain_create_ensemble(ctypes.byref(self._cfg), self.K, self._fptr(flat),
                                                             flat.size, sd, int(device), ctypes.byref(h)))
        self._h = h
        self._finish_setup(tp_params)

    @property
    def logger(self):
        return self.loggers

    @property
    def _n_models(self):
        return self.K

    # --------------------------------------------------------------- batches
    def _ens_batch(self, batches):
        """One batch dict (shared by all models) or K of them -> (stacked arrays, shared flag)."""
        if isinstance(batches, dict):
            return self._batch_ptrs(batches), 1
        if len(batches) != self.K:
            raise ValueError(f"{self.K} models but {len(batches)} batches")
        per = [self._batch_ptrs(b) for b in batches]
        return [np.ascontiguousarray(np.stack([p[i] for p in per])) for i in range(4)], 0

    def train_step(self, state=None, batches=None, keep_masks=None):
        """One update of every model on host batches (a dict: one batch for all; a list: one per
        model); keep_masks likewise one [B][D] mask or K of them.  Returns (self, K log dicts)."""
        arrs, shared = self._ens_batch(batches)
        km = None
        if keep_masks is not None:
            km = np.ascontiguousarray(np.asarray(keep_masks, np.uint8))
            want = 2 if shared else 3
            if km.ndim != want:
                raise ValueError("keep_masks must be one [B][D] mask with a shared batch, K of them otherwise")
        self._check(self._lib.fqlpop_emtrain_step_injected_ensemble(
            self._h, *[self._fptr(a) for a in arrs],
            km.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if km is not None else None, shared))
        return self, self.read_logs()

    def eval_step(self, state=None, batches=None) -> list:
        arrs, shared = self._ens_batch(batches)
        out = np.zeros((self.K, 8), np.float32)
        self._check(self._lib.fqlpop_emtrain_eval_ensemble(self._h, *[self._fptr(a) for a in arrs], shared,
                                                           self._fptr(out)))
        return [self._logs(out[k], self._eval_keys()) for k in range(self.K)]

    def read_logs_raw(self) -> np.ndarray:
        out = np.zeros((self.K, 8), np.float32)
        self._check(self._lib.fqlpop_emtrain_read_logs_ensemble(self._h, self._fptr(out)))
        return out

    def read_logs(self) -> list:
        out = self.read_logs_raw()
        return [self._logs(out[k], self._train_keys()) for k in range(self.K)]

    def flat(self, k: int, which: int = 0) -> np.ndarray:
        out = np.zeros(self.n_params, np.float32)
        self._check(self._lib.fqlpop_emtrain_get_params_model(self._h, int(k), int(which), self._fptr(out),
                                                              self.n_params))
        return out

    @property
    def params(self) -> list:
        return [unflatten(self._names, self._shapes, self.flat(k, 0)) for k in range(self.K)]

    def _sample(self, loader, k: int) -> dict:
        return loader.sample(self.config.batch_size, rng=self.val_rngs[k])

    def _val(self, step: int):
        if self.val_loader is None:
            return self._oob(step)
        logs = [self.eval_step(None, [self._sample(self.val_loader, k) for k in range(self.K)])
                for _ in range(self.config.val_batches)]
        if self.loggers:
            for k in range(self.K):
                for key in logs[0][k]:
                    self.loggers[k].log({f"val/{key}": float(np.mean([lg[k][key] for lg in logs]))}, step=step)
        self._oob(step)

    def _oob(self, step: int):
        if not self.bootstrap:
            return
        self.last_oob = self.eval_oob(self.config.val_batches, self.count)
        if self.loggers:
            for k in range(self.K):
                self.loggers[k].log({f"oob/{key}": v for key, v in self.last_oob[k].items()}, step=step)

    def train(self) -> None:
        """The reference loop once for all K models: val every 100 steps, one update of every
        model per step, one log read for all K, K log rows, a final val pass."""
        for step in range(self.config.steps):
            if step % 100 == 0:
                self._val(step)
            if self._device_sampling:
                self.steps(1)
                logs = self.read_logs() if self.loggers else None
            else:
                _, logs = self.train_step(None, [self._sample(self.train_loader, k) for k in range(self.K)])
            if self.loggers:
                lr = self.learning_rate(step)
                for k in range(self.K):
                    self.loggers[k].log({"train/learning_rate": lr,
                                         **{f"train/{key}": v for key, v in logs[k].items()}}, step=step)
        self._val(self.config.steps - 1)


class StatePredictorEnsembleTrainer(_GpuEnvModelEnsembleTrainer):
    """K StatePredictorTrainer runs (baseline or multistep) as one launch per step."""
    kind = 0
    _train_keys = StatePredictorTrainer._train_keys
    _eval_keys = StatePredictorTrainer._eval_keys


class TerminationPredictorEnsembleTrainer(_GpuEnvModelEnsembleTrainer):
    """K TerminationPredictorTrainer runs as one launch per step."""
    kind = 1
    _train_keys = TerminationPredictorTrainer._train_keys
    _eval_keys = TerminationPredictorTrainer._eval_keys
