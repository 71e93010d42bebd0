"""Population engine: one libfqlpop handle = an alpha-population of FQL agents on one GPU.

Every call below advances ALL active members with one set of member-batched
HIP launches.  This is the object the reference-shaped
surface (``fql.agents.fql.FQLAgent``, ``trainer.Trainer``) drives; it mirrors
the reference call sites it replaces:

* ``Population.step``            <- ``Experiment.train`` loop body
                                    (reference trainer/experiment.py:106-109)
* ``Population.total_loss``      <- ``agent.total_loss(val_batch, grad_params=None)``
                                    (trainer/experiment.py:114-115)
* ``Population.sample_actions``  <- ``agent.sample_actions`` (evaluator/evaluation.py:58-64)
* ``Population.state_dict``      <- ``flax.serialization.to_state_dict(agent)``
                                    (trainer/experiment.py:92,135)
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from fqlpop import _lib
from fqlpop._lib import (HP_KEYS, INFO_STRIDE, STATE_ADAM_M, STATE_ADAM_V, STATE_PARAMS,
                         TRAIN_INFO_KEYS, VAL_INFO_KEYS, check, fptr)


@dataclass
class PopulationConfig:
    """The AgentConfig fields (reference trainer/config.py:5-22) the update reads."""
    obs_dim: int = 28
    action_dim: int = 5
    hidden_dims: tuple = (512, 512, 512, 512)
    batch_size: int = 256
    num_qs: int = 2
    layer_norm: bool = True
    actor_layer_norm: bool = False
    flow_steps: int = 10
    q_agg: str = "mean"
    normalize_q_loss: bool = False
    discount: float = 0.99
    tau: float = 0.005
    lr: float = 3e-4
    use_graph: bool = True

    def to_c(self) -> _lib.Config:
        hd = tuple(self.hidden_dims)
        if len(set(hd)) != 1:
            raise ValueError(f"hidden_dims must be uniform, got {hd}")
        if self.q_agg not in ("mean", "min"):
            raise ValueError(f"q_agg must be 'mean' or 'min', got {self.q_agg!r}")
        return _lib.Config(
            obs_dim=int(self.obs_dim), action_dim=int(self.action_dim),
            hidden_dim=int(hd[0]), num_hidden=len(hd), batch_size=int(self.batch_size),
            num_qs=int(self.num_qs), layer_norm=int(bool(self.layer_norm)),
            actor_layer_norm=int(bool(self.actor_layer_norm)), flow_steps=int(self.flow_steps),
            q_agg_min=int(self.q_agg == "min"), normalize_q_loss=int(bool(self.normalize_q_loss)),
            discount=float(self.discount), tau=float(self.tau), lr=float(self.lr),
            use_graph=int(bool(self.use_graph)))

    @classmethod
    def from_agent_config(cls, cfg: dict, obs_dim: int, action_dim: int, **kw):
        """From an ``asdict(AgentConfig)`` dict (reference trainer/config.py:5-22)."""
        if tuple(cfg.get("actor_hidden_dims", (512,) * 4)) != tuple(cfg.get("value_hidden_dims", (512,) * 4)):
            raise ValueError("actor_hidden_dims must equal value_hidden_dims")
        if cfg.get("encoder") not in (None, "None"):
            raise ValueError("visual encoders are out of scope (encoder must be None)")
        return cls(obs_dim=obs_dim, action_dim=action_dim,
                   hidden_dims=tuple(cfg.get("value_hidden_dims", (512,) * 4)),
                   batch_size=int(cfg.get("batch_size", 256)),
                   layer_norm=bool(cfg.get("layer_norm", True)),
                   actor_layer_norm=bool(cfg.get("actor_layer_norm", False)),
                   flow_steps=int(cfg.get("flow_steps", 10)), q_agg=cfg.get("q_agg", "mean"),
                   normalize_q_loss=bool(cfg.get("normalize_q_loss", False)),
                   discount=float(cfg.get("discount", 0.99)), tau=float(cfg.get("tau", 0.005)),
                   lr=float(cfg.get("lr", 3e-4)), **kw)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


SPLIT_SITES = ("bc_forward", "euler_flow", "onestep_forward", "target_critic", "critic_forward", "critic_backward",
               "onestep_backward", "critic_backward_td")


def split_plan(cfg: "PopulationConfig", n_members: int) -> dict:
    """The split plan (fqlpop_split_plan; no GPU call) of an n_members population with
    ``cfg`` under the current engine options: blocks per 16-column tile per launch site
    (1 = unsplit) and whether the small-population schedule runs."""
    c = cfg.to_c()
    F = (ctypes.c_int * 8)()
    small = ctypes.c_int()
    check(_lib.load_library().fqlpop_split_plan(ctypes.byref(c), int(n_members), F, ctypes.byref(small)))
    out = dict(zip(SPLIT_SITES, [int(x) for x in F]))
    out["small_sched"] = bool(small.value)
    return out


class Population:
    """A population of FQL agents (one alpha and seed per member, and optionally its own
    lr, discount and tau) on one GPU.

    ``hparams``: None, or per member None or a dict with any of "lr", "discount", "tau";
    a missing key means the ``cfg`` value (``set_member_hparams``)."""

    def __init__(self, cfg: PopulationConfig, alphas, seeds, device: int = 0, hparams=None):
        self.lib = _lib.load_library()
        self.cfg = cfg
        alphas = _f32(alphas).reshape(-1)
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        if alphas.shape != seeds.shape:
            raise ValueError("alphas and seeds must have the same length")
        self.n = int(alphas.shape[0])
        self.alphas = alphas.copy()
        self.seeds = seeds.copy()
        self._c = cfg.to_c()
        # the engine reads its options at create: hand it this process's GPU_MAX_HW_QUEUES for
        # this create only (the option is process-wide; later populations see the old value)
        hwq = _lib.hw_queues_from_env()
        prev_hwq = _lib.get_engine_option("hw_queues") if hwq is not None else None
        if hwq is not None:
            _lib.set_engine_option("hw_queues", hwq)
        h = ctypes.c_void_p()
        try:
            check(self.lib.fqlpop_create(ctypes.byref(self._c), self.n, fptr(alphas),
                                         seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                         int(device), ctypes.byref(h)))
        finally:
            if prev_hwq is not None:
                _lib.set_engine_option("hw_queues", prev_hwq)
        self._h = h
        self.synth_capacity = None  # rows per ring once synth_create has run
        self.active = np.ones(self.n, dtype=bool)
        n = ctypes.c_int64()
        check(self.lib.fqlpop_state_size(self._h, ctypes.byref(n)))
        self.state_size = int(n.value)
        self.leaves = self._leaf_table()
        if hparams is not None:
            hparams = list(hparams)
            if len(hparams) != self.n:
                self.close()
                raise ValueError(f"hparams needs one entry per member ({self.n}), got {len(hparams)}")
            try:
                for i, hp in enumerate(hparams):
                    if hp:
                        self.set_member_hparams(i, **hp)
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------------ misc
    def close(self):
        if getattr(self, "_h", None):
            check(self.lib.fqlpop_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def flops_per_member_step(self) -> float:
        """What one train step of this population runs per member (fqlpop_train_step_flops):
        without the metrics-only third of the one-step forward under engine option
        ``lazy_metric``, which runs when the train info is read."""
        fn = getattr(self.lib, "fqlpop_train_step_flops", None)
        if fn is None:  # an A/B build of an older commit (FQLPOP_LIB): every step ran all of it
            return float(self.lib.fqlpop_flops_per_member_step(ctypes.byref(self._c)))
        return float(fn(self._h))

    @property
    def metric_evaluations(self) -> int:
        """Deferred mse evaluations launched so far (fqlpop_metric_evaluations)."""
        n = ctypes.c_int64()
        check(self.lib.fqlpop_metric_evaluations(self._h, ctypes.byref(n)))
        return int(n.value)

    def sync(self):
        check(self.lib.fqlpop_sync(self._h))

    def _leaf_table(self):
        n = ctypes.c_int()
        check(self.lib.fqlpop_num_leaves(self._h, ctypes.byref(n)))
        out = []
        name = ctypes.create_string_buffer(256)
        off = ctypes.c_int64()
        nd = ctypes.c_int()
        shp = (ctypes.c_int64 * 3)()
        for i in range(n.value):
            check(self.lib.fqlpop_leaf_info(self._h, i, name, 256, ctypes.byref(off),
                                            ctypes.byref(nd), shp))
            out.append((name.value.decode(), int(off.value), tuple(int(shp[k]) for k in range(nd.value))))
        return out

    # --------------------------------------------------------------- dataset
    def set_dataset(self, data: dict, which: str = "train"):
        """``data``: dict with observations, actions, rewards, masks,
        next_observations (row-major, any float dtype; torch CUDA tensors on
        this device are used in place)."""
        keys = ("observations", "actions", "rewards", "masks", "next_observations")
        on_dev = all(hasattr(data[k], "is_cuda") and data[k].is_cuda for k in keys)
        if on_dev:
            arrs = [data[k].contiguous().float() for k in keys]
            ptrs = [ctypes.c_void_p(a.data_ptr()) for a in arrs]
            n = int(arrs[0].shape[0])
        else:
            arrs = [_f32(data[k]) for k in keys]
            ptrs = [a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
            n = int(arrs[0].shape[0])
        check(self.lib.fqlpop_set_dataset(self._h, 0 if which == "train" else 1, *ptrs, n, int(on_dev)))

    # ---------------------------------------------------------------- active
    def set_active(self, mask):
        m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint8).reshape(-1))
        if m.shape[0] != self.n:
            raise ValueError("mask length must equal the population size")
        check(self.lib.fqlpop_set_active(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        self.active = m.astype(bool)

    @property
    def active_ids(self):
        return [int(i) for i in np.nonzero(self.active)[0]]

    # ------------------------------------------------------------ hot path
    def step(self, n_steps: int = 1):
        """n_steps population updates (device-side sampling) of every active member."""
        check(self.lib.fqlpop_step(self._h, int(n_steps)))

    def _pack_batches(self, batches):
        B = self.cfg.batch_size
        D, A = self.cfg.obs_dim, self.cfg.action_dim
        parts = []
        for b in batches:
            parts += [_f32(b["observations"]).reshape(B * D), _f32(b["actions"]).reshape(B * A),
                      _f32(b["rewards"]).reshape(B), _f32(b["masks"]).reshape(B),
                      _f32(b["next_observations"]).reshape(B * D)]
        return np.concatenate(parts)

    def _pack_noises(self, noises):
        if noises is None:
            return None
        B, A = self.cfg.batch_size, self.cfg.action_dim
        parts = []
        for nz in noises:
            parts += [_f32(nz["z_next"]).reshape(B * A), _f32(nz["x0"]).reshape(B * A),
                      _f32(nz["t"]).reshape(B), _f32(nz["z_d"]).reshape(B * A),
                      _f32(nz["z_metric"]).reshape(B * A)]
        return np.concatenate(parts)

    def _check_count(self, items, what):
        if items is not None and len(items) != len(self.active_ids):
            raise ValueError(f"one {what} per active member ({len(self.active_ids)}), got {len(items)}")

    def step_injected(self, batches, noises=None):
        """One update of every active member (in slot order) on the given host
        batches.  ``noises`` None: drawn on device; else the parity mode (see
        oracle/fql_oracle.py for the keys)."""
        self._check_count(batches, "batch")
        self._check_count(noises, "noise dict")
        pb = self._pack_batches(batches)
        pn = self._pack_noises(noises)
        check(self.lib.fqlpop_step_injected(self._h, fptr(pb), None if pn is None else fptr(pn)))

    def total_loss(self, batches=None, noises=None):
        """Validation losses of every active member; returns {member: info}.
        ``batches`` None: sampled on device from the val dataset."""
        if batches is None:
            if noises is not None:
                raise ValueError("noises need batches")
            check(self.lib.fqlpop_total_loss(self._h, None, None))
        else:
            self._check_count(batches, "batch")
            self._check_count(noises, "noise dict")
            pb = self._pack_batches(batches)
            pn = self._pack_noises(noises)
            check(self.lib.fqlpop_total_loss(self._h, fptr(pb), None if pn is None else fptr(pn)))
        return self.read_info("val")

    def read_info_array(self, which: str = "train") -> np.ndarray:
        out = np.zeros((self.n, INFO_STRIDE), dtype=np.float32)
        check(self.lib.fqlpop_read_info(self._h, 0 if which == "train" else 1, fptr(out)))
        return out

    def read_info(self, which: str = "train") -> dict:
        arr = self.read_info_array(which)
        keys = TRAIN_INFO_KEYS if which == "train" else VAL_INFO_KEYS
        return {i: {k: float(arr[i, j]) for j, k in enumerate(keys)} for i in self.active_ids}

    def sample_actions(self, member: int, observations, noise=None, seed: int = 0) -> np.ndarray:
        obs = _f32(observations)
        squeeze = obs.ndim == 1
        obs = obs.reshape(-1, self.cfg.obs_dim)
        n = obs.shape[0]
        out = np.zeros((n, self.cfg.action_dim), dtype=np.float32)
        nz = None if noise is None else _f32(noise).reshape(n, self.cfg.action_dim)
        check(self.lib.fqlpop_sample_actions(self._h, int(member), fptr(obs), n,
                                             None if nz is None else fptr(nz),
                                             ctypes.c_uint64(int(seed) & (2**64 - 1)), fptr(out)))
        return out[0] if squeeze else out

    def act(self, observations, seed: int = 0, t: int = 1, noise=None, return_noise: bool = False):
        """``sample_actions`` for every ACTIVE member in one launch (fqlpop_act), each on its
        own observations [n_active, n_envs, obs_dim] (slot order); returns actions
        [n_active, n_envs, action_dim].  ``noise`` [n_active, n_envs, action_dim] injects z;
        None draws it on the device as ``rollout`` draws its policy noise at step ``t`` (from
        1) under ``seed``.  return_noise: also the z used.  Reads parameters only; waits for
        the steps enqueued before it."""
        D, A = self.cfg.obs_dim, self.cfg.action_dim
        nz = len(self.active_ids)
        obs = _f32(observations)
        if obs.ndim != 3 or obs.shape[0] != nz or obs.shape[2] != D:
            raise ValueError(f"observations must have shape ({nz}, n_envs, {D}), got {obs.shape}")
        n_envs = int(obs.shape[1])
        z = None
        if noise is not None:
            z = _f32(noise)
            if z.shape != (nz, n_envs, A):
                raise ValueError(f"noise must have shape {(nz, n_envs, A)}, got {z.shape}")
        out = np.zeros((nz, n_envs, A), dtype=np.float32)
        used = np.zeros((nz, n_envs, A), dtype=np.float32) if return_noise else None
        check(self.lib.fqlpop_act(self._h, fptr(obs), n_envs, None if z is None else fptr(z),
                                  ctypes.c_uint64(int(seed) & (2**64 - 1)), ctypes.c_uint32(int(t) & 0xFFFFFFFF),
                                  fptr(out), None if used is None else fptr(used)))
        return (out, used) if return_noise else out

    def last_act_us(self) -> float:
        """GPU time of the act kernel in the last ``act`` call (fqlpop_act_time), microseconds."""
        us = ctypes.c_double()
        check(self.lib.fqlpop_act_time(self._h, ctypes.byref(us)))
        return us.value

    # ------------------------------------------------------ world-model eval
    def set_env_model(self, sp_flat, tp_flat, sp_hidden=(128, 256, 128), tp_hidden=(128, 128)):
        """Upload a BaselineStatePredictor / TerminationPredictor pair as flat
        flax-ordered parameter vectors (envmodel.flatten_state_predictor / ...)."""
        c = _lib.EnvModelConfig()
        c.obs_dim, c.action_dim = self.cfg.obs_dim, self.cfg.action_dim
        c.sp_num_hidden = len(sp_hidden)
        c.tp_num_hidden = len(tp_hidden)
        for i, d in enumerate(sp_hidden):
            c.sp_hidden[i] = int(d)
        for i, d in enumerate(tp_hidden):
            c.tp_hidden[i] = int(d)
        n_sp, n_tp = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.fqlpop_envmodel_param_count(ctypes.byref(c), ctypes.byref(n_sp), ctypes.byref(n_tp)))
        sp = _f32(sp_flat).reshape(-1)
        tp = _f32(tp_flat).reshape(-1)
        if sp.shape[0] != n_sp.value or tp.shape[0] != n_tp.value:
            raise ValueError(f"env-model sizes {sp.shape[0]}/{tp.shape[0]} != expected {n_sp.value}/{n_tp.value}")
        check(self.lib.fqlpop_set_env_model(self._h, ctypes.byref(c), fptr(sp), sp.shape[0], fptr(tp), tp.shape[0]))
        self._em_cfg = c

    def rollout(self, init_obs, max_steps: int, seed: int = 0, noise=None, return_obs: bool = False,
                record: bool = False):
        """World-model evaluation of every ACTIVE member in one launch.

        Returns (success [n_active, n_envs], lengths [n_active, n_envs]) and,
        with return_obs, the observations after the last step [n_active, n_envs, obs].
        With record (fqlpop_rollout_record) the transitions follow: traj_obs
        [n_active, max_steps, n_envs, obs] and traj_act [n_active, max_steps, n_envs, act],
        entry [t] the observation before step t + 1 and the clipped action taken there, 0
        from an env's episode length on."""
        obs = _f32(init_obs).reshape(-1, self.cfg.obs_dim)
        n_envs = obs.shape[0]
        na = len(self.active_ids)
        nz = None
        if noise is not None:
            nz = _f32(noise).reshape(na, int(max_steps), n_envs, self.cfg.action_dim)
        out = np.zeros((na, n_envs, 2), dtype=np.float32)
        oobs = np.zeros((na, n_envs, self.cfg.obs_dim), dtype=np.float32) if return_obs else None
        args = (self._h, fptr(obs), n_envs, int(max_steps), ctypes.c_uint64(int(seed) & (2**64 - 1)),
                None if nz is None else fptr(nz), fptr(out), None if oobs is None else fptr(oobs))
        res = [out[..., 0], out[..., 1]] + ([oobs] if return_obs else [])
        if record:
            tobs = np.zeros((na, int(max_steps), n_envs, self.cfg.obs_dim), dtype=np.float32)
            tact = np.zeros((na, int(max_steps), n_envs, self.cfg.action_dim), dtype=np.float32)
            check(self.lib.fqlpop_rollout_record(*args, fptr(tobs), fptr(tact)))
            res += [tobs, tact]
        else:
            check(self.lib.fqlpop_rollout(*args))
        return tuple(res)

    def envmodel_replay(self, init_obs, actions, next_obs=None, anchor_obs=None, lengths=None,
                        anchor_every: int = 0, return_obs: bool = False) -> dict:
        """Open-loop replay of recorded actions through the env model, every episode in one
        launch (fqlpop_envmodel_replay): init_obs [n, obs], actions [n, T, act], next_obs /
        anchor_obs None or [n, T, obs] (recorded observation after / before step t), lengths
        None or [n] in 1..T.  Every anchor_every steps (0: never) the state is reset to
        anchor_obs[:, t].  Returns {"logits" [n, T]} plus "mse" / "mae" [n, T] (over the
        observation dims, against next_obs) when next_obs is given and "obs" [n, T, obs]
        with return_obs; entries at t >= lengths are 0."""
        D, A = self.cfg.obs_dim, self.cfg.action_dim
        obs = _f32(init_obs).reshape(-1, D)
        n = obs.shape[0]
        act = _f32(actions)
        if act.ndim != 3 or act.shape[0] != n or act.shape[2] != A:
            raise ValueError(f"actions must be [n={n}, T, {A}], got {act.shape}")
        T = act.shape[1]

        def _seq(a, what):
            if a is None:
                return None
            a = _f32(a)
            if a.shape != (n, T, D):
                raise ValueError(f"{what} must be [{n}, {T}, {D}], got {a.shape}")
            return a
        nxt, anc = _seq(next_obs, "next_obs"), _seq(anchor_obs, "anchor_obs")
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int32)
            if ln.shape[0] != n:
                raise ValueError(f"lengths must have {n} entries")
        logits = np.zeros((n, T), dtype=np.float32)
        err = np.zeros((n, T, 2), dtype=np.float32) if nxt is not None else None
        oobs = np.zeros((n, T, D), dtype=np.float32) if return_obs else None
        opt = lambda a: None if a is None else fptr(a)  # noqa: E731
        check(self.lib.fqlpop_envmodel_replay(
            self._h, fptr(obs), fptr(act), opt(nxt), opt(anc),
            None if ln is None else ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            n, T, int(anchor_every), fptr(logits), opt(err), opt(oobs)))
        out = {"logits": logits}
        if err is not None:
            out["mse"], out["mae"] = err[..., 0], err[..., 1]
        if oobs is not None:
            out["obs"] = oobs
        return out

    def envmodel_step(self, observations, actions):
        """One state-predictor + termination-predictor step on the GPU:
        returns (next_observations [n, obs], termination logits [n])."""
        obs = _f32(observations).reshape(-1, self.cfg.obs_dim)
        act = _f32(actions).reshape(-1, self.cfg.action_dim)
        n = obs.shape[0]
        if act.shape[0] != n:
            raise ValueError("observations and actions differ in rows")
        nxt = np.zeros_like(obs)
        logit = np.zeros(n, dtype=np.float32)
        check(self.lib.fqlpop_envmodel_step(self._h, fptr(obs), fptr(act), n, fptr(nxt), fptr(logit)))
        return nxt, logit

    def replay_kernel_us(self) -> float:
        """GPU time of the replay kernel in the last envmodel_replay call (HIP events)."""
        us = ctypes.c_double()
        check(self.lib.fqlpop_envmodel_replay_time(self._h, ctypes.byref(us)))
        return us.value

    # --------------------------------------------------- world-model ensemble
    def set_env_model_ensemble(self, sp_flats, tp_flats, sp_hidden=(128, 256, 128), tp_hidden=(128, 128)):
        """Upload K env models of one shape (fqlpop_set_env_model_ensemble): sp_flats a
        sequence of K flat state-predictor vectors, tp_flats K flat termination-predictor
        vectors or a single one, repeated K times.  Stored apart from set_env_model's model."""
        c = _lib.EnvModelConfig()
        c.obs_dim, c.action_dim = self.cfg.obs_dim, self.cfg.action_dim
        c.sp_num_hidden = len(sp_hidden)
        c.tp_num_hidden = len(tp_hidden)
        for i, d in enumerate(sp_hidden):
            c.sp_hidden[i] = int(d)
        for i, d in enumerate(tp_hidden):
            c.tp_hidden[i] = int(d)
        sps = [_f32(s).reshape(-1) for s in sp_flats]
        k = len(sps)
        if isinstance(tp_flats, np.ndarray) and tp_flats.ndim == 1:
            tp_flats = [tp_flats]
        tps = [_f32(t).reshape(-1) for t in tp_flats]
        if len(tps) == 1 and k > 1:
            tps = tps * k
        if len(tps) != k:
            raise ValueError(f"{k} state predictors but {len(tps)} termination predictors")
        n_sp = sps[0].shape[0] if sps else 0
        n_tp = tps[0].shape[0] if tps else 0
        if any(s.shape[0] != n_sp for s in sps) or any(t.shape[0] != n_tp for t in tps):
            raise ValueError("the models of an ensemble must share one shape")
        sp = _f32(np.stack(sps)) if sps else np.zeros((1, 1), np.float32)
        tp = _f32(np.stack(tps)) if tps else np.zeros((1, 1), np.float32)
        check(self.lib.fqlpop_set_env_model_ensemble(self._h, ctypes.byref(c), k, fptr(sp), n_sp, fptr(tp), n_tp))
        self._ens_n = k

    def rollout_ensemble(self, init_obs, max_steps: int, seed: int = 0, mode: str = "per_model", noise=None,
                         choice=None, return_obs: bool = False, record: bool = False, uncertainty: bool = False):
        """World-model evaluation of every ACTIVE member under the ensemble in one launch
        (fqlpop_rollout_ensemble).  noise None or [n_active, max_steps, n_envs, act], shared
        by all models.

        mode "per_model": every member under every model; returns (success, lengths), each
        [n_active, K, n_envs], slice k bit for bit ``rollout`` after ``set_env_model(k)``.
        mode "mixed" (trajectory sampling): at step t env e steps under model
        choice[t - 1, e] (int [max_steps, n_envs]; None: drawn on the device from ``seed``,
        the same sequence for every member); returns (success, lengths) [n_active, n_envs].
        With return_obs the observations after the last step follow.

        record (mixed only; fqlpop_rollout_ensemble_record) appends traj_obs
        [n_active, max_steps, n_envs, obs], traj_act [.., act] as ``rollout(record=True)``
        and traj_model (int32 [n_active, max_steps, n_envs]: the model of each step);
        uncertainty (implies record) appends traj_unc (float32, same shape): the norm of the
        ensemble's per-coordinate standard deviation of s' at that (s, a), for which every
        step runs all K models.  All are 0 from an env's episode length on; the results
        before them do not change."""
        modes = {"per_model": _lib.ENS_PER_MODEL, "mixed": _lib.ENS_MIXED}
        if mode not in modes:
            raise ValueError(f"mode must be 'per_model' or 'mixed', got {mode!r}")
        record = bool(record or uncertainty)
        if record and mode != "mixed":
            raise ValueError("record / uncertainty need mode='mixed'")
        obs = _f32(init_obs).reshape(-1, self.cfg.obs_dim)
        n_envs = obs.shape[0]
        na = len(self.active_ids)
        nz = None
        if noise is not None:
            nz = _f32(noise).reshape(na, int(max_steps), n_envs, self.cfg.action_dim)
        ch = None
        if choice is not None:
            ch = np.ascontiguousarray(np.asarray(choice), dtype=np.int32).reshape(int(max_steps), n_envs)
        lead = (na, getattr(self, "_ens_n", 1)) if mode == "per_model" else (na,)
        out = np.zeros(lead + (n_envs, 2), dtype=np.float32)
        oobs = np.zeros(lead + (n_envs, self.cfg.obs_dim), dtype=np.float32) if return_obs else None
        args = (self._h, fptr(obs), n_envs, int(max_steps), ctypes.c_uint64(int(seed) & (2**64 - 1)),
                None if nz is None else fptr(nz), modes[mode],
                None if ch is None else ch.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                fptr(out), None if oobs is None else fptr(oobs))
        res = (out[..., 0], out[..., 1]) + ((oobs,) if return_obs else ())
        if not record:
            check(self.lib.fqlpop_rollout_ensemble(*args))
            return res
        tr = (na, int(max_steps), n_envs)
        tobs = np.zeros(tr + (self.cfg.obs_dim,), dtype=np.float32)
        tact = np.zeros(tr + (self.cfg.action_dim,), dtype=np.float32)
        tmodel = np.zeros(tr, dtype=np.int32)
        tunc = np.zeros(tr, dtype=np.float32) if uncertainty else None
        check(self.lib.fqlpop_rollout_ensemble_record(
            *args, fptr(tobs), fptr(tact), tmodel.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            None if tunc is None else fptr(tunc)))
        return res + (tobs, tact, tmodel) + ((tunc,) if uncertainty else ())

    def ensemble_kernel_us(self) -> float:
        """GPU time of the kernel of the last rollout_ensemble call (HIP events)."""
        us = ctypes.c_double()
        check(self.lib.fqlpop_rollout_ensemble_time(self._h, ctypes.byref(us)))
        return us.value

    # ------------------------------------------- training on world-model branches
    def synth_create(self, capacity_rows: int):
        """A ring of ``capacity_rows`` synthetic transitions for every member
        (fqlpop_synth_create); real_ratio starts at 1, so nothing changes until it is lowered."""
        check(self.lib.fqlpop_synth_create(self._h, int(capacity_rows)))
        self.synth_capacity = int(capacity_rows)
        # host mirror of each ring's valid rows as the host's own writes leave them
        # (synth_write, synth_append, synth_append_active, synth_clear; a collect's row count
        # is known on the device only and is not mirrored): read without synchronising
        self.synth_rows_host = np.zeros(self.n, dtype=np.int64)

    def set_real_ratio(self, real_ratio: float):
        """The share of offline rows in the training minibatch (fqlpop_synth_set_ratio): 1
        offline only, 0 ring rows only (while a member's ring is empty it draws offline
        rows).  Holds from the next enqueued step on."""
        check(self.lib.fqlpop_synth_set_ratio(self._h, float(real_ratio)))

    def collect(self, n_branches: int, horizon: int, seed: int, start_rows=None, ensemble: bool = False,
                penalty: float = 0.0):
        """Branches of every ACTIVE member in the env model of ``set_env_model``, appended to
        its ring on the device (fqlpop_synth_collect): ``n_branches`` branches of at most
        ``horizon`` steps from rows of the training dataset -- ``start_rows`` (int
        [n_branches]) or drawn on the device from ``seed`` -- the same rows for every member.
        Stream-ordered with ``step`` and ``clone_members``; returns without waiting.

        ensemble: the branches run under ``set_env_model_ensemble``'s models, a model drawn
        per branch and step from ``seed`` (fqlpop_synth_collect_ensemble; ``set_env_model`` is
        not needed).  penalty > 0 (ensemble only): rewards are lowered by penalty times the
        ensemble's disagreement at that step (``rollout_ensemble(uncertainty=True)``)."""
        sr = None
        if start_rows is not None:
            sr = np.ascontiguousarray(np.asarray(start_rows, dtype=np.int64).reshape(-1))
            if sr.shape[0] != int(n_branches):
                raise ValueError(f"start_rows needs {int(n_branches)} entries, got {sr.shape[0]}")
        if not ensemble and float(penalty) != 0.0:
            raise ValueError("penalty needs ensemble=True")
        args = (self._h, int(n_branches), int(horizon), ctypes.c_uint64(int(seed) & (2**64 - 1)),
                None if sr is None else sr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        if ensemble:
            check(self.lib.fqlpop_synth_collect_ensemble(*args, ctypes.c_float(float(penalty))))
        else:
            check(self.lib.fqlpop_synth_collect(*args))

    def synth_info(self, member: int) -> dict:
        """{"rows", "head", "appended"} of one member's ring; synchronises."""
        r, hd, ap = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.fqlpop_synth_info(self._h, int(member), ctypes.byref(r), ctypes.byref(hd), ctypes.byref(ap)))
        return {"rows": int(r.value), "head": int(hd.value), "appended": int(ap.value)}

    def synth_read(self, member: int, n: int | None = None) -> dict:
        """Ring positions 0 .. n - 1 (default: every valid row) of one member as a dataset
        dict (observations, actions, rewards, masks, next_observations); synchronises."""
        n = self.synth_info(member)["rows"] if n is None else int(n)
        D, A = self.cfg.obs_dim, self.cfg.action_dim
        out = {"observations": np.zeros((n, D), np.float32), "actions": np.zeros((n, A), np.float32),
               "rewards": np.zeros(n, np.float32), "masks": np.zeros(n, np.float32),
               "next_observations": np.zeros((n, D), np.float32)}
        check(self.lib.fqlpop_synth_read(self._h, int(member), fptr(out["observations"]), fptr(out["actions"]),
                                         fptr(out["rewards"]), fptr(out["masks"]), fptr(out["next_observations"]), n))
        return out

    def synth_clear(self, member: int = -1):
        """Empty one member's ring, or (-1) all; stream-ordered."""
        check(self.lib.fqlpop_synth_clear(self._h, int(member)))
        if int(member) < 0:
            self._rows_mirror()[:] = 0
        else:
            self._set_rows(int(member), 0)

    def _synth_rows(self, data) -> tuple[dict, int]:
        """``data`` (a ``synth_read`` dict) as float32 C-contiguous arrays and its row count;
        ValueError for a missing field, a dtype other than float32 or a wrong shape."""
        D, A = self.cfg.obs_dim, self.cfg.action_dim
        tails = {"observations": (D,), "actions": (A,), "rewards": (), "masks": (), "next_observations": (D,)}
        if not isinstance(data, dict) or any(k not in data for k in tails):
            raise ValueError(f"ring rows need the fields {tuple(tails)}")
        out, n = {}, None
        for k, tail in tails.items():
            a = np.asarray(data[k])
            if a.dtype != np.float32:
                raise ValueError(f"ring rows: {k} must be float32, got {a.dtype}")
            n = a.shape[0] if n is None and a.ndim >= 1 else n
            if a.shape != (n,) + tail:
                raise ValueError(f"ring rows: {k} must have shape {(n,) + tail}, got {a.shape}")
            out[k] = np.ascontiguousarray(a)
        return out, int(n)

    def synth_write(self, member: int, data: dict, appended: int | None = None):
        """Ring positions 0 .. n - 1 of one member become ``data`` (the dict ``synth_read``
        returns) and its counters rows = n, head = appended mod capacity, appended
        (fqlpop_synth_write; ``appended`` defaults to the row count).  Stream-ordered with
        ``step``, ``collect`` and ``clone_members``; returns without waiting."""
        rows, n = self._synth_rows(data)
        check(self.lib.fqlpop_synth_write(self._h, int(member), fptr(rows["observations"]), fptr(rows["actions"]),
                                          fptr(rows["rewards"]), fptr(rows["masks"]),
                                          fptr(rows["next_observations"]), n, n if appended is None else int(appended)))
        self._set_rows(int(member), n)

    def synth_append(self, member: int, data: dict):
        """Appends the rows of ``data`` (a dict as ``synth_read`` returns, e.g. transitions
        observed in an environment) to one member's ring as a collect appends its branches
        (fqlpop_synth_append): from the ring's head on, wrapping.  Stream-ordered as
        ``synth_write``: behind a ``collect`` it lands behind that collect's rows."""
        rows, n = self._synth_rows(data)
        check(self.lib.fqlpop_synth_append(self._h, int(member), fptr(rows["observations"]), fptr(rows["actions"]),
                                           fptr(rows["rewards"]), fptr(rows["masks"]),
                                           fptr(rows["next_observations"]), n))
        self._note_appended([int(member)], n)

    def _rows_mirror(self) -> np.ndarray:
        if getattr(self, "synth_rows_host", None) is None:
            self.synth_rows_host = np.zeros(int(getattr(self, "n", 0)), dtype=np.int64)
        return self.synth_rows_host

    def _set_rows(self, member: int, rows: int):
        m = self._rows_mirror()
        if 0 <= member < m.shape[0]:
            m[member] = rows

    def _note_appended(self, members, n: int):
        m = self._rows_mirror()
        for i in members:
            m[i] = min(int(self.synth_capacity), int(m[i]) + int(n))

    def synth_append_active(self, data: dict):
        """``synth_append`` for every ACTIVE member in one call (fqlpop_synth_append_active):
        ``data`` holds the five fields, each [n_active, n, ..] (float32), block z for the z-th
        active member in slot order.  One staging copy and two launches; rings and counters
        end as after one ``synth_append`` per active member."""
        D, A = self.cfg.obs_dim, self.cfg.action_dim
        ids = self.active_ids
        tails = {"observations": (D,), "actions": (A,), "rewards": (), "masks": (), "next_observations": (D,)}
        if not isinstance(data, dict) or any(k not in data for k in tails):
            raise ValueError(f"ring rows need the fields {tuple(tails)}")
        rows, n = {}, None
        for k, tail in tails.items():
            a = np.asarray(data[k])
            if a.dtype != np.float32:
                raise ValueError(f"ring rows: {k} must be float32, got {a.dtype}")
            n = a.shape[1] if n is None and a.ndim >= 2 else n
            if a.shape != (len(ids), n) + tail:
                raise ValueError(f"ring rows: {k} must have shape {(len(ids), n) + tail}, got {a.shape}")
            rows[k] = np.ascontiguousarray(a)
        check(self.lib.fqlpop_synth_append_active(self._h, fptr(rows["observations"]), fptr(rows["actions"]),
                                                  fptr(rows["rewards"]), fptr(rows["masks"]),
                                                  fptr(rows["next_observations"]), int(n)))
        self._note_appended(ids, int(n))

    def synth_state(self, member: int) -> dict:
        """One member's ring for a checkpoint: the ``synth_read`` dict of its valid rows plus
        "appended" and "capacity" (``load_synth_state`` puts it back); synchronises."""
        info = self.synth_info(member)
        state = self.synth_read(member, info["rows"])
        state["appended"] = info["appended"]
        state["capacity"] = int(self.synth_capacity)
        return state

    def load_synth_state(self, member: int, state: dict):
        """Restores ``synth_state``'s dict into one member's ring: rows, positions and
        counters, so that collects and draws continue bit for bit.  ValueError for a state
        of another capacity (positions and wrap would differ)."""
        if not isinstance(state, dict) or "appended" not in state or "capacity" not in state:
            raise ValueError('a ring state needs "appended" and "capacity" (Population.synth_state)')
        capacity = getattr(self, "synth_capacity", None)
        if capacity is None:
            raise ValueError("this population has no rings (synth_create)")
        if int(state["capacity"]) != int(capacity):
            raise ValueError(f"the ring state was saved at capacity {int(state['capacity'])}, this population's rings "
                             f"have capacity {int(capacity)}: positions and wrap would differ")
        rows, n = self._synth_rows(state)
        appended = int(state["appended"])
        if n != min(int(capacity), appended):
            raise ValueError(f"the ring state holds {n} rows, but appended = {appended} at capacity {int(capacity)} "
                             f"means {min(int(capacity), appended)}")
        self.synth_write(member, rows, appended)

    # ----------------------------------------------------------------- state
    def get_flat(self, member: int, which: int = STATE_PARAMS) -> np.ndarray:
        flat = np.zeros(self.state_size, dtype=np.float32)
        check(self.lib.fqlpop_get_state(self._h, int(member), int(which), fptr(flat), self.state_size))
        return flat

    def set_flat(self, member: int, flat, which: int = STATE_PARAMS):
        flat = _f32(flat).reshape(-1)
        if flat.shape[0] != self.state_size:
            raise ValueError("flat state size mismatch")
        check(self.lib.fqlpop_set_state(self._h, int(member), int(which), fptr(flat), self.state_size))

    def flat_to_tree(self, flat) -> dict:
        """Flat state -> {net: {"Dense_0/kernel": array, ...}} (oracle naming)."""
        tree = {}
        for name, off, shape in self.leaves:
            net, leaf = name.split("/", 1)
            size = int(np.prod(shape))
            tree.setdefault(net, {})[leaf] = np.asarray(flat[off:off + size]).reshape(shape).copy()
        return tree

    def tree_to_flat(self, tree) -> np.ndarray:
        flat = np.zeros(self.state_size, dtype=np.float32)
        for name, off, shape in self.leaves:
            net, leaf = name.split("/", 1)
            arr = np.asarray(tree[net][leaf], dtype=np.float32)
            if arr.shape != shape:
                raise ValueError(f"{name}: shape {arr.shape} != {shape}")
            flat[off:off + arr.size] = arr.reshape(-1)
        return flat

    def get_params(self, member: int) -> dict:
        return self.flat_to_tree(self.get_flat(member, STATE_PARAMS))

    def set_params(self, member: int, tree: dict):
        self.set_flat(member, self.tree_to_flat(tree), STATE_PARAMS)

    def get_count(self, member: int) -> int:
        c = ctypes.c_int32()
        check(self.lib.fqlpop_get_count(self._h, int(member), ctypes.byref(c)))
        return int(c.value)

    def set_count(self, member: int, count: int):
        check(self.lib.fqlpop_set_count(self._h, int(member), int(count)))

    def set_member(self, member: int, alpha: float, seed: int, reinit: bool = True):
        check(self.lib.fqlpop_set_member(self._h, int(member), float(alpha),
                                         ctypes.c_uint64(int(seed) & (2**64 - 1)), int(bool(reinit))))
        self.alphas[member] = alpha
        self.seeds[member] = seed

    def set_member_hparams(self, member: int, lr=None, discount=None, tau=None):
        """The member's learning rate, discount and target-EMA tau (fqlpop_set_member_hparams);
        None keeps the current value.  Synchronises; holds from the next enqueued step on,
        without recapturing the step graph.  Members that share (seed, alpha) and differ only
        here draw the same minibatches and noises."""
        cur = self.member_hparams(member)
        new = {"lr": lr, "discount": discount, "tau": tau}
        hp = np.array([cur[k] if new[k] is None else new[k] for k in HP_KEYS], dtype=np.float32)
        check(self.lib.fqlpop_set_member_hparams(self._h, int(member), fptr(hp)))

    def member_hparams(self, member: int) -> dict:
        """{"lr", "discount", "tau"} of one member (the float32 values the kernels read), from
        the engine's host mirror: no synchronisation."""
        hp = np.zeros(len(HP_KEYS), dtype=np.float32)
        check(self.lib.fqlpop_get_member_hparams(self._h, int(member), fptr(hp)))
        return {k: float(hp[j]) for j, k in enumerate(HP_KEYS)}

    def clone_members(self, src, dst, alphas=None, seeds=None, hparams=None):
        """Copy the complete training state of member ``src[i]`` into member ``dst[i]`` on
        the device (fqlpop_clone_members: one launch, stream-ordered between the steps, no
        host staging; it may return before the copy has run).  ``alphas`` / ``seeds`` None:
        every dst keeps its OWN current value -- not the source's, which would make the two
        members draw identical batches forever.  The dst takes the SOURCE's lr, discount and
        tau; ``hparams`` (None, one dict for every pair, or per pair None or a dict as
        ``set_member_hparams`` takes) is applied to the dst after the clone, which then
        synchronises."""
        src = np.ascontiguousarray(np.asarray(src, dtype=np.int32).reshape(-1))
        dst = np.ascontiguousarray(np.asarray(dst, dtype=np.int32).reshape(-1))
        if src.shape != dst.shape:
            raise ValueError("src and dst must have the same length")

        def per_pair(given, own, dtype):
            if given is None:  # (an index out of range: the engine refuses the whole call)
                given = own[np.clip(dst, 0, self.n - 1)]
            return np.ascontiguousarray(np.asarray(given, dtype=dtype).reshape(-1))
        al = per_pair(alphas, self.alphas, np.float32)
        sd = per_pair(seeds, self.seeds, np.uint64)
        if al.shape != dst.shape or sd.shape != dst.shape:
            raise ValueError("alphas and seeds need one entry per pair")
        ip = ctypes.POINTER(ctypes.c_int)
        check(self.lib.fqlpop_clone_members(self._h, int(dst.shape[0]), src.ctypes.data_as(ip), dst.ctypes.data_as(ip),
                                            fptr(al), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        self.alphas[dst] = al
        self.seeds[dst] = sd
        if hparams is not None:
            per = [hparams] * len(dst) if isinstance(hparams, dict) else list(hparams)
            if len(per) != len(dst):
                raise ValueError("hparams needs one entry per pair")
            for d, hp in zip(dst, per):
                if hp:
                    self.set_member_hparams(int(d), **hp)

    def clone_member(self, src: int, dst: int, alpha=None, seed=None, hparams=None):
        """``clone_members`` for one pair."""
        self.clone_members([src], [dst], None if alpha is None else [alpha], None if seed is None else [seed],
                           None if hparams is None else [hparams])

    def state_dict(self, member: int) -> dict:
        """Member state in flax ``to_state_dict`` shape: params (incl. target
        critic), Adam (count, mu, nu) -- names follow oracle/fql_oracle.py."""
        return {"params": self.get_params(member),
                "opt_state": {"count": self.get_count(member),
                              "mu": self.flat_to_tree(self.get_flat(member, STATE_ADAM_M)),
                              "nu": self.flat_to_tree(self.get_flat(member, STATE_ADAM_V))},
                "alpha": float(self.alphas[member]), "seed": int(self.seeds[member])}

    def load_state_dict(self, member: int, sd: dict):
        self.set_params(member, sd["params"])
        self.set_flat(member, self.tree_to_flat(sd["opt_state"]["mu"]), STATE_ADAM_M)
        self.set_flat(member, self.tree_to_flat(sd["opt_state"]["nu"]), STATE_ADAM_V)
        self.set_count(member, int(sd["opt_state"]["count"]))

    def set_probe(self, enable: bool = True):
        check(self.lib.fqlpop_set_probe(self._h, int(bool(enable))))

    def read_probe(self):
        """(mean duration in us, launches, (event_us, stamp_us)) of the dominant
        kernel inside step(); the pair is the last clock cross-check."""
        tot = ctypes.c_double()
        n = ctypes.c_int64()
        cc = (ctypes.c_double * 2)()
        check(self.lib.fqlpop_read_probe(self._h, ctypes.byref(tot), ctypes.byref(n), cc))
        mean = tot.value / n.value if n.value else float("nan")
        return mean, int(n.value), (float(cc[0]), float(cc[1]))

    def probe_coverage(self):
        """(blocks stamped, blocks launched) over the probed launches since set_probe."""
        seen, exp = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.fqlpop_probe_coverage(self._h, ctypes.byref(seen), ctypes.byref(exp)))
        return int(seen.value), int(exp.value)

    def dominant_kernel_info(self):
        """(kernel symbol, algorithmic FLOPs, unique HBM bytes) of one launch of
        the step's dominant kernel over the active members."""
        name = ctypes.create_string_buffer(128)
        fl = ctypes.c_double()
        by = ctypes.c_double()
        check(self.lib.fqlpop_dominant_kernel_info(self._h, name, 128, ctypes.byref(fl), ctypes.byref(by)))
        return name.value.decode(), float(fl.value), float(by.value)

    def dominant_kernel_flops(self) -> float:
        """Algorithmic FLOPs of one dominant-kernel launch (all active members)."""
        return self.dominant_kernel_info()[1]

    def time_dominant_kernel(self, iters: int = 50):
        us = ctypes.c_double()
        fl = ctypes.c_double()
        check(self.lib.fqlpop_time_dominant_kernel(self._h, int(iters), ctypes.byref(us), ctypes.byref(fl)))
        return float(us.value), float(fl.value)
