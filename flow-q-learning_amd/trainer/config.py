"""Run configuration dataclasses.

Field names, defaults and types follow the reference's trainer/config.py:5-44
(AgentConfig, ExperimentConfig, TrainerConfig) so configs, checkpoints and the
argparser round-trip unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path


@dataclass
class AgentConfig:
    seed: int = 0
    agent_name: str = "fql"
    ob_dims: int | None = None
    action_dim: int | None = None
    lr: float = 3e-4
    batch_size: int = 256
    actor_hidden_dims: tuple = (512, 512, 512, 512)
    value_hidden_dims: tuple = (512, 512, 512, 512)
    layer_norm: bool = True
    actor_layer_norm: bool = False
    discount: float = 0.99
    tau: float = 0.005
    q_agg: str = "mean"
    alpha: float = 10.0
    flow_steps: int = 10
    normalize_q_loss: bool = False
    encoder: str | None = None


@dataclass(frozen=True)
class ExperimentConfig:
    """One population member: the tuned hyper-parameters (hashable: used as a
    dict key by Trainer and the HPO strategies).  ``seed`` and ``alpha`` are the
    reference's fields; ``lr``, ``discount`` and ``tau`` [no reference counterpart] are the
    member's own values in the population engine (Population.set_member_hparams).  A
    field left None means the TrainerConfig's AgentConfig value, and appears neither in the
    experiment name nor in ``member_eval_seed``."""
    seed: int | None = None
    alpha: float | None = None
    lr: float | None = None
    discount: float | None = None
    tau: float | None = None


@dataclass
class ModelRolloutConfig:
    """Training on world-model branches (no reference counterpart, so not a TrainerConfig
    field: that class mirrors the reference's).  Off while ``branches`` is 0.  Every
    ``interval`` updates, once a group has passed ``warmup`` updates, each member rolls
    ``branches`` branches of at most ``horizon`` steps in the task's env model into its
    ring of ``buffer_rows`` rows; the training minibatch takes the share ``real_ratio`` of
    its rows from the offline data and the rest from the ring.  With ``ensemble`` the
    branches run under the task's env-model ensemble, a model drawn per branch and step
    (trajectory sampling), and ``penalty`` > 0 lowers a synthetic reward by that factor
    times the ensemble's disagreement about the step (a MOPO-style uncertainty penalty)."""
    branches: int = 0
    horizon: int = 5
    interval: int = 1000
    warmup: int = 0
    real_ratio: float = 0.5
    buffer_rows: int = 100_000
    ensemble: bool = False
    penalty: float = 0.0

    @property
    def enabled(self) -> bool:
        return self.branches > 0

    def validate(self) -> None:
        if not self.enabled:
            return
        if self.horizon < 1 or self.interval < 1 or self.warmup < 0:
            raise ValueError("model rollouts need horizon >= 1, interval >= 1 and warmup >= 0")
        if not 0.0 <= self.real_ratio <= 1.0:
            raise ValueError(f"model_real_ratio must be in [0, 1], got {self.real_ratio}")
        if not self.penalty >= 0.0 or self.penalty == float("inf"):
            raise ValueError(f"model_rollout_penalty must be finite and >= 0, got {self.penalty}")
        if self.penalty > 0.0 and not self.ensemble:
            raise ValueError("model_rollout_penalty needs --model_rollout_ensemble: the penalty is the "
                             "ensemble's disagreement")
        if self.branches * self.horizon > self.buffer_rows:
            raise ValueError(f"model_buffer_rows {self.buffer_rows} holds less than one collect "
                             f"({self.branches} branches x {self.horizon} steps)")


@dataclass
class OnlineConfig:
    """Offline-to-online fine-tuning (FQL's main.py after its offline steps; not a
    TrainerConfig field, as ModelRolloutConfig).  Off while ``steps`` is 0.  The last
    ``steps`` of the run's updates are online: for every ``utd`` updates each member acts
    once in its own ``envs`` environments (one ``Population.act`` for the whole group) and
    the observed transitions go into its ring of ``buffer_rows`` rows.  ``real_ratio`` is the
    share of offline rows in the minibatch, or "auto": n_offline / (n_offline + ring rows),
    FQL's uniform draw over dataset and online data together."""
    steps: int = 0
    envs: int = 8
    utd: int = 1
    buffer_rows: int = 100_000
    real_ratio: float | str = "auto"

    @property
    def enabled(self) -> bool:
        return self.steps > 0

    def validate(self) -> None:
        if not self.enabled:
            return
        if self.envs < 1 or self.utd < 1:
            raise ValueError("an online phase needs online_envs >= 1 and online_utd >= 1")
        if self.envs > self.buffer_rows:
            raise ValueError(f"online_buffer_rows {self.buffer_rows} holds less than one environment step "
                             f"({self.envs} envs)")
        if isinstance(self.real_ratio, str):
            if self.real_ratio != "auto":
                raise ValueError(f"online_real_ratio must be 'auto' or a number in [0, 1], got {self.real_ratio!r}")
        elif not 0.0 <= float(self.real_ratio) <= 1.0:
            raise ValueError(f"online_real_ratio must be in [0, 1], got {self.real_ratio}")

    def ratio(self, n_offline: int, ring_rows: int) -> float:
        """The real_ratio to train under when a member's ring holds ``ring_rows`` rows."""
        if self.real_ratio == "auto":
            return float(n_offline) / float(n_offline + ring_rows)
        return float(self.real_ratio)


@dataclass
class TrainerConfig:
    seed: int = 0
    steps: int = 1_000_000
    log_interval: int = 5_000
    eval_interval: int = 100_000
    save_directory: Path = Path("exp/")
    data_directory: Path = Path("data/")
    use_wandb: bool = False
    env_name: str = "cube-single-play-singletask-task2-v0"
    agent: AgentConfig = field(default_factory=AgentConfig)
    eval_episodes: int = 50
    buffer_size: int = 2_000_000
