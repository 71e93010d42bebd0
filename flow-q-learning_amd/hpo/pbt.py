"""Population-based training of alpha (and lr, discount, tau): truncation exploit + perturb explore.

[no reference counterpart: the reference ships Identity and SuccessiveHalving only]

Every ``ready_interval`` evaluations the ``k = max(1, int(n * truncation))`` (at most
``n // 2``) worst candidates, ranked by the mean of their last ``history_length`` scores,
are replaced by children of the ``k`` best: a child has its parent's alpha times a factor
from ``perturb_factors`` (clipped to ``alpha_bounds``), a fresh seed and a copy of the
parent's score history.  The population keeps its size for the whole run, so the
member-batched engine stays at the member count it is fastest at (successive halving
empties it), and the run yields an alpha schedule (``lineage``), not just one alpha.

``explore`` (default ``("alpha",)``: exactly the above) names the fields a child perturbs, a
subset of alpha, lr, discount, tau, processed in that fixed order with one
``rng.choice(perturb_factors)`` each: alpha, lr and tau are multiplied by the factor, discount
moves through ``1 - discount`` (0.99 under 1.25 becomes 0.9875: the effective horizon scales
by 1 / factor).  A field that is not explored is the parent's.  ``bounds`` maps a field to
(lo, hi), either may be None; ``alpha_bounds`` is ``bounds["alpha"]``; discount and tau are
kept in [0, 1], which the engine requires.  ``base`` gives the population defaults
(AgentConfig's lr, discount, tau) that stand in where a parent leaves an explored field None.
The member-batched engine keeps the three per member (``Population.set_member_hparams``), so
a child's values hold from its clone on.  Lineage rows carry ``parent_<f>`` / ``child_<f>``
for the explored fields beyond alpha.

``parent_of`` maps every child to its parent: the Trainer keys its cloning on it
(``Population.clone_members`` copies the parent's training state into the freed slot).

Deterministic: ties are broken by ``fqlpop.distributed.config_key`` order and every draw
comes from the strategy's own ``random.Random(seed)``; the global ``random`` /
``np.random`` streams are never touched (trainer/trainer.py, determinism note).
"""
from __future__ import annotations

import random
from collections import defaultdict

from fqlpop.distributed import config_key
from hpo.strategy import HpoStrategy
from trainer.config import ExperimentConfig

SEED_RANGE = 10000  # tune_alpha.py draws the initial seeds from range(10000) too
FIELDS = ("alpha", "lr", "discount", "tau")  # the order explored fields are perturbed in
DEFAULT_BOUNDS = {"discount": (0.0, 1.0), "tau": (0.0, 1.0)}  # the engine's ranges


class PopulationBasedTraining(HpoStrategy):
    def __init__(self, population, total_evaluations: int, ready_interval: int = 1, truncation: float = 0.25,
                 perturb_factors=(0.8, 1.25), alpha_bounds=None, history_length: int = 1, seed: int = 0,
                 state_dict: dict | None = None, explore=("alpha",), bounds=None, base=None) -> None:
        super().__init__(set(population), total_evaluations, state_dict)
        if ready_interval < 1 or history_length < 1:
            raise ValueError("ready_interval and history_length must be >= 1")
        if not 0.0 < truncation <= 0.5:
            raise ValueError("truncation must be in (0, 0.5]")
        if not perturb_factors:
            raise ValueError("perturb_factors must not be empty")
        self.ready_interval = int(ready_interval)
        self.truncation = float(truncation)
        self.perturb_factors = tuple(float(f) for f in perturb_factors)
        self.alpha_bounds = None if alpha_bounds is None else (alpha_bounds[0], alpha_bounds[1])
        unknown = [f for f in explore if f not in FIELDS]
        if unknown:
            raise ValueError(f"explore must be a subset of {FIELDS}, got {unknown}")
        self.explore = tuple(f for f in FIELDS if f in explore)
        self.bounds = dict(DEFAULT_BOUNDS)
        for f, b in (bounds or {}).items():
            if f not in FIELDS:
                raise ValueError(f"bounds: unknown field {f!r}")
            self.bounds[f] = (b[0], b[1])
        if "alpha" in self.bounds:
            if self.alpha_bounds is not None and self.alpha_bounds != self.bounds["alpha"]:
                raise ValueError("alpha_bounds and bounds['alpha'] disagree: give one of them")
            self.alpha_bounds = self.bounds["alpha"]
        self.bounds["alpha"] = self.alpha_bounds
        self.base = dict(base or {})
        for f in self.explore:
            if f != "alpha" and self.base.get(f) is None and any(getattr(c, f, None) is None for c in population):
                raise ValueError(f"explore {f!r}: a candidate leaves it None and base gives no default")
        self.history_length = int(history_length)
        self.rng = random.Random(seed)
        self.candidate_scores = defaultdict(list)
        self.performed_evaluations = 0
        self.parent_of = {}
        self.lineage = []        # one row per clone, see _exploit
        self.exploit_rounds = 0
        self.last_exploit = -1   # performed_evaluations at the last exploit round: sample() twice is idempotent
        if state_dict is not None:
            self.population = set(state_dict["population"])
            self.candidate_scores = defaultdict(list, {c: list(s) for c, s in state_dict["candidate_scores"].items()})
            self.performed_evaluations = state_dict["performed_evaluations"]
            self.parent_of = dict(state_dict["parent_of"])
            self.lineage = [dict(row) for row in state_dict["lineage"]]
            self.exploit_rounds = state_dict["exploit_rounds"]
            self.last_exploit = state_dict["last_exploit"]
            self.rng.setstate(state_dict["rng_state"])

    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["population"] = set(self.population)
        sd["candidate_scores"] = {c: list(s) for c, s in self.candidate_scores.items()}
        sd["performed_evaluations"] = self.performed_evaluations
        sd["parent_of"] = dict(self.parent_of)
        sd["lineage"] = [dict(row) for row in self.lineage]
        sd["exploit_rounds"] = self.exploit_rounds
        sd["last_exploit"] = self.last_exploit
        sd["rng_state"] = self.rng.getstate()
        return sd

    def update(self, candidate, performance: float) -> None:
        history = self.candidate_scores[candidate]
        history.append(performance)
        if len(history) > self.performed_evaluations:
            self.performed_evaluations = len(history)

    def _mean_recent(self, candidate) -> float:
        recent = self.candidate_scores[candidate][-self.history_length:]
        return sum(recent) / len(recent) if recent else float("-inf")

    def _clip(self, alpha: float, field: str = "alpha") -> float:
        bounds = self.bounds.get(field)
        if bounds is None:
            return alpha
        lo, hi = bounds
        if lo is not None:
            alpha = max(float(lo), alpha)
        if hi is not None:
            alpha = min(float(hi), alpha)
        return alpha

    def _value(self, cfg, field: str):
        v = getattr(cfg, field, None)
        return self.base.get(field) if v is None and field != "alpha" else v

    def _perturb(self, field: str, value: float, factor: float) -> float:
        if field == "discount":
            return self._clip(1.0 - (1.0 - value) * factor, field)
        return self._clip(value * factor, field)

    def _fresh_seed(self, used: set) -> int:
        if len(used) >= SEED_RANGE:
            raise RuntimeError(f"every seed in range({SEED_RANGE}) is used")
        while True:
            s = self.rng.randrange(SEED_RANGE)
            if s not in used:
                used.add(s)
                return s

    def sample(self):
        ready = (self.performed_evaluations >= self.history_length
                 and self.performed_evaluations % self.ready_interval == 0
                 and self.performed_evaluations != self.last_exploit)
        if ready:
            self._exploit()
        return self.population

    def _exploit(self) -> None:
        self.last_exploit = self.performed_evaluations
        n = len(self.population)
        k = min(max(1, int(n * self.truncation)), n // 2)
        if k < 1:
            return
        # best first; equal means in config_key order
        ranked = sorted(self.population, key=lambda c: (-self._mean_recent(c), config_key(c)))
        best, worst = ranked[:k], ranked[n - k:]
        used = {c.seed for c in list(self.candidate_scores) + list(self.population) + list(self.parent_of)
                if c.seed is not None}
        population = set(self.population)
        for loser in worst:
            parent = self.rng.choice(best)
            fields = {f: getattr(parent, f, None) for f in FIELDS}  # not explored: the parent's
            for f in self.explore:
                factor = self.rng.choice(self.perturb_factors)
                fields[f] = self._perturb(f, self._value(parent, f), factor)
            child = ExperimentConfig(seed=self._fresh_seed(used), **fields)
            self.candidate_scores[child] = list(self.candidate_scores[parent])
            self.parent_of[child] = parent
            row = {"round": self.exploit_rounds, "child": child, "parent": parent,
                   "parent_alpha": parent.alpha, "child_alpha": child.alpha,
                   "parent_score": self._mean_recent(parent)}
            for f in self.explore:
                if f != "alpha":
                    row[f"parent_{f}"], row[f"child_{f}"] = self._value(parent, f), getattr(child, f)
            self.lineage.append(row)
            population.discard(loser)
            population.add(child)
        self.population = population
        self.exploit_rounds += 1
