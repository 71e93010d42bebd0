"""Shared test helpers (not a test module)."""
from __future__ import annotations

import contextlib
import functools
from typing import NamedTuple

import numpy as np


@contextlib.contextmanager
def engine_options(**opts):
    """Process-wide engine options (fqlpop_set_engine_option) for the Population
    handles created inside the block; restored to the defaults afterwards."""
    from fqlpop import reset_engine_options, set_engine_option
    try:
        for k, v in opts.items():
            set_engine_option(k, v)
        yield
    finally:
        reset_engine_options()


# Adam moments may differ from the float64 oracle's by this fraction of each leaf's scale
# (max |oracle value|): the GPU accumulates in fp32, and the critic's first-layer
# gradient passes through four LayerNorm backwards (measured up to 1.7e-4 at B = 1024;
# the bound is 1.5x that).
MOMENT_REL = 2.5e-4


class OptimiserChecker:
    """Per-step parity of one member's update, split in two exact parts:

    1. gradients: the Adam moments m_t and v_t of every leaf against the oracle's, within
       MOMENT_REL of the leaf's scale (this covers every gradient element, small leaves too);
    2. the optimiser itself: the GPU's new parameters against optax.adam (eps outside the
       sqrt, bias corrections with count t) applied in float64 to the GPU's OWN previous
       parameters and new moments, and target_critic against the EMA of the GPU's own
       pre-update critic and target -- tight (1e-7 + 1e-6 |p|), so a skipped, partial or
       wrong update of any leaf fails, independently of how well-conditioned its
       gradient is.

    Adam normalises each update, so comparing parameters with the oracle's directly is
    ill-conditioned where a gradient element is ~0; that comparison is kept only as a
    bound (2 lr per step).  Call ``before()`` ahead of each step and ``after(...)`` after.
    """

    def __init__(self, pop, member, lr, tau, b1=0.9, b2=0.999, eps=1e-8):
        self.pop, self.member, self.lr, self.tau = pop, member, lr, tau
        self.b1, self.b2, self.eps = b1, b2, eps
        self.prev = None
        self.worst_moment = 0.0   # largest moment error seen, as a fraction of MOMENT_REL * leaf scale

    def _state(self):
        from fqlpop._lib import STATE_ADAM_M, STATE_ADAM_V, STATE_PARAMS
        return tuple(self.pop.get_flat(self.member, w).astype(np.float64)
                     for w in (STATE_PARAMS, STATE_ADAM_M, STATE_ADAM_V))

    def before(self):
        self.prev = self._state()
        self.count0 = self.pop.get_count(self.member)

    def after(self, params_o, opt_o, steps_done, tag):
        p0, _, _ = self.prev
        p1, m1, v1 = self._state()
        t = self.pop.get_count(self.member)
        assert t == self.count0 + 1, f"{tag}: count {self.count0} -> {t}"
        bc1, bc2 = 1.0 - self.b1 ** t, 1.0 - self.b2 ** t
        bad = []
        for name, off, shape in self.pop.leaves:
            net, leaf = name.split("/", 1)
            sl = slice(off, off + int(np.prod(shape)))
            for what, got, want in (("m", m1, opt_o["m"]), ("v", v1, opt_o["v"])):
                o = np.asarray(want[net][leaf], dtype=np.float64).reshape(-1)
                scale = float(np.abs(o).max()) if o.size else 0.0
                err = float(np.abs(got[sl] - o).max()) if o.size else 0.0
                if scale > 0:
                    self.worst_moment = max(self.worst_moment, err / (MOMENT_REL * scale))
                if err > MOMENT_REL * scale + 1e-30:
                    bad.append(f"{name} adam {what}: max err {err:.3g} vs leaf scale {scale:.3g}")
            if net == "target_critic":
                coff = next(o for n, o, _ in self.pop.leaves if n == "critic/" + leaf)
                want_p = self.tau * p0[coff:coff + (sl.stop - sl.start)] + (1.0 - self.tau) * p0[sl]
            else:
                want_p = p0[sl] - self.lr * (m1[sl] / bc1) / (np.sqrt(v1[sl] / bc2) + self.eps)
            d = np.abs(p1[sl] - want_p)
            if d.size and np.any(d > 1e-7 + 1e-6 * np.abs(want_p)):
                bad.append(f"{name} optimiser: max |p - adam(own p, m, v)| {float(d.max()):.3g}")
            o = np.asarray(params_o[net][leaf], dtype=np.float64).reshape(-1)
            d = np.abs(p1[sl] - o)
            if d.size and float(d.max()) > 2 * self.lr * steps_done + 1e-5:
                bad.append(f"{name} params: max diff from oracle {float(d.max()):.3g} > 2 lr per step")
        assert not bad, f"{tag}:\n" + "\n".join(bad[:20])


def em_leaf_table(names, shapes):
    """[(name, offset, size)] of a flat env-model vector from its leaf names and shapes."""
    out, o = [], 0
    for name, shp in zip(names, shapes):
        n = int(np.prod(shp))
        out.append(("/".join(name) if isinstance(name, tuple) else str(name), o, n))
        o += n
    return out


EM_GRAD_REL = 1e-3          # a leaf's moment increments: this fraction of the leaf's largest one
EM_DIFF_ULPS = 2 * 2.0 ** -23   # ... plus this much of |m1| (|v1|): the increment is a difference of two fp32 values


class EmOptimiserChecker:
    """OptimiserChecker for the env-model trainers (em_adam_kernel behind fqlpop_emtrain_* and
    fqlpop_initobs_*), from ANY state: every step is judged from the trainer's own pre-step
    (p0, m0, v0, count0), so moments need not start at zero and nothing has to be uploaded.

    ``tr`` has ``flat(which)`` (``flat(model, which)`` with ``model`` given) and ``count``;
    ``leaves`` is ``em_leaf_table(...)``.  ``before()`` ahead of the step, then
    ``after(grads, lr_init, steps)`` with the float64 oracle's gradient at the trainer's own p0
    as a flat vector:

    1. gradients, through the moment increments: m1 - 0.9 m0 against 0.1 g and v1 - 0.999 v0
       against 0.001 g^2, each element within EM_GRAD_REL of its leaf's largest expected
       increment plus EM_DIFF_ULPS |m1| (|v1|).  From non-zero moments g is a tenth of m and a
       thousandth of v: the increments, not the moments, carry it;
    2. the optimiser, exactly: p1 against optax.adam in float64 on the trainer's own p0, m1, v1
       with lr = cosine(lr_init, steps)(count0) and bias corrections at count0 + 1, within
       1e-7 + 1e-6 |p|;
    3. count == count0 + 1;
    4. the schedule's clamp: at count0 >= steps the rate is exactly 0, so p1 == p0 bitwise
       (m and v still move).

    ``measure`` returns (ratios, messages): every check's largest error as a fraction of its
    bound (``clamp`` and ``count``: 0 or inf) and one line per leaf that misses."""

    def __init__(self, tr, leaves, model=None, b1=0.9, b2=0.999, eps=1e-8):
        self.tr, self.leaves, self.model = tr, leaves, model
        self.b1, self.b2, self.eps = b1, b2, eps
        self.prev = None

    def _flat32(self, which):
        return self.tr.flat(which) if self.model is None else self.tr.flat(self.model, which)

    def _state(self):
        return tuple(np.asarray(self._flat32(w), np.float32) for w in (0, 1, 2))

    def before(self):
        """The trainer's (p0, m0, v0) as float32; keeps them for ``after``."""
        self.prev = self._state()
        self.count0 = int(self.tr.count)
        return self.prev

    def measure(self, grads, lr_init, steps):
        import math
        p0_32, m0_32, v0_32 = self.prev
        p1_32, m1_32, v1_32 = self._state()
        p0, m0, v0, p1, m1, v1 = (a.astype(np.float64) for a in (p0_32, m0_32, v0_32, p1_32, m1_32, v1_32))
        g = np.asarray(grads, np.float64).reshape(-1)
        assert g.shape == p0.shape, (g.shape, p0.shape)
        c0, t = self.count0, self.count0 + 1
        lr = lr_init * 0.5 * (1.0 + math.cos(math.pi * min(c0, steps) / steps))
        bc1, bc2 = 1.0 - self.b1 ** t, 1.0 - self.b2 ** t
        ratios = {"m": 0.0, "v": 0.0, "opt": 0.0, "clamp": 0.0, "count": 0.0}
        bad = []
        if int(self.tr.count) != t:
            ratios["count"] = float("inf")
            bad.append(f"count {c0} -> {int(self.tr.count)}")
        for name, off, n in self.leaves:
            sl = slice(off, off + n)
            for what, new, inc, want in (("m", m1[sl], m1[sl] - self.b1 * m0[sl], (1 - self.b1) * g[sl]),
                                         ("v", v1[sl], v1[sl] - self.b2 * v0[sl], (1 - self.b2) * g[sl] ** 2)):
                bound = EM_GRAD_REL * float(np.abs(want).max()) + EM_DIFF_ULPS * np.abs(new) + 1e-30
                r = float((np.abs(inc - want) / bound).max())
                ratios[what] = max(ratios[what], r)
                if not r <= 1.0:
                    bad.append(f"{name} adam {what} increment: {r:.3g} of its bound "
                               f"(largest expected {float(np.abs(want).max()):.3g})")
            want_p = p0[sl] - lr * (m1[sl] / bc1) / (np.sqrt(v1[sl] / bc2) + self.eps)
            r = float((np.abs(p1[sl] - want_p) / (1e-7 + 1e-6 * np.abs(want_p))).max())
            ratios["opt"] = max(ratios["opt"], r)
            if not r <= 1.0:
                bad.append(f"{name} optimiser: |p - adam(own p, m, v)| is {r:.3g} of its bound")
            if c0 >= steps and not np.array_equal(p1_32[sl], p0_32[sl]):
                ratios["clamp"] = float("inf")
                bad.append(f"{name}: parameters moved at count {c0} >= steps {steps} "
                           f"({int((p1_32[sl] != p0_32[sl]).sum())} elements)")
        return ratios, bad

    def after(self, grads, lr_init, steps, tag=""):
        ratios, bad = self.measure(grads, lr_init, steps)
        assert not bad, f"{tag}:\n" + "\n".join(bad[:20])
        return ratios


def em_logs_ratio(got: dict, want: dict, rel: float, abs_: float = 1e-7) -> float:
    """Largest |got - want| over pytest.approx(want, rel=rel, abs=abs_)'s tolerance, over the
    keys of ``got``; a nan matches only a nan (inf otherwise)."""
    worst = 0.0
    for k, g in got.items():
        w = float(want[k])
        if np.isnan(w) or np.isnan(g):
            if not (np.isnan(w) and np.isnan(g)):
                return float("inf")
            continue
        worst = max(worst, abs(g - w) / max(rel * abs(w), abs_))
    return worst


# ---------------------------------------------------------------------------
# trained-like states (oracle.fql_oracle.trained_like_params / trained_like_opt_state)
# ---------------------------------------------------------------------------
REL = 1e-4          # info values against the oracle, as tests/test_gpu_parity.py
TRAINED_COUNT = 1000  # the Adam count the trained-like states start from


def f32_tree(tree):
    """A float64 tree holding float32 values: what the device gets, for the oracle."""
    from oracle import fql_oracle as O
    return O.cast_tree(O.cast_tree(tree, np.float32), np.float64)


def device_tree(pop, tree):
    """The oracle's {net: {leaf: array}} tree in the library's leaf shapes (``pop.leaves``).
    They differ at num_qs = 1 only: the oracle keeps the critic's leading ensemble axis
    ([1, in, out]), the library's state layout has none there ([in, out]; include/fqlpop.h)."""
    shapes = {name: shape for name, _, shape in pop.leaves}
    return {net: {k: v[0] if v.shape == (1,) + shapes[f"{net}/{k}"] else v for k, v in leaves.items()}
            for net, leaves in tree.items() if isinstance(leaves, dict)}


def close(a, b, rel=REL, floor=1e-6):
    return abs(a - b) <= rel * max(abs(a), abs(b)) + floor


def check_info(got, want, keys, tag):
    bad = []
    for k in keys:
        g, w = got[k], float(want[k])
        if not close(g, w):
            bad.append(f"{k}: gpu={g:.8g} oracle={w:.8g} rel={abs(g - w) / max(abs(w), 1e-30):.3g}")
    assert not bad, f"{tag}:\n" + "\n".join(bad)


def info_ratio(got, want, keys, rel=REL, floor=1e-6):
    """The largest |got - want| over ``close``'s bound, over ``keys`` (<= 1: check_info passes)."""
    return max(abs(got[k] - float(want[k])) / (rel * max(abs(got[k]), abs(float(want[k]))) + floor) for k in keys)


def synthetic_rows(N, D, A, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((N, D)).astype(np.float32)
    rew = np.where(rng.uniform(size=N) < 0.05, 0.0, -1.0).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1 + 1e-5, 1 - 1e-5, (N, A)).astype(np.float32),
            "rewards": rew, "masks": (1.0 - (rew == 0)).astype(np.float32),
            "next_observations": (obs + 0.05 * rng.standard_normal((N, D))).astype(np.float32)}


class Spec(NamedTuple):
    """One population member at a trained-like state: its configuration, the seed of its
    state and of its injected batches, and how many steps the test takes from there."""
    H: int
    B: int
    seed: int
    alpha: float = 10.0
    n_steps: int = 1
    D: int = 28
    A: int = 5
    q_offset: float = -40.0
    kw: tuple = ()          # further OracleConfig / PopulationConfig fields, as sorted items
    sampled: tuple = ()     # (population seed, dataset rows): the batch and noise are the
    #                         device sampler's own draws at TRAINED_COUNT, not injected
    L: int = 4              # hidden layers, each H wide
    head_scale: float = 3.0  # trained_like_params' factor on both actors' head kernels

    def cfg(self):
        from oracle import fql_oracle as O
        return O.OracleConfig(obs_dim=self.D, action_dim=self.A, hidden_dims=(self.H,) * self.L,
                              batch_size=self.B, alpha=self.alpha, **dict(self.kw))


class TrainedMember:
    """The float64 oracle's account of one Spec, computed once per process and shared by
    every test that starts there (read-only): the state, the batches and noises of each
    step, what every clamp sees in each step, and the oracle's update of each step."""

    def __init__(self, spec: Spec):
        from oracle import fql_oracle as O
        self.spec, self.cfg = spec, spec.cfg()
        cfg, B = self.cfg, spec.B
        self.params = f32_tree(O.trained_like_params(cfg, spec.seed, q_offset=spec.q_offset,
                                                          head_scale=spec.head_scale))
        self.batches, self.noises = [], []
        if spec.sampled:
            from philox_np import draw, sample_key
            pop_seed, N = spec.sampled
            data = O.cast_tree(synthetic_rows(N, spec.D, spec.A, 5), np.float64)
            for step in range(spec.n_steps):
                idx, noise = draw(sample_key(pop_seed, spec.alpha), TRAINED_COUNT + step, B, N, spec.A)
                self.batches.append({k: v[idx] for k, v in data.items()})
                self.noises.append(noise)
        else:
            rng = np.random.default_rng([spec.seed, 1])
            for _ in range(spec.n_steps):
                self.batches.append(f32_tree(O.make_batch(cfg, B, rng)))
                self.noises.append(f32_tree(O.make_noise(cfg, B, rng)))
        _, _, g = O.loss_and_grads(cfg, self.params, self.batches[0], self.noises[0])
        self.opt = f32_tree(O.trained_like_opt_state(self.params, spec.seed, TRAINED_COUNT, g))
        self.sites, self.steps = [], []
        p, o = self.params, self.opt
        for b, n in zip(self.batches, self.noises):
            self.sites.append(O.clamp_sites(cfg, p, b, n))
            p, o, info = O.update(cfg, p, o, b, n)
            self.steps.append((p, o, info))


@functools.lru_cache(maxsize=None)
def trained_member(spec: Spec) -> TrainedMember:
    return TrainedMember(spec)


def saturated_share(x):
    return float((np.abs(x) > 1.0).mean())


def check_clamp_conditions(x, tag):
    """The conditions a trained-like state has to meet at a clamp whose input is ``x``:
    15-85 % of the entries outside [-1, 1], so that the clamp engages and also does not, and
    none within 1e-4 of +-1 (100x the float32 error of these values), so that no clamp
    decision can differ between the device and the float64 oracle."""
    share = saturated_share(x)
    assert 0.15 <= share <= 0.85, f"{tag}: {share:.3f} of the entries outside [-1, 1]"
    margin = float(np.abs(np.abs(x) - 1.0).min())
    assert margin >= 1e-4, f"{tag}: an entry within {margin:.2e} of +-1"


def check_member_conditions(tm: TrainedMember):
    for step, sites in enumerate(tm.sites):
        for k in ("a_pi", "euler", "a_next", "metric"):
            check_clamp_conditions(sites[k], f"{tm.spec} step {step} {k}")
        if tm.cfg.q_agg == "min":
            share = np.bincount(sites["q_target_argmin"], minlength=tm.cfg.num_qs) / tm.spec.B
            assert share.min() >= 0.15, f"{tm.spec} step {step}: min-Q member shares {share}"


def _specs(H, B, seeds, alphas=(4.0, 40.0, 400.0), **kw):
    extra = {k: kw.pop(k) for k in ("n_steps", "D", "A", "q_offset", "sampled", "L", "head_scale")
             if k in kw}
    out = []
    for i, s in enumerate(seeds):
        e = dict(extra)
        if "sampled" in e:   # population seeds differ per member, as the states' seeds do
            e["sampled"] = (e["sampled"][0] + i, e["sampled"][1])
        out.append(Spec(H, B, s, alphas[i], kw=tuple(sorted(kw.items())), **e))
    return tuple(out)


_MIN = dict(q_agg="min", normalize_q_loss=True, q_offset=0.0)   # mixed-sign Q

# Every state tests/test_gpu_parity_trained.py starts from.  The seeds are chosen so that the
# float64 oracle alone meets check_member_conditions (tests/test_oracle.py asserts it on the
# CPU for every entry); nothing here comes from a device's output.
TRAINED = {
    "h64": _specs(64, 64, (500, 501), n_steps=2),
    "h128_no_ln": _specs(128, 64, (501, 502), n_steps=2, layer_norm=False),
    "h1024": _specs(1024, 64, (500, 503)),
    "h512": _specs(512, 64, (500, 502, 504)),                # 1, 2 or 3 members: a prefix
    "h512_d27": _specs(512, 192, (500, 504), D=27, A=5),
    "h512_d42": _specs(512, 192, (500, 503), D=42, A=8),
    "h64_min": _specs(64, 64, (500, 502), n_steps=2, **_MIN),
    "h512_min": _specs(512, 64, (502, 504), **_MIN),
    "h512_sampled": _specs(512, 64, (500, 501), sampled=(17, 100_003)),
}
ALL_TRAINED_SPECS = tuple(sorted({s for group in TRAINED.values() for s in group}))

# sample_actions and the rollout evaluator read the one-step actor of these members
ACTION_SPECS = (TRAINED["h64"][0], TRAINED["h512"][0])
ROLLOUT_SPECS = TRAINED["h512"][:2]
ROLLOUT_ENVS, ROLLOUT_STEPS = 12, 4


def action_probe(spec: Spec, rows=50):
    """(observations, noise) in float32 for a sample_actions call on ``spec``'s state."""
    rng = np.random.default_rng([spec.seed, 2])
    return (rng.standard_normal((rows, spec.D)).astype(np.float32),
            rng.standard_normal((rows, spec.A)).astype(np.float32))


def rollout_case():
    """The env model, initial observations and per-member noise of the trained-like rollout
    test: as tests/test_gpu_envmodel.py's single-block case (termination logits far below 0,
    so nothing terminates and whole trajectories compare), with non-trivial LayerNorm."""
    import envmodel as em
    spec = em.EnvModelSpec(ROLLOUT_SPECS[0].D, ROLLOUT_SPECS[0].A)
    sp = em.init_state_predictor(spec, 0)
    rng = np.random.default_rng(7)
    for k in sp:
        if k.startswith("LayerNorm"):
            sp[k]["scale"] = (1.0 + 0.2 * rng.standard_normal(sp[k]["scale"].shape)).astype(np.float32)
            sp[k]["bias"] = (0.1 * rng.standard_normal(sp[k]["bias"].shape)).astype(np.float32)
    tp = em.init_termination_predictor(spec, 1, scale=0.1, bias=-50.0)
    obs0 = rng.standard_normal((ROLLOUT_ENVS, spec.obs_dim)).astype(np.float32)
    noise = rng.standard_normal((len(ROLLOUT_SPECS), ROLLOUT_STEPS, ROLLOUT_ENVS, spec.action_dim)).astype(np.float32)
    return spec, sp, tp, obs0, noise


def rollout_raw_actions(member: int):
    """The one-step actor's outputs before the clamp, [steps][envs][A], along the float64
    oracle's trajectory of ``rollout_case`` for ROLLOUT_SPECS[member]."""
    from oracle import envmodel_oracle as EO
    from oracle import fql_oracle as O
    _, sp, _, obs0, noise = rollout_case()
    tm = trained_member(ROLLOUT_SPECS[member])
    obs, out = obs0.astype(np.float64), []
    for t in range(ROLLOUT_STEPS):
        raw = O.sample_actions(tm.cfg, tm.params, obs, noise[member, t].astype(np.float64), clip=False)
        out.append(raw)
        obs = EO.state_predictor(sp, obs, np.clip(raw, -1.0, 1.0))
    return np.stack(out)
