"""Env-model trainers (csrc/emtrain.hip) against the float64 oracle at edge shapes and from
trained-like states: random biases in every layer of both nets (the frozen termination
predictor's too), Adam moments and a count left by device-sampled warm-up steps, the cosine
schedule at half its rate and past its end.  Every checked step is judged from the device's own
pre-step state by EmOptimiserChecker (tests/_helpers.py): gradients through the increments of
both Adam moments, the optimiser exactly, the count, the schedule's clamp; logs at the
tolerances of tests/test_gpu_emtrain.py.  The shapes are tests/_emtrain_cases.py's; every
multistep case asserts the path it ran through the trainer's ``plan``.

Each test prints ``EMPARITY <case> <check>=<largest error / bound> ...`` (pytest -s)."""
import contextlib

import numpy as np
import pytest

import _emtrain_cases as C
import envmodel as em
import initobs_np as V
from _helpers import EmOptimiserChecker, em_leaf_table, em_logs_ratio, engine_options
from envmodel import initial_observation as io
from envmodel.trainer import (EnvModelTrainerConfig, StatePredictorEnsembleTrainer, StatePredictorTrainer,
                              TerminationPredictorTrainer)
from test_gpu_emtrain import _dynamics_dataset, _Loader, _trajectory_dataset
from test_gpu_initobs import PARITY_CASES, _manifold_data

pytestmark = pytest.mark.gpu

W_SINGLE, W_MULTI, W_VAE = 1000, 200, 300


def _report(tag, ratios):
    print("EMPARITY", tag, " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def _merge(acc, ratios):
    for k, v in ratios.items():
        acc[k] = max(acc.get(k, 0.0), v)


def _trainer(kind, shape, tw, B, steps, T_=1, seed=3):
    """A trainer of ``kind`` on ``shape`` from random-bias parameters, with a small synthetic
    dataset for device-sampled warm-up; returns (trainer, frozen predictor's float64 tree)."""
    spec = C.spec_of(shape)
    D, A = spec.obs_dim, spec.action_dim
    sp, tp = C.random_bias_params(shape, 11)
    ds = _trajectory_dataset(2, D, A, seed=4) if kind == "multistep" else _dynamics_dataset(2000, D, A, seed=4)
    cfg = EnvModelTrainerConfig(steps=steps, model="multistep" if kind == "multistep" else "baseline",
                                sequence_length=T_, termination_weight=tw, batch_size=B, init_learning_rate=C.LR,
                                seed=seed)
    if kind == "termination":
        return TerminationPredictorTrainer(spec, tp, _Loader(ds), None, cfg), None
    return StatePredictorTrainer(spec, sp, _Loader(ds), None, cfg, tp_params=tp if tw > 0 else None), C.f64(tp)


def _checked_steps(tr, kind, shape, tw, tp64, B, T_, steps, p_terms, rng, others=None):
    """The checked steps of one single-model trainer (or, with ``others``, of every model of an
    ensemble trainer at once): returns the largest error / bound of every check."""
    spec = C.spec_of(shape)
    D, A = spec.obs_dim, spec.action_dim
    names, shapes = C.layout(shape, kind)
    K = 1 if others is None else others
    cks = [EmOptimiserChecker(tr, em_leaf_table(names, shapes), model=k if others else None) for k in range(K)]
    rel = C.LOG_REL_MS if kind == "multistep" else C.LOG_REL
    keep = (rng.uniform(size=(B, D)) >= 0.1) if kind == "termination" else None
    acc = {}
    for step, p_term in enumerate(p_terms):
        picked = []
        for ck in cks:
            p0 = ck.before()[0]
            tree = C.tree_of(names, shapes, p0)
            if kind == "multistep":
                draw = lambda: C.seq_batch(rng, B, T_, D, A, p_term)  # noqa: E731
            else:
                draw = lambda: C.row_batch(rng, B, D, A, p_term)  # noqa: E731
            picked.append(C.batch_with_margin(draw, lambda b: C.oracle_step(kind, tree, b, tw, tp64, keep)))
        if others:
            _, logs = tr.train_step(None, [p[0] for p in picked])
        else:
            _, logs = tr.train_step(None, picked[0][0], keep_mask=keep)
            logs = [logs]
        for k, (ck, (_, want_logs, grads)) in enumerate(zip(cks, picked)):
            r = em_logs_ratio(logs[k], want_logs, rel, C.LOG_ABS)
            assert r <= 1.0, (step, k, logs[k], want_logs)
            _merge(acc, {"logs": r})
            _merge(acc, ck.after(C.flat_of(names, grads), C.LR, steps, tag=f"step {step} model {k}"))
    return acc


# ------------------------------------------------------------------ single step
@pytest.mark.parametrize("kind,tw", [("state", 0.0), ("state", 1.0), ("termination", 0.0)])
@pytest.mark.parametrize("shape,B", C.SINGLE_CASES)
def test_single_step_trainers_from_trained_state(shape, B, kind, tw):
    """em_grad_kernel + em_adam_kernel at half the cosine rate, from non-zero moments.  With a
    frozen predictor (tw = 1) and for the termination predictor the second batch has no
    terminal row and the third only terminal rows (nan logs; the 1e-8 denominators)."""
    tr, tp64 = _trainer(kind, shape, tw, B, 2 * W_SINGLE)
    assert tr.plan == {"sweep": False, "tchunks": 1, "blocks": B // 16}
    tr.steps(W_SINGLE)
    assert tr.count == W_SINGLE
    p_terms = (0.25, 0.25) if (kind == "state" and tw == 0) else (0.3, 0.0, 1.0)
    acc = _checked_steps(tr, kind, shape, tw, tp64, B, 1, 2 * W_SINGLE, p_terms, np.random.default_rng(5))
    _report(f"{kind}-tw{tw:g}-{shape}-B{B}", acc)
    tr.close()


# -------------------------------------------------------------------- multistep
@pytest.mark.parametrize("tw", [0.0, 1.0])
@pytest.mark.parametrize("shape,T_,B,option,sweep,tchunks", C.MULTISTEP_CASES + [C.MULTISTEP_FALLBACK],
                         ids=lambda v: str(v))
def test_multistep_from_trained_state(shape, T_, B, option, sweep, tchunks, tw):
    """em_sweep_kernel + em_seq_dw_kernel (em_seq_sweep = 1), the round-5 em_seq_grad_kernel
    (= 0) and the automatic fallback (shape C, default option), each asserted through ``plan``:
    empty and uneven k-split chunks, odd T, odd T-chunk lengths, a ragged 64-tile."""
    _multistep_case(shape, T_, B, option, sweep, tchunks, tw)


def _multistep_case(shape, T_, B, option, sweep, tchunks, tw):
    ctx = engine_options(em_seq_sweep=option) if option is not None else contextlib.nullcontext()
    with ctx:
        tr, tp64 = _trainer("multistep", shape, tw, B, 2 * W_MULTI, T_)
    assert tr.plan == {"sweep": sweep, "tchunks": tchunks, "blocks": B // 16}
    tr.steps(W_MULTI)
    acc = _checked_steps(tr, "multistep", shape, tw, tp64, B, T_, 2 * W_MULTI, (0.25, 0.25),
                         np.random.default_rng(6))
    _report(f"multistep-tw{tw:g}-{shape}-T{T_}-B{B}-sweep{int(sweep)}", acc)
    tr.close()


@pytest.mark.parametrize("shape,T_,B,option,sweep,tchunks,tw",
                         [(*c[:6], tw) for c in C.MULTISTEP_EDGE_CASES for tw in c[6]], ids=lambda v: str(v))
def test_multistep_at_the_edges_of_the_sweep_plan(shape, T_, B, option, sweep, tchunks, tw):
    """The shapes at and one past every limit of the sweep's admission rule (sw_fits, em_create),
    through test_multistep_from_trained_state's checks: a step's inputs at one value per thread
    with the rewards in the last 16 threads (F) and past that (G, H); its record at SW_RQ floats
    per thread (I, L: under the default frozen predictor) and past that (J); the dynamic LDS that
    fits only without the kernel's static arrays (K); T = 1, no step ahead to load and no carried
    gradient (A).  The rows past an edge run the default option and must fall back by themselves."""
    assert sweep == (C.em_plan(shape, "multistep", tw, T_, B)["sweep"] and option != 0)
    _multistep_case(shape, T_, B, option, sweep, tchunks, tw)


@pytest.mark.parametrize("D,A,hid,tph,tw,sweep", C.PLAN_PROBES, ids=lambda v: str(v).replace(" ", ""))
def test_plan_matches_its_cpu_restatement(D, A, hid, tph, tw, sweep):
    """fqlpop_emtrain_create's choice against em_plan either side of every limit (trainers created
    and closed, no step): tests/test_emtrain_cpu.py proves on em_plan that no admitted shape
    exceeds a limit of the sweep kernel."""
    spec = em.EnvModelSpec(D, A, hid, tph)
    cfg = EnvModelTrainerConfig(steps=10, model="multistep", sequence_length=2, termination_weight=tw,
                                batch_size=16, init_learning_rate=C.LR)
    tr = StatePredictorTrainer(spec, em.init_state_predictor(spec, 0), None, None, cfg,
                               tp_params=em.init_termination_predictor(spec, 1) if tw > 0 else None)
    want = C.em_plan_dims(D, A, hid, tph, "multistep", tw, 2, 16)
    assert want["sweep"] == sweep
    assert tr.plan == {k: want[k] for k in ("sweep", "tchunks", "blocks")}
    tr.close()


def test_first_steps_from_the_constructor_state():
    """Counts 0 and 1 through the same exact checks: bias corrections at t = 1 and 2, where
    1 - b^t is far from 1 (at the trained-like counts b1's has converged)."""
    tr, tp64 = _trainer("state", "A", 1.0, 16, 50)
    acc = _checked_steps(tr, "state", "A", 1.0, tp64, 16, 1, 50, (0.25, 0.25), np.random.default_rng(7))
    assert tr.count == 2
    _report("first-steps-state-A", acc)
    tr.close()


# ------------------------------------------------------------------- the clamp
@pytest.mark.parametrize("kind,shape,B,T_,W", [("state", "B", 48, 1, W_SINGLE), ("termination", "B", 48, 1, W_SINGLE),
                                               ("multistep", "B", 32, 17, W_MULTI)])
def test_schedule_clamp(kind, shape, B, T_, W):
    """steps = W + 2: the checked steps run at counts W .. W + 3, the last two at count >=
    steps, where the rate is exactly 0: parameters bitwise unchanged, moments still moving."""
    tw = 0.0 if kind == "termination" else 1.0
    tr, tp64 = _trainer(kind, shape, tw, B, W + 2, T_)
    tr.steps(W)
    acc = _checked_steps(tr, kind, shape, tw, tp64, B, T_, W + 2, (0.25,) * 4, np.random.default_rng(8))
    assert tr.count == W + 4
    _report(f"clamp-{kind}-{shape}", acc)
    tr.close()


# -------------------------------------------------------------------- ensemble
@pytest.mark.parametrize("xcd", [0, 1])
def test_ensemble_models_from_trained_states(xcd):
    """em_adam_kernel's per-model stride s_par = ceil(P / 64) 64 with P no multiple of 64: every
    model of a K = 3 ensemble, after a warm-up that leaves their states different."""
    shape, B, K = C.ENSEMBLE_CASE
    spec = C.spec_of(shape)
    D, A = spec.obs_dim, spec.action_dim
    trees = [C.random_bias_params(shape, 20 + k) for k in range(K)]
    tp = trees[0][1]
    cfg = EnvModelTrainerConfig(steps=2 * W_SINGLE, termination_weight=1.0, batch_size=B, init_learning_rate=C.LR)
    with engine_options(em_ens_xcd=xcd):
        tr = StatePredictorEnsembleTrainer(spec, [t[0] for t in trees], _Loader(_dynamics_dataset(2000, D, A, seed=4)),
                                           None, cfg, seeds=[7, 8, 9], tp_params=tp)
    assert tr.n_params % 64 != 0
    assert tr.plan["blocks"] == B // 16
    tr.steps(W_SINGLE)
    for which in (0, 1, 2):
        assert not np.array_equal(tr.flat(0, which), tr.flat(1, which))
    acc = _checked_steps(tr, "state", shape, 1.0, C.f64(tp), B, 1, 2 * W_SINGLE, (0.25, 0.25),
                         np.random.default_rng(9), others=K)
    _report(f"ensemble-{shape}-K{K}-xcd{xcd}", acc)
    tr.close()


def test_ensemble_sweep_at_the_full_staging_width():
    """ens_enter shares em_sweep_kernel: both models of a K = 2 multistep ensemble at shape F,
    where every one of the 1024 threads stages one input value."""
    shape, T_, B, K = C.ENSEMBLE_SWEEP_CASE
    spec = C.spec_of(shape)
    D, A = spec.obs_dim, spec.action_dim
    trees = [C.random_bias_params(shape, 20 + k) for k in range(K)]
    tp = trees[0][1]
    cfg = EnvModelTrainerConfig(steps=2 * W_MULTI, model="multistep", sequence_length=T_, termination_weight=1.0,
                                batch_size=B, init_learning_rate=C.LR)
    tr = StatePredictorEnsembleTrainer(spec, [t[0] for t in trees], _Loader(_trajectory_dataset(2, D, A, seed=4)),
                                       None, cfg, seeds=[7, 8], tp_params=tp)
    assert tr.plan == {"sweep": True, "tchunks": 1, "blocks": B // 16}
    tr.steps(W_MULTI)
    for which in (0, 1, 2):
        assert not np.array_equal(tr.flat(0, which), tr.flat(1, which))
    acc = _checked_steps(tr, "multistep", shape, 1.0, C.f64(tp), B, T_, 2 * W_MULTI, (0.25, 0.25),
                         np.random.default_rng(9), others=K)
    _report(f"ensemble-multistep-{shape}-T{T_}-K{K}", acc)
    tr.close()


# ------------------------------------------------------------------------- VAE
class _ObsLoader:
    def __init__(self, obs):
        self.dataset = {"observations": obs}


def _vae_flat(spec, tree):
    return np.concatenate([np.asarray(tree[m][l][k], np.float64).reshape(-1) for m, l, k in io.leaf_names(spec)])


@pytest.mark.parametrize("case,steps,n_checked", [(c, 2 * W_VAE, 2) for c in PARITY_CASES] +
                         [(PARITY_CASES[0], W_VAE + 2, 4)],   # one clamp handle per trainer kind
                         ids=lambda v: f"obs{v[0]}-lat{v[1]}-B{v[3]}" if isinstance(v, tuple) else str(v))
def test_vae_from_trained_state(case, steps, n_checked):
    """em_vae_grad_kernel and the VAE's three em_adam_kernel launches after W_VAE device-sampled
    steps (its biases are random in the existing tests; its moments and count are not)."""
    D, L, hid, B, w = case
    spec = io.InitialObservationSpec(D, L, hid)
    rng = np.random.default_rng(200 + D)
    tree = io.init_initial_observation(spec, 1)
    for mod in tree.values():
        for layer in mod.values():
            layer["bias"] = (0.1 * rng.standard_normal(layer["bias"].shape)).astype(np.float32)
    cfg = EnvModelTrainerConfig(steps=steps, batch_size=B, init_learning_rate=C.LR, reconstruction_weight=w, seed=2)
    tr = io.InitialObservationTrainer(spec, tree, _ObsLoader(_manifold_data(1000, D, seed=1)), None, cfg)
    tr.steps(W_VAE)
    leaves = em_leaf_table(["/".join(n) for n in io.leaf_names(spec)], io.leaf_shapes(spec))
    ck = EmOptimiserChecker(tr, leaves)
    acc = {}
    for step in range(n_checked):
        ref = V.f64(io.unflatten(spec, ck.before()[0]))
        for _ in range(64):
            obs = rng.standard_normal((B, D)).astype(np.float32)
            eps = rng.standard_normal((B, L)).astype(np.float32)
            if V.relu_margin(ref, obs, eps, w) >= C.RELU_MARGIN:
                break
        else:
            raise AssertionError("no batch with a ReLU margin in 64 draws")
        _, logs = tr.train_step(None, {"observations": obs}, eps=eps)
        _, want, g = V.vae_step(ref, obs, eps, w)
        r = em_logs_ratio(logs, want, C.LOG_REL, C.LOG_ABS)
        assert r <= 1.0, (step, logs, want)
        _merge(acc, {"logs": r})
        _merge(acc, ck.after(_vae_flat(spec, g), C.LR, steps, tag=f"step {step}"))
    assert tr.count == W_VAE + n_checked
    _report(f"vae-obs{D}-{'clamp' if n_checked == 4 else 'half'}", acc)
    tr.close()
