"""Env-model trainer parity at edge shapes and trained-like states: the case table, the CPU
restatement of fqlpop_emtrain_create's plan (LDS budget, sweep or fallback, T chunks), and the
parameter / batch / oracle plumbing shared by tests/test_gpu_emtrain_trained.py and
tests/test_emtrain_cpu.py (not a test module)."""
from __future__ import annotations

import contextlib

import numpy as np

import envmodel as em
from envmodel.trainer import _leaf_shapes, unflatten
from oracle import envmodel_train_oracle as T

RELU_MARGIN = 2e-6      # tests/test_gpu_emtrain.py: no hidden pre-activation closer to zero
LR = 1e-3
LOG_REL, LOG_REL_MS, LOG_ABS = 1e-4, 2e-4, 1e-7

# (obs, act, hidden, tp_hidden): the smallest shapes that reach the named edge
SHAPES = {
    "A": (3, 1, (20,), (12,)),                  # K0 = 4: one k-step; every width below a tile or ragged
    "B": (17, 2, (50, 36), (50,)),              # widths no multiple of 4; K0 = 19; P no multiple of 64
    "C": (69, 20, (144, 272), (272, 144)),      # KS = 32 path; 9 tiles for 8 waves; no sweep plan
    "D": (42, 8, (96, 48), (48,)),              # 96: a ragged 64-tile of the dW GEMM; K0 = 50
    "E": (28, 5, (64,), (64,)),
}
SINGLE_CASES = [("A", 16), ("B", 48), ("C", 32)]          # (shape, batch size)
# (shape, T, batch size, em_seq_sweep, plan: sweep, tchunks)
MULTISTEP_CASES = [(s, T_, B, opt, bool(opt), tc if opt else 1)
                   for s, T_, B, tc in (("A", 5, 16, 1), ("B", 17, 32, 1), ("D", 35, 32, 2), ("E", 67, 16, 4))
                   for opt in (1, 0)]
MULTISTEP_FALLBACK = ("C", 4, 16, None, False, 1)         # the default option, no sweep plan
ENSEMBLE_CASE = ("B", 48, 3)                              # shape, batch size, K

# fqlpop_emtrain_create's constants (csrc/emtrain.hip)
_R, _SW_NW, _SW_FM, _SW_NT, _SW_RQ = 16, 16, 32, 1024, 10
_SW_SCR = _SW_NW * 16 * _R
LDS_BUDGET, SWEEP_LDS_BUDGET = 150 * 1024, 160 * 1024


def spec_of(shape: str) -> em.EnvModelSpec:
    D, A, hid, tph = SHAPES[shape]
    return em.EnvModelSpec(D, A, hid, tph)


def sw_op_plan(Kc: int, No: int):
    """sw_plan: (output tiles, k-split S, k-steps per chunk, k-steps)."""
    ntile, nks, S = (No + 15) >> 4, (Kc + 3) >> 2, 1
    while S < _SW_NW and ntile * S * 2 <= _SW_NW and S * 2 <= nks:
        S *= 2
    return ntile, S, (nks + S - 1) // S, nks


def _sw_op_fits(Kc, No):
    ntile, S, cks, _ = sw_op_plan(Kc, No)
    return ntile * S <= _SW_NW and cks <= _SW_FM


def em_plan(shape: str, kind: str, tw: float, T_: int = 1, B: int = 16, sweep_option: bool = True) -> dict:
    """What fqlpop_emtrain_create decides for ``kind`` in ("state", "termination", "multistep"):
    the fused step's LDS bytes, whether the multistep step takes the sweep path, its LDS bytes,
    the T chunks of the dW GEMM and the blocks per model."""
    spec = spec_of(shape)
    D = spec.obs_dim
    dims = spec.tp_dims() if kind == "termination" else spec.sp_dims()
    tdims = spec.tp_dims() if (kind != "termination" and tw > 0) else []
    ms = kind == "multistep"
    maxd = max(dims + tdims)
    fl = _R * (2 * dims[0] + sum(dims) + 3 * maxd + D + sum(tdims) + (D * (1 if tdims else 2) if ms else 0))
    plan = {"lds": 4 * fl, "sweep": False, "sweep_lds": 0, "tchunks": 1, "blocks": B // _R}
    if ms and sweep_option:
        ops = list(zip(dims[:-1], dims[1:])) + list(zip(tdims[:-1], tdims[1:]))
        fits = all(_sw_op_fits(k, n) and _sw_op_fits(n, k) for k, n in ops)
        fits = fits and _R * (dims[0] + 1 + sum(dims[:-1]) + D) <= _SW_RQ * _SW_NT
        sl = fl + _SW_SCR + 4 * dims[0]
        if fits and 4 * sl <= SWEEP_LDS_BUDGET:
            plan.update(sweep=True, sweep_lds=4 * sl, tchunks=max(1, min(4, T_ // 16)))
    return plan


def tchunk_lengths(T_: int, tchunks: int):
    return [T_ * (c + 1) // tchunks - T_ * c // tchunks for c in range(tchunks)]


# ------------------------------------------------------------------ parameters
def random_bias_params(shape: str, seed: int, scale: float = 1.0):
    """(state predictor, termination predictor) trees in float32: Dense biases 0.1 N(0, 1) in
    every layer of both (the frozen predictor's head included), LayerNorm perturbed as
    tests/test_gpu_emtrain.py does."""
    spec = spec_of(shape)
    rng = np.random.default_rng([seed, 77])
    sp = em.init_state_predictor(spec, seed, scale=scale)
    tp = em.init_termination_predictor(spec, seed + 1)
    for tree in (sp, tp):
        for mod, d in tree.items():
            if mod.startswith("Dense_"):
                d["bias"] = (0.1 * rng.standard_normal(d["bias"].shape)).astype(np.float32)
    k0 = spec.obs_dim + spec.action_dim
    sp["LayerNorm_0"]["scale"] = (1 + 0.1 * rng.standard_normal(k0)).astype(np.float32)
    sp["LayerNorm_0"]["bias"] = (0.1 * rng.standard_normal(k0)).astype(np.float32)
    return sp, tp


def f64(tree):
    return {m: {k: np.asarray(v, np.float64) for k, v in d.items()} for m, d in tree.items()}


def layout(shape: str, kind: str):
    """(leaf names, leaf shapes) of the flat vector of ``kind``'s trained net."""
    spec = spec_of(shape)
    if kind == "termination":
        names = em.tp_leaf_names(spec)
        return names, _leaf_shapes(names, spec.tp_dims())
    names = em.sp_leaf_names(spec)
    return names, _leaf_shapes(names, spec.sp_dims(), spec.obs_dim + spec.action_dim)


def tree_of(names, shapes, flat):
    """The float64 tree of a (float32) flat vector."""
    return f64(unflatten(names, shapes, np.asarray(flat)))


def flat_of(names, tree):
    return np.concatenate([np.asarray(tree[m][k], np.float64).reshape(-1) for m, k in names])


# --------------------------------------------------------------------- batches
def row_batch(rng, B, D, A, p_term=0.25):
    """p_term 0: no terminal row; 1: only terminal rows."""
    obs = rng.standard_normal((B, D)).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1, 1, (B, A)).astype(np.float32),
            "next_observations": (obs + 0.1 * rng.standard_normal((B, D))).astype(np.float32),
            "rewards": np.where(rng.uniform(size=B) < p_term, 0.0, -1.0).astype(np.float32)}


def seq_batch(rng, B, T_, D, A, p_term=0.25):
    obs = rng.standard_normal((B, T_, D)).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1, 1, (B, T_, A)).astype(np.float32),
            "next_observations": (obs + 0.1 * rng.standard_normal((B, T_, D))).astype(np.float32),
            "rewards": np.where(rng.uniform(size=(B, T_)) < p_term, 0.0, -1.0).astype(np.float32)}


@contextlib.contextmanager
def _watch_relu(lo):
    orig = T._relu_mlp_fwd

    def fwd(tree, x):
        ins, n = [], T._n_dense(tree)
        for i in range(n):
            ins.append(x)
            x = x @ T._W(tree, i) + T._b(tree, i)
            if i < n - 1:
                lo[0] = min(lo[0], float(np.abs(x).min()))
                x = np.maximum(x, 0.0)
        return x, ins

    T._relu_mlp_fwd = fwd
    try:
        yield
    finally:
        T._relu_mlp_fwd = orig


def oracle_step(kind, tree, batch, tw=0.0, tp=None, keep=None):
    """(logs, flat-ordered grads tree, smallest |pre-activation| of any hidden ReLU) of the
    float64 oracle's step of ``kind`` at ``tree``."""
    lo = [np.inf]
    with _watch_relu(lo):
        if kind == "state":
            _, logs, grads, _ = T.state_predictor_step(tree, batch, tw, 30.0, tp)
        elif kind == "multistep":
            _, logs, grads, _ = T.multistep_step(tree, batch, tw, 30.0, tp)
        else:
            _, logs, grads = T.termination_predictor_step(tree, batch, np.asarray(keep, np.float64))
    return logs, grads, lo[0]


def batch_with_margin(draw, step_fn):
    """The first of at most 64 ``draw()`` batches whose oracle step (``step_fn(batch)`` ->
    oracle_step's triple) keeps every hidden pre-activation RELU_MARGIN from zero, with that
    step's result."""
    for _ in range(64):
        b = draw()
        logs, grads, lo = step_fn(b)
        if lo >= RELU_MARGIN:
            return b, logs, grads
    raise AssertionError("no batch with a ReLU margin in 64 draws")
