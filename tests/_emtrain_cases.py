"""Env-model trainer parity at edge shapes and trained-like states: the case table, the CPU
restatement of fqlpop_emtrain_create's plan (LDS budget, sweep or fallback, T chunks), and the
parameter / batch / oracle plumbing shared by tests/test_gpu_emtrain_trained.py and
tests/test_emtrain_cpu.py (not a test module)."""
from __future__ import annotations

import contextlib
import functools

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
    # the edges of the sweep's admission rule (em_plan; csrc/emlayout.h: sw_fits, em_plan)
    "F": (55, 8, (32,), (16,)),                 # a step's inputs (A + D + 1) 16 = 1024: one per thread, rewards last
    "G": (56, 8, (32,), (16,)),                 # 1040 inputs: the rewards would be the values dropped
    "H": (69, 21, (128, 128), (128,)),          # 1456 inputs: humanoid-sized, non-default widths
    "I": (39, 5, (128, 256, 128), (64,)),       # a step's record 640 rows = SW_RQ SW_NT / 16 exactly
    "J": (40, 4, (128, 256, 128), (64,)),       # record 641
    "K": (17, 8, (128, 256, 128), (128, 256, 96, 128, 256)),   # tw > 0: dynamic sweep LDS 163 216 bytes,
                                                # within the CU's only without the kernel's static LDS
    "L": (39, 5, (128, 256, 128), (128, 256, 128)),            # I under the default frozen predictor: 150 272 bytes
}
SINGLE_CASES = [("A", 16), ("B", 48), ("C", 32)]          # (shape, batch size)
# (shape, T, batch size, em_seq_sweep, plan: sweep, tchunks)
MULTISTEP_CASES = [(s, T_, B, opt, bool(opt), tc if opt else 1)
                   for s, T_, B, tc in (("A", 5, 16, 1), ("B", 17, 32, 1), ("D", 35, 32, 2), ("E", 67, 16, 4))
                   for opt in (1, 0)]
MULTISTEP_FALLBACK = ("C", 4, 16, None, False, 1)         # the default option, no sweep plan
ENSEMBLE_CASE = ("B", 48, 3)                              # shape, batch size, K
# (shape, T, batch size, em_seq_sweep, plan: sweep, tchunks, termination weights); option None is
# the default (sweep where the plan admits it): the rows past an edge must fall back by themselves
MULTISTEP_EDGE_CASES = (
    [(s, T_, 16, opt, bool(opt), 1, tws) for s, T_, tws in (("F", 3, (0.0, 1.0)), ("I", 2, (0.0, 1.0)),
                                                             ("L", 2, (1.0,)), ("A", 1, (0.0, 1.0)))
     for opt in (1, 0)] +
    [(s, T_, 16, None, False, 1, tws) for s, T_, tws in (("G", 3, (0.0, 1.0)), ("H", 2, (0.0, 1.0)),
                                                          ("J", 2, (0.0, 1.0)), ("K", 2, (1.0,)))])
_W3, _DEEP = (128, 256, 128), (128, 256, 96, 128, 256)
# (obs, act, hidden, tp_hidden, tw, sweep): the edge rows, their neighbours one unit either side of
# each limit, and the static-LDS window (dynamic sweep LDS 162 369 .. 163 840 bytes) from just
# below (obs 15) through its middle (16, 17, 18) to just above (19)
PLAN_PROBES = (
    [(D, 8, (32,), (16,), tw, D <= 55) for D in (54, 55, 56) for tw in (0.0, 1.0)] +
    [(55, 9, (32,), (16,), 0.0, False), (69, 21, (128, 128), (128,), 1.0, False),
     (38, 5, _W3, (64,), 0.0, True), (39, 5, _W3, (64,), 0.0, True), (39, 5, _W3, _W3, 1.0, True),
     (40, 4, _W3, (64,), 0.0, False), (39, 6, _W3, (64,), 0.0, False), (17, 8, _W3, _DEEP, 0.0, True)] +
    [(D, 8, _W3, _DEEP, 1.0, D <= 15) for D in (15, 16, 17, 18, 19)])
ENSEMBLE_SWEEP_CASE = ("F", 3, 16, 2)                     # shape, T, batch size, K: a second model's slot

# fqlpop_emtrain_create's constants (csrc/emlayout.h)
_R, _SW_NW, _SW_FM, _SW_NT, _SW_RQ = 16, 16, 32, 1024, 10
_SW_SCR = _SW_NW * 16 * _R
LDS_BUDGET, SWEEP_LDS_BUDGET = 150 * 1024, 160 * 1024
CU_LDS_BYTES = 160 * 1024      # a CU's LDS: a block's dynamic and static parts together
_NLOG = 16
# em_sweep_kernel's __shared__ arrays (SW_STATIC_LDS): lsum [NLOG][R], lab [R], rowbase [R] (8 bytes
# each), mu_s, rs_s [R], cs [2][R]
SW_STATIC_LDS = 4 * _NLOG * _R + 4 * _R + 8 * _R + 2 * 4 * _R + 4 * 2 * _R


def spec_of(shape: str) -> em.EnvModelSpec:
    D, A, hid, tph = SHAPES[shape]
    return em.EnvModelSpec(D, A, hid, tph)


def sw_op_plan(Kc: int, No: int):
    """sw_plan: (output tiles, k-split S, k-steps per chunk, k-steps)."""
    ntile, nks, S = (No + 15) >> 4, (Kc + 3) >> 2, 1
    while S < _SW_NW and ntile * S * 2 <= _SW_NW and S * 2 <= nks:
        S *= 2
    return ntile, S, (nks + S - 1) // S, nks


@functools.lru_cache(maxsize=None)
def _sw_op_fits(Kc, No):
    ntile, S, cks, _ = sw_op_plan(Kc, No)
    return ntile * S <= _SW_NW and cks <= _SW_FM


_FITS_N = 320
_fits_table = []


def _op_fits(Kc, No):
    """_sw_op_fits of both directions of an op; either width may be an array (the enumeration of
    tests/test_emtrain_cpu.py), then through a table of _sw_op_fits filled on first use."""
    if np.ndim(Kc) == 0 and np.ndim(No) == 0:
        return _sw_op_fits(Kc, No) and _sw_op_fits(No, Kc)
    if not _fits_table:
        _fits_table.append(np.array([[k > 0 and n > 0 and _sw_op_fits(k, n) for n in range(_FITS_N)]
                                     for k in range(_FITS_N)]))
    return _fits_table[0][Kc, No] & _fits_table[0][No, Kc]     # (a width >= _FITS_N: an IndexError)


def em_plan_dims(D, A: int, hid, tph, kind: str, tw: float, T_: int = 1, B: int = 16,
                 sweep_option: bool = True) -> dict:
    """What fqlpop_emtrain_create decides for ``kind`` in ("state", "termination", "multistep"):
    the fused step's LDS bytes, whether the multistep step takes the sweep path, its (dynamic) LDS
    bytes, the T chunks of the dW GEMM and the blocks per model; and the sizes the sweep's rule
    bounds: a step's inputs ``nin``, its record ``record`` (floats) and the dynamic LDS bytes the
    sweep would ask for, ``sweep_need``.  ``D`` may be an array of observation widths: then
    every entry that depends on it is an array."""
    sp_dims, tp_dims = [D + A, *hid, D], [D, *tph, 1]
    dims = tp_dims if kind == "termination" else sp_dims
    tdims = tp_dims if (kind != "termination" and tw > 0) else []
    ms = kind == "multistep"
    maxd = functools.reduce(np.maximum, dims + tdims)
    fl = _R * (2 * dims[0] + sum(dims) + 3 * maxd + D + sum(tdims) + (D * (1 if tdims else 2) if ms else 0))
    sl = fl + _SW_SCR + 4 * dims[0]
    nin, record = _R * (A + D + 1), _R * (dims[0] + 1 + sum(dims[:-1]) + D)
    sweep = np.zeros(np.shape(D), bool)
    if ms and sweep_option:
        # sw_fits: every op one unit per wave, a step's inputs one value per thread, its record
        # SW_RQ per thread; em_create: dynamic + em_sweep_kernel's static LDS within the CU's
        ops = list(zip(dims[:-1], dims[1:])) + list(zip(tdims[:-1], tdims[1:]))
        fits = functools.reduce(np.logical_and, [_op_fits(k, n) for k, n in ops])
        sweep = fits & (nin <= _SW_NT) & (record <= _SW_RQ * _SW_NT) & (4 * sl + SW_STATIC_LDS <= CU_LDS_BYTES)
    plan = {"lds": 4 * fl, "sweep": sweep, "sweep_lds": np.where(sweep, 4 * sl, 0),
            "tchunks": np.where(sweep, max(1, min(4, T_ // 16)), 1), "blocks": B // _R,
            # a record: what the backward loads, and on the sweep path every layer's output gradient
            "seq_stride": np.where(sweep, record + _R * sum(dims[1:]), record) if ms else 0,
            "nin": nin, "record": record, "sweep_need": 4 * sl if ms else 0}
    if np.ndim(D) == 0:
        plan = {k: v.item() if isinstance(v, (np.ndarray, np.generic)) else v for k, v in plan.items()}
    return plan


def em_plan(shape: str, kind: str, tw: float, T_: int = 1, B: int = 16, sweep_option: bool = True) -> dict:
    """em_plan_dims of a named shape."""
    return em_plan_dims(*SHAPES[shape], kind, tw, T_, B, sweep_option)


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
