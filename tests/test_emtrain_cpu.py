"""CPU checks of the env-model trainer oracle (oracle/envmodel_train_oracle.py):
hand-written gradients vs torch autograd in float64, known answers of the focal
loss, the cosine schedule and the Adam step."""
import functools
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flow-q-learning_amd"))

from oracle import envmodel_train_oracle as T  # noqa: E402
T_ = T
import envmodel as em  # noqa: E402


def _batch(rng, B, D, A, p_term=0.2):
    obs = rng.standard_normal((B, D))
    return {"observations": obs, "actions": rng.uniform(-1, 1, (B, A)),
            "next_observations": obs + 0.1 * rng.standard_normal((B, D)),
            "rewards": np.where(rng.uniform(size=B) < p_term, 0.0, -1.0)}


def _torch_tree(tree):
    return {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in d.items()}
            for m, d in tree.items()}


def _torch_mlp(tt, x):
    n = sum(1 for k in tt if k.startswith("Dense_"))
    for i in range(n):
        x = x @ tt[f"Dense_{i}"]["kernel"] + tt[f"Dense_{i}"]["bias"]
        if i < n - 1:
            x = torch.relu(x)
    return x


def _ln_torch(x, scale, bias):
    mu = x.mean(-1, keepdim=True)
    var = torch.clamp((x * x).mean(-1, keepdim=True) - mu * mu, min=0.0)
    return (x - mu) / torch.sqrt(var + T.LN_EPS) * scale + bias


def _bce_torch(logits, z):
    return torch.nn.functional.softplus(logits) - logits * z


@pytest.mark.parametrize("tw", [0.0, 1.0])
def test_state_predictor_grads_vs_autograd(tw):
    rng = np.random.default_rng(0)
    spec = em.EnvModelSpec(7, 3, (16, 24, 16), (12, 12))
    sp = em.init_state_predictor(spec, 1)
    sp["LayerNorm_0"]["scale"] = (1 + 0.1 * rng.standard_normal(10)).astype(np.float32)
    sp["LayerNorm_0"]["bias"] = (0.1 * rng.standard_normal(10)).astype(np.float32)
    tp = em.init_termination_predictor(spec, 2)
    b = _batch(rng, 32, 7, 3)
    loss, logs, grads, _ = T.state_predictor_step(sp, b, tw, 30.0, tp)
    tt = _torch_tree(sp)
    obs = torch.tensor(b["observations"])
    x0 = torch.cat([obs, torch.tensor(b["actions"])], -1)
    h0 = _ln_torch(x0, tt["LayerNorm_0"]["scale"], tt["LayerNorm_0"]["bias"])
    pred = _torch_mlp({k: v for k, v in tt.items() if k.startswith("Dense_")}, h0) + obs
    mse = ((pred - torch.tensor(b["next_observations"])) ** 2).mean()
    total = mse
    if tw > 0:
        ttp = {m: {k: torch.tensor(np.asarray(v, np.float64)) for k, v in d.items()} for m, d in tp.items()}
        logit = _torch_mlp(ttp, pred)[:, 0]
        z = torch.tensor((b["rewards"] == 0).astype(np.float64))
        ce = _bce_torch(logit, z)
        w = 30.0
        tl = torch.where(z == 1, ce, torch.zeros_like(ce))
        fl = torch.where(z == 0, ce, torch.zeros_like(ce))
        total = mse + tw * ((w * tl + fl) / (w + 1)).mean()
    total = total / (1 + tw)
    total.backward()
    assert abs(loss - total.item()) < 1e-12
    assert abs(logs["next_observation_loss"] - mse.item()) < 1e-12
    for m, d in tt.items():
        for k, v in d.items():
            np.testing.assert_allclose(grads[m][k], v.grad.numpy(), rtol=1e-9, atol=1e-12)


def test_termination_predictor_grads_vs_autograd():
    rng = np.random.default_rng(1)
    spec = em.EnvModelSpec(9, 2, (8, 8), (16, 32, 16))
    tp = em.init_termination_predictor(spec, 3)
    b = _batch(rng, 64, 9, 2, p_term=0.3)
    keep = rng.uniform(size=(64, 9)) >= 0.1
    loss, logs, grads = T.termination_predictor_step(tp, b, keep.astype(np.float64))
    tt = _torch_tree(tp)
    x = torch.tensor(b["next_observations"]) * torch.tensor(keep.astype(np.float64)) / 0.9
    logit = _torch_mlp(tt, x)[:, 0]
    z = torch.tensor((b["rewards"] == 0).astype(np.float64))
    p = torch.sigmoid(logit)
    ce = _bce_torch(logit, z)
    pt = torch.where(z == 1, p, 1 - p)
    af = torch.where(z == 1, torch.full_like(p, 0.25), torch.full_like(p, 0.75))
    li = af * (1 - pt) ** 2 * ce
    li.mean().backward()
    assert abs(loss - li.mean().item()) < 1e-12
    for m, d in tt.items():
        for k, v in d.items():
            np.testing.assert_allclose(grads[m][k], v.grad.numpy(), rtol=1e-8, atol=1e-12)


def test_focal_known_answers():
    # logit 0: p = 0.5, ce = log 2, (1 - pt)^2 = 0.25
    li, _ = T.focal_terms(np.array([0.0, 0.0]), np.array([1.0, 0.0]))
    np.testing.assert_allclose(li, [0.25 * 0.25 * math.log(2), 0.75 * 0.25 * math.log(2)], rtol=1e-12)
    # finite differences of the per-row derivative
    x = np.linspace(-6, 6, 25)
    for z in (0.0, 1.0):
        _, d = T.focal_terms(x, np.full_like(x, z))
        h = 1e-6
        fd = (T.focal_terms(x + h, np.full_like(x, z))[0] - T.focal_terms(x - h, np.full_like(x, z))[0]) / (2 * h)
        np.testing.assert_allclose(d, fd, rtol=1e-6, atol=1e-10)


def test_cosine_schedule_and_adam_first_step():
    assert T.cosine_lr(1e-3, 100, 0) == pytest.approx(1e-3)
    assert T.cosine_lr(1e-3, 100, 50) == pytest.approx(5e-4)
    assert T.cosine_lr(1e-3, 100, 100) == pytest.approx(0.0, abs=1e-18)
    assert T.cosine_lr(1e-3, 100, 250) == pytest.approx(0.0, abs=1e-18)
    tree = {"Dense_0": {"kernel": np.ones((2, 2)), "bias": np.zeros(2)}}
    g = {"Dense_0": {"kernel": np.array([[1.0, -2.0], [0.5, 0.0]]), "bias": np.array([3.0, -1e-3])}}
    nt, _, _ = T.adam_update(tree, g, T.zeros_like_tree(tree), T.zeros_like_tree(tree), 0, 1e-3)
    # first Adam step: -lr * g / (|g| + eps)
    want = 1.0 - 1e-3 * g["Dense_0"]["kernel"] / (np.abs(g["Dense_0"]["kernel"]) + 1e-8)
    np.testing.assert_allclose(nt["Dense_0"]["kernel"], want, rtol=1e-12)


def test_env_model_argparser_matches_reference_fixture():
    """Our get_env_model_argparser / build_env_model_config_from_args against the
    REFERENCE argparser's output (tests/golden/reference_env_model_argparser.json)."""
    import json

    import argparser
    with open(os.path.join(ROOT, "tests", "golden", "reference_env_model_argparser.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 4
    for case in cases:
        cfg = argparser.build_env_model_config_from_args(argparser.get_env_model_argparser().parse_args(case["argv"]))
        d = dict(vars(cfg))
        d["save_directory"] = str(d["save_directory"])
        d["data_directory"] = str(d["data_directory"])
        d["model_config"] = {k: list(v) if isinstance(v, tuple) else v for k, v in d["model_config"].items()}
        assert d == case["config"], case["argv"]


def test_trainer_flat_layout_roundtrip():
    from envmodel.trainer import _leaf_shapes, unflatten
    spec = em.EnvModelSpec(28, 5)
    sp = em.init_state_predictor(spec, 0)
    flat = em.flatten_state_predictor(spec, sp)
    names = em.sp_leaf_names(spec)
    tree = unflatten(names, _leaf_shapes(names, spec.sp_dims(), 33), flat)
    for m in sp:
        for k in sp[m]:
            np.testing.assert_array_equal(tree[m][k], sp[m][k])
    tp = em.init_termination_predictor(spec, 1)
    names = em.tp_leaf_names(spec)
    tree = unflatten(names, _leaf_shapes(names, spec.tp_dims()), em.flatten_termination_predictor(spec, tp))
    for m in tp:
        for k in tp[m]:
            np.testing.assert_array_equal(tree[m][k], tp[m][k])


def _seq_batch(rng, B, T, D, A, p_term=0.2):
    obs = rng.standard_normal((B, T, D))
    return {"observations": obs, "actions": rng.uniform(-1, 1, (B, T, A)),
            "next_observations": obs + 0.1 * rng.standard_normal((B, T, D)),
            "rewards": np.where(rng.uniform(size=(B, T)) < p_term, 0.0, -1.0)}


@pytest.mark.parametrize("tw", [0.0, 1.0])
def test_multistep_bptt_grads_vs_autograd(tw):
    """oracle.multistep_step (hand-written BPTT) against torch autograd through the
    scanned cell (envmodel/multistep.py:31-54) in float64."""
    rng = np.random.default_rng(4)
    B, T, D, A = 3, 6, 7, 3
    spec = em.EnvModelSpec(D, A, (16, 24, 16), (12, 12))
    sp = em.init_state_predictor(spec, 1)
    sp["LayerNorm_0"]["scale"] = (1 + 0.1 * rng.standard_normal(D + A)).astype(np.float32)
    sp["LayerNorm_0"]["bias"] = (0.1 * rng.standard_normal(D + A)).astype(np.float32)
    tp = em.init_termination_predictor(spec, 2)
    b = _seq_batch(rng, B, T, D, A, p_term=0.3)
    loss, logs, grads, preds = T_.multistep_step(sp, b, tw, 30.0, tp)
    tt = _torch_tree(sp)
    ttp = {m: {k: torch.tensor(np.asarray(v, np.float64)) for k, v in d.items()} for m, d in tp.items()}
    dense = {k: v for k, v in tt.items() if k.startswith("Dense_")}
    o = torch.tensor(b["observations"][:, 0])
    act = torch.tensor(b["actions"])
    out = []
    for t in range(T):
        h0 = _ln_torch(torch.cat([o, act[:, t]], -1), tt["LayerNorm_0"]["scale"], tt["LayerNorm_0"]["bias"])
        o = _torch_mlp(dense, h0) + o
        out.append(o)
    pred = torch.stack(out, 1)
    mse = ((pred - torch.tensor(b["next_observations"])) ** 2).mean()
    total = mse
    if tw > 0:
        logit = _torch_mlp(ttp, pred)[..., 0]
        z = torch.tensor((b["rewards"] == 0).astype(np.float64))
        ce = _bce_torch(logit, z)
        tl = torch.where(z == 1, ce, torch.zeros_like(ce))
        fl = torch.where(z == 0, ce, torch.zeros_like(ce))
        total = mse + tw * ((30.0 * tl + fl) / 31.0).mean()
        assert logs["true_termination_loss"] == pytest.approx(float(tl.detach().sum() / (z == 1).sum()), rel=1e-12)
    total = total / (1 + tw)
    total.backward()
    np.testing.assert_allclose(preds, pred.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert abs(loss - total.item()) < 1e-12
    assert abs(logs["next_observation_loss"] - mse.item()) < 1e-12
    for m, d in tt.items():
        for k, v in d.items():
            np.testing.assert_allclose(grads[m][k], v.grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=f"{m}/{k}")


def test_multistep_one_step_is_the_baseline_step():
    rng = np.random.default_rng(5)
    spec = em.EnvModelSpec(9, 2, (8, 8))
    sp = em.init_state_predictor(spec, 3)
    b = _seq_batch(rng, 4, 1, 9, 2)
    l1, _, g1, _ = T_.multistep_step(sp, b)
    l0, _, g0, _ = T_.state_predictor_step(sp, {k: v[:, 0] for k, v in b.items()})
    assert l1 == pytest.approx(l0, rel=1e-13)
    for m in g0:
        for k in g0[m]:
            np.testing.assert_allclose(g1[m][k], g0[m][k], rtol=1e-12, atol=1e-15)


def test_multistep_loader_windows_like_reference():
    """train_env_model.MultistepLoader = utils/data_loader.py:25-39: [n/1000][1000] episodes,
    windows of T consecutive steps inside one episode, start in [0, 1000 - T)."""
    import train_env_model as tem
    n, D, A, T = 3000, 3, 2, 16
    rows = np.arange(n, dtype=np.float32)
    ds = {"observations": np.repeat(rows[:, None], D, 1), "actions": np.zeros((n, A), np.float32),
          "rewards": rows.copy(), "next_observations": np.repeat(rows[:, None] + 1, D, 1)}
    ld = tem.MultistepLoader(ds, T)
    assert ld.dataset["observations"].shape == (3, 1000, D) and ld.dataset["rewards"].shape == (3, 1000)
    np.random.seed(1)
    b = ld.sample(64)
    assert b["observations"].shape == (64, T, D) and b["rewards"].shape == (64, T)
    first = b["rewards"][:, 0]
    np.testing.assert_array_equal(b["rewards"], first[:, None] + np.arange(T))  # consecutive steps
    start = first % 1000
    assert (start >= 0).all() and (start < 1000 - T).all()  # never crosses an episode boundary
    np.testing.assert_array_equal(b["next_observations"][..., 0], b["rewards"] + 1)
    with pytest.raises(ValueError):
        tem.MultistepLoader({k: v[:2500] for k, v in ds.items()}, T)


# ---------------------------------------------------------------------------
# tests/test_gpu_emtrain_trained.py's checks, proven on the CPU: the case table fits the
# kernels' plans, the cases are well-conditioned at the checked bounds, and the checks catch
# the mistakes that steps from the constructor's state cannot see (tests/test_oracle.py's
# pattern: a mutated oracle plays the device).
# ---------------------------------------------------------------------------
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _emtrain_cases as C  # noqa: E402
from _helpers import EM_GRAD_REL, EmOptimiserChecker, em_leaf_table, em_logs_ratio  # noqa: E402

_MS = C.MULTISTEP_CASES + [C.MULTISTEP_FALLBACK]
_EDGE = C.MULTISTEP_EDGE_CASES


def test_case_table_fits_the_lds_budget_and_reaches_its_edges():
    for shape, B in C.SINGLE_CASES:
        for kind, tw in (("state", 0.0), ("state", 1.0), ("termination", 0.0)):
            assert C.em_plan(shape, kind, tw, 1, B)["lds"] <= C.LDS_BUDGET, (shape, kind, tw)
    assert C.em_plan("C", "state", 1.0, 1, 32)["lds"] > 0.85 * C.LDS_BUDGET      # C is near the budget
    for shape, T_, B, option, sweep, tchunks in _MS:
        for tw in (0.0, 1.0):
            plan = C.em_plan(shape, "multistep", tw, T_, B, option != 0)
            assert plan["lds"] <= C.LDS_BUDGET and plan["sweep_lds"] <= C.SWEEP_LDS_BUDGET, (shape, tw)
            assert (plan["sweep"], plan["tchunks"], plan["blocks"]) == (sweep, tchunks, B // 16), (shape, T_, tw, plan)
    # A: ops 20 -> 3 and 20 -> 4 split S = 4 over 5 k-steps in chunks of 2: 2, 2, 1 and an empty one
    for No in (3, 4):
        ntile, S, cks, nks = C.sw_op_plan(20, No)
        assert (ntile, S, cks, nks) == (1, 4, 2, 5) and (S - 1) * cks >= nks
    # B: op 50 -> 19 has S = 8 over 13 k-steps (uneven chunks); widths no multiple of 4; P % 64 != 0
    assert C.sw_op_plan(50, 19)[1:] == (8, 2, 13)
    offs = [o for _, o, _ in em_leaf_table(*C.layout("B", "state"))]
    assert 50 % 4 and 17 % 4 and any(o % 4 for o in offs)      # leaves off the 16-byte grid
    assert sum(int(np.prod(s)) for s in C.layout("B", "state")[1]) % 64 != 0
    # D: two T chunks of odd and even length; 96 is a ragged 64-tile.  E: four chunks, 16 17 17 17
    assert C.tchunk_lengths(35, 2) == [17, 18] and 96 % 64 != 0
    assert C.tchunk_lengths(67, 4) == [16, 17, 17, 17]
    # A: one block, one k-step of the first layer
    assert C.SINGLE_CASES[0] == ("A", 16) and sum(C.SHAPES["A"][:2]) == 4
    # the edge rows: every case creatable, on the path its row names, within the CU's LDS
    for shape, T_, B, option, sweep, tchunks, tws in _EDGE:
        for tw in tws:
            plan = C.em_plan(shape, "multistep", tw, T_, B, option != 0)
            assert plan["lds"] <= C.LDS_BUDGET and plan["sweep_lds"] + C.SW_STATIC_LDS <= C.CU_LDS_BYTES, (shape, tw)
            assert (plan["sweep"], plan["tchunks"], plan["blocks"]) == (sweep, tchunks, B // 16), (shape, T_, tw, plan)
    edge = {s: C.em_plan(s, "multistep", 1.0, 2, 16) for s in "FGHIJKL"}
    # F, G, H: a step's inputs at SW_NT = 1024 values exactly (rewards in threads 1008..1023), 16 and 432 past it
    assert [edge[s]["nin"] for s in "FGH"] == [1024, 1040, 1456]
    assert (55 + 8) * 16 == 1008 and [edge[s]["sweep"] for s in "FGH"] == [True, False, False]
    # I, L, J: a step's record at SW_RQ SW_NT = 10240 floats (640 rows of 16) exactly, and one row past it
    assert [edge[s]["record"] for s in "ILJ"] == [640 * 16, 640 * 16, 641 * 16]
    assert [edge[s]["sweep"] for s in "ILJ"] == [True, True, False] and edge["L"]["sweep_lds"] == 150272
    assert all(edge[s]["nin"] <= 1024 for s in "IJKL")
    # K: the dynamic part alone fits the CU's LDS, with em_sweep_kernel's static arrays it does not;
    # nothing else refuses it (without the frozen predictor it sweeps)
    assert edge["K"]["sweep_need"] == 163216 <= C.CU_LDS_BYTES < 163216 + C.SW_STATIC_LDS == 164688
    assert not edge["K"]["sweep"] and edge["K"]["lds"] == 146432 <= C.LDS_BUDGET
    assert C.em_plan("K", "multistep", 0.0, 2, 16)["sweep"] and edge["K"]["record"] <= 10240
    for D, A, hid, tph, tw, sweep in C.PLAN_PROBES:
        plan = C.em_plan_dims(D, A, hid, tph, "multistep", tw, 2, 16)
        assert plan["sweep"] == sweep and plan["lds"] <= C.LDS_BUDGET, (D, A, hid, tph, tw, plan)


def _case_step(kind, shape, tw, B, T_, seed):
    """(names, flat float32 parameters, step_fn(flat) -> (logs, flat grads)) of one case at the
    random-bias parameters, on one batch with a ReLU margin."""
    spec = C.spec_of(shape)
    D, A = spec.obs_dim, spec.action_dim
    sp, tp = C.random_bias_params(shape, 11)
    names, shapes = C.layout(shape, kind)
    tree = tp if kind == "termination" else sp
    flat = C.flat_of(names, tree).astype(np.float32)
    rng = np.random.default_rng(seed)
    keep = (rng.uniform(size=(B, D)) >= 0.1) if kind == "termination" else None

    def step(fl, b):
        return C.oracle_step(kind, C.tree_of(names, shapes, fl), b, tw, C.f64(tp), keep)

    draw = (lambda: C.seq_batch(rng, B, T_, D, A)) if kind == "multistep" else (lambda: C.row_batch(rng, B, D, A))
    b, _, _ = C.batch_with_margin(draw, lambda bb: step(flat, bb))
    return names, flat, lambda fl: step(fl, b)[:2]


_COND = [("state", s, tw, B, 1) for s, B in C.SINGLE_CASES for tw in (0.0, 1.0)] + \
        [("termination", s, 0.0, B, 1) for s, B in C.SINGLE_CASES] + \
        [("multistep", c[0], tw, c[2], c[1]) for c in _MS if c[3] != 0 for tw in (0.0, 1.0)] + \
        [("multistep", c[0], tw, c[2], c[1]) for c in _EDGE if c[3] != 0 for tw in c[6]]


@pytest.mark.parametrize("kind,shape,tw,B,T_", _COND)
def test_cases_are_well_conditioned(kind, shape, tw, B, T_):
    """A one-ulp (2^-24 relative) perturbation of every float32 parameter moves the float64
    loss and every gradient leaf by at most 1 / 100 of the bound the GPU test holds them to."""
    names, flat, step = _case_step(kind, shape, tw, B, T_, 1)
    logs0, g0 = step(flat.astype(np.float64))
    sign = np.where(np.random.default_rng(2).uniform(size=flat.size) < 0.5, -1.0, 1.0)
    logs1, g1 = step(flat.astype(np.float64) * (1.0 + sign * 2.0 ** -24))
    rel = C.LOG_REL_MS if kind == "multistep" else C.LOG_REL
    assert em_logs_ratio(logs1, logs0, rel, C.LOG_ABS) <= 0.01, (logs0, logs1)
    for m, k in names:
        d, scale = float(np.abs(g1[m][k] - g0[m][k]).max()), float(np.abs(g0[m][k]).max())
        assert d <= 0.01 * EM_GRAD_REL * scale, (m, k, d / scale)


@pytest.mark.parametrize("seed", [6, 9])
def test_edge_cases_find_their_batches_within_the_cap(seed):
    """batch_with_margin's 64 draws suffice at every edge case, for both checked steps of the GPU
    test's streams (6: test_multistep_at_the_edges_of_the_sweep_plan, 9: the ensemble case), at the
    random-bias parameters the GPU warm-up starts from."""
    cases = [c for c in _EDGE if c[3] != 0] if seed == 6 else [(*C.ENSEMBLE_SWEEP_CASE[:3], None, True, 1, (1.0,))]
    for shape, T_, B, _, _, _, tws in cases:
        spec = C.spec_of(shape)
        sp, tp = C.random_bias_params(shape, 11)
        for tw in tws:
            rng, n = np.random.default_rng(seed), [0]

            def draw():
                n[0] += 1
                return C.seq_batch(rng, B, T_, spec.obs_dim, spec.action_dim)

            for _ in range(2):
                C.batch_with_margin(draw, lambda b: C.oracle_step("multistep", C.f64(sp), b, tw, C.f64(tp)))
            print(shape, tw, "draws", n[0])
            assert n[0] <= 8, (shape, tw, n[0])      # far from the cap: no case leans on it


class _OracleDevice:
    """The float64 oracle played as the device, with named mistakes: float32 parameters and
    moments, an update count, ``flat(which)`` / ``count`` / ``train_step`` as a trainer's."""

    def __init__(self, kind, shape, tw, steps, flat, m, v, count, tp, mutations=()):
        self.kind, self.tw, self.steps, self.count, self.tp, self.mut = kind, tw, steps, count, tp, set(mutations)
        self.names, self.shapes = C.layout(shape, kind)
        self.state = [np.asarray(a, np.float32).copy() for a in (flat, m, v)]

    def flat(self, which=0):
        return self.state[which].copy()

    def train_step(self, batch, keep=None):
        tree, tp = C.tree_of(self.names, self.shapes, self.state[0]), C.f64(self.tp)
        if "tp_hidden_bias" in self.mut:
            tp["Dense_0"]["bias"] = np.zeros_like(tp["Dense_0"]["bias"])
        if "tp_head_bias" in self.mut:
            last = f"Dense_{T._n_dense(tp) - 1}"
            tp[last]["bias"] = np.zeros_like(tp[last]["bias"])
        if "dense_bias" in self.mut:
            tree["Dense_1"]["bias"] = np.zeros_like(tree["Dense_1"]["bias"])
        if "ln_bias" in self.mut:
            tree["LayerNorm_0"]["bias"] = np.zeros_like(tree["LayerNorm_0"]["bias"])
        if "stage_64" in self.mut:
            # em_sweep_kernel's input stage without the rule (A + D + 1) 16 <= SW_NT: one value per
            # thread is 64 rows; the next-observation rows past them stay the zeros of the LDS clear
            # and the reward row never reaches lab (uninitialised in the kernel: a constant here)
            A = batch["actions"].shape[-1]
            batch = dict(batch, next_observations=batch["next_observations"].copy(),
                         rewards=np.full_like(batch["rewards"], -1.0))
            batch["next_observations"][..., max(0, 64 - A):] = 0.0
        logs, grads, _ = C.oracle_step(self.kind, tree, batch, self.tw, tp, keep)
        g = C.flat_of(self.names, grads)
        p, m, v = (a.astype(np.float64) for a in self.state)
        c = self.count if "no_clamp" in self.mut else min(self.count, self.steps)
        lr = C.LR if "const_lr" in self.mut else C.LR * 0.5 * (1.0 + math.cos(math.pi * c / self.steps))
        t = self.count if "bc_count" in self.mut else self.count + 1
        b2 = 0.99 if "b2" in self.mut else 0.999
        m = 0.9 * m + 0.1 * g
        if "v_frozen" not in self.mut:
            v = b2 * v + (1 - b2) * g * g
        mh, vh = m / (1 - 0.9 ** t), v / (1 - b2 ** t)
        den = np.sqrt(vh + 1e-8) if "eps_in_sqrt" in self.mut else np.sqrt(vh) + 1e-8
        self.state = [a.astype(np.float32) for a in (p - lr * mh / den, m, v)]
        self.count += 1
        return logs


_MUT_SHAPE, _MUT_B = "B", 48


def _trained_like(kind, shape, B, count, zero_bias=False, T_=1):
    """(flat, m, v, frozen predictor) on the CPU: random biases (or the constructor's zeros),
    moments as three oracle steps leave them, rescaled to ``count`` updates."""
    spec = C.spec_of(shape)
    sp, tp = C.random_bias_params(shape, 11)
    if zero_bias:
        sp, tp = em.init_state_predictor(spec, 11), em.init_termination_predictor(spec, 12)
    names, shapes = C.layout(shape, kind)
    tree = C.f64(tp if kind == "termination" else sp)
    m, v = T.zeros_like_tree(tree), T.zeros_like_tree(tree)
    rng = np.random.default_rng(3)
    p = tree
    for i in range(3):
        b = C.seq_batch(rng, B, T_, spec.obs_dim, spec.action_dim) if kind == "multistep" else \
            C.row_batch(rng, B, spec.obs_dim, spec.action_dim)
        _, grads, _ = C.oracle_step(kind, p, b, 1.0, C.f64(tp), np.ones((B, spec.obs_dim)))
        p, m, v = T.adam_update(p, grads, m, v, i, C.LR)
    flat = C.flat_of(names, tree)     # the parameters stay the random-bias ones
    return (flat, C.flat_of(names, m) / (1 - 0.9 ** 3) * (1 - 0.9 ** count),
            C.flat_of(names, v) / (1 - 0.999 ** 3) * (1 - 0.999 ** count), tp)


def _play(mutations, count=1000, steps=2000, zero_bias=False, n_steps=2, kind="state", shape=_MUT_SHAPE, B=_MUT_B,
          T_=1):
    """Two checked steps of the (mutated) oracle device from a trained-like state through the
    GPU test's checks: the largest error / bound of each."""
    spec = C.spec_of(shape)
    rel = C.LOG_REL_MS if kind == "multistep" else C.LOG_REL
    flat, m, v, tp = _trained_like(kind, shape, B, max(count, 1), zero_bias, T_)
    if count == 0:
        m, v = np.zeros_like(m), np.zeros_like(v)
    dev = _OracleDevice(kind, shape, 1.0, steps, flat, m, v, count, tp, mutations)
    ck = EmOptimiserChecker(dev, em_leaf_table(dev.names, dev.shapes))
    rng = np.random.default_rng(4)
    acc = {}
    for _ in range(n_steps):
        tree = C.tree_of(dev.names, dev.shapes, ck.before()[0])
        b, want_logs, grads = C.batch_with_margin(
            (lambda: C.seq_batch(rng, B, T_, spec.obs_dim, spec.action_dim)) if kind == "multistep" else
            (lambda: C.row_batch(rng, B, spec.obs_dim, spec.action_dim)),
            lambda bb: C.oracle_step(kind, tree, bb, 1.0, C.f64(tp)))
        logs = dev.train_step(b)
        ratios, _ = ck.measure(C.flat_of(dev.names, grads), C.LR, steps)
        ratios["logs"] = em_logs_ratio(logs, want_logs, rel, C.LOG_ABS)
        for k, r in ratios.items():
            acc[k] = max(acc.get(k, 0.0), r)
    return acc, dev


def test_checks_pass_on_the_unmutated_oracle():
    for kw in (dict(), dict(count=0), dict(count=1000, steps=1000), dict(count=200, steps=400)):
        acc, _ = _play((), **kw)
        assert max(acc.values()) <= 0.5, (kw, acc)


@pytest.mark.parametrize("mutation,caught_by", [("tp_hidden_bias", "m"), ("tp_head_bias", "m"), ("dense_bias", "m"),
                                                ("ln_bias", "m"), ("const_lr", "opt"), ("b2", "v"),
                                                ("eps_in_sqrt", "opt"), ("v_frozen", "v")])
def test_checks_catch_mutations_from_a_trained_state(mutation, caught_by):
    """Each mistake exceeds the named bound by >= 10x from random biases, non-zero moments and
    count 1000 of 2000."""
    acc, _ = _play((mutation,))
    print(mutation, acc)
    assert acc[caught_by] >= 10.0, acc


@pytest.mark.parametrize("shape,T_", [("G", 3), ("H", 2)])
def test_checks_catch_an_input_stage_of_64_rows(shape, T_):
    """What the sweep computed at the shapes its rule now refuses: at G only the rewards are
    dropped (actions and next observations are rows 0..63 exactly), at H also 26 rows of the next
    observation.  Either exceeds the logs' and the gradients' bounds by >= 10x at the GPU test's T
    and batch size, so test_multistep_at_the_edges_of_the_sweep_plan sees the sweep run there."""
    kw = dict(count=200, steps=400, kind="multistep", shape=shape, B=16, T_=T_)
    acc, _ = _play((), **kw)
    assert max(acc.values()) <= 0.5, acc
    acc, _ = _play(("stage_64",), **kw)
    print(shape, acc)
    assert acc["logs"] >= 10.0 and acc["m"] >= 10.0, acc


def test_checks_catch_a_missing_clamp():
    """count 1000 past steps = 500: without the clamp the cosine is back at its full rate; at
    steps = count - 1 the rate is ~1e-8 of the initial one and only the bitwise check sees it."""
    acc, _ = _play(("no_clamp",), count=1000, steps=500)
    assert acc["opt"] >= 10.0 and acc["clamp"] == float("inf"), acc
    acc, _ = _play(("no_clamp",), count=1000, steps=999)
    assert acc["clamp"] == float("inf"), acc


def test_checks_catch_bias_correction_with_count():
    """At count 1000 both corrections have all but converged (1 - 0.999^t moves by 6e-4 per
    step: 1.5e-7 of a parameter, the size of the bound).  The GPU tests also run from count 200
    (multistep) and from count 0: there the mistake is >= 10x the optimiser's bound."""
    acc, _ = _play(("bc_count",), count=200, steps=400)
    print(acc)
    assert acc["opt"] >= 10.0, acc
    acc, _ = _play(("bc_count",), count=1, steps=2000)
    assert acc["opt"] >= 10.0, acc


@pytest.mark.parametrize("mutation", ["tp_hidden_bias", "tp_head_bias"])
def test_frozen_predictor_biases_are_invisible_from_the_constructor_state(mutation):
    """The converse, and the reason for these tests: with the constructor's zero biases a kernel
    that drops a bias of the frozen termination predictor computes exactly the right thing."""
    _, good = _play((), count=0, zero_bias=True)
    acc, bad = _play((mutation,), count=0, zero_bias=True)
    assert max(acc.values()) <= 0.5, acc
    for which in range(3):
        np.testing.assert_array_equal(good.flat(which), bad.flat(which))


# ---------------------------------------------------------------------------
# Admission implies capacity: every shape em_plan sends to the sweep is within each limit of
# em_sweep_kernel, restated here from the kernel (csrc/emtrain.hip), one predicate per limit and
# apart from em_plan; the rule of the commit before this check is kept as _parent_sw_admits.
# ---------------------------------------------------------------------------
_GRID_OBS = np.arange(1, 131)
_GRID_ACT = (1, 2, 5, 8, 21)
_GRID_W = (8, 20, 32, 50, 64, 96, 128, 144, 192, 256, 272)
_GRID_TP = ((16,), (64,), (128, 256, 128), (272, 144), C.SHAPES["K"][3])
_R, _NT, _NW, _FM, _RQ, _SCR = 16, 1024, 16, 32, 10, 16 * 16 * 16      # R, SW_NT, SW_NW, SW_FM, SW_RQ, SW_SCR
_units_cache = {}


def _units(Kc, No):
    """sw_plan (the kernel's own split of an op into tiles x S units of cks k-steps) against the
    kernel's two limits on it: (units and fragments fit, the split's reduction fits); a width is an
    int or the pair (a, b) for a obs + b over _GRID_OBS."""
    key = (Kc, No)
    if key not in _units_cache:
        Kc, No = (x[0] * _GRID_OBS + x[1] if isinstance(x, tuple) else np.full(_GRID_OBS.shape, x) for x in key)
        ntile, nks = (No + 15) // 16, (Kc + 3) // 4
        S = np.ones_like(ntile)
        for _ in range(4):      # S doubles from 1 to at most SW_NW = 16
            S = np.where((S < _NW) & (ntile * S * 2 <= _NW) & (S * 2 <= nks), 2 * S, S)
        # sw_compute: one unit per wave (SW_NW waves); sw_load / sw_chain: fr[SW_FM] fragments per chunk;
        # sw_compute's k-split reduction: q = tid + i SW_NT, i < 4 ("No <= 128 here ... q < 4 SW_NT")
        _units_cache[key] = ((ntile * S <= _NW) & (-(-nks // S) <= _FM), (S == 1) | (No * _R <= 4 * _NT))
    return _units_cache[key]


def _sweep_ops(A, hid, tph, tw):
    """(Kc, No) of every op of em_sweep_kernel's programs: fw_op (n layers, the frozen predictor's m
    layers and its m dX ops) and the backward sweep's dX op of every layer."""
    dims = [(1, A), *hid, (1, 0)]
    tdims = [(1, 0), *tph, 1] if tw > 0 else []
    fw = list(zip(dims[:-1], dims[1:])) + list(zip(tdims[:-1], tdims[1:]))
    return fw + [(n, k) for k, n in fw]


def _kernel_limits(A, hid, tph, tw):
    """name -> bool [obs]: each limit of em_sweep_kernel, over _GRID_OBS."""
    D = _GRID_OBS
    ops = [_units(k, n) for k, n in _sweep_ops(A, hid, tph, tw)]
    K0, n_act, tsum = D + A, D + A + sum(hid), (D + sum(tph) + 1 if tw > 0 else D)
    maxd = np.maximum(K0, max(hid + (tph if tw > 0 else ())))
    # the kernel's LDS carve-up: x0, xhat [K0][R] | acts[0..n] | gA, gB, gC [maxd][R] | nobs [D][R] | tp
    # acts (or pred [D][R]) | carry [D][R] | scr [SW_SCR] | lnacc, lnp [2][K0] each
    dyn = 4 * (_R * (2 * K0 + (n_act + D) + 3 * maxd + D + tsum + D) + _SCR + 4 * K0)
    return {
        # in_load / `if (tid < nin)`: one staged value per thread of the SW_NT
        "stage": (A + D + 1) * _R <= _NT,
        "units": np.logical_and.reduce([u for u, _ in ops]),
        "split": np.logical_and.reduce([sp for _, sp in ops]),
        # the backward sweep's rec[SW_RQ]: st[tid + j SW_NT], j < SW_RQ, covers xhat | rstd | acts | g
        "record": _R * (K0 + 1 + n_act + D) <= _RQ * _NT,
        # dynamic + the kernel's __shared__ arrays within a CU's LDS
        "lds": dyn + C.SW_STATIC_LDS <= C.CU_LDS_BYTES,
    }, dyn


def _parent_sw_admits(lims, dyn):
    """sw_fits and em_create's test before this check: op units, the record, and
    ``sl * 4 <= 160 * 1024`` on the dynamic LDS alone."""
    return lims["units"] & lims["record"] & (dyn <= 160 * 1024)


def _grid():
    for A in _GRID_ACT:
        for n in (1, 2, 3):
            for hid in itertools.product(_GRID_W, repeat=n):
                yield A, hid, (), 0.0
                for tph in _GRID_TP:
                    yield A, hid, tph, 1.0


_GRID_T, _GRID_B = 4, 16


def test_sweep_admission_implies_the_kernels_capacity():
    admitted, parent_bad, top = 0, {}, {"nin": 0, "record": 0, "lds": 0}
    for A, hid, tph, tw in _grid():
        plan = C.em_plan_dims(_GRID_OBS, A, hid, tph or (16,), "multistep", tw, _GRID_T, _GRID_B)
        ok = plan["lds"] <= C.LDS_BUDGET          # em_create accepts the shape at all
        # the fallback: the fused step's LDS beside em_seq_grad_kernel's static arrays (the same ones)
        assert (plan["lds"][ok] + C.SW_STATIC_LDS <= C.CU_LDS_BYTES).all()
        adm = plan["sweep"] & ok
        lims, dyn = _kernel_limits(A, hid, tph, tw)
        assert (dyn == plan["sweep_need"]).all(), (A, hid, tph, tw)
        for name, within in lims.items():
            assert within[adm].all(), (name, A, hid, tph, tw, _GRID_OBS[adm & ~within])
        admitted += int(adm.sum())
        for k, v in (("nin", plan["nin"]), ("record", plan["record"]), ("lds", dyn + C.SW_STATIC_LDS)):
            top[k] = max(top[k], int(v[adm].max()) if adm.any() else 0)
        padm = _parent_sw_admits(lims, dyn) & ok
        for name, within in lims.items():
            parent_bad[name] = parent_bad.get(name, 0) + int((padm & ~within).sum())
    print("admitted", admitted, "largest admitted", top, "parent admits beyond a limit", parent_bad)
    # not vacuous: the grid reaches the stage's and the record's limit exactly, and the LDS window
    assert admitted > 10000 and top["nin"] == _NT and top["record"] == _RQ * _NT
    assert C.CU_LDS_BYTES - C.SW_STATIC_LDS < top["lds"] <= C.CU_LDS_BYTES
    # red before green: the parent's rule admits shapes past the stage and past the LDS
    assert parent_bad["stage"] > 0 and parent_bad["lds"] > 0 and not (parent_bad["units"] or parent_bad["record"])


@pytest.mark.parametrize("shape,tw,limit", [("G", 0.0, "stage"), ("G", 1.0, "stage"), ("H", 1.0, "stage"),
                                            ("K", 1.0, "lds")])
def test_parent_rule_admitted_shapes_the_kernel_cannot_run(shape, tw, limit):
    D, A, hid, tph = C.SHAPES[shape]
    i = D - 1
    lims, dyn = _kernel_limits(A, hid, tph, tw)
    assert _parent_sw_admits(lims, dyn)[i] and not lims[limit][i]
    assert all(within[i] for name, within in lims.items() if name != limit)
    assert not C.em_plan(shape, "multistep", tw, 2, 16)["sweep"]


# ---------------------------------------------------------------------------
# The C++ plan itself (csrc/emlayout.h: em_plan, which fqlpop_emtrain_create copies) against
# em_plan_dims: tests/cpp/emlayout_test.cpp, a stand-alone child process under AddressSanitizer and
# UBSan, walks the grid above, SHAPES and PLAN_PROBES, checks the kernels' layouts at every shape
# and writes one record per shape.  The fields are integers: equal, no tolerance.  Every field at
# the named shapes, of every kind; over the grid (5.7 million multistep shapes) whether the shape
# is refused, the fused step's LDS and the path.
# ---------------------------------------------------------------------------
_PLAN_FIELDS = ("lds", "sweep", "sweep_lds", "tchunks", "blocks", "seq_stride", "nin", "record", "sweep_need")


_KINDS = {"state": 0, "termination": 1, "multistep": 2}      # FQLPOP_EM_*


def _named_plan_cases():
    """(label, kind, D, A, hid, tph, tw, T, B, option) of SHAPES A-L, multistep with and without the
    frozen predictor and the sweep option and the two single-step kinds, and of PLAN_PROBES."""
    for name, (D, A, hid, tph) in C.SHAPES.items():
        for tw in (0.0, 1.0):
            for T_, B, option in ((2, 16, 1), (67, 48, 1), (2, 16, 0)):
                yield name, "multistep", D, A, hid, tph, tw, T_, B, option
            yield name, "state", D, A, hid, tph, tw, 1, 32, 1
        yield name, "termination", D, A, hid, tph, 0.0, 1, 32, 1
    for D, A, hid, tph, tw, _ in C.PLAN_PROBES:
        yield f"probe {D} {A} {hid} {tph}", "multistep", D, A, hid, tph, tw, 2, 16, 1


def _shape_lines():
    def ints(v):
        return f"{len(v)} " + " ".join(str(int(x)) for x in v)

    for _, kind, D, A, hid, tph, tw, T_, B, option in _named_plan_cases():
        net = tph if kind == "termination" else hid      # the trained net's hidden widths
        yield f"shape {_KINDS[kind]} {D} {A} {ints(net)} {ints(tph if tw > 0 else ())} {tw} {T_} {B} {option}"
    yield (f"grid {_GRID_T} {_GRID_B} {ints(_GRID_OBS)} {ints(_GRID_ACT)} {ints(_GRID_W)} {len(_GRID_TP)} " +
           " ".join(ints(tp) for tp in _GRID_TP))


def _run_emlayout_test(tmp_path, src=os.path.join(ROOT, "tests", "cpp", "emlayout_test.cpp")):
    """emlayout_test's records [shapes][refused, *_PLAN_FIELDS] and its report."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler (c++, g++ or clang++) on PATH")
    exe, shapes, plans = (str(tmp_path / f) for f in ("emlayout_test", "shapes.txt", "plans.bin"))
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    with open(shapes, "w") as f:
        f.write("\n".join(_shape_lines()) + "\n")
    run = subprocess.run([exe, shapes, plans], capture_output=True, text=True)
    return np.fromfile(plans, np.int32).reshape(-1, 1 + len(_PLAN_FIELDS)), run


@functools.lru_cache(maxsize=None)
def _grid_lds_sweep():
    """em_plan_dims' (lds, sweep) over _grid(), obs fastest: two arrays of one entry per shape."""
    plans = [C.em_plan_dims(_GRID_OBS, A, hid, tph or (16,), "multistep", tw, _GRID_T, _GRID_B)
             for A, hid, tph, tw in _grid()]
    return np.concatenate([p["lds"] for p in plans]), np.concatenate([p["sweep"] for p in plans])


def _plan_mismatches(got):
    """The shapes at which emlayout_test's records differ from em_plan_dims: labels of the named
    ones, row numbers of the grid's."""
    named = list(_named_plan_cases())
    bad = []
    for row, (name, kind, D, A, hid, tph, tw, T_, B, option) in zip(got, named):
        plan = C.em_plan_dims(D, A, hid, tph, kind, tw, T_, B, bool(option))
        want = [0] + [int(plan[k]) for k in _PLAN_FIELDS] if plan["lds"] <= C.LDS_BUDGET else [1] + [0] * len(_PLAN_FIELDS)
        if row.tolist() != want:
            bad.append((f"{name} {kind} tw {tw} T {T_} B {B} option {option}", row.tolist(), want))
    lds, sweep = _grid_lds_sweep()
    grid = got[len(named):]
    assert grid.shape[0] == lds.size
    refused = lds > C.LDS_BUDGET
    want = np.stack([refused, np.where(refused, 0, lds), sweep & ~refused], 1)
    bad += [(f"grid row {i}", grid[i].tolist(), want[i].tolist()) for i in np.flatnonzero((grid[:, :3] != want).any(1))]
    return bad


def test_cpp_plan_equals_em_plan_dims_over_the_grid(tmp_path):
    got, run = _run_emlayout_test(tmp_path)
    print(run.stdout)
    assert run.returncode == 0 and " 0 failed checks" in run.stdout, run.stdout + run.stderr
    bad = _plan_mismatches(got)
    assert not bad, (len(bad), bad[:12])
    # not vacuous: shapes on either path, and shapes the fused step's budget refuses
    assert got[:, 2].sum() > 10000 and (got[:, 2] == 0).sum() > 10000 and got[:, 0].sum() > 10000
