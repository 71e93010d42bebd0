"""World-model ensemble training on the GPU (fqlpop_emtrain_create_ensemble and the
*_ensemble calls): model k of a K-model handle against the single-model trainer built with
model k's seed and initial tree, bit for bit (np.array_equal on parameters, Adam m, Adam v
and the log vector), for both block placements (engine option em_ens_xcd); the handle
contract; and the driver's batched against its sequential output, byte for byte.

No oracle of its own: the single trainer is held to the float64 oracle by
test_gpu_emtrain.py."""
import ctypes
import functools

import numpy as np
import pytest

import envmodel as em
from _helpers import engine_options
from envmodel.trainer import (EnvModelTrainerConfig, StatePredictorEnsembleTrainer, StatePredictorTrainer,
                              TerminationPredictorEnsembleTrainer, TerminationPredictorTrainer)

pytestmark = pytest.mark.gpu
SEEDS = (5, 6, 7)
E_ARG = -1


class _Loader:
    def __init__(self, ds, episode_length=None):
        self.dataset = ds
        if episode_length:
            self.episode_length = episode_length


def _dataset(n, D, A, seed=0):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    nxt = (0.9 * obs + 0.1 * np.tanh(obs[:, ::-1])).astype(np.float32)
    return {"observations": obs, "actions": act, "next_observations": nxt,
            "rewards": np.where(rng.uniform(size=n) < 0.25, 0.0, -1.0).astype(np.float32)}


def _batch(rng, B, D, A, T=None):
    lead = (B,) if T is None else (B, T)
    obs = rng.standard_normal(lead + (D,)).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1, 1, lead + (A,)).astype(np.float32),
            "next_observations": (obs + 0.1 * rng.standard_normal(lead + (D,))).astype(np.float32),
            "rewards": np.where(rng.uniform(size=lead) < 0.25, 0.0, -1.0).astype(np.float32)}


def _logvec(d):
    return np.array([d[k] for k in sorted(d)], np.float32)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _state(flat):
    """(params, Adam m, Adam v) from a flat(which) callable."""
    return tuple(flat(w) for w in (0, 1, 2))


def _assert_model_equals(ens, k, single_state, tag):
    for w, (got, want) in enumerate(zip(_state(lambda w: ens.flat(k, w)), single_state)):
        assert np.array_equal(got, want), f"{tag}: model {k} {('params', 'adam m', 'adam v')[w]} differs"


# ------------------------------------------------------------------ state predictor
SP_D, SP_A, SP_HID, SP_B = 42, 8, (64, 96), 32  # 50 inputs: the tail k-step; two blocks per model


def _sp_setup(tw):
    spec = em.EnvModelSpec(SP_D, SP_A, SP_HID, (64,))
    tp = em.init_termination_predictor(spec, 2) if tw > 0 else None
    trees = [em.init_state_predictor(spec, 10 + s) for s in SEEDS]
    ds = _dataset(2000, SP_D, SP_A)
    rng = np.random.default_rng(3)
    injected = [[_batch(rng, SP_B, SP_D, SP_A) for _ in SEEDS] for _ in range(2)]
    return spec, tp, trees, ds, injected


def _sp_cfg(tw, seed=0, B=SP_B):
    return EnvModelTrainerConfig(steps=50, termination_weight=tw, batch_size=B, seed=seed, init_learning_rate=1e-3)


@functools.lru_cache(maxsize=None)
def _sp_reference(tw):
    """The single trainers' trajectory: three device-sampled steps, then two injected ones."""
    spec, tp, trees, ds, injected = _sp_setup(tw)
    out = []
    for k, s in enumerate(SEEDS):
        tr = StatePredictorTrainer(spec, trees[k], _Loader(ds), None, _sp_cfg(tw, s), tp_params=tp)
        tr.steps(3)
        rec = {"logs3": _logvec(tr.read_logs()), "state3": _state(tr.flat), "ilogs": []}
        for step in injected:
            rec["ilogs"].append(_logvec(tr.train_step(None, step[k])[1]))
        rec["state5"] = _state(tr.flat)
        rec["count"] = tr.count
        tr.close()
        out.append(rec)
    return out


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("tw", [0.0, 1.0])
def test_state_predictor_models_equal_single_trainers(tw, xcd):
    spec, tp, trees, ds, injected = _sp_setup(tw)
    ref = _sp_reference(tw)
    with engine_options(em_ens_xcd=xcd):
        ens = StatePredictorEnsembleTrainer(spec, trees, _Loader(ds), None, _sp_cfg(tw), SEEDS, tp_params=tp)
    assert ens.K == 3
    ens.steps(3)
    logs = ens.read_logs()
    for k in range(3):
        assert _same(_logvec(logs[k]), ref[k]["logs3"]), (k, logs[k])
        _assert_model_equals(ens, k, ref[k]["state3"], "after 3 device-sampled steps")
    assert not np.array_equal(ens.flat(0), ens.flat(1))  # different seeds, different models
    for i, step in enumerate(injected):
        _, logs = ens.train_step(None, step)
        for k in range(3):
            assert _same(_logvec(logs[k]), ref[k]["ilogs"][i]), (i, k)
    for k in range(3):
        _assert_model_equals(ens, k, ref[k]["state5"], "after the injected steps")
    assert ens.count == ref[0]["count"] == 5
    ens.close()


def test_shared_batch_is_the_batch_copied_k_times():
    spec, tp, trees, ds, injected = _sp_setup(1.0)
    b = injected[0][0]
    runs = []
    for batches in (b, [b, b, b]):
        ens = StatePredictorEnsembleTrainer(spec, trees, None, None, _sp_cfg(1.0), SEEDS, tp_params=tp)
        _, logs = ens.train_step(None, batches)
        ev = ens.eval_step(None, batches)
        runs.append(([_logvec(lg) for lg in logs], [_logvec(lg) for lg in ev],
                     [_state(lambda w, k=k: ens.flat(k, w)) for k in range(3)]))
        ens.close()
    for k in range(3):
        assert _same(runs[0][0][k], runs[1][0][k]) and _same(runs[0][1][k], runs[1][1][k])
        for a, c in zip(runs[0][2][k], runs[1][2][k]):
            assert np.array_equal(a, c)
    assert not _same(runs[0][0][0], runs[0][0][1])  # one batch, three different models


# ------------------------------------------------------------- termination predictor
@pytest.mark.parametrize("xcd", [0, 1])
def test_termination_predictor_models_equal_single_trainers(xcd):
    D, A, B = 28, 5, 32
    spec = em.EnvModelSpec(D, A, (8,), (64,))
    tree = em.init_termination_predictor(spec, 4)  # one initial tree: only the seed tells the models apart
    ds = _dataset(2000, D, A, seed=1)
    rng = np.random.default_rng(8)
    batches = [_batch(rng, B, D, A) for _ in SEEDS]
    keeps = np.stack([rng.uniform(size=(B, D)) >= 0.1 for _ in SEEDS])
    cfg = lambda s: EnvModelTrainerConfig(steps=40, batch_size=B, seed=s, init_learning_rate=1e-3)  # noqa: E731
    with engine_options(em_ens_xcd=xcd):
        ens = TerminationPredictorEnsembleTrainer(spec, [tree] * 3, _Loader(ds), None, cfg(0), SEEDS)
    singles = [TerminationPredictorTrainer(spec, tree, _Loader(ds), None, cfg(s)) for s in SEEDS]
    # device sampling and device dropout: both keyed by the model's seed
    ens.steps(2)
    logs = ens.read_logs()
    for k, tr in enumerate(singles):
        tr.steps(2)
        assert _same(_logvec(logs[k]), _logvec(tr.read_logs())), k
        _assert_model_equals(ens, k, _state(tr.flat), "device dropout")
    assert not np.array_equal(ens.flat(0), ens.flat(1)) and not np.array_equal(ens.flat(1), ens.flat(2))
    # an injected batch with the Philox mask of each model's seed, then with a keep mask per model
    for km in (None, keeps):
        _, logs = ens.train_step(None, batches, keep_masks=km)
        for k, tr in enumerate(singles):
            _, want = tr.train_step(None, batches[k], keep_mask=None if km is None else km[k])
            assert _same(_logvec(logs[k]), _logvec(want)), k
            _assert_model_equals(ens, k, _state(tr.flat), "injected keep mask" if km is not None else "injected")
    ev = ens.eval_step(None, batches)
    for k, tr in enumerate(singles):
        assert _same(_logvec(ev[k]), _logvec(tr.eval_step(None, batches[k]))), k
        tr.close()
    ens.close()


# ------------------------------------------------------------------------ multistep
def _trajectory_dataset(n_ep, D, A, seed=0):
    """Episode-major rows of 1000-step trajectories: o' = 0.9 o + 0.3 tanh([o, a] M)."""
    rng = np.random.default_rng(seed)
    M = (0.3 * rng.standard_normal((D + A, D))).astype(np.float32)
    o = rng.standard_normal((n_ep, D)).astype(np.float32)
    cols = {k: [] for k in ("observations", "actions", "next_observations")}
    for _ in range(1000):
        a = rng.uniform(-1, 1, (n_ep, A)).astype(np.float32)
        o2 = (0.9 * o + 0.3 * np.tanh(np.concatenate([o, a], 1) @ M)).astype(np.float32)
        cols["observations"].append(o)
        cols["actions"].append(a)
        cols["next_observations"].append(o2)
        o = o2
    ds = {k: np.stack(v, 1).reshape(n_ep * 1000, -1) for k, v in cols.items()}
    ds["rewards"] = np.where(ds["next_observations"][:, 0] > 1.0, 0.0, -1.0).astype(np.float32)
    return ds


@functools.lru_cache(maxsize=None)
def _trajectories():
    return _trajectory_dataset(2, 28, 5, seed=5)


@pytest.mark.parametrize("tw,T,sweep,xcd", [(0.0, 16, 1, 1), (0.0, 48, 1, 0), (0.0, 48, 1, 1), (0.0, 8, 0, 1),
                                            (1.0, 16, 1, 0)])
def test_multistep_models_equal_single_trainers(tw, T, sweep, xcd):
    """One T chunk (T = 16) and three (T = 48) of the sweep path's dW GEMM, the round-5 kernel
    (em_seq_sweep = 0), and the frozen termination term: two device-sampled steps and one
    injected step with a batch per model."""
    D, A, B = 28, 5, 32
    spec = em.EnvModelSpec(D, A, (128, 256, 128), (128, 256, 128) if tw > 0 else (64,))
    rng = np.random.default_rng(7)
    trees = [em.init_state_predictor(spec, 20 + s) for s in SEEDS]
    for t in trees:
        t["LayerNorm_0"]["scale"] = (1 + 0.1 * rng.standard_normal(D + A)).astype(np.float32)
        t["LayerNorm_0"]["bias"] = (0.1 * rng.standard_normal(D + A)).astype(np.float32)
    tp = em.init_termination_predictor(spec, 2) if tw > 0 else None
    ds = _trajectories()
    batches = [_batch(rng, B, D, A, T) for _ in SEEDS]
    cfg = lambda s: EnvModelTrainerConfig(steps=50, model="multistep", sequence_length=T, termination_weight=tw,  # noqa: E731
                                          batch_size=B, seed=s, init_learning_rate=1e-3)
    with engine_options(em_seq_sweep=sweep, em_ens_xcd=xcd):
        ens = StatePredictorEnsembleTrainer(spec, trees, _Loader(ds, 1000), None, cfg(0), SEEDS, tp_params=tp)
        singles = [StatePredictorTrainer(spec, trees[k], _Loader(ds, 1000), None, cfg(s), tp_params=tp)
                   for k, s in enumerate(SEEDS)]
    ens.steps(2)
    logs = ens.read_logs()
    for k, tr in enumerate(singles):
        tr.steps(2)
        assert _same(_logvec(logs[k]), _logvec(tr.read_logs())), k
        _assert_model_equals(ens, k, _state(tr.flat), "device-sampled windows")
    _, logs = ens.train_step(None, batches)
    for k, tr in enumerate(singles):
        _, want = tr.train_step(None, batches[k])
        assert _same(_logvec(logs[k]), _logvec(want)), k
        _assert_model_equals(ens, k, _state(tr.flat), "injected windows")
        tr.close()
    ens.close()


# ------------------------------------------------------------------ placement edges
@functools.lru_cache(maxsize=None)
def _edge_reference(B, K):
    spec = em.EnvModelSpec(SP_D, SP_A, SP_HID, (64,))
    ds = _dataset(1000, SP_D, SP_A, seed=2)
    out = {}
    for k in sorted({0, 8, K - 1}):
        tr = StatePredictorTrainer(spec, em.init_state_predictor(spec, 30 + k), _Loader(ds), None,
                                   _sp_cfg(0.0, 100 + k, B))
        tr.steps(2)
        out[k] = (_logvec(tr.read_logs()), _state(tr.flat))
        tr.close()
    return spec, ds, out


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("B,K", [(16, 9), (32, 16)])
def test_more_models_than_xcds(B, K, xcd):
    """K = 9 with one block per model (padding under em_ens_xcd = 1) and K = 16 with two:
    models 0, 8 and K - 1."""
    spec, ds, ref = _edge_reference(B, K)
    with engine_options(em_ens_xcd=xcd):
        ens = StatePredictorEnsembleTrainer(spec, [em.init_state_predictor(spec, 30 + k) for k in range(K)],
                                            _Loader(ds), None, _sp_cfg(0.0, 0, B), [100 + k for k in range(K)])
    ens.steps(2)
    logs = ens.read_logs()
    assert len(logs) == K
    for k, (want_logs, want_state) in ref.items():
        assert _same(_logvec(logs[k]), want_logs), k
        _assert_model_equals(ens, k, want_state, f"K = {K}, xcd = {xcd}")
    ens.close()


# ------------------------------------------------------------------------ eval, contract
def test_eval_ensemble_equals_single_eval_and_updates_nothing():
    spec, tp, trees, ds, injected = _sp_setup(1.0)
    ens = StatePredictorEnsembleTrainer(spec, trees, _Loader(ds), None, _sp_cfg(1.0), SEEDS, tp_params=tp)
    ens.steps(1)
    before = [_state(lambda w, k=k: ens.flat(k, w)) for k in range(3)]
    ev = ens.eval_step(None, injected[0])
    ev_shared = ens.eval_step(None, injected[0][1])
    assert ens.count == 1
    for k, s in enumerate(SEEDS):
        tr = StatePredictorTrainer(spec, trees[k], _Loader(ds), None, _sp_cfg(1.0, s), tp_params=tp)
        tr.steps(1)
        assert _same(_logvec(ev[k]), _logvec(tr.eval_step(None, injected[0][k]))), k
        assert _same(_logvec(ev_shared[k]), _logvec(tr.eval_step(None, injected[0][1]))), k
        tr.close()
        _assert_model_equals(ens, k, before[k], "eval_ensemble")
    ens.close()


def test_handle_contract():
    from fqlpop import _lib
    lib = _lib.load_library()
    spec, tp, trees, ds, injected = _sp_setup(0.0)
    ens = StatePredictorEnsembleTrainer(spec, trees, _Loader(ds), None, _sp_cfg(0.0), SEEDS)
    k = ctypes.c_int()
    assert lib.fqlpop_emtrain_num_models(ens._h, ctypes.byref(k)) == 0 and k.value == 3
    arrs = [np.ascontiguousarray(injected[0][0][n]) for n in ("observations", "actions", "rewards",
                                                              "next_observations")]
    ptrs = [_lib.fptr(a) for a in arrs]
    out = np.zeros(8, np.float32)
    flat = np.zeros(ens.n_params, np.float32)
    calls = {
        "fqlpop_emtrain_step_injected_ensemble": lambda: lib.fqlpop_emtrain_step_injected(ens._h, *ptrs, None),
        "fqlpop_emtrain_eval_ensemble": lambda: lib.fqlpop_emtrain_eval(ens._h, *ptrs, _lib.fptr(out)),
        "fqlpop_emtrain_read_logs_ensemble": lambda: lib.fqlpop_emtrain_read_logs(ens._h, _lib.fptr(out)),
        "fqlpop_emtrain_get_params_model": lambda: lib.fqlpop_emtrain_get_params(ens._h, 0, _lib.fptr(flat),
                                                                                 ens.n_params),
    }
    for name, call in calls.items():
        assert call() == E_ARG, name
        assert name.encode() in lib.fqlpop_last_error(), (name, lib.fqlpop_last_error())
    assert ens.count == 0
    assert lib.fqlpop_emtrain_get_params_model(ens._h, 3, 0, _lib.fptr(flat), ens.n_params) == E_ARG
    ens.close()
    # refusals with nothing allocated: a params size mismatch, a null seeds
    cfg = ens._cfg
    both = np.zeros(3 * ens.n_params, np.float32)
    seeds = (ctypes.c_uint64 * 3)(1, 2, 3)
    h = ctypes.c_void_p()
    assert lib.fqlpop_emtrain_create_ensemble(ctypes.byref(cfg), 3, _lib.fptr(both), 3 * ens.n_params + 1, seeds, 0,
                                              ctypes.byref(h)) == E_ARG and not h.value
    assert lib.fqlpop_emtrain_create_ensemble(ctypes.byref(cfg), 3, _lib.fptr(both), 3 * ens.n_params, None, 0,
                                              ctypes.byref(h)) == E_ARG and not h.value
    # an ensemble handle of one model is the single-model handle with that seed
    one = StatePredictorEnsembleTrainer(spec, trees[:1], _Loader(ds), None, _sp_cfg(0.0, 999), SEEDS[:1])
    ref = _sp_reference(0.0)[0]
    one.steps(3)
    assert _same(_logvec(one.read_logs()[0]), ref["logs3"])
    _assert_model_equals(one, 0, ref["state3"], "K = 1")
    # and the single-model calls serve it
    assert lib.fqlpop_emtrain_read_logs(one._h, _lib.fptr(out)) == 0
    assert lib.fqlpop_emtrain_get_params(one._h, 0, _lib.fptr(flat), one.n_params) == 0
    assert np.array_equal(flat, ref["state3"][0])
    one.close()


# --------------------------------------------------------------------------- driver
def _driver_outputs(tmp_path, tag, argv, seq):
    import train_env_model as tem
    out = tem.main(argv + [f"--save_directory={tmp_path / tag}"] + (["--ensemble_sequential"] if seq else []))
    return {p.name: p.read_bytes() for p in sorted(out.iterdir()) if "_ens" in p.name}


@pytest.mark.parametrize("model,extra", [("baseline", []), ("termination_predictor", []),
                                         ("multistep", ["--sequence_length=16", "--batch_size=16"])])
def test_driver_batched_files_are_the_sequential_files(tmp_path, model, extra):
    """train_env_model.py --ensemble_size=3: the batched trainer writes byte for byte the
    .pt, _config.yaml and _log.csv files of the three runs one after the other."""
    import train_env_model as tem
    ds = _trajectory_dataset(3, 28, 5, seed=9)
    data = tmp_path / "data"
    data.mkdir()
    np.savez(data / "cube-single-play.npz", masks=(ds["rewards"] != 0).astype(np.float32), **ds)
    common = [f"--data_directory={data}", "--steps=30", "--val_batches=2"]
    files = {}
    for tag, seq in (("batched", False), ("sequential", True)):
        if model != "termination_predictor":  # the default termination_weight loads the trained predictor
            tem.main(["--model=termination_predictor", f"--save_directory={tmp_path / tag}"] + common)
        files[tag] = _driver_outputs(tmp_path, tag, [f"--model={model}", "--ensemble_size=3"] + common + extra, seq)
    want = {f"{model}_ens{k}{s}" for k in range(3) for s in (".pt", "_config.yaml", "_log.csv")}
    assert set(files["batched"]) == set(files["sequential"]) == want
    for name in sorted(want):
        assert files["batched"][name] == files["sequential"][name], name
    assert files["batched"][f"{model}_ens0.pt"] != files["batched"][f"{model}_ens1.pt"]
    assert b"val/loss" in files["batched"][f"{model}_ens2_log.csv"]
