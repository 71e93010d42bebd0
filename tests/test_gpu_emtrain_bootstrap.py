"""Bootstrapped world-model ensembles on the GPU (fqlpop_emtrain_set_bootstrap* / _get_bootstrap /
_eval_oob), against the NumPy restatement of the device draws (tests/emtrain_draw_np.py) and
the injected-batch calls: the tables and out-of-bag lists; the device draw of a train step, with
and without a table, bit for bit the injected step on the restated rows (np.array_equal on
parameters, Adam m, Adam v and the log vector); model k of an ensemble against the single
trainer of its seed; the out-of-bag evaluation against eval_ensemble on the restated units;
every refusal; and the drivers.

Shapes (tests/emtrain_boot_cases.py): obs 3, act 2, hidden (32, 32), B = 32 (two 16-row blocks
per model), 203 rows, 7 episodes of 20 rows with windows of 8, K = 1, 3 and 9 (B = 16)."""
import ctypes
import functools

import numpy as np
import pytest

import emtrain_boot_cases as C
import emtrain_draw_np as R
import envmodel as em
from _helpers import engine_options
from envmodel.trainer import (EnvModelTrainerConfig, StatePredictorEnsembleTrainer, StatePredictorTrainer,
                              TerminationPredictorEnsembleTrainer, TerminationPredictorTrainer)

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -3
KEYS = ("observations", "actions", "rewards", "next_observations")
I64P = ctypes.POINTER(ctypes.c_int64)
SWEEPS = {"state": (1,), "termination": (1,), "multistep": (1, 0)}  # em_seq_sweep: both multistep kernels
KIND_SWEEP = [(kind, sw) for kind in C.KINDS for sw in SWEEPS[kind]]


class _Loader:
    def __init__(self, ds, episode_length=None):
        self.dataset = ds
        if episode_length:
            self.episode_length = episode_length


@functools.lru_cache(maxsize=None)
def _dataset(kind):
    """Rows of a smooth map (episode-major for the multistep model), a quarter of them terminal."""
    n = C.N_EP * C.EP_LEN if kind == "multistep" else C.N_ROWS
    rng = np.random.default_rng(len(kind))
    obs = rng.standard_normal((n, C.D)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, C.A)).astype(np.float32)
    nxt = (0.9 * obs + 0.1 * np.tanh(obs[:, ::-1]) + 0.05 * act[:, :1]).astype(np.float32)
    return {"observations": obs, "actions": act, "next_observations": nxt,
            "rewards": np.where(rng.uniform(size=n) < 0.25, 0.0, -1.0).astype(np.float32)}


def _spec():
    return em.EnvModelSpec(C.D, C.A, C.HIDDEN, C.HIDDEN)


def _tree(kind, seed):
    spec = _spec()
    if kind == "termination":
        return em.init_termination_predictor(spec, 50 + seed)
    tree = em.init_state_predictor(spec, 50 + seed)
    rng = np.random.default_rng(seed)
    tree["LayerNorm_0"]["scale"] = (1 + 0.1 * rng.standard_normal(C.D + C.A)).astype(np.float32)
    tree["LayerNorm_0"]["bias"] = (0.1 * rng.standard_normal(C.D + C.A)).astype(np.float32)
    return tree


def _cfg(kind, seed, B):
    # the state predictor carries the frozen termination term; the multistep model does not
    return EnvModelTrainerConfig(steps=50, batch_size=B, seed=seed, init_learning_rate=1e-3,
                                 termination_weight=1.0 if kind == "state" else 0.0,
                                 model="multistep" if kind == "multistep" else "baseline", sequence_length=C.T)


def _make(kind, seeds, bootstrap=False, B=C.B, sweep=1, xcd=0, single=False, data=True, trees=None):
    """A trainer of ``kind``: the single-model class for ``single`` (one seed), else the ensemble."""
    spec = _spec()
    loader = _Loader(_dataset(kind), C.EP_LEN if kind == "multistep" else None) if data else None
    trees = trees or [_tree(kind, s) for s in seeds]
    tp = em.init_termination_predictor(spec, 2) if kind == "state" else None
    with engine_options(em_seq_sweep=sweep, em_ens_xcd=xcd):
        if kind == "termination":
            if single:
                return TerminationPredictorTrainer(spec, trees[0], loader, None, _cfg(kind, seeds[0], B),
                                                   bootstrap=bootstrap)
            return TerminationPredictorEnsembleTrainer(spec, trees, loader, None, _cfg(kind, 0, B), seeds,
                                                       bootstrap=bootstrap)
        if single:
            return StatePredictorTrainer(spec, trees[0], loader, None, _cfg(kind, seeds[0], B), tp_params=tp,
                                         bootstrap=bootstrap)
        return StatePredictorEnsembleTrainer(spec, trees, loader, None, _cfg(kind, 0, B), seeds, tp_params=tp,
                                             bootstrap=bootstrap)


def _batch(kind, first_rows):
    """The host batch of dataset rows (multistep: windows of T rows from each first row)."""
    ds = _dataset(kind)
    idx = np.asarray(first_rows)
    if kind == "multistep":
        idx = idx[:, None] + np.arange(C.T)
    return {k: np.ascontiguousarray(ds[k][idx]) for k in KEYS}


def _drawn_batch(kind, seed, step, B, table=None):
    if kind == "multistep":
        return _batch(kind, R.train_windows(seed, step, B, C.N_EP * C.EP_LEN, C.EP_LEN, C.T, table))
    return _batch(kind, R.train_rows(seed, step, B, C.N_ROWS, table))


def _oob_batch(kind, seed, j, draw, B, oob):
    if kind == "multistep":
        return _batch(kind, R.oob_units(seed, j, draw, B, oob, C.EP_LEN, C.T))
    return _batch(kind, R.oob_units(seed, j, draw, B, oob))


def _logvec(d):
    return np.array([d[k] for k in sorted(d)], np.float32)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _state(tr, k=None):
    """(params, Adam m, Adam v) of a single trainer, or of model k of an ensemble."""
    return tuple(tr.flat(w) if k is None else tr.flat(k, w) for w in (0, 1, 2))


def _assert_states_equal(got, want, tag):
    for name, g, w in zip(("params", "adam m", "adam v"), got, want):
        assert np.array_equal(g, w), f"{tag}: {name} differs"


def _want_tables(kind, seeds):
    n = C.n_units(kind)
    tables = [R.bootstrap_table(s, n) for s in seeds]
    return tables, [R.oob_list(t, n) for t in tables]


# ---------------------------------------------------------------- 1. tables, OOB lists
@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("kind", C.KINDS)
def test_tables_and_oob_lists_are_the_restatement(kind, K):
    seeds = C.SEEDS[K]
    tr = _make(kind, seeds, bootstrap=True, B=C.B9 if K == 9 else C.B, single=K == 1)
    tables, oobs = _want_tables(kind, seeds)
    assert tr.n_units == C.n_units(kind)
    for k in range(K):
        assert np.array_equal(tr.bootstrap_table(k), tables[k]), (kind, K, k)
        got = tr.oob_rows(k)
        assert len(got) >= 1 and np.array_equal(got, oobs[k]), (kind, K, k)
    tr.close()


# ---------------------------------------------------------------- 2. the device draw
@pytest.mark.parametrize("boot", [False, True])
@pytest.mark.parametrize("kind,sweep", KIND_SWEEP)
def test_device_draw_is_the_injected_step_on_the_restated_rows(kind, sweep, boot):
    """Three fqlpop_emtrain_step calls against three step_injected calls on the rows the
    restatement draws (through the read-back table with bootstrap on)."""
    seed = C.SEEDS[1][0]
    dev = _make(kind, (seed,), bootstrap=boot, sweep=sweep, single=True)
    inj = _make(kind, (seed,), sweep=sweep, single=True)
    table = dev.bootstrap_table() if boot else None
    if boot:
        assert np.array_equal(table, R.bootstrap_table(seed, C.n_units(kind)))
    for step in range(3):
        dev.steps(1)
        got = _logvec(dev.read_logs())
        _, want = inj.train_step(None, _drawn_batch(kind, seed, step, C.B, table))
        assert _same(got, _logvec(want)), (kind, sweep, boot, step, got, want)
    _assert_states_equal(_state(dev), _state(inj), f"{kind} sweep {sweep} bootstrap {boot}")
    assert dev.count == inj.count == 3
    if boot:  # and the table matters: the rows differ from the plain draw's
        assert not np.array_equal(R.train_rows(seed, 0, C.B, C.N_ROWS), R.train_rows(seed, 0, C.B, C.N_ROWS,
                                                                                     R.bootstrap_table(seed, C.N_ROWS)))
    dev.close()
    inj.close()


# ---------------------------------------------------------------- 3. identity table
@pytest.mark.parametrize("kind,sweep", KIND_SWEEP)
def test_identity_table_is_the_trainer_without_bootstrap(kind, sweep):
    seeds = C.SEEDS[3]
    plain = _make(kind, seeds, sweep=sweep)
    ident = _make(kind, seeds, sweep=sweep)
    ident.set_bootstrap(table=np.tile(np.arange(C.n_units(kind)), (3, 1)))
    plain.steps(3)
    ident.steps(3)
    for k in range(3):
        assert _same(_logvec(ident.read_logs()[k]), _logvec(plain.read_logs()[k])), (kind, k)
        _assert_states_equal(_state(ident, k), _state(plain, k), f"{kind} identity table, model {k}")
        assert len(ident.oob_rows(k)) == 0
    ident.set_bootstrap(False)  # dropped: the plain path again
    plain.steps(1)
    ident.steps(1)
    _assert_states_equal(_state(ident, 1), _state(plain, 1), f"{kind} after dropping the tables")
    plain.close()
    ident.close()


# ---------------------------------------------------------------- 4. the model axis
@functools.lru_cache(maxsize=None)
def _single_reference(kind, seed, B, sweep):
    """A bootstrapped single trainer of ``seed``: two device-sampled steps, one out-of-bag evaluation."""
    tr = _make(kind, (seed,), bootstrap=True, B=B, sweep=sweep, single=True)
    tr.steps(2)
    out = (_logvec(tr.read_logs()), _state(tr), _logvec(tr.eval_oob(2, 9)))
    tr.close()
    return out


@pytest.mark.parametrize("kind,sweep", KIND_SWEEP)
def test_ensemble_model_is_the_single_bootstrapped_trainer(kind, sweep):
    seeds = C.SEEDS[3]
    ens = _make(kind, seeds, bootstrap=True, sweep=sweep)
    ens.steps(2)
    logs, oob = ens.read_logs(), ens.eval_oob(2, 9)
    for k, s in enumerate(seeds):
        want_logs, want_state, want_oob = _single_reference(kind, s, C.B, sweep)
        assert _same(_logvec(logs[k]), want_logs), (kind, k)
        _assert_states_equal(_state(ens, k), want_state, f"{kind} model {k}")
        assert _same(_logvec(oob[k]), want_oob), (kind, k)
    ens.close()


@pytest.mark.parametrize("xcd", [0, 1])
def test_more_models_than_xcds(xcd):
    seeds = C.SEEDS[9]
    ens = _make("state", seeds, bootstrap=True, B=C.B9, xcd=xcd)
    ens.steps(2)
    logs, oob = ens.read_logs(), ens.eval_oob(2, 9)
    for k in (0, 7, 8):
        want_logs, want_state, want_oob = _single_reference("state", seeds[k], C.B9, 1)
        assert _same(_logvec(logs[k]), want_logs), k
        _assert_states_equal(_state(ens, k), want_state, f"K = 9, xcd {xcd}, model {k}")
        assert _same(_logvec(oob[k]), want_oob), k
    ens.close()


def test_same_seed_different_tables_diverge():
    n = C.N_ROWS
    tree = _tree("state", 1)
    tables = np.stack([np.arange(n), np.arange(n)[::-1]])
    for tab, differ in ((tables, True), (tables[[0, 0]], False)):
        ens = _make("state", (5, 5), trees=[tree, tree])
        ens.set_bootstrap(table=tab)
        ens.steps(1)
        assert np.array_equal(ens.flat(0), ens.flat(1)) != differ
        ens.close()


# ---------------------------------------------------------------- 5. out-of-bag evaluation
@pytest.mark.parametrize("kind,sweep", KIND_SWEEP)
def test_eval_oob_is_eval_ensemble_on_the_restated_units(kind, sweep):
    seeds, draw = C.SEEDS[3], 77
    ens = _make(kind, seeds, bootstrap=True, sweep=sweep)
    ens.steps(1)
    before = [_state(ens, k) for k in range(3)]
    oobs = [ens.oob_rows(k) for k in range(3)]
    one = ens.eval_oob(1, draw)
    three = ens.eval_oob(3, draw)
    terms = [ens.eval_step(None, [_oob_batch(kind, s, j, draw, C.B, oobs[k]) for k, s in enumerate(seeds)])
             for j in range(3)]
    assert ens.count == 1
    for k in range(3):
        assert _same(_logvec(one[k]), _logvec(terms[0][k])), (kind, k, one[k], terms[0][k])
        for key in three[k]:
            t = np.array([terms[j][k][key] for j in range(3)], np.float64)
            print(f"eval_oob(3) {kind} model {k} {key}: device {three[k][key]!r} mean {t.mean()!r}")
            # a three-term float32 sum and one division: a few ulp of the largest term
            assert abs(three[k][key] - t.mean()) <= 1e-6 * np.abs(t).max(), (kind, k, key)
        _assert_states_equal(_state(ens, k), before[k], f"{kind} eval_oob, model {k}")
    assert not _same(_logvec(one[0]), _logvec(ens.eval_oob(1, draw + 1)[0]))  # another draw, other units
    ens.close()


def test_eval_oob_on_a_single_model_trainer_returns_one_dict():
    seed = C.SEEDS[1][0]
    tr = _make("state", (seed,), bootstrap=True, single=True)
    logs = tr.eval_oob(1, 3)
    want = tr.eval_step(None, _oob_batch("state", seed, 0, 3, C.B, tr.oob_rows()))
    assert isinstance(logs, dict) and _same(_logvec(logs), _logvec(want))
    tr.close()


# ---------------------------------------------------------------- 6. refusals
def _raw_tables(lib, tr, K):
    n = tr.n_units
    out = []
    for k in range(K):
        t, o, no = np.zeros(n, np.int64), np.zeros(n, np.int64), ctypes.c_int64()
        assert lib.fqlpop_emtrain_get_bootstrap(tr._h, k, t.ctypes.data_as(I64P), n, o.ctypes.data_as(I64P), n,
                                                ctypes.byref(no)) == 0
        out.append((t.tobytes(), o[:no.value].tobytes()))
    return out


@pytest.mark.parametrize("kind", ["state", "multistep"])
def test_refusals_change_nothing(kind):
    from fqlpop import _lib
    lib = _lib.load_library()
    seeds, n = C.SEEDS[3], C.n_units(kind)
    logs = np.zeros((3, 8), np.float32)
    buf, no = np.zeros(3 * n + 1, np.int64), ctypes.c_int64()
    ptr = buf.ctypes.data_as(I64P)
    # no dataset yet
    bare = _make(kind, seeds, data=False)
    for rc in (lib.fqlpop_emtrain_set_bootstrap(bare._h, 1), lib.fqlpop_emtrain_set_bootstrap_table(bare._h, ptr, 3 * n),
               lib.fqlpop_emtrain_eval_oob(bare._h, 1, 0, _lib.fptr(logs)),
               lib.fqlpop_emtrain_get_bootstrap(bare._h, 0, ptr, n, None, 0, ctypes.byref(no))):
        assert rc == E_STATE
    bare.close()
    # a dataset, no tables
    tr = _make(kind, seeds)
    assert lib.fqlpop_emtrain_eval_oob(tr._h, 1, 0, _lib.fptr(logs)) == E_STATE
    assert lib.fqlpop_emtrain_get_bootstrap(tr._h, 0, ptr, n, None, 0, ctypes.byref(no)) == E_STATE
    assert b"bootstrap" in lib.fqlpop_last_error()
    tr.set_bootstrap(True)
    tr.steps(1)
    tables, state = _raw_tables(lib, tr, 3), [_state(tr, k) for k in range(3)]
    good = np.concatenate([R.bootstrap_table(s + 1, n) for s in seeds])
    low, high = good.copy(), good.copy()
    low[n + 1], high[-1] = -1, n
    refused = {
        "enable": lambda: lib.fqlpop_emtrain_set_bootstrap(tr._h, 2),
        "n too small": lambda: lib.fqlpop_emtrain_set_bootstrap_table(tr._h, good.ctypes.data_as(I64P), 3 * n - 1),
        "n of one model": lambda: lib.fqlpop_emtrain_set_bootstrap_table(tr._h, good.ctypes.data_as(I64P), n),
        "entry -1": lambda: lib.fqlpop_emtrain_set_bootstrap_table(tr._h, low.ctypes.data_as(I64P), 3 * n),
        "entry n_units": lambda: lib.fqlpop_emtrain_set_bootstrap_table(tr._h, high.ctypes.data_as(I64P), 3 * n),
        "n_batches": lambda: lib.fqlpop_emtrain_eval_oob(tr._h, 0, 0, _lib.fptr(logs)),
        "model": lambda: lib.fqlpop_emtrain_get_bootstrap(tr._h, 3, ptr, n, None, 0, ctypes.byref(no)),
        "n_units": lambda: lib.fqlpop_emtrain_get_bootstrap(tr._h, 0, ptr, n + 1, None, 0, ctypes.byref(no)),
        "oob_cap": lambda: lib.fqlpop_emtrain_get_bootstrap(tr._h, 0, ptr, n, ptr, 0, ctypes.byref(no)),
    }
    for name, call in refused.items():
        assert call() == E_ARG, name
        assert _raw_tables(lib, tr, 3) == tables, name
        for k in range(3):
            _assert_states_equal(_state(tr, k), state[k], name)
    assert tr.count == 1
    # a model whose table holds every unit has nothing out of bag: eval_oob names it
    full = np.stack([R.bootstrap_table(seeds[0], n), np.arange(n), R.bootstrap_table(seeds[2], n)])
    tr.set_bootstrap(table=full)
    tables = _raw_tables(lib, tr, 3)
    assert lib.fqlpop_emtrain_eval_oob(tr._h, 1, 0, _lib.fptr(logs)) == E_STATE
    assert b"model 1" in lib.fqlpop_last_error()
    assert _raw_tables(lib, tr, 3) == tables and tr.count == 1
    for k in range(3):
        _assert_states_equal(_state(tr, k), state[k], "empty out-of-bag list")
    # a new dataset drops the tables: bootstrap is off until it is set again
    tr._set_dataset(_dataset(kind))
    assert lib.fqlpop_emtrain_get_bootstrap(tr._h, 0, ptr, n, None, 0, ctypes.byref(no)) == E_STATE
    plain = _make(kind, seeds, bootstrap=True)  # the same history, its tables dropped by hand
    plain.steps(1)
    plain.set_bootstrap(False)
    plain.steps(1)
    tr.steps(1)
    for k in range(3):
        _assert_states_equal(_state(tr, k), _state(plain, k), "after set_dataset")
    plain.close()
    tr.close()


# ---------------------------------------------------------------- 7. drivers
def _driver_data(tmp_path):
    rng = np.random.default_rng(9)
    n, D, A = C.N_ROWS, 28, 5
    obs = rng.standard_normal((n, D)).astype(np.float32)
    ds = {"observations": obs, "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
          "next_observations": (0.9 * obs + 0.1 * np.tanh(obs[:, ::-1])).astype(np.float32),
          "rewards": np.where(rng.uniform(size=n) < 0.25, 0.0, -1.0).astype(np.float32)}
    data = tmp_path / "data"
    data.mkdir()
    np.savez(data / "cube-single-play.npz", masks=(ds["rewards"] != 0).astype(np.float32), **ds)
    return [f"--data_directory={data}", "--steps=30", "--val_batches=2", "--batch_size=32",
            "--model.hidden_dims=(32, 32)"]


def _run_driver(tmp_path, tag, argv):
    import train_env_model as tem
    out = tem.main(argv + [f"--save_directory={tmp_path / tag}"])
    return {p.name: p.read_bytes() for p in sorted(out.iterdir()) if "baseline" in p.name}


def test_driver_bootstrap_files_and_elites(tmp_path):
    import train_env_model as tem
    import tune_alpha as ta
    from argparser import build_config_from_args
    common = _driver_data(tmp_path)
    ens = ["--model=baseline", "--ensemble_size=3", "--termination_weight=0"] + common
    files = {"batched": _run_driver(tmp_path, "batched", ens + ["--bootstrap"]),
             "sequential": _run_driver(tmp_path, "sequential", ens + ["--bootstrap", "--ensemble_sequential"]),
             "plain": _run_driver(tmp_path, "plain", ens),
             "plain2": _run_driver(tmp_path, "plain2", ens)}
    want = {f"baseline_ens{k}{s}" for k in range(3) for s in (".pt", "_config.yaml", "_log.csv")}
    assert set(files["batched"]) == set(files["sequential"]) == want | {"baseline_ens_oob.csv"}
    for name in sorted(files["batched"]):
        assert files["batched"][name] == files["sequential"][name], name
    assert b"oob/next_observation_loss" in files["batched"]["baseline_ens1_log.csv"]
    # without --bootstrap: the files of a run at the earlier flags, no out-of-bag output at all
    assert set(files["plain"]) == want and files["plain"] == files["plain2"]
    assert all(b"oob/" not in v for v in files["plain"].values())
    assert files["plain"]["baseline_ens0.pt"] != files["batched"]["baseline_ens0.pt"]
    rows = files["batched"]["baseline_ens_oob.csv"].decode().splitlines()
    assert rows[0] == "model,seed,n_units,n_oob,loss,next_observation_loss" and len(rows) == 4
    cells = [r.split(",") for r in rows[1:]]
    for k, c in enumerate(cells):
        want_oob = len(R.oob_list(R.bootstrap_table(k, C.N_ROWS), C.N_ROWS))  # member k: --seed (0) + k
        assert c[:4] == [str(k), str(k), str(C.N_ROWS), str(want_oob)], c
    # the single model bootstraps too
    one = _run_driver(tmp_path, "one", ["--model=baseline", "--termination_weight=0", "--bootstrap"] + common)
    assert set(one) == {"baseline.pt", "baseline_config.yaml", "baseline_log.csv", "baseline_ens_oob.csv"}
    assert one["baseline_ens_oob.csv"].decode().splitlines()[1].split(",")[:4] == cells[0][:4]
    # tune_alpha --env_model_elites 2: the two models the CSV ranks first, as if two had been trained
    tem.main(["--model=termination_predictor", f"--save_directory={tmp_path / 'batched'}"] + common)
    order = sorted(range(3), key=lambda k: (float(cells[k][5]), k))
    args = ta.build_parser().parse_args(["--task=simulated", "--env_model=baseline", "--env_model_ensemble=3",
                                         "--env_model_elites=2", f"--save_directory={tmp_path / 'batched'}"])
    config = build_config_from_args(args)
    task = ta.make_task(args, config)
    d = tmp_path / "batched" / config.env_name / "env_models"
    assert len(task.env_models) == 2
    for (sp, _), k in zip(task.env_models, order[:2]):
        saved = em.load_flax_msgpack(d / f"baseline_ens{k}.pt")
        assert np.array_equal(np.asarray(sp.get("params", sp)["Dense_0"]["kernel"]),
                              np.asarray(saved.get("params", saved)["Dense_0"]["kernel"])), k
