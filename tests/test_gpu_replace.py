"""The env-model trainer handles on the GPU (csrc/hostmem.h's owners behind fqlpop_emtrain_*
and fqlpop_initobs_*).  Lifecycle: create -> set_dataset -> one step -> read -> close, three
times over in one process, for an ensemble trainer with K = 2 (with a frozen termination
predictor) and for the initial-observation VAE (whose sample staging also grows once); the
third round's outputs equal the first's.  Replacement: a handle whose dataset (and frozen
predictor) A was in use and then replaced by B, with refused setter calls in between, trains
bit for bit like a fresh handle that only ever saw B.

The population handle is not on the owners and has no test here.

No test here makes a device allocation fail: the failure paths run on the host, over a
counting heap (tests/test_hostmem_cpu.py)."""
import ctypes

import numpy as np
import pytest

import envmodel as em
from envmodel import initial_observation as io
from envmodel.trainer import EnvModelTrainerConfig, StatePredictorEnsembleTrainer

pytestmark = pytest.mark.gpu
D, A = 5, 2
SPEC = em.EnvModelSpec(D, A, (16,), (16,))


def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((n, D)).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
            "rewards": -np.ones(n, np.float32), "masks": np.ones(n, np.float32),
            "next_observations": (0.9 * obs).astype(np.float32)}


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"output {i}")


class _Loader:
    def __init__(self, ds):
        self.dataset = ds


def _ensemble(data_seed, rows, tp_seed):
    """A K = 2 state-predictor trainer with a frozen termination predictor (termination_weight 1)."""
    trees = [em.init_state_predictor(SPEC, 40 + k) for k in range(2)]
    cfg = EnvModelTrainerConfig(steps=50, termination_weight=1.0, batch_size=16, seed=0, init_learning_rate=1e-3)
    return StatePredictorEnsembleTrainer(SPEC, trees, _Loader(_dataset(rows, data_seed)), None, cfg, (5, 6),
                                         tp_params=em.init_termination_predictor(SPEC, tp_seed))


def _ensemble_state(tr):
    return [tr.read_logs_raw()] + [tr.flat(k, w) for k in range(2) for w in range(3)]


def _emtrain_round():
    tr = _ensemble(7, 200, 2)
    tr.steps(1)
    out = _ensemble_state(tr)
    tr.close()
    return out


def _initobs_round():
    spec = io.InitialObservationSpec(D, 3, (16,))
    cfg = EnvModelTrainerConfig(steps=50, batch_size=16, init_learning_rate=1e-3, reconstruction_weight=10.0, seed=3)
    tr = io.InitialObservationTrainer(spec, io.init_initial_observation(spec, 1), _Loader(_dataset(50, 8)), None, cfg)
    tr.steps(1)
    logs = tr.read_logs()
    out = [np.array([logs[k] for k in sorted(logs)])] + [tr.flat(w) for w in range(3)]
    out += [tr.sample(17, seed=2), tr.sample(40, seed=2)]  # the staging pair, then grown
    tr.close()
    return out


@pytest.mark.parametrize("one_round", [_emtrain_round, _initobs_round], ids=["emtrain_ensemble", "initobs"])
def test_lifecycle_three_times(one_round):
    rounds = [one_round() for _ in range(3)]
    _assert_same(rounds[2], rounds[0])
    # (entry 0 is a log vector: the env-model trainer's logs are NaN where a class has no rows)
    assert all(np.isfinite(a).all() for a in rounds[0][1:])
    assert any(np.abs(a).max() > 0 for a in rounds[0])


def _refused(lib, rc, text):
    assert rc == -1 and text.encode() in lib.fqlpop_last_error(), (rc, lib.fqlpop_last_error())


def test_emtrain_replacement_is_complete_and_refusals_change_nothing():
    fresh = _ensemble(9, 157, 3)
    fresh.steps(2)
    want = _ensemble_state(fresh)
    fresh.close()
    tr = _ensemble(7, 200, 2)
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((16, D)).astype(np.float32)
    batch = {"observations": obs, "actions": rng.uniform(-1, 1, (16, A)).astype(np.float32),
             "rewards": -np.ones(16, np.float32), "next_observations": (0.9 * obs).astype(np.float32)}
    tr.eval_step(None, batch)  # predictor A is in use; an evaluation moves no state
    tflat = em.flatten_termination_predictor(SPEC, em.init_termination_predictor(SPEC, 3)).astype(np.float32)
    lib, f = tr._lib, tr._fptr
    _refused(lib, lib.fqlpop_emtrain_set_frozen_termination(tr._h, f(tflat), tflat.size - 1), "size mismatch")
    _refused(lib, lib.fqlpop_emtrain_set_dataset(tr._h, f(obs), f(obs), f(obs), f(obs), 0), "n_rows must be > 0")
    tr._check(lib.fqlpop_emtrain_set_frozen_termination(tr._h, f(tflat), tflat.size))
    tr._set_dataset(_dataset(157, 9))
    tr.steps(2)
    got = _ensemble_state(tr)
    tr.close()
    _assert_same(got, want)
    assert np.abs(got[2]).max() > 0  # Adam's first moment: the steps ran


def test_initobs_replacement_is_complete_and_refusals_change_nothing():
    spec = io.InitialObservationSpec(D, 3, (16,))
    cfg = EnvModelTrainerConfig(steps=50, batch_size=16, init_learning_rate=1e-3, reconstruction_weight=10.0, seed=3)

    def trainer(rows, seed):
        return io.InitialObservationTrainer(spec, io.init_initial_observation(spec, 1), _Loader(_dataset(rows, seed)),
                                            None, cfg)

    def state(tr):
        logs = tr.read_logs()
        return [np.array([logs[k] for k in sorted(logs)])] + [tr.flat(w) for w in range(3)] + [tr.sample(17, seed=2)]

    fresh = trainer(61, 9)
    fresh.steps(2)
    want = state(fresh)
    fresh.close()
    tr = trainer(50, 8)
    tr.sample(40, seed=1)  # dataset A's handle has a staging pair already
    b = _dataset(61, 9)["observations"]
    _refused(tr._lib, tr._lib.fqlpop_initobs_set_dataset(tr._h, tr._fptr(b), 0), "n_rows must be > 0")
    assert tr._lib.fqlpop_initobs_sample(tr._h, 0, ctypes.c_uint64(0), None, tr._fptr(b)) == -1
    tr._check(tr._lib.fqlpop_initobs_set_dataset(tr._h, tr._fptr(b), len(b)))
    tr.steps(2)
    got = state(tr)
    tr.close()
    _assert_same(got, want)
