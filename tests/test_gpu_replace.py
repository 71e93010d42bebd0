"""The handles of the C ABI on the GPU, all of them on csrc/hostmem.h's owners: the env-model
trainer handles (fqlpop_emtrain_*, fqlpop_initobs_*) and the population handle (fqlpop_*, whose
setters replace the structs of csrc/popmem.h).

Lifecycle: create -> set up -> use -> read -> close, three times over in one process; the third
round's outputs equal the first's.  For an ensemble trainer with K = 2 (with a frozen
termination predictor), for the initial-observation VAE (whose sample staging also grows once)
and for the population at the set-up of tests/test_gpu_synth.py with a dataset, an env model,
a K = 2 ensemble and rings: one collect from start rows, two train steps, one recorded
rollout; with and without the step's graph.

Replacement: a handle whose dataset and model A were in use and then replaced by B, with
refused setter calls in between, goes on bit for bit like a handle that only ever saw B.  A
refused fqlpop_set_env_model leaves the model that is set intact: the same rollout as before.

No test here makes a device allocation fail: the failure paths run on the host, over a
counting heap (tests/test_hostmem_cpu.py, tests/test_popmem_cpu.py)."""
import ctypes

import numpy as np
import pytest

import envmodel as em
from envmodel import initial_observation as io
from envmodel.trainer import EnvModelTrainerConfig, StatePredictorEnsembleTrainer
import test_gpu_synth as SY
from _helpers import synthetic_rows
from test_gpu_ensemble import SPEC as POP_SPEC, _env_model, _set_ensemble, _set_single

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


# ------------------------------------------------------------------ the population handle
def _pop_models(seeds):
    return [_env_model(POP_SPEC, tp_bias=-12.0, tp_scale=1.0, seed=s) for s in seeds]


def _pop_outputs(pop):
    """One recorded rollout from ROWS1, then every member's state, train info and ring."""
    out = list(pop.rollout(SY._data()["observations"][SY.ROWS1], SY.T, seed=SY.SEED1, record=True, return_obs=True))
    for m in range(pop.n):
        out += SY._state(pop, m) + [SY._info_row(pop, m)]
        ring, info = pop.synth_read(m), pop.synth_info(m)
        out += [np.array([info[k] for k in sorted(info)])] + [ring[k] for k in sorted(ring)]
    return out


def _population_round(use_graph):
    pop = SY._pop(2, use_graph=use_graph)  # create, set_dataset, set_env_model
    _set_ensemble(pop, _pop_models((11, 12)))
    pop.synth_create(1000)
    pop.collect(SY.E, SY.T, SY.SEED1, start_rows=SY.ROWS1)
    pop.step(2)
    out = _pop_outputs(pop)
    pop.close()
    return out


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_population_lifecycle_three_times(use_graph):
    rounds = [_population_round(use_graph) for _ in range(3)]
    _assert_same(rounds[2], rounds[0])
    assert all(np.isfinite(a).all() for a in rounds[0])
    assert rounds[0][1].min() >= 1 and np.abs(rounds[0][2]).max() > 0  # the rollout ran: lengths, final observations
    per_member = (len(rounds[0]) - 5) // 2  # (after the rollout's five: params, m, v, count, info, ring info, ring)
    for m in range(2):
        state = rounds[0][5 + m * per_member:]
        assert np.abs(state[1]).max() > 0 and np.abs(state[2]).max() > 0  # Adam m, v: the steps ran
        assert state[3] == 2                                             # the step count
        assert state[5].min() > 0 and len(state[6]) > 0                  # the collect filled the ring


def _pop_refused(pop, rc, text):
    assert rc == -1 and text.encode() in pop.lib.fqlpop_last_error(), (rc, pop.lib.fqlpop_last_error())


def _rollout_a(pop):
    return pop.rollout(SY._data()["observations"][SY.ROWS1], SY.T, seed=SY.SEED1, record=True, return_obs=True)


def _refused_set_env_model(pop):
    """fqlpop_set_env_model with one state-predictor parameter too few (another model's values)."""
    from fqlpop._lib import fptr
    sp, tp = _pop_models((13,))[0]
    sp, tp = em.flatten_state_predictor(POP_SPEC, sp), em.flatten_termination_predictor(POP_SPEC, tp)
    rc = pop.lib.fqlpop_set_env_model(pop._h, ctypes.byref(pop._em_cfg), fptr(sp), sp.size - 1, fptr(tp), tp.size)
    _pop_refused(pop, rc, "parameter count mismatch")


def test_population_refused_set_env_model_keeps_the_model():
    pop = SY._pop(2)
    pop.step(1)
    before = _rollout_a(pop)
    _refused_set_env_model(pop)
    after = _rollout_a(pop)
    pop.close()
    _assert_same(after, before)
    assert before[1].min() >= 1 and np.abs(before[2]).max() > 0 and np.abs(before[3]).max() > 0  # the rollout ran


def test_population_replacement_is_complete_and_refusals_change_nothing():
    from fqlpop._lib import STATE_ADAM_M, STATE_ADAM_V, STATE_PARAMS, fptr
    data_b, model_b, ens_b = synthetic_rows(1501, SY.D, SY.A, 6), _pop_models((12,))[0], _pop_models((13, 12))
    obs0 = data_b["observations"][:SY.E]

    def use_b(pop):
        outs = list(pop.rollout(obs0, SY.T, seed=3, record=True, return_obs=True))
        outs += list(pop.rollout_ensemble(obs0, SY.T, seed=4, mode="mixed", return_obs=True))
        pop.step(2)
        for m in range(2):
            outs += SY._state(pop, m) + [SY._info_row(pop, m)]
        return outs

    pop = SY._pop(2)  # dataset A, model A
    _set_ensemble(pop, _pop_models((11, 12)))
    pop.step(1)
    _rollout_a(pop)
    pop.rollout_ensemble(obs0, SY.T, seed=4, mode="mixed")  # A's model and ensemble are in use
    first = [SY._state(pop, m) for m in range(2)]

    a = SY._data()
    keys = ("observations", "actions", "rewards", "masks", "next_observations")
    rc = pop.lib.fqlpop_set_dataset(pop._h, 0, *[a[k].ctypes.data_as(ctypes.c_void_p) for k in keys], 0, 0)
    _pop_refused(pop, rc, "n_rows out of range")
    _refused_set_env_model(pop)
    sp = np.stack([em.flatten_state_predictor(POP_SPEC, m[0]) for m in ens_b])
    tp = np.stack([em.flatten_termination_predictor(POP_SPEC, m[1]) for m in ens_b])
    rc = pop.lib.fqlpop_set_env_model_ensemble(pop._h, ctypes.byref(pop._em_cfg), 0, fptr(sp), sp.shape[1], fptr(tp),
                                               tp.shape[1])
    _pop_refused(pop, rc, "n_models must be in 1..16")
    pop.set_dataset(data_b)
    _set_single(pop, model_b)
    _set_ensemble(pop, ens_b)
    got = use_b(pop)
    pop.close()

    twin = SY._pop(2, env_model=False, data=data_b)  # only ever B, at the state after the same first step
    _set_single(twin, model_b)
    _set_ensemble(twin, ens_b)
    for m in range(2):
        for which, flat in zip((STATE_PARAMS, STATE_ADAM_M, STATE_ADAM_V), first[m]):
            twin.set_flat(m, flat, which)
        twin.set_count(m, int(first[m][3]))
    want = use_b(twin)
    twin.close()
    _assert_same(got, want)
    assert np.abs(first[0][1]).max() > 0 and np.abs(got[-4]).max() > 0  # Adam's first moment: the steps ran
