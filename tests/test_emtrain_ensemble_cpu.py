"""Host side of world-model ensemble training (fqlpop_emtrain_*_ensemble), no GPU: the
symbols and their ctypes signatures, the block placement map, argument refusals that come
before any GPU call, the loaders' optional rng, and the driver's flags."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flow-q-learning_amd"))

from fqlpop import _lib  # noqa: E402

E_ARG = -1  # FQLPOP_E_ARG
NEW_SYMBOLS = ("fqlpop_emtrain_create_ensemble", "fqlpop_emtrain_num_models",
               "fqlpop_emtrain_step_injected_ensemble", "fqlpop_emtrain_eval_ensemble",
               "fqlpop_emtrain_read_logs_ensemble", "fqlpop_emtrain_get_params_model",
               "fqlpop_emtrain_ensemble_block_map")


def test_symbols_exist_with_argtypes():
    lib = _lib.load_library()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGS[name][1]), name
        assert fn.restype is ctypes.c_int
    assert len(lib.fqlpop_emtrain_create_ensemble.argtypes) == 7
    assert len(lib.fqlpop_emtrain_ensemble_block_map.argtypes) == 7


def _map(K, bpm, mode, lin):
    g, m, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = _lib.load_library().fqlpop_emtrain_ensemble_block_map(K, bpm, mode, lin, ctypes.byref(g), ctypes.byref(m),
                                                               ctypes.byref(b))
    return rc, g.value, m.value, b.value


@pytest.mark.parametrize("mode", [0, 1])
def test_block_map_covers_every_block_once(mode):
    for K in range(1, 17):
        for bpm in (1, 2, 3, 16, 64):
            rc, grid, _, _ = _map(K, bpm, mode, 0)
            assert rc == 0
            seen, per_xcd, pads = set(), {}, 0
            for lin in range(grid):
                rc, g, m, b = _map(K, bpm, mode, lin)
                assert rc == 0 and g == grid
                if m < 0:
                    assert m == -1
                    pads += 1
                    continue
                assert 0 <= m < K and 0 <= b < bpm
                assert (m, b) not in seen, (K, bpm, mode, lin)
                seen.add((m, b))
                per_xcd.setdefault(lin % 8, set()).add(m)
            assert seen == {(m, b) for m in range(K) for b in range(bpm)}, (K, bpm, mode)
            assert grid == K * bpm + pads
            if mode == 0:
                assert pads == 0 and grid == K * bpm
                assert [_map(K, bpm, 0, lin)[2:] for lin in range(grid)] == \
                    [(m, b) for m in range(K) for b in range(bpm)]  # model-major
            else:
                cap = math.ceil(K / 8)
                assert all(len(s) <= cap for s in per_xcd.values()), (K, bpm, per_xcd)
            # past the grid: refused
            assert _map(K, bpm, mode, grid)[0] == E_ARG


def test_block_map_refusals():
    assert _map(0, 16, 0, 0)[0] == E_ARG
    assert _map(17, 16, 0, 0)[0] == E_ARG
    assert _map(4, 0, 0, 0)[0] == E_ARG
    assert _map(4, 16, 2, 0)[0] == E_ARG
    assert _map(4, 16, 1, -1)[0] == E_ARG


def _cfg():
    c = _lib.EmTrainConfig()
    c.kind, c.obs_dim, c.action_dim, c.num_hidden = _lib.EM_STATE_PREDICTOR, 6, 2, 1
    c.hidden_dims[0] = 16
    c.batch_size, c.steps, c.init_lr = 16, 10, 1e-3
    return c


def test_create_ensemble_refusals_come_before_any_gpu_call():
    """n_models 0 and 17, a null seeds and a params size mismatch: FQLPOP_E_ARG (on a machine
    without a GPU, so nothing touched one)."""
    lib = _lib.load_library()
    c = _cfg()
    n = ctypes.c_int64()
    assert lib.fqlpop_emtrain_param_count(ctypes.byref(c), ctypes.byref(n)) == 0
    P = n.value
    seeds = (ctypes.c_uint64 * 17)(*range(17))
    flat = np.zeros(17 * P, np.float32)
    h = ctypes.c_void_p()
    for K in (0, 17):
        assert lib.fqlpop_emtrain_create_ensemble(ctypes.byref(c), K, _lib.fptr(flat), K * P, seeds, 0,
                                                  ctypes.byref(h)) == E_ARG
        assert b"n_models" in lib.fqlpop_last_error()
        assert not h.value
    assert lib.fqlpop_emtrain_create_ensemble(ctypes.byref(c), 3, _lib.fptr(flat), 3 * P, None, 0,
                                              ctypes.byref(h)) == E_ARG
    assert b"seeds" in lib.fqlpop_last_error() and not h.value
    assert lib.fqlpop_emtrain_create_ensemble(ctypes.byref(c), 3, _lib.fptr(flat), 3 * P - 1, seeds, 0,
                                              ctypes.byref(h)) == E_ARG
    assert b"size mismatch" in lib.fqlpop_last_error() and not h.value
    assert lib.fqlpop_emtrain_create_ensemble(ctypes.byref(c), 3, _lib.fptr(flat), P, seeds, 0,
                                              ctypes.byref(h)) == E_ARG  # one model's count for three
    assert not h.value


def test_em_ens_xcd_is_an_engine_option():
    before = _lib.get_engine_option("em_ens_xcd")
    assert before in (0, 1)
    try:
        for v in (0, 1):
            _lib.set_engine_option("em_ens_xcd", v)
            assert _lib.get_engine_option("em_ens_xcd") == v
        with pytest.raises(_lib.FqlpopError):
            _lib.set_engine_option("em_ens_xcd", 2)
    finally:
        _lib.reset_engine_options()
    assert _lib.get_engine_option("em_ens_xcd") == before


def _rows(n, D=3, A=2):
    rows = np.arange(n, dtype=np.float32)
    return {"observations": np.repeat(rows[:, None], D, 1), "actions": np.zeros((n, A), np.float32),
            "rewards": rows.copy(), "next_observations": np.repeat(rows[:, None] + 1, D, 1)}


@pytest.mark.parametrize("kind", ["step", "multistep", "initial_observation"])
def test_loaders_take_an_rng(kind):
    """rng = RandomState(s), at construction or per call, draws what the global stream draws
    after np.random.seed(s); the default is still the global stream."""
    import train_env_model as tem
    ds = _rows(3000)
    make = {"step": lambda **kw: tem.StepLoader(ds, **kw),
            "multistep": lambda **kw: tem.MultistepLoader(ds, 16, **kw),
            "initial_observation": lambda **kw: tem.InitialObservationLoader(ds, **kw)}[kind]
    for s in (0, 7):
        np.random.seed(s)
        ld = make()
        want = [ld.sample(8), ld.sample(8)]
        ld = make(rng=np.random.RandomState(s))
        got_ctor = [ld.sample(8), ld.sample(8)]
        rng = np.random.RandomState(s)
        ld = make()
        np.random.seed(12345)  # the global stream is not what a call with rng draws from
        got_call = [ld.sample(8, rng=rng), ld.sample(8, rng=rng)]
        for got in (got_ctor, got_call):
            for g, w in zip(got, want):
                assert g.keys() == w.keys()
                for k in w:
                    np.testing.assert_array_equal(g[k], w[k])


def test_driver_flags():
    import train_env_model as tem
    p = tem.build_parser()
    assert p.parse_args([]).ensemble_sequential is False
    a = p.parse_args(["--ensemble_size=3", "--ensemble_sequential"])
    assert a.ensemble_sequential is True and a.ensemble_size == 3
    assert set(tem.BATCHED_KINDS) <= {"baseline", "multistep", "termination_predictor"}
    for extra in ([], ["--ensemble_sequential"]):
        with pytest.raises(ValueError, match="ensemble_size"):
            tem.main(["--model=initial_observation", "--ensemble_size=2"] + extra)
