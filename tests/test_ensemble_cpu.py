"""World-model ensembles without a GPU: the three C ABI entry points are exported and
declared, the driver scripts parse the new flags and keep their defaults, the loader finds
the files of an ensemble, and the per-member score aggregation."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("fqlpop_set_env_model_ensemble", "fqlpop_rollout_ensemble", "fqlpop_rollout_ensemble_time")


def test_library_exports_and_declares_the_ensemble_entry_points():
    import fqlpop
    from fqlpop import _lib
    lib = fqlpop.load_library()
    for name in NEW_SYMBOLS:
        assert name in fqlpop.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == _lib._SIGS[name][1]
    assert len(_lib._SIGS["fqlpop_set_env_model_ensemble"][1]) == 7
    sig = _lib._SIGS["fqlpop_rollout_ensemble"][1]
    assert len(sig) == 10 and sig[4] is ctypes.c_uint64 and sig[6] is ctypes.c_int
    assert sig[7] is ctypes.POINTER(ctypes.c_int32)
    assert (_lib.ENS_PER_MODEL, _lib.ENS_MIXED, _lib.ENS_MAX_MODELS) == (0, 1, 16)


def test_ensemble_entry_points_reject_null_handles_without_gpu():
    import fqlpop
    lib = fqlpop.load_library()
    us = ctypes.c_double()
    assert lib.fqlpop_rollout_ensemble_time(None, ctypes.byref(us)) == -1
    assert lib.fqlpop_rollout_ensemble(None, None, 4, 3, 0, None, 0, None, None, None) == -1
    assert lib.fqlpop_set_env_model_ensemble(None, None, 2, None, 0, None, 0) == -1
    assert b"null" in lib.fqlpop_last_error()


def test_tune_alpha_parses_the_ensemble_flags():
    import tune_alpha
    p = tune_alpha.build_parser()
    d = p.parse_args([])
    assert d.env_model_ensemble == 0 and d.ensemble_score == "mean"  # the single model, as before
    a = p.parse_args(["--task", "simulated", "--env_model_ensemble", "5", "--ensemble_score", "min"])
    assert a.env_model_ensemble == 5 and a.ensemble_score == "min"
    assert p.parse_args(["--ensemble_score", "mixed"]).ensemble_score == "mixed"
    with pytest.raises(SystemExit):
        p.parse_args(["--ensemble_score", "median"])
    # the reference's flags still reach the trainer config unchanged
    from argparser import build_config_from_args, get_argparser
    assert build_config_from_args(d) == build_config_from_args(get_argparser().parse_args([]))


def test_train_env_model_parses_ensemble_size():
    import train_env_model as tem
    from argparser import build_env_model_config_from_args, get_env_model_argparser
    p = tem.build_parser()
    d = p.parse_args([])
    assert d.ensemble_size == 0
    cfg, name = tem.member_config(d, None)  # without the flag: the reference's config and file name
    assert name == "baseline"
    assert cfg == build_env_model_config_from_args(get_env_model_argparser().parse_args([]))
    a = p.parse_args(["--model", "multistep", "--seed", "40", "--ensemble_size", "3"])
    assert a.ensemble_size == 3
    got = [tem.member_config(a, k) for k in range(3)]
    assert [n for _, n in got] == ["multistep_ens0", "multistep_ens1", "multistep_ens2"]
    assert [c.seed for c, _ in got] == [40, 41, 42]
    assert all(c.model == "multistep" for c, _ in got)
    with pytest.raises(ValueError):
        tem.main(["--model", "initial_observation", "--ensemble_size", "2"])


def _touch(d, *names):
    for n in names:
        (d / n).write_bytes(b"")


def test_ensemble_file_discovery(tmp_path):
    from task.offline_task_simulated import ensemble_model_names
    k = 3
    _touch(tmp_path, *[f"multistep_ens{i}.pt" for i in range(k)], "termination_predictor.pt")
    # the shared termination predictor only
    assert ensemble_model_names(tmp_path, "multistep", k) == [
        (f"multistep_ens{i}", "termination_predictor") for i in range(k)]
    # two of three per-member termination predictors: still the shared one
    _touch(tmp_path, "termination_predictor_ens0.pt", "termination_predictor_ens1.pt")
    assert ensemble_model_names(tmp_path, "multistep", k)[2] == ("multistep_ens2", "termination_predictor")
    # all K
    _touch(tmp_path, "termination_predictor_ens2.pt")
    assert ensemble_model_names(tmp_path, "multistep", k) == [
        (f"multistep_ens{i}", f"termination_predictor_ens{i}") for i in range(k)]
    # a missing member is named
    with pytest.raises(FileNotFoundError, match=r"multistep_ens3\.pt"):
        ensemble_model_names(tmp_path, "multistep", 4)
    (tmp_path / "multistep_ens1.pt").unlink()
    with pytest.raises(FileNotFoundError, match=r"multistep_ens1\.pt"):
        ensemble_model_names(tmp_path, "multistep", k)
    with pytest.raises(FileNotFoundError, match=r"baseline_ens0\.pt"):
        ensemble_model_names(tmp_path, "baseline", 2)


def test_ensemble_files_load_into_the_task(tmp_path):
    import envmodel as em
    from envmodel.flax_msgpack import msgpack_serialize
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations, load_env_model_ensemble
    env = "cube-single-play-singletask-task2-v0"
    d = tmp_path / env / "env_models"
    d.mkdir(parents=True)
    spec = em.EnvModelSpec(28, 5, (16, 8), (8,))
    tp = em.init_termination_predictor(spec, 9)
    (d / "termination_predictor.pt").write_bytes(msgpack_serialize({"params": tp}))
    for k in range(2):
        (d / f"baseline_ens{k}.pt").write_bytes(msgpack_serialize({"params": em.init_state_predictor(spec, k)}))
    models = load_env_model_ensemble(tmp_path, env, "baseline", 2)
    assert len(models) == 2
    assert all(em.spec_from_trees(sp, t) == spec for sp, t in models)
    want = [em.flatten_state_predictor(spec, em.init_state_predictor(spec, k)) for k in range(2)]
    for (sp, _), w in zip(models, want):
        np.testing.assert_array_equal(em.flatten_state_predictor(spec, sp), w)
    assert not np.array_equal(want[0], want[1])
    ds = {"observations": np.zeros((2000, 28), np.float32), "actions": np.zeros((2000, 5), np.float32)}
    task = OfflineTaskWithSimulatedEvaluations(env, model="baseline", save_directory=tmp_path, dataset=ds,
                                               ensemble_size=2, ensemble_score="min")
    assert len(task.env_models) == 2 and task.spec == spec and task.ensemble_score == "min"
    np.testing.assert_array_equal(em.flatten_state_predictor(spec, task.sp_tree), want[0])  # reset / step: model 0
    with pytest.raises(FileNotFoundError, match=r"baseline_ens2\.pt"):
        OfflineTaskWithSimulatedEvaluations(env, model="baseline", save_directory=tmp_path, dataset=ds,
                                            ensemble_size=3)
    with pytest.raises(ValueError, match="ensemble_score"):
        OfflineTaskWithSimulatedEvaluations(env, dataset=ds, ensemble_score="median")


def test_ensemble_score_aggregation():
    from task.offline_task_simulated import ensemble_scores
    rates, lens = [0.5, 0.25, 0.75, 0.5], [10.0, 20.0, 5.0, 9.0]
    m = ensemble_scores(rates, lens, "mean")
    assert m == {"success": 0.5, "episode_length": 11.0, "success_std": pytest.approx(np.sqrt(0.03125)),
                 "success_min": 0.25, "success_max": 0.75}
    lo = ensemble_scores(rates, lens, "min")
    assert lo["success"] == 0.25 and lo["episode_length"] == 20.0  # the worst model's own episodes
    assert (lo["success_std"], lo["success_min"], lo["success_max"]) == (
        m["success_std"], m["success_min"], m["success_max"])
    mx = ensemble_scores(rates, lens, "mixed", mixed=(0.4, 12.0))
    assert mx["success"] == 0.4 and mx["episode_length"] == 12.0
    assert (mx["success_min"], mx["success_max"]) == (0.25, 0.75)
    for r in (m, lo, mx):
        assert all(type(v) is float for v in r.values())  # scalars only: the dict goes to the eval CSV
    # one model: exactly its own score, no spread
    one = ensemble_scores([np.float32(0.3)], [np.float32(17.5)], "mean")
    assert one == {"success": float(np.float32(0.3)), "episode_length": 17.5, "success_std": 0.0,
                   "success_min": float(np.float32(0.3)), "success_max": float(np.float32(0.3))}
    assert ensemble_scores([np.float32(0.3)], [np.float32(17.5)], "min")["success"] == float(np.float32(0.3))
    with pytest.raises(ValueError):
        ensemble_scores(rates, lens, "median")
    with pytest.raises(ValueError):
        ensemble_scores(rates, lens, "mixed")
