"""Host side of bootstrapped world-model ensembles (fqlpop_emtrain_set_bootstrap* / _get_bootstrap /
_eval_oob), no GPU: the symbols and their ctypes signatures, the refusals that come before any
GPU call, the drivers' flags, the elite selection from <model>_ens_oob.csv, and the NumPy
restatement of the device draws (tests/emtrain_draw_np.py) on its own: range, diversity, the
bootstrap's 63.2 % distinct share, the out-of-bag complement, and that no model the GPU tests
bootstrap has an empty out-of-bag list."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flow-q-learning_amd"))

import emtrain_boot_cases as C  # noqa: E402
import emtrain_draw_np as R  # noqa: E402
from fqlpop import _lib  # noqa: E402

E_ARG = -1  # FQLPOP_E_ARG
I64P = ctypes.POINTER(ctypes.c_int64)
NEW_SYMBOLS = {"fqlpop_emtrain_set_bootstrap": [ctypes.c_void_p, ctypes.c_int],
               "fqlpop_emtrain_set_bootstrap_table": [ctypes.c_void_p, I64P, ctypes.c_int64],
               "fqlpop_emtrain_get_bootstrap": [ctypes.c_void_p, ctypes.c_int, I64P, ctypes.c_int64, I64P,
                                                ctypes.c_int64, I64P],
               "fqlpop_emtrain_eval_oob": [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_float)]}


def test_symbols_exist_with_argtypes():
    lib = _lib.load_library()
    for name, args in NEW_SYMBOLS.items():
        assert name in _lib.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args, name
        assert fn.restype is ctypes.c_int


def test_header_names_the_salts_the_restatement_uses():
    text = open(os.path.join(ROOT, "include", "fqlpop.h")).read()
    assert f"#define FQLPOP_EM_SALT_BOOT 0x{R.SALT_BOOT:X}u" in text
    assert f"#define FQLPOP_EM_SALT_OOB 0x{R.SALT_OOB:X}u" in text
    assert len({R.SALT_ROW, R.SALT_EP, R.SALT_BOOT, R.SALT_OOB}) == 4


def test_null_arguments_are_refused_before_any_gpu_call():
    lib = _lib.load_library()
    one = (ctypes.c_int64 * 1)(0)
    n = ctypes.c_int64()
    out = (ctypes.c_float * 8)()
    assert lib.fqlpop_emtrain_set_bootstrap(None, 1) == E_ARG
    assert lib.fqlpop_emtrain_set_bootstrap_table(None, one, 1) == E_ARG
    assert lib.fqlpop_emtrain_get_bootstrap(None, 0, one, 1, None, 0, ctypes.byref(n)) == E_ARG
    assert lib.fqlpop_emtrain_eval_oob(None, 1, 0, out) == E_ARG
    assert lib.fqlpop_last_error()


# ------------------------------------------------------------------------ drivers
def test_driver_flags_parse():
    import evaluate_env_model as eem
    import train_env_model as tem
    import tune_alpha as ta
    p = tem.build_parser()
    assert p.parse_args([]).bootstrap is False
    a = p.parse_args(["--bootstrap", "--ensemble_size=3", "--ensemble_sequential"])
    assert a.bootstrap is True and a.ensemble_size == 3
    assert p.parse_args(["--bootstrap"]).ensemble_size == 0  # the single model bootstraps too
    with pytest.raises(ValueError, match="bootstrap"):
        tem.main(["--model=initial_observation", "--bootstrap"])
    for parser in (ta.build_parser(), eem.get_argparser()):
        assert parser.parse_args([]).env_model_elites == 0
        a = parser.parse_args(["--env_model_ensemble=5", "--env_model_elites=2"])
        assert (a.env_model_ensemble, a.env_model_elites) == (5, 2)


def _write_oob_csv(d, losses, model="baseline"):
    import train_env_model as tem
    tem.write_oob_csv(d / f"{model}_ens_oob.csv",
                      [{"model": k, "seed": 40 + k, "n_units": 203, "n_oob": 70 + k, "loss": 2 * v,
                        "next_observation_loss": v} for k, v in enumerate(losses)])


def test_elites_are_the_lowest_oob_losses_ties_to_the_lower_index(tmp_path):
    from task.offline_task_simulated import select_elites
    _write_oob_csv(tmp_path, [0.5, 0.25, 0.75, 0.25, 0.125])
    assert select_elites(tmp_path, "baseline", 5, 1) == [4]
    assert select_elites(tmp_path, "baseline", 5, 2) == [4, 1]      # models 1 and 3 tie: the lower index
    assert select_elites(tmp_path, "baseline", 5, 3) == [4, 1, 3]
    assert select_elites(tmp_path, "baseline", 5, 5) == [4, 1, 3, 0, 2]
    header = (tmp_path / "baseline_ens_oob.csv").read_text().splitlines()[0]
    assert header.split(",")[:4] == ["model", "seed", "n_units", "n_oob"]


def test_elites_errors(tmp_path):
    from task.offline_task_simulated import select_elites
    _write_oob_csv(tmp_path, [0.5, 0.25, 0.75])
    for bad in (0, -1, 4):
        with pytest.raises(ValueError, match="env_model_elites"):
            select_elites(tmp_path, "baseline", 3, bad)
    with pytest.raises(FileNotFoundError, match="multistep_ens_oob.csv"):
        select_elites(tmp_path, "multistep", 3, 2)
    with pytest.raises(ValueError, match="models 0..4"):  # a CSV of another ensemble size
        select_elites(tmp_path, "baseline", 5, 2)


def test_tune_alpha_elites_errors_come_from_make_task(tmp_path):
    import tune_alpha as ta
    from argparser import build_config_from_args
    argv = ["--task=simulated", "--env_model=baseline", f"--save_directory={tmp_path}", "--env_model_ensemble=3"]
    for elites, exc in ((4, ValueError), (2, FileNotFoundError)):
        args = ta.build_parser().parse_args(argv + [f"--env_model_elites={elites}"])
        with pytest.raises(exc, match="env_model_elites" if exc is ValueError else "baseline_ens_oob.csv"):
            ta.make_task(args, build_config_from_args(args))


# -------------------------------------------------------------------- host memory
def test_table_handles_under_sanitizers(tmp_path):
    """csrc/emboot.h over a counting heap (tests/cpp/emboot_test.cpp), a stand-alone child
    process under AddressSanitizer and UBSan: allocate, replace, a dataset change, drop, destroy."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "emboot_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "cpp", "emboot_test.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failed checks, 0 live allocations" in run.stdout, run.stdout


# -------------------------------------------------------------------- restatement
def test_bootstrap_table_range_diversity_and_distinct_share():
    n = 10_000
    tables = [R.bootstrap_table(seed, n) for seed in range(5)]
    for seed, t in enumerate(tables):
        assert t.dtype == np.int64 and t.shape == (n,)
        assert t.min() >= 0 and t.max() < n
        # 1 - 1/e of the units occur; the share's standard deviation is 0.31 / sqrt(n) = 0.003
        share = len(np.unique(t)) / n
        assert abs(share - 0.632) <= 0.02, (seed, share)
    for i in range(5):
        for j in range(i + 1, 5):
            assert not np.array_equal(tables[i], tables[j]), (i, j)


def test_oob_list_is_the_ascending_complement():
    n = 1000
    t = R.bootstrap_table(3, n)
    oob = R.oob_list(t, n)
    assert np.all(np.diff(oob) > 0)
    assert set(oob.tolist()) == set(range(n)) - set(t.tolist())
    assert len(oob) + len(np.unique(t)) == n
    assert np.array_equal(R.oob_list(np.arange(n), n), np.zeros(0, np.int64))


def test_one_unit():
    t = R.bootstrap_table(9, 1)
    assert np.array_equal(t, [0])
    assert len(R.oob_list(t, 1)) == 0


def test_draws_index_through_the_table():
    B, n = 32, 203
    rows = R.train_rows(5, 2, B, n)
    assert rows.shape == (B,) and rows.min() >= 0 and rows.max() < n
    assert not np.array_equal(rows, R.train_rows(5, 3, B, n)) and not np.array_equal(rows, R.train_rows(6, 2, B, n))
    table = R.bootstrap_table(5, n)
    assert np.array_equal(R.train_rows(5, 2, B, n, table), table[rows])
    assert np.array_equal(R.train_rows(5, 2, B, n, np.arange(n)), rows)
    base = R.train_windows(5, 2, B, 140, 20, 8)
    assert np.all(base % 20 < 12) and np.all(base // 20 < 7)
    rev = np.arange(7)[::-1]
    assert np.array_equal(R.train_windows(5, 2, B, 140, 20, 8, rev), (6 - base // 20) * 20 + base % 20)
    oob = R.oob_list(table, n)
    u = R.oob_units(5, 1, 77, B, oob)
    assert set(u.tolist()) <= set(oob.tolist())
    assert not np.array_equal(u, R.oob_units(5, 2, 77, B, oob)) and not np.array_equal(u, R.oob_units(5, 1, 78, B, oob))
    assert np.array_equal(R.oob_units(5, 1, 77 + (1 << 32), B, oob), u)  # the low word of draw


@pytest.mark.parametrize("kind,seed", C.all_cases())
def test_no_gpu_case_has_an_empty_out_of_bag_list(kind, seed):
    n = C.n_units(kind)
    assert len(R.oob_list(R.bootstrap_table(seed, n), n)) >= 1, (kind, seed)
