"""CPU tests of the host writes into a synthetic-transition ring (fqlpop_synth_write,
fqlpop_synth_append) and the ring checkpoint: the two symbols, their refusal of a null handle
without a GPU, the ValueErrors ``Population.load_synth_state`` raises before the C call, the
ring model (tests/synth_np.HostRing) under append sequences against the invariant a write must
preserve, and csrc/popmem.h's row stage under AddressSanitizer and UBSan
(tests/cpp/rowstage_test.cpp, a stand-alone child process)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import synth_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, A = 3, 2
NEW = ("fqlpop_synth_write", "fqlpop_synth_append")


def _rows(n, seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return {"observations": rng.standard_normal((n, D)).astype(dtype), "actions": rng.uniform(-1, 1, (n, A)).astype(dtype),
            "rewards": -np.ones(n, dtype), "masks": np.ones(n, dtype),
            "next_observations": rng.standard_normal((n, D)).astype(dtype)}


def test_symbols_declared_exported_and_bound():
    import fqlpop
    from fqlpop import _lib
    header = open(os.path.join(ROOT, "include", "fqlpop.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = fqlpop.load_library()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} is not declared"
        assert name in fqlpop.EXPORTED_SYMBOLS and hasattr(lib, name)
        # documented in its neighbours' style: a comment right above, marked as the engine's own
        doc = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "[no reference counterpart]" in doc, name
    F, I64 = _lib._F, ctypes.c_int64
    assert _lib._SIGS["fqlpop_synth_write"] == (ctypes.c_int, [_lib._P, ctypes.c_int, F, F, F, F, F, I64, I64])
    assert _lib._SIGS["fqlpop_synth_append"] == (ctypes.c_int, [_lib._P, ctypes.c_int, F, F, F, F, F, I64])


def test_null_handle_is_an_argument_error_without_gpu():
    import fqlpop
    from fqlpop._lib import fptr
    lib = fqlpop.load_library()
    r = _rows(2)
    arrays = [fptr(r[k]) for k in S.FIELDS]
    assert lib.fqlpop_synth_write(None, 0, *arrays, 2, 2) == -1
    assert b"null handle" in lib.fqlpop_last_error()
    assert lib.fqlpop_synth_append(None, 0, *arrays, 2) == -1
    assert b"null handle" in lib.fqlpop_last_error()
    assert lib.fqlpop_synth_write(None, 0, None, None, None, None, None, 0, 0) == -1
    assert lib.fqlpop_synth_append(None, 0, None, None, None, None, None, 0) == -1


class _NoCalls:
    """Stands where the library would: any C call is the test's failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the ValueError must come first")


def _handleless(capacity=10):
    from fqlpop import Population, PopulationConfig
    pop = object.__new__(Population)
    pop.cfg = PopulationConfig(obs_dim=D, action_dim=A)
    pop.lib, pop._h, pop.synth_capacity = _NoCalls(), None, capacity
    return pop


def _state(n, appended=None, capacity=10, **kw):
    return dict(_rows(n, **kw), appended=n if appended is None else appended, capacity=capacity)


def test_load_synth_state_value_errors_come_before_the_c_call():
    pop = _handleless(10)
    with pytest.raises(ValueError, match=r"capacity 12\b.*capacity 10\b"):   # names both capacities
        pop.load_synth_state(0, _state(4, capacity=12))
    bad = _state(4)
    bad["actions"] = bad["actions"].astype(np.float64)
    with pytest.raises(ValueError, match="actions must be float32"):
        pop.load_synth_state(0, bad)
    bad = _state(4)
    bad["observations"] = bad["observations"][:, :2]
    with pytest.raises(ValueError, match=r"observations must have shape \(4, 3\)"):
        pop.load_synth_state(0, bad)
    bad = _state(4)
    bad["rewards"] = bad["rewards"][:3]                                      # fields of unequal lengths
    with pytest.raises(ValueError, match=r"rewards must have shape \(4,\)"):
        pop.load_synth_state(0, bad)
    bad = _state(4)
    bad["masks"] = bad["masks"].reshape(4, 1)
    with pytest.raises(ValueError, match="masks must have shape"):
        pop.load_synth_state(0, bad)
    bad = _state(4)
    del bad["next_observations"]
    with pytest.raises(ValueError, match="need the fields"):
        pop.load_synth_state(0, bad)
    for key in ("appended", "capacity"):
        bad = _state(4)
        del bad[key]
        with pytest.raises(ValueError, match="appended.*capacity"):
            pop.load_synth_state(0, bad)
    with pytest.raises(ValueError, match="a ring state"):
        pop.load_synth_state(0, None)
    # rows = min(capacity, appended): 4 rows cannot have 25 appended, nor 10 rows 4
    with pytest.raises(ValueError, match=r"holds 4 rows.*appended = 25.*means 10"):
        pop.load_synth_state(0, _state(4, appended=25))
    with pytest.raises(ValueError, match=r"holds 10 rows.*appended = 4.*means 4"):
        pop.load_synth_state(0, _state(10, appended=4))
    with pytest.raises(ValueError, match="no rings"):
        _handleless(None).load_synth_state(0, _state(4))
    # synth_write / synth_append check the rows the same way
    with pytest.raises(ValueError, match="float32"):
        pop.synth_append(0, _rows(2, dtype=np.float64))
    with pytest.raises(ValueError, match="must have shape"):
        pop.synth_write(0, dict(_rows(2), rewards=np.zeros((2, 2), np.float32)))


def test_valid_state_reaches_the_c_call_with_its_counters():
    """The one path that does call: what load_synth_state hands to fqlpop_synth_write."""
    pop = _handleless(10)
    calls = []

    class Lib:
        @staticmethod
        def fqlpop_synth_write(h, member, obs, act, rew, mask, nobs, n, appended):
            calls.append((member, n, appended, np.ctypeslib.as_array(obs, (n, D)).copy()))
            return 0
    pop.lib = Lib()
    st = _state(10, appended=37, seed=3)
    pop.load_synth_state(1, st)
    st5 = _state(5, seed=4)
    pop.load_synth_state(0, {k: (v[::1] if isinstance(v, np.ndarray) else v) for k, v in st5.items()})
    assert [(c[0], c[1], c[2]) for c in calls] == [(1, 10, 37), (0, 5, 5)]
    np.testing.assert_array_equal(calls[0][3], st["observations"])
    np.testing.assert_array_equal(calls[1][3], st5["observations"])


@pytest.mark.parametrize("capacity", [1, 7, 20])
def test_host_ring_appends_keep_the_counter_invariant(capacity):
    """Every ring the engine builds has rows = min(capacity, appended) and head = appended mod
    capacity -- what fqlpop_synth_write requires of its arguments -- and position p holds the
    latest row i with i mod capacity = p."""
    rng = np.random.default_rng(capacity)
    ring = S.HostRing(capacity, D, A)
    sizes = [0, 1, capacity, capacity - 1, 0, min(capacity, 3), capacity, 1, 1] + rng.integers(0, capacity + 1, 12).tolist()
    log = []
    for i, n in enumerate(sizes):
        piece = _rows(n, seed=100 + i)
        ring.append(piece)
        log.append(piece)
        total = sum(p["rewards"].shape[0] for p in log)
        assert ring.info() == {"rows": min(capacity, total), "head": total % capacity, "appended": total}
    flat = {k: np.concatenate([p[k] for p in log]) for k in S.FIELDS}
    total = flat["rewards"].shape[0]
    assert total > 2 * capacity                                  # wrapped more than once
    for p in range(capacity):
        i = max(j for j in range(total) if j % capacity == p)
        for k in S.FIELDS:
            np.testing.assert_array_equal(ring.data[k][p], flat[k][i])
    with pytest.raises(ValueError):
        ring.append(_rows(capacity + 1))                         # n > capacity is refused
    # a ring rebuilt from its valid rows and `appended` alone (what a checkpoint stores) is the
    # same ring: positions, counters and the next append
    twin = S.HostRing(capacity, D, A)
    valid = ring.valid()
    for k in S.FIELDS:
        twin.data[k][:ring.rows] = valid[k]
    twin.rows, twin.appended, twin.head = ring.rows, ring.appended, ring.appended % capacity
    more = _rows(min(capacity, 2), seed=999)
    ring.append(more)
    twin.append(more)
    assert twin.info() == ring.info()
    for k in S.FIELDS:
        np.testing.assert_array_equal(twin.valid()[k], ring.valid()[k])


@pytest.mark.parametrize("interval,warmup", [(4, 4), (4, 0), (4, 5), (4, 8), (1000, 2500), (1, 0), (3, 1), (5, 5)])
def test_collect_number_is_the_running_count_of_a_lock_step_run(interval, warmup):
    """A collect is seeded by the update it follows (trainer.collect_number), so that a
    candidate deferred to a later invocation gets its lock-step seeds; in a lock-step run that
    number is the count of the collects before it, which seeded the collects until now."""
    from trainer.config import ModelRolloutConfig
    from trainer.trainer import collect_number
    mr = ModelRolloutConfig(branches=1, horizon=1, interval=interval, warmup=warmup)
    steps = 12 * interval + 1
    done = 0
    for cur in range(1, steps):
        if cur % interval == 0 and cur >= warmup:        # Trainer._train_with_rollouts' condition
            assert collect_number(cur, mr) == done, (cur, done)
            done += 1
    assert done >= 10


def test_row_stage_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "rowstage_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "cpp", "rowstage_test.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failed checks, 0 live allocations" in run.stdout, run.stdout
    assert "0 double frees" in run.stdout, run.stdout
