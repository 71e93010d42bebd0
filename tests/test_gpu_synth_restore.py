"""Host writes into a synthetic-transition ring on the GPU (fqlpop_synth_write,
fqlpop_synth_append) and the ring checkpoint built on the first.  Every comparison is bitwise:
the feature moves bytes and restates the collect's order rule.

Set-up as tests/test_gpu_synth.py (whose helpers are used): H = 512 x 4, D = 28, A = 5, B = 64,
2 members, 20 branches of horizon 8 (at most 160 transitions a collect, about 130), rings of a
few hundred rows so that the second collect wraps."""
import functools
import pickle
import random

import numpy as np
import pytest

import synth_np as S
from _helpers import synthetic_rows
from test_gpu_ensemble import SPEC, _env_model
from test_gpu_synth import (A, D, E, ENV, ROWS1, ROWS2, SEED1, SEED2, T, _assert_ring, _assert_same, _data, _model,
                            _pop, _state)

pytestmark = pytest.mark.gpu
SEED3 = 23
EMPTY = {"rows": 0, "head": 0, "appended": 0}


def _ring_bytes(pop, m):
    """Counters and the bytes of the valid rows of one member's ring."""
    return pop.synth_info(m), {k: v.tobytes() for k, v in pop.synth_read(m).items()}


def _assert_rings_equal(pa, ma, pb, mb, tag):
    ia, ba = _ring_bytes(pa, ma)
    ib, bb = _ring_bytes(pb, mb)
    assert ia == ib, f"{tag}: counters {ia} != {ib}"
    for k in S.FIELDS:
        assert ba[k] == bb[k], f"{tag}: {k} of member {ma} / {mb}"


def _rows(n, seed):
    return synthetic_rows(n, D, A, seed)


def _host_from_state(state):
    host = S.HostRing(state["capacity"], D, A)
    n = state["rewards"].shape[0]
    for k in S.FIELDS:
        host.data[k][:n] = state[k]
    host.rows, host.appended, host.head = n, state["appended"], state["appended"] % state["capacity"]
    return host


class Ctx:
    pass


@pytest.fixture(scope="module")
def src():
    """A population whose rings (capacity 200) two collects have wrapped, and each member's
    ``synth_state`` (shared, read-only)."""
    c = Ctx()
    c.pop = _pop(2, capacity=200)
    c.pop.collect(E, T, SEED1, start_rows=ROWS1)
    c.pop.collect(E, T, SEED2, start_rows=ROWS2)
    c.states = [c.pop.synth_state(m) for m in range(2)]
    for st in c.states:
        assert st["capacity"] == 200 and st["appended"] > 200 and st["rewards"].shape[0] == 200
    yield c
    c.pop.close()


# ------------------------------------------------------------------ 1. write round trip
@pytest.mark.parametrize("case,use_graph", [("wrapped", True), ("wrapped", False), ("unwrapped", True),
                                            ("unwrapped", False), ("member1_only", True)])
def test_write_round_trip_continues_bitwise(case, use_graph):
    capacity = 1000 if case == "unwrapped" else 200
    p, q = _pop(2, capacity=capacity, use_graph=use_graph), _pop(2, capacity=capacity, use_graph=use_graph)
    for pop in (p, q):
        pop.step(1)          # at rho = 1 on empty rings: q's step graph exists before the write
    p.collect(E, T, SEED1, start_rows=ROWS1)
    p.collect(E, T, SEED2, start_rows=ROWS2)
    states = [p.synth_state(m) for m in range(2)]
    for st in states:
        n = st["rewards"].shape[0]
        print(f"{case}: {n} rows, appended {st['appended']}, capacity {st['capacity']}")
        assert (st["appended"] > capacity and n == capacity) if capacity == 200 else (n == st["appended"] < capacity)
    members = [1] if case == "member1_only" else [0, 1]
    if case == "member1_only":
        q.collect(E, T, SEED3)                       # member 0 keeps a ring of its own
        own0 = _ring_bytes(q, 0)
        assert own0[0] != p.synth_info(0)
    for m in members:
        q.load_synth_state(m, states[m])
    for m in members:
        _assert_rings_equal(p, m, q, m, f"{case}: after the write")
    if case == "member1_only":
        assert _ring_bytes(q, 0) == own0, "the write to member 1 touched member 0's ring"
    for pop in (p, q):
        pop.collect(E, T, SEED3 + 1)                 # device-drawn starts; wraps again at capacity 200
        pop.set_real_ratio(0.5)
    for step in range(3):
        p.step(1)
        q.step(1)
        for m in members:
            _assert_same(p, m, q, m, f"{case} graph {use_graph} step {step}")
    for m in members:
        _assert_rings_equal(p, m, q, m, f"{case}: after the third collect")
    p.close()
    q.close()


# ------------------------------------------------------------------ 2. append against the ring model
CAP2 = 350
X1, X2, X3 = _rows(1, 31), _rows(300, 32), _rows(CAP2, 33)


@functools.lru_cache(maxsize=None)
def _collect_pieces():
    """Per member the rows of the two collects, from a twin that only collects (a collect does
    not depend on the ring it appends to)."""
    twin = _pop(2, capacity=1000)
    twin.collect(E, T, SEED1, start_rows=ROWS1)
    first = [twin.synth_read(m) for m in range(2)]
    twin.collect(E, T, SEED2, start_rows=ROWS2)
    both = [twin.synth_read(m) for m in range(2)]
    twin.close()
    out = []
    for m in range(2):
        n1 = first[m]["rewards"].shape[0]
        assert both[m]["rewards"].shape[0] > n1 > 0
        out.append((first[m], {k: v[n1:] for k, v in both[m].items()}))
    return out


@functools.lru_cache(maxsize=None)
def _append_sequence(sync: bool):
    """collect, append X1, append X2 (wraps), collect | read | append X3, step: the appends go
    to member 1.  Without ``sync`` nothing synchronises between an append and the collect or
    the step enqueued behind it."""
    pop = _pop(2, capacity=CAP2)
    pop.set_real_ratio(0.5)

    def wait():
        if sync:
            pop.sync()
    pop.collect(E, T, SEED1, start_rows=ROWS1)
    wait()
    pop.synth_append(1, X1)
    wait()
    pop.synth_append(1, X2)
    wait()
    pop.collect(E, T, SEED2, start_rows=ROWS2)
    mid = [(pop.synth_info(m), pop.synth_read(m)) for m in range(2)]
    pop.synth_append(1, X3)
    wait()
    pop.step(1)
    end = [(pop.synth_info(m), pop.synth_read(m), _state(pop, m), pop.read_info_array("train")[m]) for m in range(2)]
    pop.close()
    return mid, end


def _assert_host(info, rows, host, tag):
    assert info == host.info(), f"{tag}: counters {info} != {host.info()}"
    want = host.valid()
    for k in S.FIELDS:
        np.testing.assert_array_equal(rows[k], want[k], err_msg=f"{tag}: {k}")


def test_appends_follow_the_ring_model():
    pieces = _collect_pieces()
    mid, end = _append_sequence(False)
    h0, h1 = S.HostRing(CAP2, D, A), S.HostRing(CAP2, D, A)
    h0.append(pieces[0][0])
    h0.append(pieces[0][1])
    for piece in (pieces[1][0], X1, X2, pieces[1][1]):
        h1.append(piece)
    assert h1.appended > CAP2 and h0.appended < CAP2     # member 1 wrapped (inside X2), member 0 did not
    _assert_host(mid[0][0], mid[0][1], h0, "member 0 (collects only)")
    _assert_host(mid[1][0], mid[1][1], h1, "member 1 after collect, X1, X2, collect")
    h1.append(X3)                                        # n = capacity: every position rewritten, from head on
    _assert_host(end[1][0], end[1][1], h1, "member 1 after X3")
    _assert_host(end[0][0], end[0][1], h0, "member 0 at the end")
    assert h1.head != 0                                  # X3 wrapped


def test_appends_are_stream_ordered():
    a, b = _append_sequence(False), _append_sequence(True)
    for m in range(2):
        assert a[0][m][0] == b[0][m][0] and a[1][m][0] == b[1][m][0]
        for k in S.FIELDS:
            np.testing.assert_array_equal(a[0][m][1][k], b[0][m][1][k], err_msg=f"mid {m} {k}")
            np.testing.assert_array_equal(a[1][m][1][k], b[1][m][1][k], err_msg=f"end {m} {k}")
        for x, y in zip(a[1][m][2], b[1][m][2]):
            np.testing.assert_array_equal(x, y, err_msg=f"member {m}: state after the step")
        np.testing.assert_array_equal(a[1][m][3], b[1][m][3], err_msg=f"member {m}: train info")


def test_append_into_an_empty_ring_and_an_inactive_member():
    pop = _pop(2, capacity=CAP2)
    pop.set_active([True, False])
    pop.synth_append(1, X2)                              # empty, and member 1 is inactive
    pop.collect(E, T, SEED1, start_rows=ROWS1)           # active members only: member 0
    pop.synth_append(1, X1)
    pop.synth_append(1, {k: v[:0] for k, v in X1.items()})   # n = 0: nothing
    host = S.HostRing(CAP2, D, A)
    host.append(X2)
    host.append(X1)
    _assert_ring(pop, 1, host, "inactive member 1")
    assert pop.synth_info(1) == {"rows": 301, "head": 301, "appended": 301}
    h0 = S.HostRing(CAP2, D, A)
    h0.append(_collect_pieces()[0][0])
    _assert_ring(pop, 0, h0, "member 0")
    pop.close()


# ------------------------------------------------------------------ 3. appended rows are what training reads
def test_appended_rows_train_as_a_dataset_of_them():
    """The rho = 0 identity of test_gpu_synth.py with the ring filled by synth_append alone."""
    a = _pop(2, capacity=1000)
    for m in range(2):
        a.synth_append(m, X2)
    a.set_real_ratio(0.0)
    twins = [_pop(1, env_model=False, param_seeds=[m], seeds=[m + 1], data=X2) for m in range(2)]
    for step in range(3):
        a.step(1)
        for m in range(2):
            twins[m].step(1)
            _assert_same(a, m, twins[m], 0, f"rho 0 on appended rows, step {step}")
    for pop in twins + [a]:
        pop.close()


# ------------------------------------------------------------------ 4. clone after write
def test_clone_copies_a_written_ring(src):
    pop = _pop(3, capacity=200)
    pop.collect(E, T, SEED3)
    pop.load_synth_state(0, src.states[1])
    pop.clone_members([0], [2], alphas=[float(pop.alphas[0])], seeds=[int(pop.seeds[0])])
    for m in (0, 2):
        _assert_rings_equal(pop, m, src.pop, 1, f"member {m}")
    assert pop.synth_info(1)["appended"] < 200           # member 1 keeps its one collect
    pop.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_change_nothing(src):
    import fqlpop
    from fqlpop import FqlpopError
    from fqlpop._lib import fptr
    pop, lib = _pop(2, capacity=200, env_model=False), fqlpop.load_library()
    for m in range(2):
        pop.load_synth_state(m, src.states[m])
    before = [_ring_bytes(pop, m) for m in range(2)]
    x = _rows(5, 41)
    arrays = [fptr(x[k]) for k in S.FIELDS]

    def unchanged(tag):
        for m in range(2):
            assert _ring_bytes(pop, m) == before[m], f"after {tag}"

    def refused(tag, code, fn, *a, **kw):
        with pytest.raises(FqlpopError, match=f"error {code}:"):
            fn(*a, **kw)
        unchanged(tag)

    def refused_c(tag, code, fn, *a):
        assert fn(*a) == code, tag
        unchanged(tag)
    refused_c("null handle, write", -1, lib.fqlpop_synth_write, None, 0, *arrays, 5, 5)
    refused_c("null handle, append", -1, lib.fqlpop_synth_append, None, 0, *arrays, 5)
    for member in (-1, 2):
        refused(f"write member {member}", -1, pop.synth_write, member, x)
        refused(f"append member {member}", -1, pop.synth_append, member, x)
    for i in range(5):                                   # a null array with n > 0
        holed = arrays[:i] + [None] + arrays[i + 1:]
        refused_c(f"write, null array {i}", -1, lib.fqlpop_synth_write, pop._h, 0, *holed, 5, 5)
        refused_c(f"append, null array {i}", -1, lib.fqlpop_synth_append, pop._h, 0, *holed, 5)
    refused_c("write n < 0", -1, lib.fqlpop_synth_write, pop._h, 0, *arrays, -1, 5)
    refused_c("append n < 0", -1, lib.fqlpop_synth_append, pop._h, 0, *arrays, -1)
    big = _rows(201, 42)
    refused("write n > capacity", -1, pop.synth_write, 0, big, 201)
    refused("write n > capacity, appended large", -1, pop.synth_write, 0, big, 1000)
    refused("append n > capacity", -1, pop.synth_append, 0, big)
    refused("write appended < n", -1, pop.synth_write, 0, x, 4)
    refused("write n < min(capacity, appended)", -1, pop.synth_write, 0, x, 7)
    refused("write n < capacity <= appended", -1, pop.synth_write, 0, x, 300)
    refused_c("write n = 0, appended > 0", -1, lib.fqlpop_synth_write, pop._h, 0, *([None] * 5), 0, 3)
    bare = _pop(1, env_model=False)                      # no rings
    for fn in (bare.synth_write, bare.synth_append):
        with pytest.raises(FqlpopError, match="error -3:"):
            fn(0, x)
    bare.close()
    # what is not refused: an empty append does nothing; n = 0, appended = 0 empties the ring
    assert lib.fqlpop_synth_append(pop._h, 0, *([None] * 5), 0) == 0
    unchanged("an empty append")
    assert lib.fqlpop_synth_write(pop._h, 1, *([None] * 5), 0, 0) == 0
    assert pop.synth_info(1) == EMPTY and _ring_bytes(pop, 0) == before[0]
    full = dict(_rows(200, 43), appended=200, capacity=200)  # n = capacity = appended: head back at 0
    pop.load_synth_state(1, full)
    assert pop.synth_info(1) == {"rows": 200, "head": 0, "appended": 200}
    _assert_host(pop.synth_info(1), pop.synth_read(1), _host_from_state(full), "a full, unwrapped ring")
    pop.close()


# ------------------------------------------------------------------ 6. chunked equals uninterrupted
def _ensemble_models():
    return [_env_model(SPEC, tp_bias=-12.0, tp_scale=1.0, seed=s) for s in (11, 12)]


def _trainer_parts(path, variant, branches, state=None):
    from hpo.identity import Identity
    from hpo.pbt import PopulationBasedTraining
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    from trainer.config import AgentConfig, ExperimentConfig, ModelRolloutConfig, TrainerConfig
    from trainer.trainer import Trainer
    cfg = TrainerConfig(steps=16, eval_interval=8, log_interval=2, save_directory=path, env_name=ENV, seed=3,
                        agent=AgentConfig(batch_size=64))
    kw = dict(env_models=_ensemble_models()) if variant == "ensemble" else dict(env_model=_model())
    task = OfflineTaskWithSimulatedEvaluations(ENV, dataset=_data(), num_evaluation_envs=4, max_episode_steps=6, **kw)
    mr_kw = dict(ensemble=True, penalty=1.0) if variant == "ensemble" else {}
    mr = ModelRolloutConfig(branches=branches, horizon=4, interval=4, warmup=4, real_ratio=0.5, buffer_rows=60, **mr_kw)
    pairs = [(3.0, 1), (30.0, 2), (300.0, 3), (1000.0, 4)][:4 if variant == "pbt" else 2]
    configs = [ExperimentConfig(seed=s, alpha=a) for a, s in pairs]
    strategy_state = state["strategy"] if state else None
    if variant == "pbt":
        strategy = PopulationBasedTraining(set(configs), total_evaluations=8, ready_interval=1, seed=0,
                                           state_dict=strategy_state)
    else:
        strategy = Identity(population=configs, total_evaluations=0, state_dict=strategy_state)
    trainer = Trainer(task, strategy, cfg, state_dict=state["trainer"] if state else None, model_rollouts=mr)
    return trainer, task


def _checkpoint(trainer):
    """What tune_alpha.py writes, through pickle."""
    return pickle.loads(pickle.dumps({"trainer": trainer.state_dict(), "strategy": trainer.strategy.state_dict()}))


def _train_in_chunks(path, variant, branches, chunks):
    """``Trainer.train`` once per entry of ``chunks`` (its max_evaluations), each time after
    the first in a new Trainer and Population restored from the pickled checkpoint."""
    random.seed(7)
    np.random.seed(7)
    state = None
    for i, evaluations in enumerate(chunks):
        trainer, task = _trainer_parts(path, variant, branches, state)
        trainer.train(max_evaluations=evaluations)
        if i + 1 < len(chunks):
            state = _checkpoint(trainer)
            trainer.population.close()
            task.close()
    pop, out = trainer.population, {}
    for cfg, exp in trainer.experiments.items():
        m = trainer.member_of[cfg]
        csvs = {g: (path / ENV / exp.experiment_name / f"{g}.csv").read_text() for g in ("train", "val", "eval")}
        ring = _ring_bytes(pop, m) if branches else None
        out[cfg] = (_state(pop, m), ring, csvs, exp.current_step)
    collect_index = trainer.collect_index
    pop.close()
    task.close()
    return out, collect_index


def _assert_runs_equal(one, other, tag):
    (a, ia), (b, ib) = one, other
    assert ia == ib, f"{tag}: collect_index {ia} != {ib}"
    assert set(a) == set(b), f"{tag}: candidates differ"
    for cfg in a:
        assert a[cfg][3] == b[cfg][3] == 16, f"{tag}: {cfg} steps"
        for x, y, what in zip(a[cfg][0], b[cfg][0], ("params and target", "adam m", "adam v", "count")):
            np.testing.assert_array_equal(x, y, err_msg=f"{tag}: {cfg} {what}")
        assert a[cfg][1] == b[cfg][1], f"{tag}: {cfg} ring"
        for g in ("train", "val", "eval"):
            assert a[cfg][2][g] == b[cfg][2][g], f"{tag}: {cfg} {g}.csv"


@pytest.mark.parametrize("variant", ["single", "ensemble", "pbt"])
def test_chunked_run_equals_the_uninterrupted_one(tmp_path, variant):
    """Collects follow updates 4, 8 and 12; the checkpoint is written after update 8, so updates
    9-12 draw from a ring that has to cross the restart (under pbt a clone's copy too)."""
    n = 8 if variant == "pbt" else 4
    whole = _train_in_chunks(tmp_path / "whole", variant, 12, [n])
    halves = _train_in_chunks(tmp_path / "halves", variant, 12, [n // 2, n // 2])
    assert whole[1] == 3
    for cfg, (_, ring, _, _) in whole[0].items():
        assert ring[0]["appended"] > 60, (cfg, ring[0])          # 60 rows: the rings wrapped
    _assert_runs_equal(whole, halves, variant)


def test_chunked_run_without_rollouts_is_the_control(tmp_path):
    """branches = 0: the same comparison on the code path every other mode resumes by."""
    whole = _train_in_chunks(tmp_path / "whole", "single", 0, [4])
    halves = _train_in_chunks(tmp_path / "halves", "single", 0, [2, 2])
    assert whole[1] == 0
    _assert_runs_equal(whole, halves, "control")


# ------------------------------------------------------------------ 7. the driver
DRIVER_FLAGS = ["--steps=8", "--eval_interval=8", "--log_interval=4", "--agent.batch_size=64", "--agent.layer_norm",
                "--eval_episodes=4", "--synthetic_rows=2003", "--task=simulated", "--max_episode_steps=6",
                "--number_of_alphas=2", "--model_rollout_branches=12", "--model_rollout_horizon=4",
                "--model_rollout_interval=4", "--model_rollout_warmup=0", "--model_real_ratio=0.5",
                "--model_buffer_rows=200"]


def _tree_equal(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), f"{path}: keys"
        for k in a:
            _tree_equal(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), f"{path}: length"
        for i, (x, y) in enumerate(zip(a, b)):
            _tree_equal(x, y, f"{path}[{i}]")
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=path)


def _drive(save, runs, flags=DRIVER_FLAGS):
    import tune_alpha
    for evaluations in runs:
        tune_alpha.main([f"--save_directory={save}", f"--max_evaluations={evaluations}"] + flags)
    with open(save / ENV / "checkpoint.pkl", "rb") as f:
        experiments = pickle.load(f)["trainer"]["experiments"]
    return {(cfg.alpha, cfg.seed): exp for cfg, exp in experiments.items()}


def _assert_checkpoints_equal(a, b):
    assert set(a) == set(b) and len(a) == 2
    for key in sorted(a):                                # the figures first, then the assertions
        ra, rb = a[key]["synth_ring"], b[key]["synth_ring"]
        same_ring = ra["appended"] == rb["appended"] and all(ra[k].tobytes() == rb[k].tobytes() for k in S.FIELDS)
        print(f"(alpha, seed) {key}: step {a[key]['current_step']} / {b[key]['current_step']}, ring rows "
              f"{ra['rewards'].shape[0]} / {rb['rewards'].shape[0]}, appended {ra['appended']} / {rb['appended']}, "
              f"ring bytes equal: {same_ring}")
    for key in sorted(a):
        assert a[key]["current_step"] == b[key]["current_step"]
        assert a[key]["synth_ring"]["appended"] > 0
        _tree_equal(a[key]["synth_ring"], b[key]["synth_ring"], f"{key} synth_ring")
        _tree_equal(a[key]["agent"], b[key]["agent"], f"{key} agent")


def test_driver_run_twice_equals_run_once(tmp_path):
    """``tune_alpha.main`` twice with --max_evaluations=1 on one save directory against once with
    --max_evaluations=2 on another, with test_tune_alpha_driver_with_model_rollouts's flags.

    At these flags (8 steps, one round, two candidates) --max_evaluations=1 trains the first
    candidate alone and defers the second to the next invocation, where it trains alone as
    well: the first candidate's ring has to cross the restart untouched, and the deferred
    candidate's collect (after its update 4) has to get the seed it has when both train in lock
    step.  ``Trainer._train_with_rollouts`` therefore seeds a collect by the update it follows
    and not by the number of collects the run has made, which was 1 here for the deferred
    candidate against 0 in the one run (15 against 12 rows appended, other bytes)."""
    chunked = _drive(tmp_path / "chunked", [1, 1])
    once = _drive(tmp_path / "once", [2])
    _assert_checkpoints_equal(chunked, once)


def test_driver_resumed_at_a_round_boundary_equals_run_once(tmp_path):
    """The same flags but 16 steps (two rounds of two evaluations): twice --max_evaluations=2
    against once --max_evaluations=4.  The collects follow updates 4, 8 and 12, the restart
    update 8."""
    flags = ["--steps=16"] + [f for f in DRIVER_FLAGS if not f.startswith("--steps=")]
    chunked = _drive(tmp_path / "chunked", [2, 2], flags)
    once = _drive(tmp_path / "once", [4], flags)
    _assert_checkpoints_equal(chunked, once)


# ------------------------------------------------------------------ 8. old checkpoints
def test_checkpoints_without_the_key_and_keys_without_rings(tmp_path):
    trainer, task = _trainer_parts(tmp_path / "a", "single", 12)
    trainer.train(max_evaluations=2)
    state = _checkpoint(trainer)
    assert all(e["synth_ring"]["appended"] > 0 and "synth_ring" not in e["agent"]
               for e in state["trainer"]["experiments"].values())
    params = {cfg: trainer.population.get_flat(m) for cfg, m in trainer.member_of.items()}
    trainer.population.close()
    task.close()
    # a run resumed with rollouts switched off: the key is ignored
    off, task = _trainer_parts(tmp_path / "a", "single", 0, state)
    assert off.population.synth_capacity is None
    for cfg, m in off.member_of.items():
        np.testing.assert_array_equal(off.population.get_flat(m), params[cfg])
    assert all("synth_ring" not in e for e in off.state_dict()["experiments"].values())
    off.population.close()
    task.close()
    # a checkpoint from before rings were saved: it loads, and the rings are empty
    for e in state["trainer"]["experiments"].values():
        del e["synth_ring"]
    old, task = _trainer_parts(tmp_path / "a", "single", 12, state)
    for cfg, m in old.member_of.items():
        assert old.population.synth_info(m) == EMPTY
        np.testing.assert_array_equal(old.population.get_flat(m), params[cfg])
        assert old.experiments[cfg].current_step == 8
    assert old.collect_index == 2
    old.train(max_evaluations=2)
    assert all(old.population.synth_info(m)["appended"] > 0 for m in old.member_of.values())
    old.population.close()
    task.close()
