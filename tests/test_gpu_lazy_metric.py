"""Engine option ``lazy_metric``: a train step runs the one-step actor forward on [s'; s] only
and leaves the metrics-only third (z_metric, the ``mse`` info value) to be evaluated when the
train info is read, or just before a call overwrites what that evaluation reads
(runtime.cpp, materialise_metric).  The deferred evaluation is the same forward kernel on the
same inputs and the same reduction, so a ``lazy_metric=1`` population must be BIT-IDENTICAL
to a ``lazy_metric=0`` one with the same seeds and data: every comparison here is
``array_equal`` on float32."""
import numpy as np
import pytest

from _helpers import engine_options, synthetic_rows

pytestmark = pytest.mark.gpu

SMALL = dict(D=5, A=2, B=64, n=2)      # 4 column tiles per third, 2 members
CUBE = dict(D=28, A=5, B=256, n=1)     # cube shapes, 1 member: the split forms run
N_INFO = 13


def _pop(lazy, D, A, B, n, probe=False, **opts):
    from fqlpop import Population, PopulationConfig
    with engine_options(lazy_metric=lazy, **opts):
        pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(512,) * 4, batch_size=B),
                         [3.0 * 3.3 ** i for i in range(n)], [11 + i for i in range(n)])
    pop.set_dataset(synthetic_rows(5_000, D, A, 3))
    if probe:
        pop.set_probe(True)
    return pop


def _pair(shape, probe=False, lazy_opts=None):
    return _pop(1, probe=probe, **shape, **(lazy_opts or {})), _pop(0, probe=probe, **shape)


def _info(pop):
    return pop.read_info_array()[:, :N_INFO].copy()


def _same_state(lazy, eager, tag):
    for i in range(lazy.n):
        for w in (0, 1, 2):  # parameters (with the target critic), Adam m, Adam v
            x, y = lazy.get_flat(i, w), eager.get_flat(i, w)
            assert np.array_equal(x, y), f"{tag}: member {i} state {w} differs (max |d| {np.abs(x - y).max()})"


def _same_info(lazy, eager, tag):
    a, b = _info(lazy), _info(eager)
    assert np.all(np.isfinite(b)) and float(np.abs(b[:, 9]).min()) > 0.0, f"{tag}: eager info {b}"
    assert np.array_equal(a, b), f"{tag}: train info differs\nlazy  {a}\neager {b}"


@pytest.mark.parametrize("shape,probe,lazy_opts", [
    (SMALL, False, None), (SMALL, True, None), (SMALL, False, {"split": 0}), (CUBE, False, None),
], ids=["small", "small-probe", "small-unsplit-vs-auto", "cube-1-member"])
def test_step_and_read_five_times(shape, probe, lazy_opts):
    lazy, eager = _pair(shape, probe, lazy_opts)
    try:
        for it in range(5):
            for p in (lazy, eager):
                p.step(1)
            _same_info(lazy, eager, f"step {it}")
            _same_state(lazy, eager, f"step {it}")
        assert lazy.metric_evaluations == 5 and eager.metric_evaluations == 0
        assert lazy.flops_per_member_step < eager.flops_per_member_step
    finally:
        lazy.close()
        eager.close()


def test_three_steps_one_read():
    lazy, eager = _pair(SMALL)
    try:
        for p in (lazy, eager):
            p.step(3)
        _same_info(lazy, eager, "after step(3)")
        _same_state(lazy, eager, "after step(3)")
        assert lazy.metric_evaluations == 1
    finally:
        lazy.close()
        eager.close()


def test_second_read_launches_nothing():
    lazy = _pop(1, **SMALL)
    try:
        assert lazy.metric_evaluations == 0
        lazy.read_info_array()  # nothing stepped yet: nothing pending
        assert lazy.metric_evaluations == 0
        lazy.step(2)
        first = lazy.read_info_array().copy()
        assert lazy.metric_evaluations == 1
        second = lazy.read_info_array().copy()
        assert lazy.metric_evaluations == 1
        assert np.array_equal(first, second)
    finally:
        lazy.close()


def _set_flat(pop):
    pop.set_flat(0, pop.get_flat(1))


def _clone(pop):
    pop.clone_members([0], [1])


def _deactivate(pop):
    pop.set_active([1, 0])


def _batches(shape, seed):
    D, A, B = shape["D"], shape["A"], shape["B"]
    rng = np.random.default_rng(seed)
    return [{"observations": rng.standard_normal((B, D)).astype(np.float32),
             "actions": rng.uniform(-1, 1, (B, A)).astype(np.float32),
             "rewards": -np.ones(B, np.float32), "masks": np.ones(B, np.float32),
             "next_observations": rng.standard_normal((B, D)).astype(np.float32)} for _ in range(shape["n"])]


def _noises(shape, seed):
    A, B = shape["A"], shape["B"]
    rng = np.random.default_rng(seed)
    return [{"z_next": rng.standard_normal((B, A)).astype(np.float32),
             "x0": rng.standard_normal((B, A)).astype(np.float32),
             "t": rng.uniform(size=B).astype(np.float32),
             "z_d": rng.standard_normal((B, A)).astype(np.float32),
             "z_metric": rng.standard_normal((B, A)).astype(np.float32)} for _ in range(shape["n"])]


def _total_loss(pop):
    pop.total_loss(_batches(SMALL, 9), _noises(SMALL, 10))


def _total_loss_sampled(pop):
    pop.total_loss()


def _step_injected(pop):
    pop.step_injected(_batches(SMALL, 7), _noises(SMALL, 8))


@pytest.mark.parametrize("between", [_set_flat, _clone, _deactivate, _total_loss, _total_loss_sampled, _step_injected],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_read_after_a_call_that_overwrites_the_inputs(between):
    """Step, then a call that overwrites what the pending evaluation reads (a parameter
    buffer, the active slots, os_in / act_t), then read: every member's info, the overwritten,
    cloned or deactivated member's included, is what the eager population reports."""
    lazy, eager = _pair(SMALL)
    try:
        for p in (lazy, eager):
            p.step(2)
            between(p)
        _same_info(lazy, eager, between.__name__)
        if between is _total_loss or between is _total_loss_sampled:
            assert np.array_equal(lazy.read_info_array("val"), eager.read_info_array("val"))
        _same_state(lazy, eager, between.__name__)
        # and the populations go on identically (the deactivated member stays behind)
        for p in (lazy, eager):
            p.step(1)
        _same_info(lazy, eager, between.__name__ + ", next step")
        _same_state(lazy, eager, between.__name__ + ", next step")
    finally:
        lazy.close()
        eager.close()
