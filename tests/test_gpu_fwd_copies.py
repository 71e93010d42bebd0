"""Engine option ``fwd_copies``: in a train step the unsplit streamed forwards write the copies
derived from the hidden kernels they stream anyway (bit 1: the W^T copies the step's streamed
backward reads, from the BC, one-step and critic forwards; bit 2: the target EMA of those
kernels, from the target forward into the other buffer of the target pair), and the fused
optimiser epilogue leaves them out.  Same values, same arithmetic (``ema_target``), so a
population with any value of the option must be BIT-IDENTICAL to one with ``fwd_copies=0``
given the same seeds and data: every comparison here is ``array_equal`` on float32, of the
parameters (with the target critic), Adam m and v, and the train info after every step."""
import numpy as np
import pytest

from _helpers import engine_options, synthetic_rows

pytestmark = pytest.mark.gpu

CUBE = dict(D=28, A=5)    # layer 0: one ring pass plus the tail k-step
NOTAIL = dict(D=24, A=4)  # layer 0: no tail k-step
N_INFO = 13
STEPS = 3


def _pop(fwd_copies, D, A, B, n, ln=True, q_agg="mean", **opts):
    from fqlpop import Population, PopulationConfig
    with engine_options(fwd_copies=fwd_copies, **opts):
        pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(512,) * 4, batch_size=B,
                                          layer_norm=ln, q_agg=q_agg),
                         [3.0 * 3.3 ** i for i in range(n)], [11 + i for i in range(n)])
    pop.set_dataset(synthetic_rows(5_000, D, A, 3))
    return pop


def _info(pop):
    return pop.read_info_array()[:, :N_INFO].copy()


def _same(new, ref, tag):
    a, b = _info(new), _info(ref)
    assert np.all(np.isfinite(b)), f"{tag}: reference info {b}"
    assert np.array_equal(a, b), f"{tag}: train info differs\nfwd_copies {a}\nreference  {b}"
    for i in range(ref.n):
        for w in (0, 1, 2):  # parameters (with the target critic), Adam m, Adam v
            x, y = new.get_flat(i, w), ref.get_flat(i, w)
            assert np.array_equal(x, y), f"{tag}: member {i} state {w} differs (max |d| {np.abs(x - y).max()})"


def _run_pair(value, steps=STEPS, **kw):
    new, ref = _pop(value, **kw), _pop(0, **kw)
    try:
        for it in range(steps):
            for p in (new, ref):
                p.step(1)
            _same(new, ref, f"step {it}")
    finally:
        new.close()
        ref.close()


# The library takes batch sizes that are multiples of 64 only (fqlpop_create refuses B = 16 and
# B = 48), so a producing forward never has fewer than 4 column tiles.  B = 64, 128, 192, 256
# give 4, 8, 12, 16 tiles at the target forward and 8, 16, 24, 32 at the BC, critic and (lazy
# metric) one-step forwards; the eager one-step forward has 12 at B = 64 (below).  That covers
# fewer tiles than the 16 ring passes of a layer (4, 8, 12: a tile owns 4, 2, 1-2 passes), a
# non-divisor of 16 (12), exactly 16, and tiles >= 16 that own nothing (24, 32).
@pytest.mark.parametrize("B,shape,ln,q_agg,n", [
    (64, CUBE, True, "mean", 1), (64, NOTAIL, False, "min", 3),
    (128, CUBE, True, "min", 2), (128, NOTAIL, False, "mean", 1),
    (192, CUBE, False, "min", 2), (192, NOTAIL, True, "mean", 3),
    (256, CUBE, True, "mean", 1), (256, NOTAIL, False, "min", 2),
], ids=lambda v: v if isinstance(v, str) else None)
def test_unsplit_kernels_both_copies(B, shape, ln, q_agg, n):
    _run_pair(3, B=B, n=n, ln=ln, q_agg=q_agg, split=0, **shape)


@pytest.mark.parametrize("value", [1, 2])
@pytest.mark.parametrize("B,shape,ln", [(192, CUBE, True), (256, NOTAIL, False), (256, CUBE, True)])
def test_unsplit_kernels_one_half(value, B, shape, ln):
    _run_pair(value, B=B, n=2, ln=ln, split=0, **shape)


def test_eager_metric_forward_three_thirds():
    """lazy_metric 0: the one-step forward runs 3B columns (12 tiles at B = 64)."""
    _run_pair(3, B=64, n=2, split=0, lazy_metric=0, **CUBE)


@pytest.mark.parametrize("value", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2])
def test_plan_on_auto(value, n):
    """1 / 2 cube members with the split plan on auto: the split launch sites keep the optimiser's
    copies, the unsplit ones (if any) take the forwards', in the same step."""
    _run_pair(value, B=256, n=n, **CUBE)


def _deactivate_reactivate(pop):
    pop.set_active([1, 0, 1])
    pop.step(1)
    pop.set_active([1, 1, 1])


def _set_flat(pop):
    pop.set_flat(0, pop.get_flat(1))


def _validate_and_read(pop):
    pop.total_loss()
    pop.read_info_array()       # the deferred metric
    pop.read_info_array("val")


def _clone(pop):
    pop.clone_members([0], [2])


@pytest.mark.parametrize("between", [_deactivate_reactivate, _set_flat, _validate_and_read, _clone],
                         ids=lambda f: f.__name__.lstrip("_"))
@pytest.mark.parametrize("opts", [dict(split=0), dict()], ids=["unsplit", "auto"])
def test_state_transitions(between, opts):
    """Two steps, a call that changes the active set, writes a member's state, runs a validation
    pass and the deferred metric, or clones a member; then two more steps."""
    kw = dict(B=64, n=3, **CUBE, **opts)
    new, ref = _pop(3, **kw), _pop(0, **kw)
    try:
        for p in (new, ref):
            p.step(2)
            between(p)
        _same(new, ref, between.__name__)
        for it in range(2):
            for p in (new, ref):
                p.step(1)
            _same(new, ref, f"{between.__name__}, step {it} after")
    finally:
        new.close()
        ref.close()
