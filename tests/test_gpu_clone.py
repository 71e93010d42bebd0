"""GPU tests of the on-device member clone (fqlpop_clone_members / Population.clone_members):
the copy is complete (a clone and its source stay bit-identical under equal batches, noise,
alpha and seed), stream-ordered between the steps, refuses bad arguments without touching
any state, and keeps the poison contract of a failed split launch.

Configurations (both engine paths):
  S  obs 28, act 5, hidden (512,) x 4, critic LayerNorm, 6 members: the streamed kernels
     with W^T arenas.  B = 256, not 32: the engine takes batch sizes that are multiples of
     64 only, and 256 is the size (the one test_gpu_split.py uses) at which the default plan
     of 6 members is unsplit while 2 active members run the split plan -- asserted below.
  P  hidden (64,) x 4, B = 64, 4 members: the per-layer path (test_gpu_surface.py's config).
All comparisons are bitwise (np.array_equal on the uint32 view): a copy has no tolerance.
"""
import numpy as np
import pytest

from oracle import fql_oracle as O

pytestmark = pytest.mark.gpu

CONF = {
    "S": dict(hidden=(512,) * 4, B=256, n=6, dst=4),
    "P": dict(hidden=(64,) * 4, B=64, n=4, dst=3),
}
E_ARG, E_STATE = "fqlpop error -1", "fqlpop error -3"


def _data(N, D, A, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((N, D)).astype(np.float32)
    rew = np.where(rng.uniform(size=N) < 0.05, 0.0, -1.0).astype(np.float32)
    return {"observations": obs, "actions": rng.uniform(-1 + 1e-5, 1 - 1e-5, (N, A)).astype(np.float32),
            "rewards": rew, "masks": (1.0 - (rew == 0)).astype(np.float32),
            "next_observations": (obs + 0.05 * rng.standard_normal((N, D))).astype(np.float32)}


DATA = _data(20_000, 28, 5, 4)


def _pop(conf, n=None):
    from fqlpop import Population, PopulationConfig
    c = CONF[conf]
    n = n or c["n"]
    pop = Population(PopulationConfig(hidden_dims=c["hidden"], batch_size=c["B"]),
                     [3.0 * 2.5 ** i for i in range(n)], [11 + i for i in range(n)])
    pop.set_dataset(DATA)
    return pop


def _state(pop, i):
    """(params, Adam m, Adam v) as uint32 and the update count of member i."""
    return [pop.get_flat(i, w).view(np.uint32) for w in (0, 1, 2)] + [pop.get_count(i)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def _inject(pop, conf, same, seed=5):
    """One injected step of the active members; the members in `same` get one batch and noise."""
    c = CONF[conf]
    ocfg = O.OracleConfig(hidden_dims=c["hidden"], batch_size=c["B"])
    rng = np.random.default_rng(seed)
    shared = (O.cast_tree(O.make_batch(ocfg, c["B"], rng), np.float32),
              O.cast_tree(O.make_noise(ocfg, c["B"], rng), np.float32))
    batches, noises = [], []
    for i in pop.active_ids:
        b, z = shared if i in same else (O.cast_tree(O.make_batch(ocfg, c["B"], rng), np.float32),
                                         O.cast_tree(O.make_noise(ocfg, c["B"], rng), np.float32))
        batches.append(b)
        noises.append(z)
    pop.step_injected(batches, noises)


def _info_rows(pop, a, b):
    info = pop.read_info_array().view(np.uint32)
    return info[a], info[b]


def test_plans_of_the_s_config():
    from fqlpop import PopulationConfig
    from fqlpop.population import SPLIT_SITES, split_plan
    cfg = PopulationConfig(hidden_dims=CONF["S"]["hidden"], batch_size=CONF["S"]["B"])
    assert all(split_plan(cfg, 6)[s] == 1 for s in SPLIT_SITES)
    assert any(split_plan(cfg, 2)[s] > 1 for s in SPLIT_SITES)


@pytest.mark.parametrize("conf", ["S", "P"])
def test_state_is_bit_equal_after_odd_and_even_flips(conf):
    pop = _pop(conf)
    d = CONF[conf]["dst"]
    pop.step(3)  # Adam moments nonzero, target != critic, the double buffer flipped 3 times
    own_alpha = float(pop.alphas[d])
    pop.clone_members([0], [d], seeds=[int(pop.seeds[0])])  # alpha kept
    s0, sd = _state(pop, 0), _state(pop, d)
    assert s0[3] == 3 and np.any(s0[1]) and np.any(s0[2])
    assert _same(s0, sd)
    assert float(pop.alphas[d]) == own_alpha and int(pop.seeds[d]) == int(pop.seeds[0])
    pop.step(1)  # different alphas: the two diverge; 4 flips now
    assert not _same(_state(pop, 0), _state(pop, d))
    pop.clone_member(0, d)
    s0, sd = _state(pop, 0), _state(pop, d)
    assert s0[3] == 4 and _same(s0, sd)
    pop.close()


@pytest.mark.parametrize("conf,active,pre", [("S", None, 3), ("S", None, 4), ("S", (0, 4), 3), ("P", None, 3)])
def test_copy_is_complete(conf, active, pre):
    """Not only what get_state shows: a clone with its source's alpha and seed steps exactly as
    the source does (a stale W^T or params_nx copy would not)."""
    pop = _pop(conf)
    d = CONF[conf]["dst"]
    if active is not None:
        pop.set_active([i in active for i in range(pop.n)])
    pop.step(pre)
    pop.clone_members([0], [d], alphas=[float(pop.alphas[0])], seeds=[int(pop.seeds[0])])
    _inject(pop, conf, same=(0, d))
    assert _same(_state(pop, 0), _state(pop, d))
    ra, rb = _info_rows(pop, 0, d)
    assert np.array_equal(ra, rb)
    pop.step(2)  # device draws: same seed and alpha give the same sampling key
    s0, sd = _state(pop, 0), _state(pop, d)
    assert s0[3] == pre + 3 and _same(s0, sd)
    ra, rb = _info_rows(pop, 0, d)
    assert np.array_equal(ra, rb)
    if active is None:  # (the other members went their own way)
        assert not _same(_state(pop, 1), s0)
    pop.close()


@pytest.mark.parametrize("conf", ["S", "P"])
def test_alpha_takes_effect(conf):
    pop = _pop(conf)
    d = CONF[conf]["dst"]
    pop.step(3)
    a0, seed0 = float(pop.alphas[0]), int(pop.seeds[0])
    pop.clone_members([0], [d], alphas=[a0 * 1.25], seeds=[seed0])
    assert pop.alphas[d] == np.float32(a0 * 1.25)
    before = _state(pop, d)
    _inject(pop, conf, same=(0, d))
    t0, td = pop.get_params(0), pop.get_params(d)
    for net in ("critic", "target_critic", "actor_bc_flow"):
        for leaf in t0[net]:
            assert np.array_equal(t0[net][leaf].view(np.uint32), td[net][leaf].view(np.uint32)), (net, leaf)
    assert any(not np.array_equal(t0["actor_onestep_flow"][leaf], td["actor_onestep_flow"][leaf])
               for leaf in t0["actor_onestep_flow"])
    # the engine's alpha of the clone is pop.alphas[d]: the same step from the same state with
    # that value stated again through set_member gives the same bits
    after = _state(pop, d)
    for w in (0, 1, 2):
        pop.set_flat(d, before[w].view(np.float32), w)
    pop.set_count(d, before[3])
    pop.set_member(d, float(pop.alphas[d]), seed0, reinit=False)
    _inject(pop, conf, same=(0, d))
    assert _same(_state(pop, d), after)
    pop.close()


def test_several_pairs_with_a_shared_source():
    pop, twin = _pop("S"), _pop("S")
    pop.step(3)
    twin.step(3)
    pop.clone_members([0, 0, 1], [3, 4, 5], seeds=[101, 102, 103])
    st = [_state(pop, i) for i in range(6)]
    assert _same(st[3], st[0]) and _same(st[4], st[0]) and _same(st[5], st[1])
    assert not _same(st[0], st[1])
    assert [int(s) for s in pop.seeds[3:]] == [101, 102, 103]
    pop.step(2)
    twin.step(2)
    st = [_state(pop, i) for i in range(6)]
    for i in range(6):
        for j in range(i + 1, 6):
            assert not np.array_equal(st[i][0], st[j][0]), (i, j)
    # members not written by the clone are where an identical population without it is
    for i in (0, 1, 2):
        assert _same(st[i], _state(twin, i)), i
    pop.close()
    twin.close()


def test_inactive_destination():
    pop = _pop("S")
    init = _state(pop, 5)
    pop.set_active([1, 1, 1, 1, 1, 0])
    pop.step(3)
    assert _same(_state(pop, 5), init)
    pop.clone_members([0], [5], alphas=[float(pop.alphas[0])], seeds=[int(pop.seeds[0])])
    snap = _state(pop, 0)
    assert _same(_state(pop, 5), snap)
    # the others step on while the clone waits (the parameter buffers swap under it): it keeps
    # the state it was given whichever buffer is current when it is activated
    pop.step(1)
    assert _same(_state(pop, 5), snap)
    pop.clone_members([0], [5], alphas=[float(pop.alphas[0])], seeds=[int(pop.seeds[0])])
    pop.set_active([1] * 6)
    _inject(pop, "S", same=(0, 5))
    assert _same(_state(pop, 0), _state(pop, 5))
    ra, rb = _info_rows(pop, 0, 5)
    assert np.array_equal(ra, rb)
    pop.step(2)
    s0 = _state(pop, 0)
    assert s0[3] == 7 and _same(s0, _state(pop, 5))
    pop.close()


def test_inactive_clone_steps_from_either_buffer():
    """A clone made into a slot that does not step, activated after an ODD number of further
    steps of the others, trains from the state it was given (not from the older half of the
    source's double buffer)."""
    pop, twin = _pop("S"), _pop("S")
    for p in (pop, twin):
        p.set_active([1, 1, 1, 1, 1, 0])
        p.step(3)
    a0, seed0 = float(pop.alphas[0]), int(pop.seeds[0])
    pop.clone_members([0], [5], alphas=[a0], seeds=[seed0])
    pop.step(1)
    only5 = [0, 0, 0, 0, 0, 1]
    pop.set_active(only5)
    pop.step(2)
    # the twin's member 0 after 3 + 2 steps alone is what the clone must have reached
    twin.set_active([1, 0, 0, 0, 0, 0])
    twin.step(2)
    assert _same(_state(pop, 5), _state(twin, 0))
    pop.close()
    twin.close()


def test_stream_order():
    def run(sync):
        pop = _pop("S")
        for call in (lambda: pop.step(3),
                     lambda: pop.clone_members([0, 1], [4, 5], seeds=[201, 202]),
                     lambda: pop.step(2)):
            call()
            if sync:
                pop.sync()
        out = [_state(pop, i) for i in range(6)]
        pop.close()
        return out
    a, b = run(False), run(True)
    for i in range(6):
        assert _same(a[i], b[i]), i
    assert not _same(a[4], a[0])


def test_bad_arguments_are_refused_and_change_nothing():
    from fqlpop import FqlpopError
    pop = _pop("P")
    pop.step(1)
    before = [_state(pop, i) for i in range(4)]
    alphas, seeds = pop.alphas.copy(), pop.seeds.copy()
    bad = {"dst == src": ([1], [1]), "duplicate dst": ([0, 1], [2, 2]), "dst is also a src": ([0, 2], [2, 3]),
           "src out of range": ([4], [1]), "dst out of range": ([0], [4]), "negative index": ([-1], [1]),
           "n_pairs = 0": ([], [])}
    for what, (src, dst) in bad.items():
        with pytest.raises(FqlpopError, match=E_ARG):
            pop.clone_members(src, dst, alphas=[7.0] * len(src), seeds=[9] * len(src))
        pop.sync()
        for i in range(4):
            assert _same(_state(pop, i), before[i]), (what, i)
        assert np.array_equal(pop.alphas, alphas) and np.array_equal(pop.seeds, seeds), what
    with pytest.raises(FqlpopError, match=E_ARG):
        pop.clone_members([0], [4])  # defaults with an index out of range
    pop.step(1)  # alpha and seed on the device are unchanged too: as a twin that made no such call
    twin = _pop("P")
    twin.step(2)
    for i in range(4):
        assert _same(_state(pop, i), _state(twin, i)), i
    pop.close()
    twin.close()


def test_poison_contract():
    """As test_split_failure_is_sticky_until_restored: a poisoned source is refused; a clone
    from a restored member restores the destination without any set_state on it."""
    from fqlpop import FqlpopError
    from fqlpop._lib import check
    pop = _pop("S", n=2)
    pop.step(2)
    pop.sync()
    saved = [pop.get_flat(0, w) for w in (0, 1, 2)]
    check(pop.lib.fqlpop_debug_fail_split(pop._h))
    with pytest.raises(FqlpopError, match=E_STATE):
        pop.clone_members([0], [1])
    with pytest.raises(FqlpopError, match="member 1"):
        pop.get_flat(1, 0)
    for w in (0, 1, 2):
        pop.set_flat(0, saved[w], w)
    with pytest.raises(FqlpopError, match="member 1"):
        pop.step(1)
    pop.clone_members([0], [1])
    assert _same(_state(pop, 1), _state(pop, 0))  # member 1 exports again
    pop.step(1)
    pop.sync()
    assert np.all(np.isfinite(pop.read_info_array()[:, :13]))
    pop.close()
