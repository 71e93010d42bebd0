"""Population-based training of alpha, host side (hpo/pbt.py): the exploit / explore
decision on hand-made scores, ready_interval, determinism and resume, and the C ABI
declaration of the on-device member clone.  No GPU."""
import os
import pickle
import random
import re

import numpy as np

from fqlpop.distributed import config_key
from hpo.pbt import PopulationBasedTraining
from trainer.config import ExperimentConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (0.8, 1.25)


def _configs(n=8):
    return [ExperimentConfig(alpha=float(3 * 2 ** i), seed=100 + i) for i in range(n)]


def _feed(strategy, scores):
    for c in sorted(strategy.population, key=config_key):
        strategy.update(c, scores(c))


def _by_alpha(c):
    return c.alpha


def test_exploit_replaces_the_worst_with_perturbed_children_of_the_best():
    cfgs = _configs()
    st = PopulationBasedTraining(set(cfgs), 0, truncation=0.25, perturb_factors=FACTORS, seed=3)
    assert st.sample() == set(cfgs)  # no scores yet
    _feed(st, _by_alpha)  # the two largest alphas are best, the two smallest worst
    new = st.sample()
    assert len(new) == 8
    assert cfgs[0] not in new and cfgs[1] not in new and set(cfgs[2:]) <= new
    children = sorted(new - set(cfgs), key=config_key)
    assert len(children) == 2
    used = {c.seed for c in cfgs}
    for ch in children:
        parent = st.parent_of[ch]
        assert parent in (cfgs[6], cfgs[7])
        assert any(ch.alpha == parent.alpha * f for f in FACTORS)
        assert ch.seed not in used and 0 <= ch.seed < 10000
        used.add(ch.seed)
        assert st.candidate_scores[ch] == st.candidate_scores[parent]
        assert st.candidate_scores[ch] is not st.candidate_scores[parent]
    assert [r["round"] for r in st.lineage] == [0, 0]
    assert {r["child"] for r in st.lineage} == set(children)
    assert all(st.parent_of[r["child"]] == r["parent"] for r in st.lineage)
    for r in st.lineage:
        assert r["parent_alpha"] == r["parent"].alpha and r["child_alpha"] == r["child"].alpha
        assert r["parent_score"] == r["parent"].alpha  # the hand-made score
    assert st.sample() == new  # no new evaluation: no second exploit
    # constant size over 5 rounds, every seed used once
    for _ in range(4):
        _feed(st, _by_alpha)
        assert len(st.sample()) == 8
    assert st.exploit_rounds == 5 and len(st.lineage) == 10
    seeds = [c.seed for c in st.candidate_scores]
    assert len(seeds) == len(set(seeds)) == 8 + 10


def test_alpha_is_clipped_to_the_bounds():
    cfgs = _configs()
    hi = cfgs[7].alpha * 1.1
    st = PopulationBasedTraining(set(cfgs), 0, truncation=0.25, perturb_factors=(1.25,), alpha_bounds=(None, hi))
    _feed(st, _by_alpha)
    new = st.sample()
    for ch in new - set(cfgs):
        parent = st.parent_of[ch]
        assert ch.alpha == min(parent.alpha * 1.25, hi)
    assert any(ch.alpha == hi for ch in new - set(cfgs)) or all(st.parent_of[c] == cfgs[6] for c in new - set(cfgs))
    lo = PopulationBasedTraining(set(cfgs), 0, truncation=0.25, perturb_factors=(0.01,), alpha_bounds=(5.0, 1e4))
    _feed(lo, _by_alpha)
    assert all(ch.alpha == 5.0 for ch in lo.sample() - set(cfgs))


def test_truncation_count_and_history_mean():
    cfgs = _configs(5)
    # k = max(1, int(5 * 0.5)) = 2, capped at 5 // 2 = 2
    st = PopulationBasedTraining(set(cfgs), 0, truncation=0.5, history_length=2)
    _feed(st, _by_alpha)
    assert st.sample() == set(cfgs)  # fewer than history_length scores
    _feed(st, lambda c: -3.0 * c.alpha)  # mean of the last two: -alpha -> the smallest alphas are best now
    new = st.sample()
    assert len(new - set(cfgs)) == 2 and cfgs[3] not in new and cfgs[4] not in new
    assert all(st.parent_of[c] in cfgs[:2] for c in new - set(cfgs))
    one = PopulationBasedTraining({cfgs[0]}, 0)
    one.update(cfgs[0], 1.0)
    assert one.sample() == {cfgs[0]}  # n // 2 = 0: nothing to replace


def test_ties_are_broken_by_config_key():
    cfgs = _configs()
    st = PopulationBasedTraining(set(cfgs), 0, truncation=0.25)
    _feed(st, lambda c: 0.5)  # all equal: config_key order ranks them
    new = st.sample()
    # best = first two in config_key order, worst = last two
    assert cfgs[6] not in new and cfgs[7] not in new and set(cfgs[:6]) <= new
    assert all(st.parent_of[c] in cfgs[:2] for c in new - set(cfgs))


def test_ready_interval_three():
    cfgs = _configs()
    st = PopulationBasedTraining(set(cfgs), 0, ready_interval=3, truncation=0.25)
    pops = []
    for r in range(1, 8):
        before = set(st.population)
        _feed(st, _by_alpha)
        after = st.sample()
        pops.append(after)
        if r % 3 == 0:
            assert after != before and len(after) == 8
        else:
            assert after == before
    assert st.exploit_rounds == 2


def test_deterministic_resumable_and_global_rng_untouched():
    cfgs = _configs()

    def score(c):  # depends on the candidate only, so both instances see the same
        return ((c.seed * 2654435761) % 1000) / 1000.0 + c.alpha * 1e-3

    def make(**kw):
        return PopulationBasedTraining(set(cfgs), 0, truncation=0.25, history_length=2, seed=7, **kw)
    a, b = make(), make()
    random.seed(123)
    np.random.seed(123)
    py_state, np_state = random.getstate(), np.random.get_state()
    resumed = None
    for r in range(6):
        for st in (a, b, resumed):
            if st is not None:
                _feed(st, score)
        sa, sb = a.sample(), b.sample()
        assert sa == sb
        if resumed is not None:
            assert resumed.sample() == sa and resumed.parent_of == a.parent_of
        if r == 2:  # rebuild mid-run from a pickled state_dict
            resumed = make(state_dict=pickle.loads(pickle.dumps(a.state_dict())))
            assert resumed.population == a.population
    assert a.lineage == b.lineage == resumed.lineage and len(a.lineage) == 2 * 5
    assert a.state_dict()["performed_evaluations"] == resumed.performed_evaluations == 6
    assert random.getstate() == py_state
    now = np.random.get_state()
    assert now[0] == np_state[0] and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    other = PopulationBasedTraining(set(cfgs), 0, truncation=0.25, history_length=2, seed=8)
    for r in range(6):
        _feed(other, score)
        other.sample()
    assert other.lineage != a.lineage  # the seed matters


def test_other_strategies_expose_no_parent_of():
    from hpo.identity import Identity
    from hpo.successive_halving import SuccessiveHalving
    cfgs = _configs(4)
    assert not hasattr(Identity(cfgs, 0), "parent_of")
    assert not hasattr(SuccessiveHalving(set(cfgs), 8), "parent_of")
    assert hasattr(PopulationBasedTraining(set(cfgs), 0), "parent_of")


def test_clone_members_is_declared_and_exported():
    import fqlpop
    header = open(os.path.join(ROOT, "include", "fqlpop.h")).read()
    decl = re.search(r"int\s+fqlpop_clone_members\s*\(([^)]*)\)\s*;", header)
    assert decl is not None
    args = " ".join(decl.group(1).split())
    assert args == ("fqlpop_t* h, int n_pairs, const int* src, const int* dst, const float* alphas, "
                    "const uint64_t* seeds")
    assert "fqlpop_clone_members" in fqlpop.EXPORTED_SYMBOLS
    lib = fqlpop.load_library()
    assert hasattr(lib, "fqlpop_clone_members")
    assert hasattr(fqlpop.Population, "clone_members") and hasattr(fqlpop.Population, "clone_member")
