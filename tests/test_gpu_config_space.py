"""The FQL update, and the forwards that read the same states, across the configuration space
fqlpop_create accepts, against the float64 oracle: depth 1-10 (every other parity test runs
four hidden layers), num_qs 1, 3 and 4 (two), head widths 1-7 and inputs from 3 to 65 rows
(5 or 8 actions, 26-42 observations), flow_steps 2 and 16 (3 or 10).  These axes select code
paths, not only sizes (tests/config_space_cases.py names what each case reaches):

1. update parity of every case from its trained-like state, at the project's bounds (REL on
   the 13 info values, MOMENT_REL of each leaf's scale on the Adam moments, the optimiser step
   and the EMA exact on the device's own state), the H = 512 depth and num_qs cases also with
   split = 0, and the plan that ran as the library reports it;
2. the state layout: no ensemble axis at num_qs = 1, leaves in sorted-name order at L = 10;
3. a population that constructs also steps: (num_qs, num_hidden) around the transpose
   launch's 32-matrix table;
4. sample_actions, act, total_loss and rollout on the same members.  No test trains.

The states' conditions (every clamp engages and also does not; each Q is the minimum in a good
share of the rows) are asserted on the CPU by tests/test_oracle.py, which also shows that a
two-Q aggregate and a layer-ordered state would move what is checked here."""
import numpy as np
import pytest

from oracle import envmodel_oracle as EO
from oracle import fql_oracle as O
from _helpers import (ROLLOUT_ENVS, ROLLOUT_STEPS, TRAINED_COUNT, action_probe, check_info,
                      device_tree, engine_options, rollout_case, trained_member)
from config_space_cases import CASES, TR_CASES, UNSPLIT_TOO, tr_spec
from test_gpu_parity_trained import _population, _run_parity, _state

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5   # sample_actions and act against the oracle, as tests/test_gpu_parity.py
FORWARD_SITES = ("bc_forward", "euler_flow", "onestep_forward", "target_critic", "critic_forward")


def _config(s0):
    from fqlpop import PopulationConfig
    return PopulationConfig(obs_dim=s0.D, action_dim=s0.A, hidden_dims=(s0.H,) * s0.L, batch_size=s0.B,
                            **dict(s0.kw))


def _parity(case, specs, tag):
    report = {}
    try:
        pop, _ = _run_parity(specs, report=report)
    finally:
        print(f"{case} {tag}: worst info error {report.get('info', float('nan')):.3g} of REL's bound, worst moment "
              f"error {report.get('moment', float('nan')):.3g} of MOMENT_REL's")
    return pop


# ------------------------------------------------------------------ 1. update parity
def _check_kernel(case, name, split=True):
    """The dominant kernel the library reports for the case."""
    if CASES[case][0].H != 512 or case in ("h512_l9", "k0_65", "k0_os65"):
        assert name.startswith("gemm_fwd"), name            # the per-layer Euler GEMMs
    elif case in ("h512_l1", "h512_l2") or not split:      # (the split Euler needs three hidden layers)
        assert name == "euler_flow_kernel", name
    else:                                                   # two members at H = 512: the split plan
        assert name.startswith("split_fwd_kernel<HEAD_EULER>"), name


@pytest.mark.parametrize("case", list(CASES))
def test_update_parity(case):
    pop = _parity(case, CASES[case], "default")
    _check_kernel(case, pop.dominant_kernel_info()[0])
    pop.close()


@pytest.mark.parametrize("case", UNSPLIT_TOO)
def test_update_parity_unsplit(case):
    """split = 0: the unsplit streamed kernels (the per-layer path at L = 9 either way)."""
    with engine_options(split=0):
        pop = _parity(case, CASES[case], "split=0")
        _check_kernel(case, pop.dominant_kernel_info()[0], split=False)
        pop.close()


def test_split_plan_at_depth_one_and_two():
    """L = 1: nothing splits.  L = 2: split backward clusters behind unsplit forwards.  L = 3:
    the forwards split too."""
    from fqlpop import split_plan
    plan = {L: split_plan(_config(CASES[f"h512_l{L}"][0]), 2) for L in (1, 2, 3)}
    assert all(plan[1][k] == 1 for k in FORWARD_SITES + ("critic_backward", "onestep_backward", "critic_backward_td"))
    assert all(plan[2][k] == 1 for k in FORWARD_SITES), plan[2]
    assert plan[2]["critic_backward"] > 1 and plan[2]["onestep_backward"] > 1, plan[2]
    assert all(plan[3][k] > 1 for k in FORWARD_SITES), plan[3]
    with engine_options(split=0):
        assert all(v == 1 for k, v in split_plan(_config(CASES["h512_l3"][0]), 2).items() if k != "small_sched")


# ------------------------------------------------------------------ 2. state layout
@pytest.mark.parametrize("case", ["h512_e1", "h64_e1", "h512_e3_min", "h512_e4", "h64_e4_min"])
def test_critic_leaves_ensemble_axis(case):
    """The critic's leaves are [E, ...] at E > 1 and have no ensemble axis at E = 1, where the
    oracle keeps [1, ...] (device_tree squeezes it); the actors' never have one."""
    from fqlpop import Population
    s = CASES[case][0]
    E, cfg = dict(s.kw)["num_qs"], s.cfg()
    pop = Population(_config(s), [1.0], [0])
    want = O.init_params(cfg, 0)
    for name, _, shape in pop.leaves:
        net, leaf = name.split("/", 1)
        oshape = want[net][leaf].shape
        if net in ("critic", "target_critic"):
            assert oshape[0] == E and shape == (oshape if E > 1 else oshape[1:]), (name, shape, oshape)
        else:
            assert shape == oshape, (name, shape, oshape)
    assert sum(int(np.prod(shape)) for _, _, shape in pop.leaves) == pop.state_size
    tree = device_tree(pop, O.cast_tree(trained_member(s).params, np.float32))
    pop.set_params(0, tree)
    back = pop.get_params(0)
    for net in O.NETS:
        for k, v in tree[net].items():
            assert np.array_equal(back[net][k], v), (net, k)
    pop.close()


def test_leaf_order_at_ten_layers():
    """Leaves are in sorted-name order, Dense_10 before Dense_2, and every leaf round-trips
    bitwise through set_params / get_params to its own place in the flat state."""
    from fqlpop import Population
    s = CASES["h64_l10"][0]
    pop = Population(_config(s), [1.0], [0])
    names = [n for n, _, _ in pop.leaves]
    assert names == [f"{net}/{k}" for net in sorted(O.NETS) for k in O.leaf_order(s.cfg(), net)]
    for net in O.NETS:
        assert names.index(f"{net}/Dense_10/kernel") < names.index(f"{net}/Dense_2/kernel")
    off = 0
    for _, o, shape in pop.leaves:   # contiguous, in that order
        assert o == off
        off += int(np.prod(shape))
    rng = np.random.default_rng(3)
    tree = {}
    for name, _, shape in pop.leaves:
        net, leaf = name.split("/", 1)
        tree.setdefault(net, {})[leaf] = rng.standard_normal(shape).astype(np.float32)
    pop.set_params(0, tree)
    flat = pop.get_flat(0)
    for name, o, shape in pop.leaves:
        net, leaf = name.split("/", 1)
        assert np.array_equal(flat[o:o + int(np.prod(shape))], tree[net][leaf].reshape(-1)), name
    back = pop.get_params(0)
    assert all(np.array_equal(back[net][k], v) for net in tree for k, v in tree[net].items())
    pop.close()


# ------------------------------------------------------------------ 3. accept or refuse, never later
@pytest.mark.parametrize("num_qs,num_hidden", TR_CASES)
def test_accepted_population_steps(num_qs, num_hidden):
    """(E + 2) * (L - 1) hidden kernels have W^T copies: 42, 36 and 35 of them are more than one
    transpose launch's table of 32 holds, 30 fit.  A population fqlpop_create accepts takes its
    first step after a host-side parameter write, at parity; or it is refused at construction."""
    from fqlpop import FqlpopError, Population
    spec = tr_spec(num_qs, num_hidden)
    try:
        Population(_config(spec), [spec.alpha], [11]).close()
    except FqlpopError as e:
        assert (num_qs, num_hidden) != (4, 6), "this population worked before"
        assert "num_qs" in str(e) and "num_hidden" in str(e), e
        return
    _parity(f"tr_e{num_qs}_l{num_hidden}", (spec,), "default").close()


# ------------------------------------------------------------------ 4. forwards on the same states
@pytest.mark.parametrize("case", ["h512_l1", "h512_l9", "h64_l10", "a1", "d2_a2"])
def test_sample_actions_parity(case):
    for spec in CASES[case]:
        pop = _population((spec,))
        tm = trained_member(spec)
        obs, z = action_probe(spec)
        got = pop.sample_actions(0, obs, noise=z)
        want = O.sample_actions(tm.cfg, tm.params, obs.astype(np.float64), z.astype(np.float64))
        print(f"{case} seed {spec.seed}: max |a - oracle| = {float(np.abs(got - want).max()):.3g}")
        assert got.shape == want.shape and np.all(np.abs(got) <= 1.0)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        pop.close()


def _act_inputs(specs, n_envs):
    rng = np.random.default_rng([specs[0].seed, 3, n_envs])
    return (rng.standard_normal((len(specs), n_envs, specs[0].D)).astype(np.float32),
            rng.standard_normal((len(specs), n_envs, specs[0].A)).astype(np.float32))


@pytest.mark.parametrize("case", ["h512_l1", "h512_l9", "a1", "k0_64"])
def test_act_parity(case):
    specs = CASES[case]
    pop = _population(specs)
    for n_envs in (1, 17):
        obs, z = _act_inputs(specs, n_envs)
        got = pop.act(obs, noise=z)
        want = np.stack([O.sample_actions(tm.cfg, tm.params, obs[i].astype(np.float64), z[i].astype(np.float64))
                         for i, tm in enumerate(map(trained_member, specs))])
        print(f"{case} n_envs={n_envs}: max |act - oracle| = {float(np.abs(got - want).max()):.3g}")
        assert got.shape == want.shape and np.all(np.abs(got) <= 1.0)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    pop.close()


def test_act_refuses_a_wide_input():
    """obs_dim + action_dim = 65: trains (test_update_parity[k0_os65]), act is unsupported."""
    from fqlpop import FqlpopError
    specs = CASES["k0_os65"]
    pop = _population(specs)
    obs, z = _act_inputs(specs, 4)
    with pytest.raises(FqlpopError, match="error -4:"):
        pop.act(obs, noise=z)
    pop.close()


@pytest.mark.parametrize("case", ["h512_l2", "h512_e4_min", "h64_e1"])
def test_total_loss_parity(case):
    specs = CASES[case]
    pop = _population(specs)
    members = [trained_member(s) for s in specs]
    before = _state(pop)
    info = pop.total_loss([O.cast_tree(tm.batches[0], np.float32) for tm in members],
                          [O.cast_tree(tm.noises[0], np.float32) for tm in members])
    for i, tm in enumerate(members):
        _, want = O.total_loss(tm.cfg, tm.params, tm.batches[0], tm.noises[0])
        check_info(info[i], want, O.VAL_INFO_KEYS, f"val {case} member {i}")
        assert pop.get_count(i) == TRAINED_COUNT
    for a, b in zip(_state(pop), before):
        assert np.array_equal(a, b)
    pop.close()


def _with_env_model(specs):
    import envmodel as em
    pop = _population(specs)
    spec, sp, tp, obs0, noise = rollout_case()
    pop.set_env_model(em.flatten_state_predictor(spec, sp), em.flatten_termination_predictor(spec, tp),
                      spec.sp_hidden, spec.tp_hidden)
    return pop, sp, tp, obs0, noise


@pytest.mark.parametrize("case", ["h512_l1", "h512_l8"])
def test_rollout_parity(case):
    """The rollout kernel at the two ends of the depths it serves (12 envs, 4 steps)."""
    specs = CASES[case]
    pop, sp, tp, obs0, noise = _with_env_model(specs)
    assert noise.shape[:3] == (len(specs), ROLLOUT_STEPS, ROLLOUT_ENVS)
    succ, length, oobs = pop.rollout(obs0, ROLLOUT_STEPS, noise=noise, return_obs=True)[:3]
    for i, s in enumerate(specs):
        tm = trained_member(s)
        want = EO.rollout(tm.cfg, tm.params, sp, tp, obs0.astype(np.float64), noise[i].astype(np.float64),
                          ROLLOUT_STEPS)
        np.testing.assert_array_equal(succ[i], want[0])
        np.testing.assert_array_equal(length[i], want[1])
        print(f"{case} member {i}: max |obs - oracle| = {float(np.abs(oobs[i] - want[2]).max()):.3g}")
        np.testing.assert_allclose(oobs[i], want[2], rtol=2e-3, atol=2e-4)
    pop.close()


def test_rollout_refuses_nine_layers():
    from fqlpop import FqlpopError
    pop, _, _, obs0, noise = _with_env_model(CASES["h512_l9"])
    with pytest.raises(FqlpopError, match="512, num_hidden <= 8"):
        pop.rollout(obs0, ROLLOUT_STEPS, noise=noise)
    pop.close()


def test_sixteen_layers_are_refused_at_construction():
    """8 L + 6 trainable leaves: the optimiser's table of 128 holds 15 hidden layers."""
    from fqlpop import FqlpopError, Population, PopulationConfig
    with pytest.raises(FqlpopError, match="error -1:.*too many leaves"):
        Population(PopulationConfig(hidden_dims=(64,) * 16, batch_size=64), [1.0], [0])
    Population(PopulationConfig(hidden_dims=(64,) * 15, batch_size=64), [1.0], [0]).close()
