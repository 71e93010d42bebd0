"""``Population.act`` (fqlpop_act, act_kernel): every active member's one-step policy on its own
observations in one launch, against the float64 oracle (tests/act_np.py) at the project's
``sample_actions`` tolerance, against the old per-member path, and against the rollout
evaluator's policy.  Populations are trained-like members uploaded with ``set_params``; no
test here trains.
"""
from __future__ import annotations

import numpy as np
import pytest

import act_np as N
from _helpers import ROLLOUT_SPECS, ROLLOUT_STEPS, device_tree, rollout_case, trained_member
from oracle import fql_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5   # sample_actions against the oracle, as tests/test_gpu_parity.py


def _population(specs, seeds=None):
    """One member per spec (one configuration), its trained-like parameters uploaded."""
    from fqlpop import Population, PopulationConfig
    s0 = specs[0]
    pc = PopulationConfig(obs_dim=s0.D, action_dim=s0.A, hidden_dims=(s0.H,) * s0.L, batch_size=s0.B, **dict(s0.kw))
    pop = Population(pc, [s.alpha for s in specs], list(seeds or [11 + i for i in range(len(specs))]))
    for i, s in enumerate(specs):
        pop.set_params(i, device_tree(pop, O.cast_tree(trained_member(s).params, np.float32)))
    return pop


def _check_against_raw(got, raw, tag):
    want = np.clip(raw, -1.0, 1.0)
    err = np.abs(got - want)
    print(f"{tag}: max |act - oracle| = {float(err.max()):.3g}")
    assert np.all(np.abs(got) <= 1.0), tag
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=tag)
    assert np.array_equal(np.abs(got) == 1.0, np.abs(raw) > 1.0), f"{tag}: clamp decisions differ"


@pytest.mark.parametrize("group", N.PARITY_GROUPS)
def test_act_parity_injected(group):
    """Injected z: every member of the group, at 1, 17 and 50 envs, against the oracle."""
    specs = N.GROUPS[group][:2]
    pop = _population(specs)
    for n_envs in N.N_ENVS:
        obs, noise, raw = N.group_inputs(group, n_envs, range(len(specs)))
        got = pop.act(obs, noise=noise)
        assert got.shape == (len(specs), n_envs, specs[0].A) and got.dtype == np.float32
        _check_against_raw(got, raw, f"{group} n_envs={n_envs}")
    pop.close()


def test_act_parity_depth_two():
    """hidden_dims (64, 64): one streamed hidden layer after layer 0, oracle-initialised."""
    from fqlpop import Population, PopulationConfig
    cfg = O.OracleConfig(obs_dim=28, action_dim=5, hidden_dims=(64, 64), batch_size=64)
    params = [O.cast_tree(O.init_params(cfg, 20 + i), np.float32) for i in range(2)]
    pop = Population(PopulationConfig(obs_dim=28, action_dim=5, hidden_dims=(64, 64), batch_size=64), [3.0, 30.0], [1, 2])
    for i, p in enumerate(params):
        pop.set_params(i, p)
    rng = np.random.default_rng(5)
    for n_envs in N.N_ENVS:
        obs = rng.standard_normal((2, n_envs, 28)).astype(np.float32)
        z = rng.standard_normal((2, n_envs, 5)).astype(np.float32)
        got = pop.act(obs, noise=z)
        want = np.stack([O.sample_actions(cfg, O.cast_tree(params[i], np.float64), obs[i].astype(np.float64),
                                          z[i].astype(np.float64)) for i in range(2)])
        print(f"depth 2 n_envs={n_envs}: max err {float(np.abs(got - want).max()):.3g}")
        assert np.all(np.abs(got) <= 1.0)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    pop.close()


def test_act_slot_indirection():
    """Three members, the middle one inactive: row z is slot active_ids[z]'s action on its own
    observations, bitwise what that member gives as the only active one."""
    specs = N.GROUPS["h512"]
    pop = _population(specs)
    n_envs = 17
    obs, noise, raw = N.group_inputs("h512", n_envs)
    pop.set_active([True, False, True])
    assert pop.active_ids == [0, 2]
    got = pop.act(obs[[0, 2]], noise=noise[[0, 2]])
    assert got.shape == (2, n_envs, specs[0].A)
    _check_against_raw(got, raw[[0, 2]], "slots 0, 2")
    for z, m in enumerate((0, 2)):
        only = [i == m for i in range(3)]
        pop.set_active(only)
        alone = pop.act(obs[[m]], noise=noise[[m]])
        assert np.array_equal(alone[0], got[z]), f"slot {m} alone differs from its row {z}"
    pop.close()


@pytest.mark.parametrize("group", ("h64", "h512", "h512_d42"))
def test_act_agrees_with_sample_actions(group):
    """The per-member path on the same z (another summation order: close, not bitwise)."""
    specs = N.GROUPS[group][:2]
    pop = _population(specs)
    obs, noise, _ = N.group_inputs(group, 50, range(len(specs)))
    got = pop.act(obs, noise=noise)
    for m in range(len(specs)):
        old = pop.sample_actions(m, obs[m], noise=noise[m])
        print(f"{group} member {m}: max |act - sample_actions| = {float(np.abs(got[m] - old).max()):.3g}")
        np.testing.assert_allclose(got[m], old, rtol=RTOL, atol=ATOL)
    pop.close()


@pytest.mark.parametrize("group", ("h512", "h512_d42"), ids=("A5", "A8"))
def test_act_device_noise(group):
    """noise=None: the z is rollout_kernel's draw at step t under the member's key, and the
    actions are those of the same z injected."""
    specs = N.GROUPS[group][:2]
    pop = _population(specs)
    n_envs, seed, t = 17, 1234, 3
    obs, _, _ = N.group_inputs(group, n_envs, range(len(specs)))
    a, z = pop.act(obs, seed=seed, t=t, return_noise=True)
    assert np.array_equal(pop.act(obs, noise=z), a)
    for m, s in enumerate(specs):
        want = N.device_noise(seed, int(pop.seeds[m]), float(pop.alphas[m]), n_envs, t, s.A)
        err = float(np.abs(z[m] - want).max())
        print(f"{group} member {m}: max |z - rollout_noise| = {err:.3g}")
        assert err <= 1e-3
    a2, z2 = pop.act(obs, seed=seed, t=t, return_noise=True)
    assert np.array_equal(a2, a) and np.array_equal(z2, z)
    a3, z3 = pop.act(obs, seed=seed, t=t + 1, return_noise=True)
    assert not np.array_equal(z3, z) and not np.array_equal(a3, a)
    pop.close()


def test_act_is_the_evaluators_policy():
    """Along a recorded world-model rollout with device noise, ``act`` on the recorded
    observation of step t at (seed, t + 1) gives the action the rollout took there."""
    import envmodel as em
    pop = _population(ROLLOUT_SPECS)
    spec, sp, tp, obs0, _ = rollout_case()
    pop.set_env_model(em.flatten_state_predictor(spec, sp), em.flatten_termination_predictor(spec, tp),
                      spec.sp_hidden, spec.tp_hidden)
    seed = 77
    _, length, tobs, tact = pop.rollout(obs0, ROLLOUT_STEPS, seed=seed, record=True)
    assert np.all(length == ROLLOUT_STEPS)  # (the case's env model never terminates)
    for t in range(ROLLOUT_STEPS):
        got = pop.act(tobs[:, t], seed=seed, t=t + 1)
        print(f"step {t}: max |act - rollout action| = {float(np.abs(got - tact[:, t]).max()):.3g}")
        np.testing.assert_allclose(got, tact[:, t], rtol=RTOL, atol=ATOL)
    pop.close()


def test_act_refusals():
    from fqlpop import FqlpopError, Population, PopulationConfig
    pop = _population(N.GROUPS["h64"][:1])
    obs, noise, _ = N.group_inputs("h64", 4, [0])
    with pytest.raises(FqlpopError, match="error -1:"):
        pop.act(obs, seed=1, t=0)                       # device noise counts steps from 1
    assert pop.act(obs, noise=noise, t=0).shape == (1, 4, 5)   # (t is not read with injected z)
    with pytest.raises(FqlpopError, match="error -1:"):
        pop.act(np.zeros((1, 0, 28), np.float32), noise=np.zeros((1, 0, 5), np.float32))
    pop.set_active([False])
    assert pop.act(np.zeros((0, 4, 28), np.float32)).shape == (0, 4, 5)   # no active member: nothing to do
    pop.close()
    wide = Population(PopulationConfig(obs_dim=60, action_dim=5, hidden_dims=(64,) * 4, batch_size=64), [10.0], [1])
    with pytest.raises(FqlpopError, match="error -4:"):
        wide.act(np.zeros((1, 4, 60), np.float32), noise=np.zeros((1, 4, 5), np.float32))
    wide.close()
