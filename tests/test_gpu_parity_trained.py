"""HIP path vs the float64 oracle from a TRAINED-LIKE state (oracle.fql_oracle.
trained_like_params / trained_like_opt_state), where tests/test_gpu_parity.py starts
from the initial one.

At the initial state every Dense bias and LayerNorm bias is 0, every LayerNorm scale 1,
target_critic == critic, the Adam moments are 0 and no actor output comes near +-1, so a
kernel that drops or mis-indexes one of those terms, evaluates the TD target with the online
critic, lets the Q gradient through a saturated clip, clamps at the wrong place or mishandles
non-zero moments computes exactly what a correct one does.  Here all of these are random per
member and per ensemble member, 15-85 % of what each clamp sees lies outside [-1, 1], and
Adam continues from count 1000 (tests/_helpers.py: TRAINED; tests/test_oracle.py asserts the
conditions on the CPU and that each such mistake moves a checked quantity by 10x its bound).

Same bounds as from the initial state: info values within REL = 1e-4, Adam moments within
MOMENT_REL of each leaf's scale, the optimiser step and the EMA exact on the device's own
state (tests/_helpers.OptimiserChecker)."""
import numpy as np
import pytest

from oracle import envmodel_oracle as EO
from oracle import fql_oracle as O
from _helpers import (ACTION_SPECS, ROLLOUT_SPECS, ROLLOUT_STEPS, TRAINED, TRAINED_COUNT,
                      OptimiserChecker, action_probe, check_info, close, device_tree, engine_options, info_ratio,
                      rollout_case, rollout_raw_actions, saturated_share, synthetic_rows, trained_member)

pytestmark = pytest.mark.gpu


def _population(specs, use_graph=True):
    """A population of ``specs`` (one configuration) at their trained-like states: params,
    Adam m and v and the count uploaded, a different state per member."""
    from fqlpop import Population, PopulationConfig
    from fqlpop._lib import STATE_ADAM_M, STATE_ADAM_V
    s0 = specs[0]
    assert all((s.H, s.L, s.B, s.D, s.A, s.kw, s.n_steps) == (s0.H, s0.L, s0.B, s0.D, s0.A, s0.kw, s0.n_steps)
               for s in specs)
    assert len({s.seed for s in specs}) == len(specs)
    pc = PopulationConfig(obs_dim=s0.D, action_dim=s0.A, hidden_dims=(s0.H,) * s0.L, batch_size=s0.B,
                          use_graph=use_graph, **dict(s0.kw))
    seeds = [s.sampled[0] if s.sampled else 11 + i for i, s in enumerate(specs)]
    pop = Population(pc, [s.alpha for s in specs], seeds)
    for i, s in enumerate(specs):
        tm = trained_member(s)
        pop.set_params(i, device_tree(pop, O.cast_tree(tm.params, np.float32)))
        pop.set_flat(i, pop.tree_to_flat(device_tree(pop, tm.opt["m"])), STATE_ADAM_M)
        pop.set_flat(i, pop.tree_to_flat(device_tree(pop, tm.opt["v"])), STATE_ADAM_V)
        pop.set_count(i, TRAINED_COUNT)
    return pop


def _state(pop):
    return [pop.get_flat(i, w) for i in range(pop.n) for w in (0, 1, 2)]


def _run_parity(specs, use_graph=True, report=None):
    """Step ``specs`` from their trained-like states on the oracle's batches and noises
    (injected, or for a sampled Spec drawn by the device sampler from the dataset) and check
    every step of every member against the oracle.  Returns (population, info of the last
    step).  ``report``: a dict that receives the worst info and moment errors as fractions of
    REL's and MOMENT_REL's bounds, before anything is asserted."""
    pop = _population(specs, use_graph)
    members = [trained_member(s) for s in specs]
    sampled = bool(specs[0].sampled)
    if sampled:
        pop.set_dataset(synthetic_rows(specs[0].sampled[1], specs[0].D, specs[0].A, 5))
    checks = [OptimiserChecker(pop, i, tm.cfg.lr, tm.cfg.tau) for i, tm in enumerate(members)]
    info = None
    if report is None:
        report = {}
    report.update(info=0.0, moment=0.0)
    errors = []
    for step in range(specs[0].n_steps):
        for c in checks:
            c.before()
        if sampled:
            pop.step(1)
        else:
            pop.step_injected([O.cast_tree(tm.batches[step], np.float32) for tm in members],
                              [O.cast_tree(tm.noises[step], np.float32) for tm in members])
        info = pop.read_info("train")
        for i, tm in enumerate(members):
            params_o, opt_o, info_o = tm.steps[step]
            tag = f"{specs[i]} step {step} member {i}"
            report["info"] = max(report["info"], info_ratio(info[i], info_o, O.TRAIN_INFO_KEYS))
            for check in (lambda: check_info(info[i], info_o, O.TRAIN_INFO_KEYS, tag),
                          lambda: checks[i].after(params_o, opt_o, step + 1, tag)):
                try:   # every member is measured before the first miss is raised
                    check()
                except AssertionError as e:
                    errors.append(str(e))
            report["moment"] = max(report["moment"], checks[i].worst_moment)
        assert not errors, "\n".join(errors)
    for i in range(len(specs)):
        assert pop.get_count(i) == TRAINED_COUNT + specs[0].n_steps
    return pop, info


@pytest.mark.parametrize("use_graph", [False, True])
def test_update_parity_small(use_graph):
    """H = 64: the per-layer GEMM epilogues, head_write, the loss kernels, unfused Adam."""
    _run_parity(TRAINED["h64"], use_graph=use_graph)[0].close()


@pytest.mark.parametrize("name", ["h128_no_ln", "h1024"])
def test_update_parity_per_layer_widths(name):
    """The per-layer path without the critic's LayerNorm, and the widest hidden size."""
    _run_parity(TRAINED[name])[0].close()


def test_update_parity_unsplit_streamed():
    """H = 512, three members, split = 0: the streamed forward and backward, the persistent
    Euler kernel, and the fused dW + Adam epilogue continuing from non-zero moments."""
    with engine_options(split=0):
        pop, _ = _run_parity(TRAINED["h512"])
        assert pop.dominant_kernel_info()[0] == "euler_flow_kernel"
        pop.close()


@pytest.mark.parametrize("n", [1, 2])
def test_update_parity_split_auto(n):
    """H = 512 at the default options: one and two members run the split forward, Euler
    and backward clusters."""
    pop, _ = _run_parity(TRAINED["h512"][:n])
    assert pop.dominant_kernel_info()[0].startswith("split_fwd_kernel")
    pop.close()


@pytest.mark.parametrize("option", ["euler_fused", "stream_fwd", "stream_bwd", "fused_adam"])
def test_update_parity_fallbacks(option):
    """Each fallback of the H = 512 path, switched on alone, against the oracle."""
    with engine_options(**{option: 0}):
        _run_parity(TRAINED["h512"][:2])[0].close()


@pytest.mark.parametrize("name", ["h512_d27", "h512_d42"])
def test_update_parity_layer0_and_tiles(name):
    """(obs, act) = (27, 5): the layer-0 tail k-step; (42, 8): two ring passes; B = 192: an
    odd number of 64-row tiles."""
    _run_parity(TRAINED[name])[0].close()


@pytest.mark.parametrize("name", ["h64_min", "h512_min"])
def test_update_parity_q_min_normalized(name):
    """q_agg = min where each ensemble member is the minimum in a good share of the rows,
    and normalize_q_loss with Q of mixed signs (lambda != 1 / |mean Q|)."""
    _run_parity(TRAINED[name])[0].close()


def test_production_step_at_large_count():
    """fqlpop_step on a dataset from count 1000: the device sampler keyed by that count
    (tests/philox_np.draw(key, 1000, ...)), then the same check as the injected steps."""
    _run_parity(TRAINED["h512_sampled"])[0].close()


@pytest.mark.parametrize("name", ["h64", "h512"])
def test_total_loss_parity(name):
    """The validation path on the first step's batch; it leaves params, moments and count
    as they were."""
    specs = TRAINED[name][:2]
    pop = _population(specs)
    members = [trained_member(s) for s in specs]
    before = _state(pop)
    info = pop.total_loss([O.cast_tree(tm.batches[0], np.float32) for tm in members],
                          [O.cast_tree(tm.noises[0], np.float32) for tm in members])
    for i, tm in enumerate(members):
        # the update's first ten info values are total_loss's (tests/test_oracle.py)
        check_info(info[i], tm.steps[0][2], O.VAL_INFO_KEYS, f"val {specs[i]}")
        assert pop.get_count(i) == TRAINED_COUNT
    for a, b in zip(_state(pop), before):
        assert np.array_equal(a, b)
    pop.close()


@pytest.mark.parametrize("spec", ACTION_SPECS, ids=lambda s: f"h{s.H}")
def test_sample_actions_parity(spec):
    """HEAD_ACT's clamp: the share of saturated outputs is the oracle's (15-85 %)."""
    pop = _population((spec,))
    tm = trained_member(spec)
    obs, z = action_probe(spec)
    got = pop.sample_actions(0, obs, noise=z)
    raw = O.sample_actions(tm.cfg, tm.params, obs.astype(np.float64), z.astype(np.float64), clip=False)
    assert np.allclose(got, np.clip(raw, -1.0, 1.0), rtol=1e-4, atol=1e-5)
    assert np.all(np.abs(got) <= 1.0)
    assert np.array_equal(np.abs(got) == 1.0, np.abs(raw) > 1.0)
    assert 0.15 <= saturated_share(raw) <= 0.85
    pop.close()


def test_rollout_matches_oracle():
    """The rollout kernel reads the one-step actor's biases and clamps its head on every
    step: trajectories and recorded actions against the oracle's."""
    import envmodel as em
    pop = _population(ROLLOUT_SPECS)
    spec, sp, tp, obs0, noise = rollout_case()
    pop.set_env_model(em.flatten_state_predictor(spec, sp), em.flatten_termination_predictor(spec, tp),
                      spec.sp_hidden, spec.tp_hidden)
    succ, length, oobs, _, tact = pop.rollout(obs0, ROLLOUT_STEPS, noise=noise, return_obs=True, record=True)
    for i, s in enumerate(ROLLOUT_SPECS):
        tm = trained_member(s)
        want = EO.rollout(tm.cfg, tm.params, sp, tp, obs0.astype(np.float64), noise[i].astype(np.float64),
                          ROLLOUT_STEPS)
        np.testing.assert_array_equal(succ[i], want[0])
        np.testing.assert_array_equal(length[i], want[1])
        np.testing.assert_allclose(oobs[i], want[2], rtol=2e-3, atol=2e-4)
        raw = rollout_raw_actions(i)
        np.testing.assert_allclose(tact[i], np.clip(raw, -1.0, 1.0), rtol=2e-3, atol=2e-4)
        assert np.array_equal(np.abs(tact[i]) == 1.0, np.abs(raw) > 1.0)
    pop.close()


# ---- GPU-vs-GPU identities from the trained-like state (tests/test_gpu_split.py and
# tests/test_gpu_parity.py assert them from the device init, where every bias is 0) ----
def _stepped(specs, opts):
    with engine_options(**opts):
        pop, info = _run_parity(specs)
        out = (_state(pop), info, pop.dominant_kernel_info()[0])
        pop.close()
    return out


@pytest.mark.parametrize("n", [1, 2])
def test_split_bit_identical_to_unsplit(n):
    specs = TRAINED["h512"][:n]
    ref = _stepped(specs, {"split": 0})
    assert ref[2] == "euler_flow_kernel"
    for F in (8, 4, 2):
        got = _stepped(specs, {"split": F})
        assert got[2].startswith("split_fwd_kernel"), got[2]
        assert got[1] == ref[1], f"split {F}: info differs"
        for j, (a, b) in enumerate(zip(got[0], ref[0])):
            assert np.array_equal(a, b), f"split {F}: state {j} differs (max |d| {np.abs(a - b).max()})"


def test_fused_dw_optimiser_tile_variants_bit_identical():
    specs = TRAINED["h512"][:2]
    ref = _stepped(specs, {"dw_tile_critic": 6, "dw_tile_actor": 6})
    got = _stepped(specs, {})
    assert got[1] == ref[1]
    for a, b in zip(got[0], ref[0]):
        assert np.array_equal(a, b)


def test_euler_fused_matches_per_layer_path():
    """As tests/test_gpu_parity.py's test of that name: equal to within fp32 reassociation."""
    specs = TRAINED["h512"][:1]
    a, b = _stepped(specs, {"euler_fused": 1})[1], _stepped(specs, {"euler_fused": 0})[1]
    for k in O.TRAIN_INFO_KEYS:
        assert close(a[0][k], b[0][k], rel=2e-5), (k, a[0][k], b[0][k])
