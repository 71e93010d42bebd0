"""World-model ensembles on the GPU (fqlpop_set_env_model_ensemble,
fqlpop_rollout_ensemble): the per-model mode against K single-model rollouts bit for bit,
the mixed mode (a model per env and step) against a float64 composition of the oracles, the
device's model draw against its NumPy restatement, and the simulated task scoring
candidates under an ensemble."""
import csv

import numpy as np
import pytest

import envmodel as em
from oracle import envmodel_oracle as EO
from oracle import fql_oracle as O

pytestmark = pytest.mark.gpu
H = 512  # the rollout kernels stream the 512-wide actor
SPEC = em.EnvModelSpec(28, 5, (64, 128), (64,))
MODEL_SEEDS = (11, 12, 13)
N_ENVS, STEPS = 20, 12  # one full 16-env tile plus a 4-env tile


def _population(n, obs_dim=28, act_dim=5, seed=0):
    from fqlpop import Population, PopulationConfig
    pop = Population(PopulationConfig(obs_dim=obs_dim, action_dim=act_dim, hidden_dims=(H,) * 4, batch_size=64),
                     [10.0] * n, list(range(1, n + 1)))
    cfg = O.OracleConfig(obs_dim=obs_dim, action_dim=act_dim, hidden_dims=(H,) * 4, batch_size=64)
    params = []
    for i in range(n):
        p = O.cast_tree(O.init_params(cfg, seed + i), np.float32)
        pop.set_params(i, p)
        params.append(O.cast_tree(p, np.float64))
    return pop, cfg, params


def _env_model(spec, tp_bias=0.0, tp_scale=1.0, seed=0):
    sp = em.init_state_predictor(spec, seed)
    for k in sp:  # non-trivial LayerNorm parameters
        if k.startswith("LayerNorm"):
            rng = np.random.default_rng(seed + 7)
            sp[k]["scale"] = (1.0 + 0.2 * rng.standard_normal(sp[k]["scale"].shape)).astype(np.float32)
            sp[k]["bias"] = (0.1 * rng.standard_normal(sp[k]["bias"].shape)).astype(np.float32)
    tp = em.init_termination_predictor(spec, seed + 1, scale=tp_scale, bias=tp_bias)
    return sp, tp


def _models(tp_bias, tp_scale):
    return [_env_model(SPEC, tp_bias, tp_scale, seed=s) for s in MODEL_SEEDS]


def _set_single(pop, model):
    pop.set_env_model(em.flatten_state_predictor(SPEC, model[0]), em.flatten_termination_predictor(SPEC, model[1]),
                      SPEC.sp_hidden, SPEC.tp_hidden)


def _set_ensemble(pop, models):
    pop.set_env_model_ensemble([em.flatten_state_predictor(SPEC, sp) for sp, _ in models],
                               [em.flatten_termination_predictor(SPEC, tp) for _, tp in models],
                               SPEC.sp_hidden, SPEC.tp_hidden)


def _inputs():
    """The issue's construction: obs0, then the noise, then the choices from default_rng(5)."""
    rng = np.random.default_rng(5)
    obs0 = rng.standard_normal((N_ENVS, 28)).astype(np.float32)
    noise = rng.standard_normal((2, STEPS, N_ENVS, 5)).astype(np.float32)
    choice = rng.integers(0, 3, (STEPS, N_ENVS)).astype(np.int32)
    choice[2, :16] = 1  # a tile-step on which all 16 columns agree: two models skipped
    return obs0, noise, choice


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    c.pop, c.cfg, c.params = _population(2)
    c.quiet = _models(-50.0, 0.1)   # nothing terminates
    c.term = _models(-12.0, 1.0)    # some episodes terminate
    c.obs0, c.noise, c.choice = _inputs()
    yield c
    c.pop.close()


# ------------------------------------------------------------------ 1. per-model
@pytest.mark.parametrize("which", ["quiet", "term"])
@pytest.mark.parametrize("device_noise", [False, True])
def test_per_model_equals_single_model_rollouts_bitwise(ctx, which, device_noise):
    models = getattr(ctx, which)
    kw = dict(seed=7) if device_noise else dict(noise=ctx.noise)
    _set_ensemble(ctx.pop, models)
    succ, length, oobs = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, mode="per_model", return_obs=True, **kw)
    assert succ.shape == (2, 3, N_ENVS) and oobs.shape == (2, 3, N_ENVS, 28)
    for k, model in enumerate(models):
        _set_single(ctx.pop, model)
        s, l, o = ctx.pop.rollout(ctx.obs0, STEPS, return_obs=True, **kw)
        np.testing.assert_array_equal(succ[:, k], s, err_msg=f"model {k}")
        np.testing.assert_array_equal(length[:, k], l, err_msg=f"model {k}")
        np.testing.assert_array_equal(oobs[:, k], o, err_msg=f"model {k}")
    if which == "quiet":
        assert succ.sum() == 0 and (length == STEPS).all()
    else:
        assert 0 < succ.mean() < 1
    assert not np.array_equal(oobs[:, 0], oobs[:, 1])  # the models differ
    assert ctx.pop.ensemble_kernel_us() > 0


# --------------------------------------------------------------- 2. mixed, oracle
def _mixed_oracle(cfg, params, models, obs0, noise, choice, steps):
    """One member in float64: env e steps under models[choice[t - 1, e]] at step t; a done
    env keeps its observation.  Returns (success, length, final obs, min |logit| over
    every live env at every step)."""
    obs = obs0.astype(np.float64)
    n = obs.shape[0]
    done = np.zeros(n, bool)
    success, length = np.zeros(n), np.zeros(n)
    margin = np.inf
    for t in range(1, steps + 1):
        a = O.sample_actions(cfg, params, obs, noise[t - 1].astype(np.float64))
        nxt, logit = np.zeros_like(obs), np.zeros(n)
        for k, (sp, tp) in enumerate(models):
            m = choice[t - 1] == k
            if m.any():
                nxt[m] = EO.state_predictor(sp, obs[m], a[m])
                logit[m] = EO.termination_predictor(tp, nxt[m])
        live = ~done
        margin = min(margin, float(np.abs(logit[live]).min()))
        term = logit > 0
        new = live & (term | (t >= steps))
        success[live & term] = 1.0
        length[new] = t
        obs = np.where(live[:, None], nxt, obs)
        done |= new
        if done.all():
            break
    return success, length, obs, margin


def _tile_steps(choice):
    """The model sets of the full tile's steps and of the partial tile's."""
    return [set(r[:16].tolist()) for r in choice], [set(r[16:].tolist()) for r in choice]


def test_choices_cover_the_kernel_paths(ctx):
    full, part = _tile_steps(ctx.choice)
    assert any(s == {0, 1, 2} for s in full)   # all three chains in one tile-step
    assert any(len(s) == 1 for s in full)       # all 16 agree: the skip path
    assert any(len(s) > 1 for s in part)        # the partial tile mixes too
    assert set(np.unique(ctx.choice)) == {0, 1, 2}


def test_mixed_matches_oracle_without_terminations(ctx):
    steps = 6
    _set_ensemble(ctx.pop, ctx.quiet)
    succ, length, oobs = ctx.pop.rollout_ensemble(ctx.obs0, steps, mode="mixed", noise=ctx.noise[:, :steps],
                                                  choice=ctx.choice[:steps], return_obs=True)
    assert succ.shape == (2, N_ENVS)
    for i in range(2):
        s, l, obs, _ = _mixed_oracle(ctx.cfg, ctx.params[i], ctx.quiet, ctx.obs0, ctx.noise[i], ctx.choice, steps)
        assert s.sum() == 0 and (l == steps).all()
        np.testing.assert_array_equal(succ[i], s)
        np.testing.assert_array_equal(length[i], l)
        np.testing.assert_allclose(oobs[i], obs, rtol=2e-3, atol=2e-4)


def test_mixed_terminations_match_oracle(ctx):
    _set_ensemble(ctx.pop, ctx.term)
    succ, length = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, mode="mixed", noise=ctx.noise, choice=ctx.choice)
    want_succ = []
    for i in range(2):
        s, l, _, margin = _mixed_oracle(ctx.cfg, ctx.params[i], ctx.term, ctx.obs0, ctx.noise[i], ctx.choice, STEPS)
        # the float32 drift after 12 steps is bounded by the 2e-3 observation tolerance: no flag can flip
        assert margin >= 0.1, margin
        np.testing.assert_array_equal(succ[i], s, err_msg=f"member {i}")
        np.testing.assert_array_equal(length[i], l, err_msg=f"member {i}")
        want_succ.append(s)
    assert 0 < np.mean(want_succ) < 1  # both outcomes occur


# ------------------------------------------------------------- 3. exact selection
@pytest.mark.parametrize("which", ["quiet", "term"])
def test_mixed_with_a_constant_choice_is_that_models_slice(ctx, which):
    _set_ensemble(ctx.pop, getattr(ctx, which))
    ps, pl, po = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, mode="per_model", noise=ctx.noise, return_obs=True)
    for k in range(3):
        ms, ml, mo = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, mode="mixed", noise=ctx.noise,
                                              choice=np.full((STEPS, N_ENVS), k, np.int32), return_obs=True)
        np.testing.assert_array_equal(ms, ps[:, k])
        np.testing.assert_array_equal(ml, pl[:, k])
        # the mixed mode returns an env's observation after ITS last step; the per-model mode,
        # as fqlpop_rollout, keeps stepping a finished env until its tile is done: compare the
        # envs that ran to the end (all of them when nothing terminates)
        ran = pl[:, k] == STEPS
        assert ran.any() and (which == "term" or ran.all())
        np.testing.assert_array_equal(mo[ran], po[:, k][ran])


# ---------------------------------------------------------------- 4. device draw
def _device_choice(seed, steps, n_envs, n_models):
    from philox_np import philox4x32_10
    t, e = np.meshgrid(np.arange(1, steps + 1, dtype=np.uint32), np.arange(n_envs, dtype=np.uint32), indexing="ij")
    ctr = np.stack([e, t, np.full_like(e, 0x5E12), np.zeros_like(e)], -1)
    w0 = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[..., 0].astype(np.uint64)
    return ((w0 * np.uint64(n_models)) >> np.uint64(32)).astype(np.int32)


def test_device_draw_is_the_restated_philox(ctx):
    seed = 0x1234_5678_9ABC
    _set_ensemble(ctx.pop, ctx.quiet)
    ch = _device_choice(seed, STEPS, N_ENVS, 3)
    assert set(np.unique(ch)) == {0, 1, 2}
    a = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, seed=seed, mode="mixed", noise=ctx.noise, return_obs=True)
    b = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, seed=seed, mode="mixed", noise=ctx.noise, choice=ch,
                                 return_obs=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # device noise too: the same seed twice, then another seed
    c = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, seed=seed, mode="mixed", return_obs=True)
    d = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, seed=seed, mode="mixed", return_obs=True)
    for x, y in zip(c, d):
        np.testing.assert_array_equal(x, y)
    e = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, seed=seed + 1, mode="mixed", noise=ctx.noise, return_obs=True)
    assert not np.array_equal(a[2], e[2])  # the same noise: only the model sequence differs


# ------------------------------------------------------------ 5. per-env semantics
@pytest.mark.parametrize("which", ["quiet", "term"])
def test_mixed_episode_does_not_depend_on_its_tile(ctx, which):
    _set_ensemble(ctx.pop, getattr(ctx, which))
    full = ctx.pop.rollout_ensemble(ctx.obs0, STEPS, mode="mixed", noise=ctx.noise, choice=ctx.choice,
                                    return_obs=True)
    few = ctx.pop.rollout_ensemble(ctx.obs0[:7], STEPS, mode="mixed", noise=ctx.noise[:, :, :7],
                                   choice=ctx.choice[:, :7], return_obs=True)
    for x, y in zip(full, few):
        np.testing.assert_array_equal(x[:, :7], y)
    if which == "term":
        assert (full[1] < STEPS).any()  # some env stopped early, and still agrees


# ------------------------------------------------------- 6. isolation and errors
def test_ensemble_is_apart_from_the_single_model_and_checks_its_arguments():
    from fqlpop import FqlpopError
    pop, _, _ = _population(2)
    obs0, noise, choice = _inputs()
    models = _models(-12.0, 1.0)
    with pytest.raises(FqlpopError, match="no env model ensemble"):
        pop.rollout_ensemble(obs0, STEPS)
    _set_single(pop, models[2])
    before = pop.rollout(obs0, STEPS, noise=noise, return_obs=True)
    _set_ensemble(pop, models[:2])
    after = pop.rollout(obs0, STEPS, noise=noise, return_obs=True)
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    good = pop.rollout_ensemble(obs0, STEPS, noise=noise)
    sp = em.flatten_state_predictor(SPEC, models[0][0])
    tp = em.flatten_termination_predictor(SPEC, models[0][1])
    for n in (0, 17):
        with pytest.raises(FqlpopError, match="error -1"):
            pop.set_env_model_ensemble([sp] * n, [tp] * n, SPEC.sp_hidden, SPEC.tp_hidden)
    with pytest.raises(FqlpopError, match="error -1"):
        pop.set_env_model_ensemble([sp[:-1]] * 2, [tp] * 2, SPEC.sp_hidden, SPEC.tp_hidden)
    with pytest.raises(FqlpopError, match="error -1"):
        pop.set_env_model_ensemble([sp] * 2, [tp[:-1]] * 2, SPEC.sp_hidden, SPEC.tp_hidden)
    bad = choice.copy() % 2
    bad[5, 3] = 2  # = K
    with pytest.raises(FqlpopError, match="error -1"):
        pop.rollout_ensemble(obs0, STEPS, mode="mixed", noise=noise, choice=bad)
    with pytest.raises(FqlpopError, match="error -1"):
        pop.rollout_ensemble(obs0, STEPS, mode="per_model", noise=noise, choice=choice % 2)
    # the refused calls changed nothing: the two-model ensemble still answers as before
    again = pop.rollout_ensemble(obs0, STEPS, noise=noise)
    for x, y in zip(good, again):
        np.testing.assert_array_equal(x, y)
    # a single termination predictor is repeated
    pop.set_env_model_ensemble([em.flatten_state_predictor(SPEC, m[0]) for m in models], tp,
                               SPEC.sp_hidden, SPEC.tp_hidden)
    assert pop.rollout_ensemble(obs0, 3, noise=noise[:, :3])[0].shape == (2, 3, N_ENVS)
    pop.close()


# ------------------------------------------------------------ 7. task and trainer
def _task_models():
    spec = em.EnvModelSpec(28, 5)
    return [(em.init_state_predictor(spec, s), em.init_termination_predictor(spec, s + 1)) for s in (0, 5)]


def test_simulated_task_trainer_halving_under_an_ensemble(tmp_path):
    from hpo.successive_halving import SuccessiveHalving
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    from trainer.config import AgentConfig, ExperimentConfig, TrainerConfig
    from trainer.trainer import Trainer
    task = OfflineTaskWithSimulatedEvaluations(n_rows=20_000, n_val_rows=2_000, num_evaluation_envs=20,
                                               max_episode_steps=25, env_models=_task_models(),
                                               ensemble_score="mean")
    agent = AgentConfig(actor_hidden_dims=(H,) * 4, value_hidden_dims=(H,) * 4, batch_size=64)
    cfg = TrainerConfig(agent=agent, steps=40, eval_interval=10, log_interval=10, save_directory=tmp_path)
    configs = [ExperimentConfig(alpha=a, seed=s) for a, s in [(3.0, 1), (10.0, 2), (30.0, 3), (100.0, 4)]]
    strategy = SuccessiveHalving(set(configs), total_evaluations=8, fraction=0.5, history_length=1)
    tr = Trainer(task, strategy, cfg)
    tr.train(max_evaluations=100)
    assert len(tr.candidates) < len(configs)  # halving on the ensemble scores
    scores = [v for vs in strategy.candidate_scores.values() for v in vs]
    assert scores and all(0.0 <= v <= 1.0 for v in scores)
    files = sorted(tmp_path.rglob("eval.csv"))
    assert files
    rows = 0
    for path in files:
        with open(path) as f:
            for row in csv.DictReader(f):
                assert {"success", "episode_length", "success_std", "success_min", "success_max"} <= set(row)
                assert float(row["success_min"]) <= float(row["success"]) <= float(row["success_max"])
                assert float(row["success_std"]) >= 0.0
                rows += 1
    assert rows >= len(configs)


@pytest.mark.parametrize("score", ["mean", "min", "mixed"])
def test_one_model_ensemble_scores_as_the_single_model_task(score):
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    m0 = _task_models()[0]
    kw = dict(n_rows=20_000, n_val_rows=2_000, num_evaluation_envs=20, max_episode_steps=25)
    plain = OfflineTaskWithSimulatedEvaluations(env_model=m0, **kw)
    ens = OfflineTaskWithSimulatedEvaluations(env_models=[m0], ensemble_score=score, **kw)
    pop, _, _ = _population(2)
    want = plain.evaluate_members(pop, [0, 1], seed=3)
    got = ens.evaluate_members(pop, [0, 1], seed=3)
    for m in (0, 1):
        assert got[m]["success"] == want[m]["success"]
        assert got[m]["episode_length"] == want[m]["episode_length"]
        assert got[m]["success_std"] == 0.0 and got[m]["success_min"] == got[m]["success_max"] == want[m]["success"]
    pop.close()


# ------------------------------------------------------- 8. the two driver scripts
def test_drivers_train_and_score_an_ensemble(tmp_path):
    """train_env_model.py --ensemble_size 2 (seeds 3 and 4, the reference's file names with
    _ens<k>), then tune_alpha.py --task simulated --env_model_ensemble 2 scoring under both."""
    import train_env_model as tem
    import tune_alpha
    env = "cube-single-play-singletask-task2-v0"
    rng = np.random.default_rng(9)
    n, D, A = 3000, 28, 5
    obs = rng.standard_normal((n, D)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    rew = np.where(obs[:, 0] > 1.0, 0.0, -1.0).astype(np.float32)
    data = tmp_path / "data"
    data.mkdir()
    np.savez(data / "cube-single-play.npz", observations=obs, actions=act,
             next_observations=(0.9 * obs + 0.1 * np.tanh(obs[:, ::-1])).astype(np.float32), rewards=rew,
             masks=(rew != 0).astype(np.float32))
    common = [f"--data_directory={data}", f"--save_directory={tmp_path}", "--val_batches=2", "--steps=60"]
    tem.main(["--model=termination_predictor"] + common)
    out = tem.main(["--model=baseline", "--termination_weight=0", "--seed=3", "--ensemble_size=2"] + common)
    for k in range(2):
        for suffix in (".pt", "_config.yaml", "_log.csv"):
            assert (out / f"baseline_ens{k}{suffix}").exists()
    assert not (out / "baseline.pt").exists()
    flats = [em.load_flax_msgpack(out / f"baseline_ens{k}.pt")["params"]["Dense_0"]["kernel"] for k in range(2)]
    assert not np.array_equal(flats[0], flats[1])  # seeds 3 and 4
    tune_alpha.main([f"--save_directory={tmp_path}", "--steps=20", "--eval_interval=10", "--log_interval=10",
                     f"--agent.actor_hidden_dims={(H,) * 4}", f"--agent.value_hidden_dims={(H,) * 4}",
                     "--agent.batch_size=64", "--eval_episodes=20", "--synthetic_rows=5000", "--task=simulated",
                     "--env_model=baseline", "--max_episode_steps=10", "--number_of_alphas=2",
                     "--number_of_seeds=1", "--max_evaluations=100", "--env_model_ensemble=2",
                     "--ensemble_score=min"])
    files = [p for p in (tmp_path / env).rglob("eval.csv")]
    assert len(files) == 2
    for path in files:
        with open(path) as f:
            rows = list(csv.DictReader(f))
        assert rows
        for row in rows:
            assert float(row["success"]) == float(row["success_min"]) <= float(row["success_max"])
    with pytest.raises(FileNotFoundError, match=r"baseline_ens2\.pt"):
        tune_alpha.main([f"--save_directory={tmp_path}", "--task=simulated", "--env_model=baseline",
                         "--env_model_ensemble=3", "--number_of_alphas=1", "--synthetic_rows=5000"])
