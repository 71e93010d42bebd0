"""Branching under the world-model ensemble on the GPU (fqlpop_rollout_ensemble_record,
fqlpop_synth_collect_ensemble): the record outputs change nothing and match the float64
oracle, the disagreement u one step at a time against its float64 restatement, rings against
the recorded mixed rollout bit for bit, the penalised rewards, training on the penalised
ring, errors, the Trainer and the driver.

Set-up as tests/test_gpu_ensemble.py and tests/test_gpu_synth.py: H = 512, D = 28, A = 5,
2 members, the K = 3 env models of seeds 11, 12, 13, 20 envs (a full 16-column tile and a
4-column one), 12 steps for rollouts, horizon 8 for collects, 2 003 offline rows.

ROWS_E (collects under the three ``term`` models, seed 21) was chosen on the CPU with the
float64 oracle under the restated device noise (synth_np.rollout_noise) and model draw
(test_gpu_ensemble._device_choice), slot by slot among 60 candidate rows each: for both
members branch 10 ends early, branches 2, 5 and 18 terminate at the horizon, the other 16 are
truncated there, and every termination logit is at least 0.15 from 0.  The tests assert the
condition from the device's own lengths."""
import csv
import functools

import numpy as np
import pytest

import synth_ens_np as SE
import synth_np as S
from oracle import fql_oracle as O
from philox_np import sample_key
from test_gpu_ensemble import _device_choice, _inputs, _mixed_oracle, _models, _population, _set_ensemble
from test_gpu_synth import (ENV, ROWS1, ROWS2, SEED1, SEED2, _assert_ring, _assert_same, _cfg, _data, _init_params,
                            _model, _pop)

pytestmark = pytest.mark.gpu
H, D, A = 512, 28, 5
N_ENVS, STEPS = 20, 12
E, T = 20, 8
N_ROWS = 2003
SEED_E = 21
ROWS_E = np.array([862, 164, 1772, 1863, 1006, 686, 846, 1279, 1713, 1672, 686, 1956, 687, 324, 1552, 995, 1436, 1435,
                   1243, 681])
PENALTY = 0.5


@functools.lru_cache(maxsize=None)
def _term():
    return _models(-12.0, 1.0)


@functools.lru_cache(maxsize=None)
def _quiet():
    return _models(-50.0, 0.1)


def _order(length):
    """(t, e) of a call's valid transitions in the order they are appended."""
    return [(t, e) for t in range(T) for e in range(E) if t < length[e]]


def _read_all(pop):
    return [pop.synth_read(m) for m in range(2)], [pop.synth_info(m) for m in range(2)]


def _assert_bytes_equal(a, b, tag, skip=()):
    for k in S.FIELDS:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), f"{tag}: {k}"


class Ctx:
    pass


@pytest.fixture(scope="module")
def ens():
    """test_gpu_ensemble's population and inputs, with the recorded mixed rollout under the
    ``term`` models (host noise and choice) shared by the trace and disagreement tests."""
    c = Ctx()
    c.pop, c.cfg, c.params = _population(2)
    c.obs0, c.noise, c.choice = _inputs()
    _set_ensemble(c.pop, _term())
    c.rec = c.pop.rollout_ensemble(c.obs0, STEPS, mode="mixed", noise=c.noise, choice=c.choice, return_obs=True,
                                   record=True, uncertainty=True)
    yield c
    c.pop.close()


@pytest.fixture(scope="module")
def ctx():
    """One population with rings under the ``term`` ensemble: the recorded mixed rollout from
    ROWS_E, the rings after collect(ensemble=True) and, after a clear, after the same collect
    with penalty 0.5 (the device state the later tests start from).  Shared, read-only."""
    c = Ctx()
    c.pop = _pop(2, capacity=1000)
    _set_ensemble(c.pop, _term())
    c.obs_rows = _data()["observations"][ROWS_E]
    c.rec = c.pop.rollout_ensemble(c.obs_rows, T, seed=SEED_E, mode="mixed", record=True, uncertainty=True,
                                   return_obs=True)
    c.succ, c.length, c.oobs, c.tobs, c.tact, c.tmodel, c.tunc = c.rec
    c.recorded = [S.transitions(c.succ[m], c.length[m], c.oobs[m], c.tobs[m], c.tact[m]) for m in range(2)]
    c.pop.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True)
    c.rings0, c.info0 = _read_all(c.pop)
    c.pop.synth_clear()
    c.pop.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True, penalty=PENALTY)
    c.rings_p, c.info_p = _read_all(c.pop)
    yield c
    c.pop.close()


# ------------------------------------------------------------------ 1. record changes nothing
@pytest.mark.parametrize("which", ["term", "quiet"])
@pytest.mark.parametrize("device_draws", [False, True])
def test_record_changes_nothing(ens, which, device_draws):
    kw = dict(seed=7) if device_draws else dict(noise=ens.noise, choice=ens.choice)
    _set_ensemble(ens.pop, _term() if which == "term" else _quiet())
    base = ens.pop.rollout_ensemble(ens.obs0, STEPS, mode="mixed", return_obs=True, **kw)
    try:
        if which == "quiet":
            assert base[0].sum() == 0 and (base[1] == STEPS).all()
        elif not device_draws:
            assert 0 < base[0].mean() < 1
        for unc in (True, False):
            rec = ens.pop.rollout_ensemble(ens.obs0, STEPS, mode="mixed", return_obs=True, record=True,
                                           uncertainty=unc, **kw)
            assert len(rec) == (7 if unc else 6)
            assert rec[3].shape == (2, STEPS, N_ENVS, D) and rec[4].shape == (2, STEPS, N_ENVS, A)
            assert rec[5].shape == (2, STEPS, N_ENVS) and rec[5].dtype == np.int32
            for x, y, what in zip(base, rec, ("success", "length", "out_obs")):
                assert x.tobytes() == y.tobytes(), f"{which}, device draws {device_draws}, uncertainty {unc}: {what}"
    finally:
        _set_ensemble(ens.pop, _term())  # the state the module fixture leaves


# ------------------------------------------------------------------ 2. traces vs the oracle
def test_traces_match_the_float64_oracle(ens):
    succ, length, oobs, tobs, tact, tmodel, tunc = ens.rec
    t_idx = np.arange(STEPS)[:, None]
    for i in range(2):
        s, l, obs, margin, want_obs, want_act = SE.mixed_oracle_traces(ens.cfg, ens.params[i], _term(), ens.obs0,
                                                                       ens.noise[i], ens.choice, STEPS)
        s0, l0, obs_0, margin0 = _mixed_oracle(ens.cfg, ens.params[i], _term(), ens.obs0, ens.noise[i], ens.choice,
                                               STEPS)
        np.testing.assert_array_equal(s, s0)        # the helper with traces is the composition without
        np.testing.assert_array_equal(l, l0)
        np.testing.assert_array_equal(obs, obs_0)
        assert margin == margin0 and margin >= 0.1, margin
        np.testing.assert_array_equal(succ[i], s)
        np.testing.assert_array_equal(length[i], l)
        ran = t_idx < l[None, :]                     # [STEPS, N_ENVS]
        assert ran.any() and (~ran).any()
        np.testing.assert_array_equal(tmodel[i][ran], ens.choice[ran])
        for a in (tobs[i], tact[i], tmodel[i], tunc[i]):
            assert (a[~ran] == 0).all()
        assert (tunc[i][ran] > 0).all()
        np.testing.assert_allclose(tobs[i], want_obs, rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(tact[i], want_act, rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(oobs[i], obs, rtol=2e-3, atol=2e-4)


# ------------------------------------------------------------------ 3. u, one step at a time
def test_disagreement_matches_its_float64_restatement(ens):
    """u_ref is the float64 formula on the device's OWN recorded (s, a) under the three models,
    so no multi-step drift enters.  The bound, per entry:

    u = |C P|_F / sqrt(K) with P the [K, D] predictions and C the centring over k, an
    orthogonal projection.  For a perturbation E of P, |u(P + E) - u(P)| <= |C E|_F / sqrt(K)
    <= |E|_F / sqrt(K) <= max_k |E_k|_2 (reverse triangle inequality; a projection does not
    lengthen).  The device's s'_k is within the project's one-step env-model tolerance of the
    float64 one (test_envmodel_step_matches_oracle: |E_k| <= tol_k = 1e-5 + 1e-4 |s'_k| per
    element), so |u - u_ref| <= max_k |tol_k|_2; the check allows the issue's 2 max_k |tol_k|_2.

    Float32 rounding of the reduction, with eps = 2^-24: r_k = s'_k - s'_0 is one rounding, a
    square two more, and Q sums (K - 1) D of them in sequence, so x = Q / K and
    y = |m|^2 / K^2 each carry at most (K D + 6) eps relative error; then
    |d(x - y)| <= (K D + 6) eps (x + y) + eps |x - y| and the square root halves the relative
    error: |du| <= (K D + 6) eps (x + y) / (2 u) + eps u.  At these shapes (K = 3, D = 28) that
    is below 1e-5 u, against a first term of about 1e-3.

    Against vacuity u_ref is at least 10 times the bound on every checked entry: the three
    models are independently initialised (measured on the CPU: u_ref / bound >= 459)."""
    _, length, _, tobs, tact, _, tunc = ens.rec
    K, eps = 3, 2.0 ** -24
    worst, least, n = 0.0, np.inf, 0
    for i in range(2):
        for t in range(STEPS):
            live = t < length[i]
            if not live.any():
                continue
            P = SE.predictions(_term(), tobs[i, t][live], tact[i, t][live])      # [K, n, D]
            u_ref = SE.disagreement(P)
            r = P - P[0]
            x, y = (r * r).sum((0, 2)) / K, (r.sum(0) ** 2).sum(-1) / K ** 2
            tol = 2.0 * np.sqrt(((1e-5 + 1e-4 * np.abs(P)) ** 2).sum(-1)).max(0)
            tol = tol + (K * D + 6) * eps * (x + y) / (2.0 * u_ref) + eps * u_ref
            err = np.abs(tunc[i, t][live].astype(np.float64) - u_ref)
            worst, least, n = max(worst, float((err / tol).max())), min(least, float((u_ref / tol).min())), n + err.size
            assert (u_ref >= 10.0 * tol).all(), (i, t, float((u_ref / tol).min()))
            assert (err <= tol).all(), (i, t, float((err / tol).max()))
    print(f"{n} entries: largest |u - u_ref| / bound {worst:.4f}, least u_ref / bound {least:.1f}")
    assert n > 2 * STEPS * 4


# ------------------------------------------------------------------ 4. exact zero
def test_identical_models_give_exactly_zero():
    pop = _pop(2, capacity=1000, env_model=False)
    _set_ensemble(pop, [_term()[0]] * 3)
    obs_rows = _data()["observations"][ROWS_E]
    rec = pop.rollout_ensemble(obs_rows, T, seed=SEED_E, mode="mixed", record=True, uncertainty=True)
    assert rec[-1].shape == (2, T, E) and (rec[-1] == 0.0).all()
    assert (rec[1] > 0).all() and np.abs(rec[2]).max() > 0          # the rollout did run
    pop.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True)
    plain, info = _read_all(pop)
    pop.synth_clear()
    pop.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True, penalty=3.0)
    pen, info_p = _read_all(pop)
    assert info == info_p and info[0]["rows"] > 0
    for m in range(2):
        _assert_bytes_equal(pen[m], plain[m], f"member {m}: penalty 3 under identical models")
    pop.close()


# ------------------------------------------------------------------ 5. the ring is the recorded mixed rollout
def test_ring_is_the_recorded_mixed_rollout_bitwise(ctx):
    for m in range(2):
        ln, sc = ctx.length[m], ctx.succ[m]
        print(f"member {m}: lengths {ln.astype(int).tolist()} success {sc.astype(int).tolist()}")
        assert (ln < T).any(), "no branch ends before the horizon"
        assert ((ln == T) & (sc == 0)).any(), "no branch is truncated at the horizon"
        assert ((ln == T) & (sc == 1)).any(), "no branch terminates exactly at the horizon"
        host = S.HostRing(1000, D, A)
        host.append(ctx.recorded[m])
        assert host.rows == int(ln.sum()) < E * T
        assert ctx.info0[m] == host.info()
        for k in S.FIELDS:
            np.testing.assert_array_equal(ctx.rings0[m][k], host.valid()[k], err_msg=f"member {m} {k}")
        assert int((ctx.rings0[m]["masks"] == 0).sum()) == int(sc.sum())
        np.testing.assert_array_equal(ctx.rings0[m]["rewards"], -ctx.rings0[m]["masks"])
    # the device's model draw is the restated one, the same for both members
    ran = np.arange(T)[:, None] < ctx.length[0][None, :]
    np.testing.assert_array_equal(ctx.tmodel[0][ran], _device_choice(SEED_E, T, E, 3)[ran])
    assert set(np.unique(ctx.tmodel[0][ran])) == {0, 1, 2}


def test_ensemble_ring_wraps_around(ctx):
    pop = _pop(2, capacity=200, env_model=False)
    _set_ensemble(pop, _term())
    r2 = pop.rollout_ensemble(_data()["observations"][ROWS2], T, seed=SEED2, mode="mixed", record=True,
                              return_obs=True)
    rec2 = [S.transitions(r2[0][m], r2[1][m], r2[2][m], r2[3][m], r2[4][m]) for m in range(2)]
    pop.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True)
    pop.collect(E, T, SEED2, start_rows=ROWS2, ensemble=True)
    for m in range(2):
        host = S.HostRing(200, D, A)
        host.append(ctx.recorded[m])
        host.append(rec2[m])
        assert host.appended > 200 and host.rows == 200 and host.head == host.appended % 200
        _assert_ring(pop, m, host, "two ensemble collects, capacity 200")
    pop.close()


# ------------------------------------------------------------------ 6. relation to the single-model collect
def test_one_model_ensemble_is_the_single_model_collect_but_for_early_ends():
    """test_gpu_synth's branches (ROWS1, SEED1, the env model of seed 11: 5 end early): a
    one-model ensemble draws model 0 at every step, so the rings agree in every byte except the
    last next_observations of a branch that ended before its tile-mates, where the single-model
    ring holds its tile's last observation and the ensemble ring the branch's own s'."""
    pop = _pop(2, capacity=1000)
    pop.collect(E, T, SEED1, start_rows=ROWS1)
    single, info_s = _read_all(pop)
    pop.synth_clear()
    _set_ensemble(pop, [_model()])
    obs_rows = _data()["observations"][ROWS1]
    succ, length, oobs = pop.rollout_ensemble(obs_rows, T, seed=SEED1, mode="mixed", return_obs=True)
    pop.collect(E, T, SEED1, start_rows=ROWS1, ensemble=True)
    ens_r, info_e = _read_all(pop)
    assert info_s == info_e
    cfg = _cfg()
    n_early = 0
    for m in range(2):
        ln = length[m].astype(int)
        tile_end = np.array([ln[(e // 16) * 16:(e // 16) * 16 + 16].max() for e in range(E)])
        order = _order(ln)
        assert len(order) == info_e[m]["rows"]
        early = np.array([t + 1 == ln[e] and ln[e] < tile_end[e] for t, e in order])
        n_early += int(early.sum())
        _assert_bytes_equal(ens_r[m], single[m], f"member {m}", skip=("next_observations",))
        a, b = ens_r[m]["next_observations"], single[m]["next_observations"]
        assert a[~early].tobytes() == b[~early].tobytes(), f"member {m}: next_observations"
        nz = S.rollout_noise(SEED1, sample_key(int(pop.seeds[m]), float(pop.alphas[m])), E, T, A)
        s, l, final, margin, _, _ = SE.mixed_oracle_traces(cfg, O.cast_tree(_init_params(m), np.float64), [_model()],
                                                           obs_rows, nz, np.zeros((T, E), np.int32), T)
        assert margin >= 0.1, margin
        np.testing.assert_array_equal(l, ln)
        np.testing.assert_array_equal(s, succ[m])
        for i in np.flatnonzero(early):
            e = order[i][1]
            assert a[i].tobytes() == oobs[m, e].tobytes()
            assert a[i].tobytes() != b[i].tobytes()   # the single-model ring holds another observation there
            np.testing.assert_allclose(a[i], final[e], rtol=2e-3, atol=2e-4)
    assert n_early >= 1
    pop.close()


# ------------------------------------------------------------------ 7. penalised rewards
def test_penalised_rewards(ctx):
    below = 0
    for m in range(2):
        assert ctx.info_p[m] == ctx.info0[m]
        _assert_bytes_equal(ctx.rings_p[m], ctx.rings0[m], f"member {m}: penalty {PENALTY}", skip=("rewards",))
        u = np.array([ctx.tunc[m][t, e] for t, e in _order(ctx.length[m])], np.float32)
        assert u.shape == ctx.rings0[m]["rewards"].shape and (u > 0).all()
        want = ctx.rings0[m]["rewards"].astype(np.float64) - PENALTY * u.astype(np.float64)
        np.testing.assert_allclose(ctx.rings_p[m]["rewards"], want, rtol=1e-6, atol=0)
        np.testing.assert_allclose(ctx.rings_p[m]["rewards"],
                                   SE.penalised(ctx.recorded[m], ctx.length[m], ctx.tunc[m], PENALTY)["rewards"],
                                   rtol=1e-6, atol=0)
        below += int((ctx.rings_p[m]["rewards"] < -1).sum())
    assert below >= 1


# ------------------------------------------------------------------ 8. training reads the penalised ring
@pytest.mark.parametrize("use_graph", [True, False])
def test_rho0_trains_on_the_penalised_ring(ctx, use_graph):
    a = _pop(2, capacity=1000, use_graph=use_graph, env_model=False)
    _set_ensemble(a, _term())
    a.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True, penalty=PENALTY)
    a.set_real_ratio(0.0)
    a.step(2)
    for m in range(2):
        b = _pop(1, use_graph=use_graph, env_model=False, param_seeds=[m], seeds=[m + 1], data=ctx.rings_p[m])
        b.step(2)
        _assert_same(a, m, b, 0, f"rho 0 on the penalised ring, graph {use_graph}")
        b.close()
    a.close()


# ------------------------------------------------------------------ 9. errors
def test_errors_leave_the_rings_unchanged(ctx):
    from fqlpop import FqlpopError
    pop = ctx.pop

    def refused(code, fn, *a, **kw):
        with pytest.raises(FqlpopError, match=f"error {code}:"):
            fn(*a, **kw)
    for bad in (-0.5, float("nan"), float("inf")):
        refused(-1, pop.collect, E, T, 1, ensemble=True, penalty=bad)
    refused(-1, pop.collect, 126, 8, 1, ensemble=True)               # 1008 transitions > capacity 1000
    refused(-1, pop.collect, 0, T, 1, ensemble=True)
    for bad in (-1, N_ROWS):
        rows = ROWS_E.copy()
        rows[7] = bad
        refused(-1, pop.collect, E, T, 1, start_rows=rows, ensemble=True, penalty=1.0)
    with pytest.raises(ValueError, match="mixed"):
        pop.rollout_ensemble(ctx.obs_rows, T, mode="per_model", record=True)
    with pytest.raises(ValueError, match="mixed"):
        pop.rollout_ensemble(ctx.obs_rows, T, mode="per_model", uncertainty=True)
    with pytest.raises(ValueError, match="ensemble"):
        pop.collect(E, T, 1, penalty=1.0)                            # a penalty under the single model
    # the C call itself refuses record in per-model mode (FQLPOP_E_ARG), before any launch
    import ctypes
    from fqlpop import _lib
    out, oobs = np.zeros((2, 3, E, 2), np.float32), np.zeros((2, 3, E, D), np.float32)
    tobs, tact = np.full((2, T, E, D), 7.0, np.float32), np.full((2, T, E, A), 7.0, np.float32)
    rc = pop.lib.fqlpop_rollout_ensemble_record(pop._h, _lib.fptr(ctx.obs_rows), E, T, ctypes.c_uint64(1), None,
                                                _lib.ENS_PER_MODEL, None, _lib.fptr(out), _lib.fptr(oobs),
                                                _lib.fptr(tobs), _lib.fptr(tact), None, None)
    assert rc == -1 and (tobs == 7.0).all() and (tact == 7.0).all() and not out.any()
    for m in range(2):
        assert pop.synth_info(m) == ctx.info_p[m]
        _assert_bytes_equal(pop.synth_read(m), ctx.rings_p[m], f"member {m} after the refused calls")
    # no ensemble set: the single model does not stand in for it
    single = _pop(1, capacity=1000)
    with pytest.raises(FqlpopError, match="error -3:.*no env model ensemble"):
        single.collect(E, T, 1, ensemble=True)
    assert single.synth_info(0) == {"rows": 0, "head": 0, "appended": 0}
    single.close()
    # ... and the ensemble collect does not need the single model
    only_ens = _pop(1, capacity=1000, env_model=False)
    _set_ensemble(only_ens, _term())
    refused(-3, only_ens.collect, E, T, 1)
    only_ens.collect(E, T, SEED_E, start_rows=ROWS_E, ensemble=True)
    assert only_ens.synth_info(0) == ctx.info0[0]
    _assert_bytes_equal(only_ens.synth_read(0), ctx.rings0[0], "without set_env_model")
    only_ens.close()
    no_rings = _pop(1, env_model=False)
    _set_ensemble(no_rings, _term())
    refused(-3, no_rings.collect, E, T, 1, ensemble=True)
    no_rings.close()


# ------------------------------------------------------------------ 10. Trainer and driver
def test_trainer_trains_on_penalised_ensemble_branches(tmp_path):
    from hpo.identity import Identity
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    from trainer.config import AgentConfig, ExperimentConfig, ModelRolloutConfig, TrainerConfig
    from trainer.trainer import Trainer

    def run(path, **mr_kw):
        cfg = TrainerConfig(steps=12, eval_interval=12, log_interval=2, save_directory=path, env_name=ENV, seed=3,
                            agent=AgentConfig(batch_size=64))
        task = OfflineTaskWithSimulatedEvaluations(ENV, dataset=_data(), num_evaluation_envs=4, max_episode_steps=6,
                                                   env_models=_term())
        configs = [ExperimentConfig(seed=1, alpha=3.0), ExperimentConfig(seed=2, alpha=30.0)]
        mr = ModelRolloutConfig(branches=12, horizon=4, interval=4, warmup=4, real_ratio=0.5, buffer_rows=300, **mr_kw)
        trainer = Trainer(task, Identity(population=configs, total_evaluations=0), cfg, model_rollouts=mr)
        trainer.train(max_evaluations=2)
        rings = [trainer.population.synth_read(trainer.member_of[c]) for c in configs]
        infos = [trainer.population.synth_info(trainer.member_of[c]) for c in configs]
        csvs = []
        for c in configs:
            with open(path / ENV / trainer.experiments[c].experiment_name / "train.csv") as f:
                csvs.append(list(csv.DictReader(f)))
        n = trainer.collect_index
        trainer.population.close()
        task.close()
        return rings, infos, csvs, n
    rings, infos, csvs, n = run(tmp_path / "pen", ensemble=True, penalty=1.0)
    assert n == 2 and all(i["appended"] > 0 for i in infos), (n, infos)       # after updates 4 and 8
    assert all(len(rows) == 6 for rows in csvs)                                # steps 2, 4, ..., 12
    assert all((r["rewards"] < -1).any() for r in rings)                       # the penalty reached the rings
    rings0, infos0, csvs0, _ = run(tmp_path / "plain", ensemble=True)
    assert all((r["rewards"] >= -1).all() for r in rings0)
    for a, b in zip(csvs, csvs0):
        # equal until the first collect (update 4); the penalised rewards change the losses after it
        assert a[:2] == b[:2] and a[-1] != b[-1]


def test_tune_alpha_driver_with_ensemble_branches(tmp_path, monkeypatch):
    import envmodel as em
    import tune_alpha
    from envmodel.flax_msgpack import msgpack_serialize
    from trainer.trainer import Trainer
    spec = em.EnvModelSpec(D, A)
    d = tmp_path / ENV / "env_models"
    d.mkdir(parents=True)
    for k in range(2):
        (d / f"baseline_ens{k}.pt").write_bytes(msgpack_serialize({"params": em.init_state_predictor(spec, 20 + k)}))
    (d / "termination_predictor.pt").write_bytes(msgpack_serialize({"params": em.init_termination_predictor(spec, 9)}))
    made = []

    class Recording(Trainer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(tune_alpha, "Trainer", Recording)
    tune_alpha.main([f"--save_directory={tmp_path}", "--steps=8", "--eval_interval=8", "--log_interval=4",
                     "--agent.batch_size=64", "--agent.layer_norm", "--eval_episodes=4", "--synthetic_rows=2003",
                     "--task=simulated", "--env_model=baseline", "--max_episode_steps=6", "--number_of_alphas=2",
                     "--max_evaluations=2", "--model_rollout_branches=12", "--model_rollout_horizon=4",
                     "--model_rollout_interval=4", "--model_rollout_warmup=0", "--model_real_ratio=0.5",
                     "--model_buffer_rows=200", "--env_model_ensemble=2", "--model_rollout_ensemble",
                     "--model_rollout_penalty=1.0"])
    assert (tmp_path / ENV / "checkpoint.pkl").exists()
    t = made[0]
    assert t.model_rollouts.ensemble and t.model_rollouts.penalty == 1.0
    assert t.collect_index == 1 and all(t.population.synth_info(m)["appended"] > 0 for m in t.member_of.values())
    assert any((t.population.synth_read(m)["rewards"] < -1).any() for m in t.member_of.values())
    assert len(list((tmp_path / ENV).rglob("train.csv"))) == 2 and len(list((tmp_path / ENV).rglob("eval.csv"))) == 2
