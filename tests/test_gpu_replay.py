"""GPU tests of the recorded-action replay (fqlpop_envmodel_replay, replay_kernel), the
rollout traces (fqlpop_rollout_record) and the evaluate_env_model.py driver.

Oracle: a float64 loop over oracle.envmodel_oracle's state_predictor and
termination_predictor.  Tolerances are the project's existing ones: rtol 1e-4 / atol 1e-5
at step 0 (test_envmodel_step_matches_oracle) and rtol 2e-3 / atol 2e-4 for the later
steps of an open-loop chain (the rollout tests), for the observations, the logits and
both error columns."""
import ctypes
import functools

import numpy as np
import pytest

import envmodel as em
from oracle import envmodel_oracle as EO
from oracle import fql_oracle as O

pytestmark = pytest.mark.gpu

DEFAULT_SP, DEFAULT_TP = (128, 256, 128), (128, 128)
SHAPES = {  # obs, act, state predictor, termination predictor, episodes, steps
    "a": (28, 5, DEFAULT_SP, DEFAULT_TP, 37, 6),   # two full blocks and a 5-column one
    "b": (42, 8, (64, 96), (40,), 17, 5),          # (A + 2D) * 16 staged values > 512 threads
    "c": (56, 8, DEFAULT_SP, DEFAULT_TP, 16, 3),   # K0 = 64 (the limit), one exact block
}


def _env_model(spec, tp_bias=0.0, tp_scale=1.0, seed=0):
    sp = em.init_state_predictor(spec, seed)
    for k in sp:  # non-trivial LayerNorm parameters
        if k.startswith("LayerNorm"):
            rng = np.random.default_rng(seed + 7)
            sp[k]["scale"] = (1.0 + 0.2 * rng.standard_normal(sp[k]["scale"].shape)).astype(np.float32)
            sp[k]["bias"] = (0.1 * rng.standard_normal(sp[k]["bias"].shape)).astype(np.float32)
    tp = em.init_termination_predictor(spec, seed + 1, scale=tp_scale, bias=tp_bias)
    return sp, tp


def _population(obs_dim, act_dim, hidden=64, n=1):
    from fqlpop import Population, PopulationConfig
    return Population(PopulationConfig(obs_dim=obs_dim, action_dim=act_dim, hidden_dims=(hidden,) * 4, batch_size=64),
                      [10.0] * n, list(range(1, n + 1)))


def _upload(pop, spec, sp, tp):
    pop.set_env_model(em.flatten_state_predictor(spec, sp), em.flatten_termination_predictor(spec, tp),
                      spec.sp_hidden, spec.tp_hidden)


def _oracle(sp, tp, init_obs, actions, anchor_obs, anchor_every):
    """float64 replay: predicted observations [n, T, D] and logits [n, T]."""
    x = init_obs.astype(np.float64)
    obs, logits = [], []
    for t in range(actions.shape[1]):
        if anchor_every > 0 and t > 0 and t % anchor_every == 0:
            x = anchor_obs[:, t].astype(np.float64)
        x = EO.state_predictor(sp, x, actions[:, t].astype(np.float64))
        obs.append(x)
        logits.append(EO.termination_predictor(tp, x).reshape(-1))
    return np.stack(obs, 1), np.stack(logits, 1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Models and inputs of one shape (read-only, shared by the tests)."""
    D, A, sp_h, tp_h, n, T = SHAPES[name]
    spec = em.EnvModelSpec(D, A, sp_h, tp_h)
    sp, tp = _env_model(spec, seed=3)
    rng = np.random.default_rng(17)
    c = {"spec": spec, "sp": sp, "tp": tp, "n": n, "T": T,
         "init": rng.standard_normal((n, D)).astype(np.float32),
         "act": rng.uniform(-1, 1, (n, T, A)).astype(np.float32),
         "anchor": rng.standard_normal((n, T, D)).astype(np.float32),
         "noise": (0.1 * rng.standard_normal((n, T, D)))}
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _full_run_a():
    """Shape (a), open loop, all outputs: the run the lengths / column tests compare with."""
    c = _case("a")
    want_obs, _ = _oracle(c["sp"], c["tp"], c["init"], c["act"], c["anchor"], 0)
    nxt = (want_obs + c["noise"]).astype(np.float32)
    pop = _population(28, 5)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    r = pop.envmodel_replay(c["init"], c["act"], next_obs=nxt, return_obs=True)
    pop.close()
    return nxt, r


def _assert_close(got, want, what):
    print(f"{what}: step 0 max |d| {np.abs(got[:, 0] - want[:, 0]).max():.3e}, "
          f"later {np.abs(got[:, 1:] - want[:, 1:]).max() if got.shape[1] > 1 else 0.0:.3e}")
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-4, atol=1e-5, err_msg=f"{what} step 0")
    np.testing.assert_allclose(got[:, 1:], want[:, 1:], rtol=2e-3, atol=2e-4, err_msg=f"{what} steps 1..")


# --------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("anchor_every", [0, 1, 2])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_replay_matches_oracle(name, anchor_every):
    c = _case(name)
    want_obs, want_logit = _oracle(c["sp"], c["tp"], c["init"], c["act"], c["anchor"], anchor_every)
    nxt = (want_obs + c["noise"]).astype(np.float32)  # a non-trivial error curve
    d = want_obs - nxt.astype(np.float64)
    pop = _population(c["spec"].obs_dim, c["spec"].action_dim)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    r = pop.envmodel_replay(c["init"], c["act"], next_obs=nxt, anchor_obs=c["anchor"], anchor_every=anchor_every,
                            return_obs=True)
    pop.close()
    assert r["obs"].shape == want_obs.shape and r["logits"].shape == want_logit.shape
    _assert_close(r["obs"], want_obs, "obs")
    _assert_close(r["logits"], want_logit, "logits")
    _assert_close(r["mse"], (d * d).mean(-1), "mse")
    _assert_close(r["mae"], np.abs(d).mean(-1), "mae")
    assert r["mse"].min() > 1e-3  # the curve is not trivially 0


# --------------------------------------------------------------------- 2. lengths
def test_replay_lengths_mask_outputs():
    c = _case("a")
    nxt, full = _full_run_a()
    n, T = c["n"], c["T"]
    lengths = np.array(([1, 3, T, 2, T, 5] * 7)[:n], np.int32)
    lengths[32:] = [2, 1, 3, 1, 2]  # the last block stops early: all its columns <= 3
    pop = _population(28, 5)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    r = pop.envmodel_replay(c["init"], c["act"], next_obs=nxt, lengths=lengths, return_obs=True)
    pop.close()
    valid = np.arange(T)[None, :] < lengths[:, None]
    for k in ("logits", "mse", "mae", "obs"):
        v = valid if r[k].ndim == 2 else valid[..., None]
        np.testing.assert_array_equal(r[k], np.where(v, full[k], 0.0).astype(np.float32), err_msg=k)
    assert np.all(full["logits"] != 0) and np.all(full["mse"] != 0)  # the zeros above are the mask's


# ---------------------------------------------------------- 3. column independence
def test_replay_columns_independent():
    c = _case("a")
    nxt, full = _full_run_a()
    pop = _population(28, 5)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    part = pop.envmodel_replay(c["init"][5:9], c["act"][5:9], next_obs=nxt[5:9], return_obs=True)
    one = pop.envmodel_replay(c["init"][36], c["act"][36:37], next_obs=nxt[36:37], return_obs=True)
    pop.close()
    for k in ("logits", "mse", "mae", "obs"):
        np.testing.assert_array_equal(part[k], full[k][5:9], err_msg=k)
        np.testing.assert_array_equal(one[k], full[k][36:37], err_msg=k)


# ------------------------------------------------- 4. agreement with envmodel_step
def test_replay_equals_chained_envmodel_step():
    c = _case("a")
    n, T = 20, 4
    init, act = c["init"][:n], c["act"][:n, :T]
    pop = _population(28, 5)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    r = pop.envmodel_replay(init, act, return_obs=True)
    r1 = pop.envmodel_replay(init, act[:, :1], return_obs=True)
    x = init
    for t in range(T):
        x, logit = pop.envmodel_step(x, act[:, t])
        np.testing.assert_array_equal(r["obs"][:, t], x, err_msg=f"obs step {t}")
        np.testing.assert_array_equal(r["logits"][:, t], logit, err_msg=f"logit step {t}")
        if t == 0:
            np.testing.assert_array_equal(r1["obs"][:, 0], x)
            np.testing.assert_array_equal(r1["logits"][:, 0], logit)
    pop.close()
    assert set(r) == {"logits", "obs"}  # no error columns without next_obs


# ------------------------------------------- 5. closing the loop with the rollout
def _actor_population(n, seed=0):
    pop = _population(28, 5, hidden=512, n=n)
    cfg = O.OracleConfig(obs_dim=28, action_dim=5, hidden_dims=(512,) * 4, batch_size=64)
    for i in range(n):
        pop.set_params(i, O.cast_tree(O.init_params(cfg, seed + i), np.float32))
    return pop


def test_rollout_record_replays_bitwise():
    pop = _actor_population(2)
    spec = em.EnvModelSpec(28, 5)
    sp, tp = _env_model(spec, tp_bias=-50.0, tp_scale=0.1)  # nothing terminates
    _upload(pop, spec, sp, tp)
    n_envs, steps = 12, 4
    rng = np.random.default_rng(5)
    obs0 = rng.standard_normal((n_envs, 28)).astype(np.float32)
    noise = rng.standard_normal((2, steps, n_envs, 5)).astype(np.float32)
    plain = pop.rollout(obs0, steps, noise=noise, return_obs=True)
    succ, length, last, tobs, tact = pop.rollout(obs0, steps, noise=noise, return_obs=True, record=True)
    for x, y in zip(plain, (succ, length, last)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(length, np.full((2, n_envs), steps, np.float32))
    assert tobs.shape == (2, steps, n_envs, 28) and tact.shape == (2, steps, n_envs, 5)
    assert np.abs(tact).max() <= 1.0 and np.abs(tact).min() > 0.0  # clipped actions, all written
    for m in range(2):
        np.testing.assert_array_equal(tobs[m, 0], obs0)
        r = pop.envmodel_replay(obs0, tact[m].transpose(1, 0, 2), return_obs=True)
        for t in range(steps - 1):
            np.testing.assert_array_equal(r["obs"][:, t], tobs[m, t + 1], err_msg=f"member {m} step {t}")
        np.testing.assert_array_equal(r["obs"][:, steps - 1], last[m], err_msg=f"member {m} last step")
    pop.close()


def test_rollout_record_stops_at_termination():
    pop = _actor_population(3)
    spec = em.EnvModelSpec(28, 5, (64, 128), (64,))
    sp, tp = _env_model(spec, tp_bias=-14.0, tp_scale=1.0, seed=11)  # ends some episodes
    _upload(pop, spec, sp, tp)
    n_envs, steps = 40, 12
    rng = np.random.default_rng(5)
    obs0 = rng.standard_normal((n_envs, 28)).astype(np.float32)
    noise = rng.standard_normal((3, steps, n_envs, 5)).astype(np.float32)
    plain = pop.rollout(obs0, steps, noise=noise)
    succ, length, tobs, tact = pop.rollout(obs0, steps, noise=noise, record=True)
    pop.close()
    np.testing.assert_array_equal(plain[0], succ)
    np.testing.assert_array_equal(plain[1], length)
    assert 0 < succ.mean() < 1 and length.min() < steps  # some episodes end early
    ran = np.arange(steps)[None, :, None] < length[:, None, :]  # [member, t, env]
    assert not tobs[~ran].any() and not tact[~ran].any()
    assert np.all(np.any(tobs != 0, axis=-1) == ran)
    assert np.all(np.any(tact != 0, axis=-1) == ran)


# ----------------------------------------------------------- 6. any hidden width
def test_replay_on_hidden_64_population():
    from fqlpop import FqlpopError
    c = _case("a")
    pop = _population(28, 5, hidden=64)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    r = pop.envmodel_replay(c["init"][:3], c["act"][:3, :2])
    assert r["logits"].shape == (3, 2) and np.all(np.isfinite(r["logits"])) and np.all(r["logits"] != 0)
    with pytest.raises(FqlpopError, match="512"):
        pop.rollout(c["init"][:3], 2)
    pop.close()


# --------------------------------------------------------------------- 7. errors
def test_replay_errors():
    from fqlpop import FqlpopError
    from fqlpop._lib import fptr
    c = _case("a")
    init, act, anchor = c["init"][:4], c["act"][:4], c["anchor"][:4]
    pop = _population(28, 5)
    with pytest.raises(FqlpopError, match=r"error -3: no env model"):
        pop.envmodel_replay(init, act)
    _upload(pop, c["spec"], c["sp"], c["tp"])
    with pytest.raises(FqlpopError, match="error -1"):  # anchor_every without anchor_obs
        pop.envmodel_replay(init, act, anchor_every=2)
    for bad in ([1, 0, 2, 3], [1, 2, c["T"] + 1, 3]):   # a length outside 1..T
        with pytest.raises(FqlpopError, match="error -1"):
            pop.envmodel_replay(init, act, lengths=bad)
    with pytest.raises(FqlpopError, match="error -1"):  # T = 0
        pop.envmodel_replay(init, act[:, :0])
    with pytest.raises(FqlpopError, match="error -1"):  # n = 0
        pop.envmodel_replay(init[:0], act[:0])
    # out_err without next_obs (the Python surface never asks for that): the C ABI refuses
    logits = np.zeros((4, c["T"]), np.float32)
    err = np.zeros((4, c["T"], 2), np.float32)
    rc = pop.lib.fqlpop_envmodel_replay(pop._h, fptr(np.ascontiguousarray(init)), fptr(np.ascontiguousarray(act)),
                                        None, None, None, 4, c["T"], 0, fptr(logits), fptr(err), None)
    assert rc == -1 and b"next_obs" in pop.lib.fqlpop_last_error()
    rc = pop.lib.fqlpop_envmodel_replay(pop._h, fptr(np.ascontiguousarray(init)), fptr(np.ascontiguousarray(act)),
                                        None, None, None, 4, -1, 0, fptr(logits), None, None)
    assert rc == -1
    ok = pop.envmodel_replay(init, act, anchor_obs=anchor, anchor_every=2)  # the handle still works
    assert np.all(np.isfinite(ok["logits"]))
    pop.close()


# ------------------------------------------------------------------------ 8. CLI
def test_evaluate_env_model_driver(tmp_path, capsys):
    import csv
    import json

    import yaml

    import evaluate_env_model as eem
    from envmodel.flax_msgpack import msgpack_serialize
    from evaluator.env_model_evaluator import CSV_COLUMNS, episodes_from_dataset, summarise
    D, A, rows = 28, 5, 3000
    rng = np.random.default_rng(2)
    obs = rng.standard_normal((rows, D)).astype(np.float32)
    ds = {"observations": obs, "actions": rng.uniform(-0.9, 0.9, (rows, A)).astype(np.float32),
          "next_observations": (obs + 0.05 * rng.standard_normal((rows, D))).astype(np.float32),
          "rewards": -np.ones(rows, np.float32), "masks": (rng.random(rows) > 0.2).astype(np.float32)}
    data = tmp_path / "data"
    data.mkdir()
    np.savez(data / "cube-single-play.npz", **ds)
    spec = em.EnvModelSpec(D, A, (64, 96), (40,))
    sp, tp = _env_model(spec, seed=5)
    env_name = "cube-single-play-singletask-task2-v0"
    models = tmp_path / "exp" / env_name / "env_models"
    models.mkdir(parents=True)
    for name, tree, hidden in (("baseline", sp, spec.sp_hidden), ("termination_predictor", tp, spec.tp_hidden)):
        (models / f"{name}.pt").write_bytes(msgpack_serialize({"params": tree}))
        (models / f"{name}_config.yaml").write_text(yaml.safe_dump({"hidden_dims": list(hidden), "latent_dim": 4}))
    path = eem.main([f"--data_directory={data}", f"--save_directory={tmp_path / 'exp'}", "--model=baseline",
                     "--horizon", "12", "--eval_episodes", "3", "--seed=4"])
    assert path == models / "baseline_trajectory_comparison.csv"
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["horizon"] == 12 and summary["episodes"] == 3 and 0.0 <= summary["real2sim_success"] <= 1.0
    with open(path) as f:
        table = list(csv.DictReader(f))
    assert len(table) == 12 and [int(r["step"]) for r in table] == list(range(12))
    # the same episodes replayed directly
    from task.offline_task_npz import load_npz_dataset
    loaded = load_npz_dataset(data / "cube-single-play.npz")
    ep = episodes_from_dataset(loaded, 3, 12, seed=4)
    pop = _population(D, A)
    _upload(pop, spec, sp, tp)
    r = pop.envmodel_replay(ep["init_obs"], ep["actions"], next_obs=ep["next_obs"], lengths=ep["lengths"])
    pop.close()
    want = summarise(r["mse"], r["mae"], r["logits"], ep["masks"], ep["lengths"])
    assert summary["real2sim_success"] == want["real2sim_success"]
    assert summary["recorded_success"] == want["recorded_success"]
    for k in CSV_COLUMNS:
        np.testing.assert_array_equal(np.array([float(r[k]) for r in table]), np.asarray(want[k], np.float64),
                                      err_msg=k)
