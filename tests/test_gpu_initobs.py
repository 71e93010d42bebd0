"""GPU parity of the initial-observation VAE (fqlpop_initobs_*) against the float64
restatement in tests/initobs_np.py: injected steps (logs, Adam moments, parameters), eval,
the decoder-only sampler with given and device-drawn latents, device-sampled training,
error paths, and train_env_model.py -> simulated task end to end."""
import ctypes

import numpy as np
import pytest

import initobs_np as V
from envmodel import initial_observation as io
from envmodel.trainer import EnvModelTrainerConfig

pytestmark = pytest.mark.gpu

# A hidden unit whose float64 pre-activation is within fp32 rounding of zero can take the
# other side of the ReLU in the fp32 kernel (tests/test_gpu_emtrain.py, RELU_MARGIN): batches
# are drawn until every pre-activation is at least this far from zero.
RELU_MARGIN = 2e-6
PARITY_CASES = [  # obs, latent, hidden, B, reconstruction weight
    (28, 4, (128,), 32, 10.0),    # two blocks (the partial sum); 28 pads a 16-tile
    (42, 5, (64, 32), 48, 1.0),   # the reversed decoder; an odd latent
    (69, 20, (64,), 16, 10.0),    # wide input (> 64); heads wider than one 16-tile
]
LR, STEPS = 1e-3, 50


def parity_setup(case, n_batches=4):
    """(spec, params tree, [(obs, eps)] with a ReLU margin for the float64 trajectory)."""
    D, L, hid, B, w = case
    spec = io.InitialObservationSpec(D, L, hid)
    rng = np.random.default_rng(100 + D)
    tree = io.init_initial_observation(spec, 1)
    for mod in tree.values():
        for layer in mod.values():
            layer["bias"] = (0.1 * rng.standard_normal(layer["bias"].shape)).astype(np.float32)
    ref, m, v = V.f64(tree), V.zeros_like(tree), V.zeros_like(tree)
    batches = []
    for step in range(n_batches):
        for _ in range(64):
            obs = rng.standard_normal((B, D)).astype(np.float32)
            eps = rng.standard_normal((B, L)).astype(np.float32)
            if V.relu_margin(ref, obs, eps, w) >= RELU_MARGIN:
                break
        else:
            raise AssertionError("no batch with a ReLU margin in 64 draws")
        batches.append((obs, eps))
        _, _, g = V.vae_step(ref, obs, eps, w)
        ref, m, v = V.adam_update(ref, g, m, v, step, V.cosine_lr(LR, STEPS, step))
    return spec, tree, batches


def _leaves(tree):
    return [(m, l, k, tree[m][l][k]) for m in sorted(tree) for l in sorted(tree[m]) for k in sorted(tree[m][l])]


def assert_moments_close(got, want):
    """Adam's moments are linear / quadratic in the gradients: 1e-3 of each leaf's scale."""
    for m, l, k, w in _leaves(want):
        np.testing.assert_allclose(got[m][l][k], w, rtol=1e-3, atol=1e-3 * float(np.abs(w).max()) + 1e-12,
                                   err_msg=f"{m}/{l}/{k}")


def assert_params_close(got, want, steps, lr=LR):
    """All but 1e-3 of a leaf's elements within (1e-4 rel, 3e-6 steps abs); every one within
    2 lr per step (Adam normalises each update: tests/test_gpu_emtrain.py)."""
    for m, l, k, w in _leaves(want):
        g = np.asarray(got[m][l][k], np.float64)
        bad = ~np.isclose(g, w, rtol=1e-4, atol=3e-6 * steps)
        assert bad.mean() <= 1e-3, (m, l, k, int(bad.sum()), bad.size)
        assert np.abs(g - w).max() <= 2 * lr * steps, (m, l, k)


def _trainer(spec, tree, B, w, steps=STEPS, seed=0, loader=None):
    cfg = EnvModelTrainerConfig(steps=steps, batch_size=B, init_learning_rate=LR, reconstruction_weight=w, seed=seed)
    return io.InitialObservationTrainer(spec, tree, loader, None, cfg)


@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: f"obs{c[0]}-lat{c[1]}-B{c[3]}")
def test_injected_steps_and_eval_match_restatement(case):
    D, L, hid, B, w = case
    spec, tree, batches = parity_setup(case)
    tr = _trainer(spec, tree, B, w)
    ref, m, v = V.f64(tree), V.zeros_like(tree), V.zeros_like(tree)
    for step in range(3):
        obs, eps = batches[step]
        _, logs = tr.train_step(None, {"observations": obs}, eps=eps)
        _, want, g = V.vae_step(ref, obs, eps, w)
        print(step, logs, want)
        for k in want:
            assert logs[k] == pytest.approx(want[k], rel=1e-4, abs=1e-7), (step, k)
        ref, m, v = V.adam_update(ref, g, m, v, step, V.cosine_lr(LR, STEPS, step))
        assert_moments_close(io.unflatten(spec, tr.flat(1)), m)
        assert_moments_close(io.unflatten(spec, tr.flat(2)), v)
        assert_params_close(tr.params, ref, step + 1)
    assert tr.count == 3
    # eval: the restatement's losses of the current parameters; nothing moves
    before = [tr.flat(i) for i in range(3)]
    obs, eps = batches[3]
    logs = tr.eval_step(None, {"observations": obs}, eps=eps)
    _, want, _ = V.vae_step(V.f64(tr.params), obs, eps, w)
    for k in want:
        assert logs[k] == pytest.approx(want[k], rel=1e-4), k
    assert tr.count == 3
    for i in range(3):
        np.testing.assert_array_equal(tr.flat(i), before[i])
    tr.close()


def test_sampler_matches_numpy_decoder():
    spec = io.InitialObservationSpec(28, 4, (128, 256, 128))
    tree = io.init_initial_observation(spec, 2)
    rng = np.random.default_rng(0)
    for layer in tree["decoder"].values():
        layer["bias"] = (0.1 * rng.standard_normal(layer["bias"].shape)).astype(np.float32)
    dec = V.f64(tree)["decoder"]
    sm = io.InitialObservationSampler(spec, {"decoder": tree["decoder"]})
    for n in (1, 50, 4096):
        z = rng.standard_normal((n, 4)).astype(np.float32)
        want, _ = V.decode(dec, z)
        got = sm.sample(n, 0, z=z)
        assert got.shape == (n, 28)
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), n
        # device-drawn latents: the host restatement of the Philox normals through the decoder
        want, _ = V.decode(dec, V.device_z(11, n, 4))
        got = sm.sample(n, 11)
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), n
        np.testing.assert_array_equal(got, sm.sample(n, 11))
        assert not np.array_equal(got, sm.sample(n, 12))
    # a row's draw does not depend on n
    np.testing.assert_array_equal(sm.sample(50, 11), sm.sample(4096, 11)[:50])
    sm.close()


def _manifold_data(n=1000, D=28, seed=0):
    """tanh(z W) + b + 0.01 noise with a 2-dimensional z; W ~ N(0, 1), b ~ 0.1 N(0, 1) (offsets
    that Adam's 400 cosine-decayed steps of at most 1e-3 each, 0.2 in all, can reach)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2))
    W, b = rng.standard_normal((2, D)), 0.1 * rng.standard_normal(D)
    return (np.tanh(z @ W) + b + 0.01 * rng.standard_normal((n, D))).astype(np.float32)


class _Loader:
    def __init__(self, obs):
        self.dataset = {"observations": obs}


def test_device_sampled_training_learns_and_is_deterministic():
    """400 device-sampled steps, twice: bit-identical; the held-batch loss falls and decoded
    samples have the data's per-feature moments.  The float64 restatement of this exact run
    (rows, eps and z from initobs_np.device_rows / device_eps / device_z, seed 5) on the CPU:
    held loss 1.520 -> 0.119, largest mean gap 0.064, std ratios 0.80 - 1.02."""
    D, L, B, w, steps = 28, 4, 256, 10.0, 400
    data = _manifold_data()
    spec = io.InitialObservationSpec(D, L, (128,))
    tree = io.init_initial_observation(spec, 0)
    held, held_eps = data[:B], np.random.default_rng(1).standard_normal((B, L)).astype(np.float32)
    runs = []
    for _ in range(2):
        tr = _trainer(spec, tree, B, w, steps=steps, seed=5, loader=_Loader(data))
        before = tr.eval_step(None, held, eps=held_eps)["loss"]
        tr.steps(steps)
        after = tr.eval_step(None, held, eps=held_eps)["loss"]
        assert tr.count == steps
        runs.append((before, after, tr.flat(), tr.sample(1000, seed=0)))
        tr.close()
    np.testing.assert_array_equal(runs[0][2], runs[1][2])  # same seed -> bit-identical
    before, after, _, gen = runs[0]
    print("held loss", before, after)
    assert after < 0.5 * before, (before, after)
    gap = np.abs(gen.mean(0) - data.mean(0)).max()
    ratio = gen.std(0) / data.std(0)
    print("mean gap", gap, "std ratio", ratio.min(), ratio.max())
    assert gap <= 0.25
    assert ratio.min() >= 0.6 and ratio.max() <= 1.3


def test_step_noise_is_fresh():
    """eps is keyed by the update count.  The same batch from the same parameters at counts 1
    and 0 (the count-0 handle is a fresh one holding the parameters of count 1): kl, a function
    of the parameters and the batch alone, agrees, and reconstruction_loss and loss, which see
    eps, differ -- as they do from the host restatement's draw of the other count."""
    D, L, B, w = 28, 4, 32, 10.0
    spec, tree, batches = parity_setup(PARITY_CASES[0])
    obs = batches[0][0]
    a = _trainer(spec, tree, B, w, seed=3)
    a.train_step(None, obs)                       # count 0 -> 1
    p1 = a.params
    _, logs1 = a.train_step(None, obs)            # at count 1
    b = _trainer(spec, p1, B, w, seed=3)
    _, logs0 = b.train_step(None, obs)            # the same parameters at count 0
    assert logs0["kl"] == logs1["kl"]
    assert abs(logs0["reconstruction_loss"] - logs1["reconstruction_loss"]) > 1e-4 * logs1["reconstruction_loss"]
    assert logs0["loss"] != logs1["loss"]
    for count, logs in ((0, logs0), (1, logs1)):
        _, want, _ = V.vae_step(V.f64(p1), obs, V.device_eps(3, count, B, L), w)
        for k in want:
            assert logs[k] == pytest.approx(want[k], rel=1e-4, abs=1e-7), (count, k)
    a.close()
    b.close()


def _raw_create(**kw):
    from fqlpop._lib import InitObsConfig, fptr, load_library
    lib = load_library()
    c = InitObsConfig()
    d = dict(obs_dim=28, latent_dim=4, hidden=(128,), batch_size=32, steps=10, init_lr=1e-3,
             reconstruction_weight=1.0, seed=0)
    d.update(kw)
    hid = d.pop("hidden")
    c.num_hidden = d.pop("num_hidden", len(hid))
    for i, h in enumerate(hid[:8]):
        c.hidden_dims[i] = h
    for k, val in d.items():
        setattr(c, k, val)
    n = ctypes.c_int64(-1)
    rc = lib.fqlpop_initobs_param_count(ctypes.byref(c), ctypes.byref(n))
    if rc != 0:
        return lib, rc, None, lib.fqlpop_last_error().decode()
    flat = np.zeros(n.value, np.float32)
    h = ctypes.c_void_p()
    rc = lib.fqlpop_initobs_create(ctypes.byref(c), fptr(flat), flat.size, 0, ctypes.byref(h))
    return lib, rc, h, lib.fqlpop_last_error().decode()


def test_error_paths():
    E_ARG, E_STATE, E_UNSUPPORTED = -1, -3, -4
    for kw in (dict(latent_dim=0), dict(latent_dim=65), dict(batch_size=100), dict(hidden=(8,) * 7),
               dict(hidden=(), num_hidden=0), dict(hidden=(513,)), dict(hidden=(0,))):
        _, rc, h, msg = _raw_create(**kw)
        assert rc == E_ARG and msg and not h, (kw, rc, msg)
    # six 512-wide layers: 2 x 3072 hidden activations x 16 rows x 4 bytes alone exceed 160 KB
    _, rc, h, msg = _raw_create(hidden=(512,) * 6)
    assert rc == E_UNSUPPORTED and "LDS" in msg and not h, (rc, msg)
    lib, rc, h, msg = _raw_create()
    assert rc == 0, msg
    from fqlpop._lib import fptr
    assert lib.fqlpop_initobs_step(h, 1) == E_STATE
    assert "set_dataset" in lib.fqlpop_last_error().decode()
    obs, logs = np.zeros((32, 28), np.float32), np.zeros(4, np.float32)
    assert lib.fqlpop_initobs_eval(h, fptr(obs), None, fptr(logs)) == E_ARG
    assert "eps" in lib.fqlpop_last_error().decode()
    out = np.zeros((1, 28), np.float32)
    assert lib.fqlpop_initobs_sample(h, 0, 0, None, fptr(out)) == E_ARG
    assert lib.fqlpop_initobs_sample(h, 1, 0, None, None) == E_ARG
    assert lib.fqlpop_initobs_set_dataset(h, None, 10) == E_ARG
    assert lib.fqlpop_initobs_set_dataset(h, fptr(obs), 0) == E_ARG
    n = ctypes.c_int64(-1)
    assert lib.fqlpop_initobs_get_count(h, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.fqlpop_initobs_destroy(h) == 0


def test_train_driver_then_simulated_task_from_generated_starts(tmp_path):
    """train_env_model.py --model=initial_observation writes the two files; the simulated task
    loads them and rolls a population out from decoded starts."""
    import envmodel as em
    import train_env_model as tem
    from fqlpop import Population, PopulationConfig
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    import yaml
    D, A, n = 28, 5, 8000
    rng = np.random.default_rng(0)
    obs = np.repeat(_manifold_data(n // 1000, D, seed=4), 1000, axis=0)  # 8 episodes; row 1000 k = start k
    ds = {"observations": obs, "actions": rng.uniform(-1, 1, (n, A)).astype(np.float32),
          "next_observations": obs, "rewards": np.full(n, -1.0, np.float32), "masks": np.ones(n, np.float32)}
    data = tmp_path / "data"
    data.mkdir()
    np.savez(data / "cube-single-play.npz", **ds)
    env = "cube-single-play-singletask-task2-v0"
    out = tem.main(["--model=initial_observation", "--steps=50", "--model.hidden_dims=(64,)", "--model.latent_dim=3",
                    "--reconstruction_weight=10", f"--env_name={env}", f"--data_directory={data}",
                    f"--save_directory={tmp_path / 'exp'}", "--val_batches=2"])
    with open(out / "initial_observation_config.yaml") as f:
        assert yaml.safe_load(f) == {"hidden_dims": [64], "latent_dim": 3}
    tree = em.load_flax_msgpack(out / "initial_observation.pt")["params"]
    assert tree["decoder"]["Dense_0"]["kernel"].shape == (3, 64) and tree["encoder"]["Dense_2"]["kernel"].shape == (64, 3)
    assert (out / "initial_observation_log.csv").exists()
    import evaluate_initial_observation_model as eio
    csv_path = eio.main([f"--env_name={env}", f"--data_directory={data}", f"--save_directory={tmp_path / 'exp'}",
                         "--num_samples=200"])
    lines = open(csv_path).read().strip().splitlines()
    assert len(lines) == 1 + D + 2 and lines[-1].startswith("pc_1,")

    # the world models beside it, so that the task and evaluate_env_model.py load everything from files
    common = [f"--env_name={env}", f"--data_directory={data}", f"--save_directory={tmp_path / 'exp'}",
              "--val_batches=1", "--steps=20"]
    tem.main(["--model=termination_predictor"] + common)
    tem.main(["--model=baseline", "--termination_weight=0"] + common)
    import evaluate_env_model as eem
    eem.main(["--model=baseline", "--eval_episodes=4", "--horizon=10", "--initial_observations=model"] + common)
    task = OfflineTaskWithSimulatedEvaluations(env, model="baseline", save_directory=tmp_path / "exp", dataset=ds,
                                               num_evaluation_envs=20, max_episode_steps=10,
                                               initial_observations="model")
    a, b, c = task.reset_observations(1), task.reset_observations(1), task.reset_observations(2)
    assert a.shape == (20, D) and a.dtype == np.float32 and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)
    want, _ = V.decode(V.f64({"decoder": tree["decoder"]})["decoder"], V.device_z(1, 20, 3))  # the saved decoder
    assert np.abs(a - want).max() <= 1e-4 * np.abs(want).max()
    pop = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(512,) * 4, batch_size=64), [10.0], [1])
    res = task.evaluate_members(pop, [0], seed=1)
    assert np.isfinite(res[0]["success"]) and np.isfinite(res[0]["episode_length"])
    pop.close()
    task.close()
