"""Initial-observation VAE, the parts that need no GPU: the float64 restatement
(tests/initobs_np.py) against torch autograd, the C ABI's declarations and exports, the
flax tree order and file format, the loader, the host restatement of the device's normal
draw, and the simulated task's unchanged default."""
import os
import re

import numpy as np
import pytest
import torch

import initobs_np as V
from envmodel import initial_observation as io
from envmodel.flax_msgpack import msgpack_restore, msgpack_serialize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INITOBS_SYMBOLS = ("param_count", "create", "destroy", "set_dataset", "step", "step_injected", "eval", "read_logs",
                   "get_params", "get_count", "sync", "sample")


def _torch_step(tree, x, eps, w):
    t = {m: {l: {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in d.items()}
             for l, d in ls.items()} for m, ls in tree.items()}
    enc, dec = t["encoder"], t["decoder"]
    n = len(dec) - 1
    x, eps = torch.tensor(x, dtype=torch.float64), torch.tensor(eps, dtype=torch.float64)
    h = x
    for i in range(n):
        h = torch.relu(h @ enc[f"Dense_{i}"]["kernel"] + enc[f"Dense_{i}"]["bias"])
    mu = h @ enc[f"Dense_{n}"]["kernel"] + enc[f"Dense_{n}"]["bias"]
    lv = h @ enc[f"Dense_{n + 1}"]["kernel"] + enc[f"Dense_{n + 1}"]["bias"]
    z = mu + eps * torch.exp(0.5 * lv)
    for i in range(n):
        z = torch.relu(z @ dec[f"Dense_{i}"]["kernel"] + dec[f"Dense_{i}"]["bias"])
    xhat = z @ dec[f"Dense_{n}"]["kernel"] + dec[f"Dense_{n}"]["bias"]
    rec = torch.mean((x - xhat) ** 2)
    kl = -0.5 * torch.mean(1 + lv - mu ** 2 - torch.exp(lv))
    loss = (w * rec + kl) / (w + 1)
    loss.backward()
    grads = {m: {l: {k: v.grad.numpy() for k, v in d.items()} for l, d in ls.items()} for m, ls in t.items()}
    return loss.item(), {"reconstruction_loss": rec.item(), "kl": kl.item(), "loss": loss.item()}, grads


@pytest.mark.parametrize("w", [1.0, 10.0])
@pytest.mark.parametrize("hidden,latent", [((128,), 4), ((64, 32), 5)])
def test_restatement_gradients_match_autograd(w, hidden, latent):
    spec = io.InitialObservationSpec(28, latent, hidden)
    tree = V.f64(io.init_initial_observation(spec, 3))
    rng = np.random.default_rng(0)
    for mod in tree.values():  # non-zero biases, so that every term of the backward counts
        for layer in mod.values():
            layer["bias"] = 0.1 * rng.standard_normal(layer["bias"].shape)
    x, eps = rng.standard_normal((32, 28)), rng.standard_normal((32, latent))
    loss, logs, grads = V.vae_step(tree, x, eps, w)
    tloss, tlogs, tgrads = _torch_step(tree, x, eps, w)
    assert loss == pytest.approx(tloss, rel=1e-12)
    for k in tlogs:
        assert logs[k] == pytest.approx(tlogs[k], rel=1e-12)
    for mod in tgrads:
        for layer in tgrads[mod]:
            for leaf, want in tgrads[mod][layer].items():
                got = grads[mod][layer][leaf]
                assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (mod, layer, leaf)


def test_header_declares_and_library_exports_initobs_symbols():
    import fqlpop
    text = open(os.path.join(ROOT, "include", "fqlpop.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fqlpop_initobs_\w+)\s*\(", text))
    want = {f"fqlpop_initobs_{s}" for s in INITOBS_SYMBOLS}
    assert declared == want
    assert all(re.fullmatch(r"fqlpop_[a-z_]+", s) for s in declared)
    assert want <= set(fqlpop.EXPORTED_SYMBOLS)
    lib = fqlpop.load_library()
    assert not [s for s in want if not hasattr(lib, s)]


def test_tree_round_trip_and_file_format(tmp_path):
    spec = io.InitialObservationSpec(28, 5, (64, 32))
    tree = io.init_initial_observation(spec, 1)
    names = io.leaf_names(spec)
    assert names[:2] == [("decoder", "Dense_0", "bias"), ("decoder", "Dense_0", "kernel")]
    assert [n[0] for n in names] == ["decoder"] * 6 + ["encoder"] * 8
    assert names == sorted(names)
    shapes = dict(zip(names, io.leaf_shapes(spec)))
    assert shapes[("decoder", "Dense_0", "kernel")] == (5, 32)   # hidden_dims reversed
    assert shapes[("decoder", "Dense_2", "kernel")] == (64, 28)
    assert shapes[("encoder", "Dense_2", "kernel")] == (32, 5)   # mu
    assert shapes[("encoder", "Dense_3", "kernel")] == (32, 5)   # logvar, from the same hidden layer
    flat = io.flatten(spec, tree)
    assert flat.size == sum(int(np.prod(s)) for s in shapes.values())
    np.testing.assert_array_equal(flat[:32], tree["decoder"]["Dense_0"]["bias"])
    np.testing.assert_array_equal(flat[32:32 + 160], tree["decoder"]["Dense_0"]["kernel"].reshape(-1))
    back = io.unflatten(spec, flat)
    for mod, layer, leaf in names:
        np.testing.assert_array_equal(back[mod][layer][leaf], tree[mod][layer][leaf])
    # the .pt bytes: flax msgpack with the decoder where the reference's visualiser reads it
    restored = msgpack_restore(msgpack_serialize({"params": tree}))
    np.testing.assert_array_equal(restored["params"]["decoder"]["Dense_2"]["kernel"],
                                  tree["decoder"]["Dense_2"]["kernel"])
    io.save_initial_observation_model(tmp_path, spec, tree)
    spec2, params2 = io.load_initial_observation_model(tmp_path)
    assert (spec2.obs_dim, spec2.latent_dim, spec2.hidden_dims) == (28, 5, (64, 32))
    np.testing.assert_array_equal(io.flatten(spec2, params2), flat)
    with pytest.raises(ValueError):
        io.InitialObservationSpec(28, 4, (8,) * 7)


def test_initial_observation_loader_takes_episode_starts():
    from train_env_model import InitialObservationLoader
    n = 3500
    ds = {"observations": np.arange(n * 2, dtype=np.float32).reshape(n, 2), "actions": np.zeros((n, 1), np.float32),
          "rewards": np.arange(n, dtype=np.float32)}
    ld = InitialObservationLoader(ds)
    np.testing.assert_array_equal(ld.indices, [0, 1000, 2000, 3000])
    np.testing.assert_array_equal(ld.dataset["observations"], ds["observations"][[0, 1000, 2000, 3000]])
    np.testing.assert_array_equal(ld.dataset["rewards"], [0, 1000, 2000, 3000])
    b = ld.sample(64)
    assert b["observations"].shape == (64, 2)
    assert set(b["rewards"].tolist()) <= {0.0, 1000.0, 2000.0, 3000.0}
    assert len(ds["observations"]) == n  # the caller's dataset is left alone


def test_host_restatement_of_device_eps_is_standard_normal():
    n = 100_000
    e = V.device_eps(seed=1234, step=7, B=n // 4, L=4).reshape(-1)
    assert e.size == n
    # mean ~ N(0, 1/n); variance estimate has sd sqrt(2/n)
    assert abs(e.mean()) <= 3.0 / np.sqrt(n)
    assert abs(e.var() - 1.0) <= 3.0 * np.sqrt(2.0 / n)
    np.testing.assert_array_equal(e, V.device_eps(1234, 7, n // 4, 4).reshape(-1))
    assert not np.array_equal(e, V.device_eps(1234, 8, n // 4, 4).reshape(-1))   # fresh per step
    assert not np.array_equal(e, V.device_eps(1235, 7, n // 4, 4).reshape(-1))
    z = V.device_z(5, 1000, 4)
    assert z.shape == (1000, 4) and not np.array_equal(z, V.device_eps(5, 0, 1000, 4))  # own salt
    rows = V.device_rows(9, 3, 256, 1000)
    assert rows.min() >= 0 and rows.max() < 1000 and len(set(rows.tolist())) > 200


def test_simulated_task_default_is_unchanged_and_model_needs_files(tmp_path):
    from task.offline_task_simulated import OfflineTaskWithSimulatedEvaluations
    task = OfflineTaskWithSimulatedEvaluations(n_rows=5000, n_val_rows=1000, num_evaluation_envs=7, seed=0)
    starts = task.train_dataset["observations"][::1000]
    got = task.reset_observations(3)
    idx = np.random.default_rng(3).integers(0, len(starts), size=7)
    np.testing.assert_array_equal(got, starts[idx].astype(np.float32))
    assert task.initial_observation_source == "dataset"
    with pytest.raises(FileNotFoundError):
        OfflineTaskWithSimulatedEvaluations(n_rows=2000, n_val_rows=1000, initial_observations="model")
    em_dir = tmp_path / task.env_name / "env_models"
    em_dir.mkdir(parents=True)
    with pytest.raises(FileNotFoundError):
        io.load_initial_observation_model(em_dir)
    with pytest.raises(ValueError):
        OfflineTaskWithSimulatedEvaluations(n_rows=2000, n_val_rows=1000, initial_observations="vae")


def test_distribution_rows_statistics():
    from evaluate_initial_observation_model import distribution_rows
    rng = np.random.default_rng(0)
    real = rng.standard_normal((40, 3)) * np.array([3.0, 1.0, 0.1]) + np.array([1.0, 0.0, -2.0])
    rows = distribution_rows(real, real + 0.5)
    assert [r[0] for r in rows] == ["feature_0", "feature_1", "feature_2", "pc_0", "pc_1"]
    for i in range(3):
        assert rows[i][1] == pytest.approx(real[:, i].mean()) and rows[i][2] == pytest.approx(real[:, i].std())
        assert rows[i][3] == pytest.approx(real[:, i].mean() + 0.5) and rows[i][4] == pytest.approx(real[:, i].std())
    # the leading direction carries the widest feature; projections of the real data are centred
    assert rows[3][2] > rows[4][2] > 0.5 and abs(rows[3][1]) < 1e-12
    assert rows[3][2] == pytest.approx(np.linalg.svd(real - real.mean(0), compute_uv=False)[0] / np.sqrt(40))
