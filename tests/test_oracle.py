"""CPU tests of the oracle (oracle/fql_oracle.py): known answers, finite
differences, an independent autograd implementation, and the golden fixture."""
import math
import os

import numpy as np
import pytest

from oracle import fql_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def small_cfg(**kw):
    kw.setdefault("hidden_dims", (16, 16, 16, 16))
    kw.setdefault("batch_size", 8)
    return O.OracleConfig(**kw)


def test_gelu_tanh_formula_and_grad():
    x = np.linspace(-6, 6, 101)
    want = 0.5 * x * (1 + np.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    assert np.allclose(O.gelu(x), want, rtol=0, atol=0)
    eps = 1e-6
    fd = (O.gelu(x + eps) - O.gelu(x - eps)) / (2 * eps)
    assert np.allclose(O.gelu_grad(x), fd, atol=1e-8)


def test_layer_norm_fast_variance():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((4, 32)) * 3 + 1
    mu, rstd = O.layer_norm_stats(g)
    assert np.allclose(mu[:, 0], g.mean(1))
    assert np.allclose(1 / rstd[:, 0] ** 2, g.var(1) + 1e-6)
    # constant row: fast variance may round below zero -> clipped, rstd = 1/sqrt(eps)
    mu, rstd = O.layer_norm_stats(np.full((1, 8), 0.3))
    assert np.isclose(rstd[0, 0], 1 / math.sqrt(1e-6))


def test_init_shapes_and_counts():
    cfg = O.OracleConfig()
    p = O.init_params(cfg, 0)
    count = {net: sum(v.size for v in p[net].values()) for net in O.NETS}
    # 809 985 per critic member, 808 453 bc, 807 941 onestep
    assert count["critic"] == 2 * 809_985
    assert count["target_critic"] == count["critic"]
    assert count["actor_bc_flow"] == 808_453
    assert count["actor_onestep_flow"] == 807_941
    lim = math.sqrt(6 / (33 + 512))
    assert np.abs(p["critic"]["Dense_0/kernel"]).max() <= lim
    assert np.all(p["critic"]["Dense_0/bias"] == 0) and np.all(p["critic"]["LayerNorm_0/scale"] == 1)


def test_euler_with_zero_velocity_net_is_clipped_noise():
    cfg = small_cfg()
    p = O.init_params(cfg, 0)
    for k in p["actor_bc_flow"]:
        p["actor_bc_flow"][k] = np.zeros_like(p["actor_bc_flow"][k])
    z = np.random.default_rng(1).standard_normal((8, 5)) * 2
    out = O.compute_flow_actions(cfg, p, np.zeros((8, 28)), z)
    assert np.array_equal(out, np.clip(z, -1, 1))


def test_euler_constant_velocity_integrates_exactly():
    cfg = small_cfg()
    p = O.init_params(cfg, 0)
    net = p["actor_bc_flow"]
    for k in net:
        net[k] = np.zeros_like(net[k])
    net["Dense_4/bias"] = np.full(5, 0.3)  # v = 0.3 everywhere
    z = np.zeros((4, 5))
    out = O.compute_flow_actions(cfg, p, np.zeros((4, 28)), z)
    assert np.allclose(out, 0.3)


def _loss_only(cfg, params, batch, noise):
    loss, _, _ = O.loss_and_grads(cfg, params, batch, noise, want_grads=False)
    return loss


# (name, config fields, q_offset of trained_like_params or None for init_params).  The
# trained-like states have non-zero biases, LayerNorm scale != 1 and bias != 0, target !=
# critic and a good share of saturated actor outputs; "min" keeps Q centred at 0 (mixed
# signs), where normalize_q_loss's lambda is not 1 / |mean Q| and the min is a real choice.
STATES = [
    ("init", {}, None),
    ("trained", {}, -40.0),
    ("trained_min", {"q_agg": "min", "normalize_q_loss": True}, 0.0),
    ("trained_actor_ln", {"actor_layer_norm": True}, -40.0),
]
FD_KEYS = [
    ("critic", "Dense_0/kernel"), ("critic", "LayerNorm_1/scale"), ("critic", "Dense_4/bias"),
    ("actor_bc_flow", "Dense_2/kernel"), ("actor_onestep_flow", "Dense_0/kernel"),
    ("actor_onestep_flow", "Dense_4/kernel"),
]
FD_KEYS_TRAINED = FD_KEYS + [
    ("critic", "Dense_2/bias"), ("critic", "LayerNorm_0/bias"), ("actor_bc_flow", "Dense_4/bias"),
    ("actor_onestep_flow", "Dense_1/bias"),
]
FD_KEYS_ACTOR_LN = [("actor_onestep_flow", "LayerNorm_2/scale"), ("actor_bc_flow", "LayerNorm_0/bias")]


def _state_params(cfg, seed, q_offset):
    return O.init_params(cfg, seed) if q_offset is None else O.trained_like_params(cfg, seed, q_offset=q_offset)


def _fd_cases():
    for name, kw, q_offset in STATES[1:]:
        keys = FD_KEYS_TRAINED + (FD_KEYS_ACTOR_LN if kw.get("actor_layer_norm") else [])
        for net, key in keys:
            yield pytest.param(kw, q_offset, net, key, id=f"{name}-{net}-{key}")


@pytest.mark.parametrize("net,key", FD_KEYS)
def test_gradients_match_finite_differences(net, key):
    _check_finite_differences({}, None, net, key)


@pytest.mark.parametrize("kw,q_offset,net,key", list(_fd_cases()))
def test_gradients_match_finite_differences_trained(kw, q_offset, net, key):
    _check_finite_differences(kw, q_offset, net, key)


def _check_finite_differences(kw, q_offset, net, key, seed=3):
    # each net's own objective: critic <- critic loss (the actor's Q term reads
    # frozen critic params); bc <- BC loss (the Euler target is stop-gradient);
    # onestep <- actor loss, with normalize_q_loss's lambda held (it is a stop-gradient)
    cfg = small_cfg(alpha=3.0, **kw)
    rng = np.random.default_rng(7)
    params = _state_params(cfg, seed, q_offset)
    batch, noise = O.make_batch(cfg, 8, rng), O.make_noise(cfg, 8, rng)
    # clip(a_pi) has a kink at +-1, where a central difference is not the gradient: probe on
    # the rows whose a_pi entries are all at least 1e-3 away from it
    a_pi = O.sample_actions(cfg, params, batch["observations"], noise["z_d"], clip=False)
    rows = np.all(np.abs(np.abs(a_pi) - 1.0) >= 1e-3, axis=1)
    assert rows.sum() >= 6
    batch = {k: v[rows] for k, v in batch.items()}
    noise = {k: v[rows] for k, v in noise.items()}
    if q_offset is not None:  # the state is worth probing: the clip engages and also does not
        assert 0 < (np.abs(a_pi[rows]) > 1.0).sum() < a_pi[rows].size
    _, info0, grads = O.loss_and_grads(cfg, params, batch, noise)
    lam = -info0["actor/q_loss"] / info0["actor/q"]
    assert cfg.normalize_q_loss or lam == 1.0
    arr = params[net][key]
    flat_idx = rng.choice(arr.size, size=min(6, arr.size), replace=False)
    eps = 1e-6

    def objective(pp):
        _, info, _ = O.loss_and_grads(cfg, pp, batch, noise, want_grads=False)
        if net == "critic":
            return info["critic/critic_loss"]
        if net == "actor_bc_flow":  # the flow target (distill) is a stop-gradient path
            return info["actor/bc_flow_loss"]
        return info["actor/bc_flow_loss"] + cfg.alpha * info["actor/distill_loss"] - lam * info["actor/q"]

    for fi in flat_idx:
        idx = np.unravel_index(fi, arr.shape)
        orig = arr[idx]
        arr[idx] = orig + eps
        lp = objective(params)
        arr[idx] = orig - eps
        lm = objective(params)
        arr[idx] = orig
        fd = (lp - lm) / (2 * eps)
        g = grads[net][key][idx]
        assert abs(fd - g) <= 1e-6 + 1e-5 * abs(g), (net, key, idx, fd, g)


def test_gradients_match_torch_autograd():
    _check_torch_autograd(None)


@pytest.mark.parametrize("q_offset", [-40.0, 0.0], ids=["q_minus_40", "mixed_sign_q"])
def test_gradients_match_torch_autograd_trained(q_offset):
    _check_torch_autograd(q_offset)


def _check_torch_autograd(q_offset):
    torch = pytest.importorskip("torch")  # noqa: F841
    from oracle.fql_torch import grads_autograd
    for kw in ({}, {"q_agg": "min", "normalize_q_loss": True}, {"layer_norm": False, "actor_layer_norm": True},
               {"actor_layer_norm": True}):
        cfg = small_cfg(**kw)
        rng = np.random.default_rng(11)
        p = _state_params(cfg, 2, q_offset)
        b, n = O.make_batch(cfg, 8, rng), O.make_noise(cfg, 8, rng)
        loss, info, g = O.loss_and_grads(cfg, p, b, n)
        l2, i2, g2 = grads_autograd(cfg, p, b, n)
        assert abs(loss - l2) < 1e-10
        for k in info:
            assert abs(info[k] - i2[k]) < 1e-10, k
        for net in O.NETS:
            for k in g[net]:
                assert np.allclose(g[net][k], g2[net][k], atol=1e-11, rtol=1e-9), (kw, net, k)


def test_adam_first_step_closed_form_and_ema():
    cfg = small_cfg()
    rng = np.random.default_rng(3)
    p = O.init_params(cfg, 1)
    b, n = O.make_batch(cfg, 8, rng), O.make_noise(cfg, 8, rng)
    _, _, g = O.loss_and_grads(cfg, p, b, n)
    p1, opt, info = O.update(cfg, p, O.init_opt_state(p), b, n)
    for net in ("critic", "actor_bc_flow", "actor_onestep_flow"):
        for k in p[net]:
            gg = g[net][k]
            # step 1: m_hat = g, v_hat = g^2 -> p - lr * g / (|g| + eps)
            want = p[net][k] - cfg.lr * gg / (np.abs(gg) + 1e-8)
            assert np.allclose(p1[net][k], want, rtol=1e-9, atol=1e-14), (net, k)
    for k in p["critic"]:
        want = cfg.tau * p["critic"][k] + (1 - cfg.tau) * p["target_critic"][k]
        assert np.allclose(p1["target_critic"][k], want)
    assert opt["count"] == 1
    # grad stats include the zero target leaves
    assert info["grad/max"] >= 0.0 >= info["grad/min"]


def test_total_loss_matches_update_info():
    cfg = small_cfg()
    rng = np.random.default_rng(4)
    p = O.init_params(cfg, 1)
    b, n = O.make_batch(cfg, 8, rng), O.make_noise(cfg, 8, rng)
    loss, vinfo = O.total_loss(cfg, p, b, n)
    _, _, tinfo = O.update(cfg, p, O.init_opt_state(p), b, n)
    for k in O.VAL_INFO_KEYS:
        assert vinfo[k] == tinfo[k]
    assert np.isclose(loss, vinfo["critic/critic_loss"] + vinfo["actor/actor_loss"])


def test_oracle_reproduces_golden_fixture():
    g = np.load(os.path.join(GOLDEN, "oracle_update_h64.npz"))
    H, B, alpha = g["config"]
    cfg = O.OracleConfig(hidden_dims=(int(H),) * 4, batch_size=int(B), alpha=float(alpha))
    p = {net: {} for net in O.NETS}
    for key in g.files:
        if key.startswith("params_in/"):
            _, net, leaf = key.split("/", 2)
            p[net][leaf] = g[key].astype(np.float64)
    opt = O.init_opt_state(p)
    for step in range(2):
        b = {k.split("/", 1)[1]: g[k].astype(np.float64) for k in g.files if k.startswith(f"batch{step}/")}
        n = {k.split("/", 1)[1]: g[k].astype(np.float64) for k in g.files if k.startswith(f"noise{step}/")}
        p, opt, info = O.update(cfg, p, opt, b, n)
        got = np.array([info[k] for k in O.TRAIN_INFO_KEYS])
        assert np.allclose(got, g[f"info{step}"], rtol=1e-12, atol=1e-14)
    for key in g.files:
        if key.startswith("params_out/"):
            _, net, leaf = key.split("/", 2)
            assert np.array_equal(p[net][leaf].astype(np.float32), g[key])


# ---------------------------------------------------------------------------
# the trained-like state: what it can see that the initial state cannot
# ---------------------------------------------------------------------------
def _edit(params, fn):
    """A copy of ``params`` with fn(net, leaf name, array) -> array applied to every leaf."""
    return {net: {k: fn(net, k, v.copy()) for k, v in p.items()} for net, p in params.items()}


def _zero_dense_bias(nets):
    return lambda net, k, v: v * 0.0 if net in nets and k.startswith("Dense_") and k.endswith("/bias") else v


# name -> (edit of the parameters or None, _mutant keyword of O.update or None, Adam reset)
KERNEL_MISTAKES = {
    "critic Dense biases dropped": (_zero_dense_bias(("critic",)), None, False),
    "target critic Dense biases dropped": (_zero_dense_bias(("target_critic",)), None, False),
    "BC flow actor Dense biases dropped": (_zero_dense_bias(("actor_bc_flow",)), None, False),
    "one-step actor Dense biases dropped": (_zero_dense_bias(("actor_onestep_flow",)), None, False),
    "ensemble member 1 reads member 0's Dense biases": (
        lambda net, k, v: np.stack([v[0]] * len(v)) if net in ("critic", "target_critic") and k.startswith("Dense_")
        and k.endswith("/bias") else v, None, False),
    "LayerNorm scale taken as 1": (lambda net, k, v: v * 0.0 + 1.0 if k.endswith("/scale") else v, None, False),
    "LayerNorm bias taken as 0": (
        lambda net, k, v: v * 0.0 if k.startswith("LayerNorm") and k.endswith("/bias") else v, None, False),
    "TD target from the online critic": (None, "target_is_critic", False),
    "Q gradient through a saturated clip(a_pi)": (None, "inside_all_true", False),
    "Euler result not clipped": (None, "euler_unclipped", False),
    "a_next not clipped": (None, "a_next_unclipped", False),
    "metric actions not clipped": (None, "metric_unclipped", False),
    "Adam restarted from m = v = 0, count = 0": (None, None, True),
}
# What the initial state, at its first step, cannot see (this test documents it).  It does see
# a missing Euler clip -- the flow starts from N(0, 1) noise, a third of which is outside
# [-1, 1], and hardly moves it -- and nothing else in the list.
BLIND_AT_INIT = set(KERNEL_MISTAKES) - {"Euler result not clipped"}


def _moved(cfg, right, wrong):
    """The checked quantities that differ between two oracle updates by at least 10x the bound
    the GPU tests hold them to: info values (REL, with its floor), and each leaf's new Adam
    m and v (MOMENT_REL of the leaf's scale)."""
    from _helpers import MOMENT_REL, REL
    (_, opt_r, info_r), (_, opt_w, info_w) = right, wrong
    out = []
    for k in O.TRAIN_INFO_KEYS:
        a, b = float(info_r[k]), float(info_w[k])
        if abs(a - b) >= 10 * (REL * max(abs(a), abs(b)) + 1e-6):
            out.append(k)
    for what in ("m", "v"):
        for net in O.TRAINABLE:
            for k, a in opt_r[what][net].items():
                if np.abs(a - opt_w[what][net][k]).max() >= 10 * MOMENT_REL * np.abs(a).max() > 0:
                    out.append(f"{net}/{k} adam {what}")
    return out


def _with_mistake(cfg, params, opt, batch, noise, mistake):
    edit, mutant, reset = KERNEL_MISTAKES[mistake]
    if edit is not None:
        params = _edit(params, edit)
    if mutant == "target_is_critic":
        params = dict(params, target_critic=params["critic"])
        mutant = None
    if reset:
        opt = O.init_opt_state(params)
    return O.update(cfg, params, opt, batch, noise, _mutant=mutant)


@pytest.mark.parametrize("mistake", list(KERNEL_MISTAKES))
@pytest.mark.parametrize("variant", ["q_minus_40", "min_mixed_sign_q"])
def test_trained_like_state_separates_kernel_mistakes(variant, mistake):
    """Each way a kernel could be wrong that the initial state hides -- an update computed
    with that mistake equals the correct one there -- moves, from the trained-like state the
    GPU parity tests start at, at least one quantity those tests check by 10x its bound."""
    from _helpers import TRAINED, trained_member
    tm = trained_member(TRAINED["h64" if variant == "q_minus_40" else "h64_min"][0])
    cfg, b, n = tm.cfg, tm.batches[0], tm.noises[0]
    moved = _moved(cfg, tm.steps[0], _with_mistake(cfg, tm.params, tm.opt, b, n, mistake))
    assert moved, f"{mistake}: nothing moves at the trained-like state"
    print(f"{mistake}: moves {moved[:6]}{' ...' if len(moved) > 6 else ''}")
    # the same mistake from init_params (first step, zero moments), same batch and noise
    p0 = O.init_params(cfg, tm.spec.seed)
    o0 = O.init_opt_state(p0)
    moved0 = _moved(cfg, O.update(cfg, p0, o0, b, n), _with_mistake(cfg, p0, o0, b, n, mistake))
    if mistake in BLIND_AT_INIT:
        assert not moved0, f"{mistake}: the initial state sees it too ({moved0[:6]})"
    else:
        assert moved0


def _trained_specs():
    from _helpers import ALL_TRAINED_SPECS
    return ALL_TRAINED_SPECS


@pytest.mark.parametrize("spec", _trained_specs(), ids=lambda s: f"h{s.H}-b{s.B}-d{s.D}-seed{s.seed}-a{s.alpha:g}"
                         + ("-min" if s.q_offset == 0 else "") + ("-sampled" if s.sampled else ""))
def test_trained_like_state_conditions(spec):
    """Conditions on every state tests/test_gpu_parity_trained.py starts from, in float64: at
    each clamp (a_pi, the Euler result, a_next, the metric actions) 15-85 % of the entries
    are outside [-1, 1] and none within 1e-4 of +-1, at every step the test takes; with
    q_agg = min each ensemble member is the minimum in at least 15 % of the rows; and the
    state is trained-like (target != critic in every leaf, moments non-zero except the
    target's)."""
    _check_state_conditions(spec)


def _config_space_specs():
    from config_space_cases import CASES, TR_CASES, tr_spec
    out = [pytest.param(s, id=f"{name}-{i}") for name, group in CASES.items() for i, s in enumerate(group)]
    return out + [pytest.param(tr_spec(e, l), id=f"tr_e{e}_l{l}") for e, l in TR_CASES]


@pytest.mark.parametrize("spec", _config_space_specs())
def test_trained_like_state_conditions_config_space(spec):
    """The same conditions on every state of tests/config_space_cases.py."""
    _check_state_conditions(spec)


def _check_state_conditions(spec):
    from _helpers import check_member_conditions, trained_member
    tm = trained_member(spec)
    check_member_conditions(tm)
    head_bias = f"Dense_{spec.L}/bias"
    for k, v in tm.params["critic"].items():
        d = np.abs(tm.params["target_critic"][k] - v)
        assert (d > 0).mean() > 0.99 and d.mean() >= 0.1 * np.abs(v - (spec.q_offset if k == head_bias else 0)).mean(), k
    for net in O.TRAINABLE:
        for k, m in tm.opt["m"][net].items():
            assert m.all() and (tm.opt["v"][net][k] > 0).all(), (net, k)
            assert m.size < 16 or ((m > 0).any() and (m < 0).any()), (net, k)
    assert not any(np.any(x) for w in ("m", "v") for x in tm.opt[w]["target_critic"].values())
    assert tm.opt["count"] == 1000
    if spec.q_offset == 0:   # mixed-sign Q: normalize_q_loss's lambda is not 1 / |mean Q|
        info = tm.steps[0][2]
        assert abs(info["actor/q_loss"]) < 0.99


def test_trained_like_action_and_rollout_conditions():
    """The same clamp conditions for what the sample_actions and rollout GPU tests feed the
    one-step actor's head."""
    from _helpers import (ACTION_SPECS, ROLLOUT_SPECS, action_probe, check_clamp_conditions, rollout_raw_actions,
                          trained_member)
    for spec in ACTION_SPECS:
        tm = trained_member(spec)
        obs, z = action_probe(spec)
        raw = O.sample_actions(tm.cfg, tm.params, obs.astype(np.float64), z.astype(np.float64), clip=False)
        check_clamp_conditions(raw, f"sample_actions {spec}")
    for i, spec in enumerate(ROLLOUT_SPECS):
        check_clamp_conditions(rollout_raw_actions(i), f"rollout {spec}")


# ---------------------------------------------------------------------------
# the configuration space beyond small_cfg's four hidden layers, two Qs and five actions
# (tests/config_space_cases.py runs the device there)
# ---------------------------------------------------------------------------
_MIN_KW = {"q_agg": "min", "normalize_q_loss": True}
CONFIG_SPACE = {
    "l1": {"hidden_dims": (16,)},
    "l2": {"hidden_dims": (16, 16)},
    "l10": {"hidden_dims": (16,) * 10},
    "e1": {"num_qs": 1},
    "e1_min": {"num_qs": 1, **_MIN_KW},
    "e3": {"num_qs": 3},
    "e3_min": {"num_qs": 3, **_MIN_KW},
    "e4": {"num_qs": 4},
    "e4_min": {"num_qs": 4, **_MIN_KW},
    "a1": {"obs_dim": 3, "action_dim": 1},
    "s2": {"flow_steps": 2},
}


def _config_space_q_offset(kw):
    return 0.0 if kw.get("q_agg") == "min" else -40.0


@pytest.mark.parametrize("name", list(CONFIG_SPACE))
def test_gradients_match_torch_autograd_config_space(name):
    """The oracle's hand-written backward against torch autograd at the trained-like state, at
    the depths, ensemble sizes, head width and flow_steps the other checks never leave."""
    pytest.importorskip("torch")
    from oracle.fql_torch import grads_autograd
    kw = CONFIG_SPACE[name]
    cfg = small_cfg(**kw)
    rng = np.random.default_rng(11)
    p = O.trained_like_params(cfg, 2, q_offset=_config_space_q_offset(kw))
    b, n = O.make_batch(cfg, 8, rng), O.make_noise(cfg, 8, rng)
    loss, info, g = O.loss_and_grads(cfg, p, b, n)
    l2, i2, g2 = grads_autograd(cfg, p, b, n)
    assert abs(loss - l2) < 1e-10
    for k in info:
        assert abs(info[k] - i2[k]) < 1e-10, k
    for net in O.NETS:
        assert set(g[net]) == set(g2[net]) == set(O.leaf_order(cfg, net))
        for k in g[net]:
            assert g[net][k].shape == p[net][k].shape == g2[net][k].shape, (net, k)
            assert np.allclose(g[net][k], g2[net][k], atol=1e-11, rtol=1e-9), (name, net, k)


def _config_space_fd_cases():
    for name, kw in CONFIG_SPACE.items():
        L = len(kw.get("hidden_dims", (16,) * 4))
        # one probe per net: the critic's first kernel (the whole backward chain), the BC
        # actor's head, the one-step actor's first kernel
        for net, key in (("critic", "Dense_0/kernel"), ("actor_bc_flow", f"Dense_{L}/kernel"),
                         ("actor_onestep_flow", "Dense_0/kernel")):
            yield pytest.param(kw, net, key, FD_STATE_SEED.get(name, 3), id=f"{name}-{net}")


# with one action and eight rows, state 3 saturates no a_pi entry; state 8 saturates four
FD_STATE_SEED = {"a1": 8}


@pytest.mark.parametrize("kw,net,key,seed", list(_config_space_fd_cases()))
def test_gradients_match_finite_differences_config_space(kw, net, key, seed):
    _check_finite_differences(kw, _config_space_q_offset(kw), net, key, seed=seed)


def _first_two_only(tm):
    """critic/critic_loss and actor/q of ``tm``'s first step as an update would report them
    that aggregates only the first two ensemble members, in the TD target and in the actor's Q
    term (a plain restatement on the oracle's forwards)."""
    cfg, p, b, n = tm.cfg, tm.params, tm.batches[0], tm.noises[0]
    a_next = O.sample_actions(cfg, p, b["next_observations"], n["z_next"])
    qt, _ = O.value_forward(cfg, p["target_critic"], b["next_observations"], a_next)
    q_next = qt[:2].min(0) if cfg.q_agg == "min" else qt[:2].mean(0)
    y = b["rewards"] + cfg.discount * b["masks"] * q_next
    q, _ = O.value_forward(cfg, p["critic"], b["observations"], b["actions"])
    a_pi = O.sample_actions(cfg, p, b["observations"], n["z_d"])
    qpi, _ = O.value_forward(cfg, p["critic"], b["observations"], a_pi)
    return ((q - y[None]) ** 2).mean(), qpi[:2].mean(0).mean(), qt, qpi


@pytest.mark.parametrize("case", ["h512_e3_min", "h512_e4_min", "h512_e4", "h64_e4_min"])
def test_more_than_two_qs_separate_a_two_q_aggregate(case):
    """At num_qs 3 and 4 an update that aggregates only the first two ensemble members, as
    every other parity test's E = 2 would let pass, moves critic/critic_loss (the TD target)
    and actor/q (the actor's Q term) by at least 10x REL."""
    from _helpers import REL, trained_member
    from config_space_cases import CASES
    for spec in CASES[case]:
        tm = trained_member(spec)
        info = tm.steps[0][2]
        loss2, q2, qt, qpi = _first_two_only(tm)
        # the restatement with every member is the oracle's own value
        q_next = qt.min(0) if tm.cfg.q_agg == "min" else qt.mean(0)
        assert np.isclose(qpi.mean(0).mean(), info["actor/q"], rtol=1e-12, atol=0)
        assert not np.allclose(q_next, qt[:2].min(0) if tm.cfg.q_agg == "min" else qt[:2].mean(0))
        for key, wrong in (("critic/critic_loss", loss2), ("actor/q", q2)):
            right = float(info[key])
            assert abs(right - wrong) >= 10 * (REL * max(abs(right), abs(wrong)) + 1e-6), (spec, key, right, wrong)


def test_two_digit_layers_sort_by_name_not_by_layer():
    """At ten hidden layers the flat state's leaf order (flax: sorted by name) puts Dense_10
    before Dense_2: a flat vector assembled in layer order differs from the correct one."""
    from _helpers import trained_member
    from config_space_cases import CASES
    tm = trained_member(CASES["h64_l10"][0])
    for net in O.NETS:
        names = O.leaf_order(tm.cfg, net)
        assert names.index("Dense_10/kernel") < names.index("Dense_2/kernel")
        by_layer = sorted(names, key=lambda k: (k.split("_")[0], int(k.split("_")[1].split("/")[0]), k))
        assert by_layer != names and sorted(by_layer) == names
        right = np.concatenate([tm.params[net][k].reshape(-1) for k in names])
        wrong = np.concatenate([tm.params[net][k].reshape(-1) for k in by_layer])
        assert right.shape == wrong.shape and (right != wrong).mean() > 0.5

