"""Per-member lr, discount and tau (fqlpop_set_member_hparams): the kernels read their
member's row of the device array by SLOT.

1. a mixed population against the float64 oracle from trained-like states, each member under
   its own OracleConfig (at the initial state target == critic and tau cannot be seen);
2. a mixed population against uniform twins whose PopulationConfig carries one member's values
   and which never call the new API: bitwise, on device-sampled steps;
3. the same with a member deactivated, so that the launch index differs from the slot;
4. a captured step graph sees a change without recapture;
5. the exact corners lr = 0, tau = 0, tau = 1;
6. clone_members copies the source's hparams, set_member keeps the slot's;
7. the argument checks of the ABI;
8. the tune_alpha.py driver: --lrs grids, resume, --pbt_explore.

Tolerances are the project's own: _helpers.REL for info values, OptimiserChecker with the
member's own lr and tau for the moments and the exact optimiser / EMA step.  (Depths other than
four, num_hidden = 1 among them, are stepped by tests/test_gpu_config_space.py.)"""
import csv
import ctypes
import functools
import pickle

import numpy as np
import pytest
import yaml

from oracle import fql_oracle as O
from _helpers import (TRAINED_COUNT, OptimiserChecker, check_info, engine_options, synthetic_rows,
                      trained_member)
from member_hparams_cases import HP0, HP1, HP2, MIXED

pytestmark = pytest.mark.gpu
ENV = "cube-single-play-singletask-task2-v0"
SMALL = "(64, 64, 64, 64)"
D, A, B = 28, 5, 64
ROWS = 20_011
CYCLE = (None, HP0, HP1, HP2)   # member i of the sampled populations has CYCLE[i % 4]


def _f32(hp):
    return {k: float(np.float32(v)) for k, v in hp.items()}


def _state(pop, i):
    return [pop.get_flat(i, w) for w in (0, 1, 2)]


def _same(a, b, tag):
    for j, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{tag}: state {j} differs in {int((x != y).sum())} elements"


# ----------------------------------------------------------- 1. oracle parity
def _trained_population(specs, hparams, use_graph=True):
    """``specs`` at their trained-like states in one population whose config has the default
    lr, discount and tau; member i gets ``hparams[i]`` through the new API."""
    from fqlpop import Population, PopulationConfig
    from fqlpop._lib import STATE_ADAM_M, STATE_ADAM_V
    s0 = specs[0]
    pc = PopulationConfig(obs_dim=s0.D, action_dim=s0.A, hidden_dims=(s0.H,) * s0.L, batch_size=s0.B,
                          use_graph=use_graph)
    pop = Population(pc, [s.alpha for s in specs], [11 + i for i in range(len(specs))], hparams=hparams)
    for i, s in enumerate(specs):
        tm = trained_member(s)
        pop.set_params(i, O.cast_tree(tm.params, np.float32))
        pop.set_flat(i, pop.tree_to_flat(tm.opt["m"]), STATE_ADAM_M)
        pop.set_flat(i, pop.tree_to_flat(tm.opt["v"]), STATE_ADAM_V)
        pop.set_count(i, TRAINED_COUNT)
    return pop


def _inject(pop, members, step):
    pop.step_injected([O.cast_tree(tm.batches[step], np.float32) for tm in members],
                      [O.cast_tree(tm.noises[step], np.float32) for tm in members])


def _run_mixed_parity(specs):
    pop = _trained_population(specs, [dict(s.kw) for s in specs])
    members = [trained_member(s) for s in specs]
    for i, tm in enumerate(members):
        assert (tm.cfg.lr, tm.cfg.discount, tm.cfg.tau) == tuple(dict(specs[i].kw)[k] for k in ("lr", "discount", "tau"))
    checks = [OptimiserChecker(pop, i, tm.cfg.lr, tm.cfg.tau) for i, tm in enumerate(members)]
    for step in range(specs[0].n_steps):
        for c in checks:
            c.before()
        _inject(pop, members, step)
        info = pop.read_info("train")
        for i, tm in enumerate(members):
            params_o, opt_o, info_o = tm.steps[step]
            tag = f"{specs[i]} step {step} member {i}"
            check_info(info[i], info_o, O.TRAIN_INFO_KEYS, tag)
            checks[i].after(params_o, opt_o, step + 1, tag)
    pop.close()


def test_oracle_parity_adam_kernel():
    """H = 64, two steps: loss_critic_kernel's discount and adam_kernel's lr and tau."""
    _run_mixed_parity(MIXED["h64"])


def test_oracle_parity_fused_epilogue():
    """H = 512 on the split launches: the fused dW epilogue and the small leaves riding in it."""
    _run_mixed_parity(MIXED["h512"])


def test_oracle_parity_unfused_at_h512():
    with engine_options(fused_adam=0):
        _run_mixed_parity(MIXED["h512"])


@pytest.mark.parametrize("name", ["h64", "h512"])
def test_total_loss_uses_the_members_discount(name):
    specs = MIXED[name]
    pop = _trained_population(specs, [dict(s.kw) for s in specs])
    members = [trained_member(s) for s in specs]
    info = pop.total_loss([O.cast_tree(tm.batches[0], np.float32) for tm in members],
                          [O.cast_tree(tm.noises[0], np.float32) for tm in members])
    for i, tm in enumerate(members):
        _, want = O.total_loss(tm.cfg, tm.params, tm.batches[0], tm.noises[0])
        check_info(info[i], want, O.VAL_INFO_KEYS, f"val {specs[i]}")
    pop.close()


# ------------------------------------------- 2, 3. uniform twins, slot != launch index
def _alphas_seeds(n):
    return [3.0 * 1.5 ** i for i in range(n)], [21 + i for i in range(n)]


@functools.lru_cache(maxsize=None)
def _sampled_run(H, n, use_graph, uniform=None, drop=None):
    """3 device-sampled steps of an n-member population.  ``uniform`` None: member i has
    CYCLE[i % 4] through the new API; else the index of the CYCLE entry the PopulationConfig
    carries for everyone, and the new API is never called.  ``drop``: a member deactivated
    before the steps.  Returns per member (info row, params, m, v), None for the dropped one."""
    from fqlpop import Population, PopulationConfig
    kw = dict(CYCLE[uniform] or {}) if uniform is not None else {}
    pc = PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * 4, batch_size=B, use_graph=use_graph, **kw)
    alphas, seeds = _alphas_seeds(n)
    if uniform is None:
        pop = Population(pc, alphas, seeds, hparams=[CYCLE[i % 4] for i in range(n)])
    else:
        pop = Population(pc, alphas, seeds)
    pop.set_dataset(synthetic_rows(ROWS, D, A, 5))
    if drop is not None:
        pop.set_active([i != drop for i in range(n)])
    pop.step(3)
    info = pop.read_info_array("train")
    out = [None if i == drop else (info[i].copy(), *_state(pop, i)) for i in range(n)]
    pop.close()
    return out


def _assert_rows_equal(got, want, tag):
    assert np.array_equal(got[0], want[0]), f"{tag}: info row differs"
    _same(got[1:], want[1:], tag)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("H,n", [(512, 4), (64, 16)])
def test_mixed_population_equals_uniform_twins(H, n, use_graph):
    mixed = _sampled_run(H, n, use_graph)
    for u in range(4):
        twin = _sampled_run(H, n, use_graph, uniform=u)
        for i in range(u, n, 4):
            _assert_rows_equal(mixed[i], twin[i], f"H={H} member {i} vs uniform {CYCLE[u]}")
    # and the values matter: the same member under other values is another member
    assert not np.array_equal(mixed[1][1], _sampled_run(H, n, use_graph, uniform=0)[1][1])


def test_hparams_follow_the_slot_not_the_launch_index():
    full = _sampled_run(64, 16, True)
    part = _sampled_run(64, 16, True, drop=0)
    assert part[0] is None
    for i in range(1, 16):
        _assert_rows_equal(part[i], full[i], f"member {i} at launch index {i - 1}")


# ------------------------------------------------------- 4. graph sees a change
@functools.lru_cache(maxsize=None)
def _change_run(H, use_graph, change):
    from fqlpop import Population, PopulationConfig
    pc = PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(H,) * 4, batch_size=B, use_graph=use_graph)
    alphas, seeds = _alphas_seeds(3)
    pop = Population(pc, alphas, seeds)
    pop.set_dataset(synthetic_rows(ROWS, D, A, 5))
    pop.step(2)
    if change:
        pop.set_member_hparams(1, **HP2)
    pop.step(2)
    info = pop.read_info_array("train")
    out = [(info[i].copy(), *_state(pop, i)) for i in range(3)]
    pop.close()
    return out


@pytest.mark.parametrize("H", [64, 512])
def test_captured_graph_sees_a_change(H):
    graph, eager, plain = _change_run(H, True, True), _change_run(H, False, True), _change_run(H, True, False)
    for i in range(3):
        _assert_rows_equal(graph[i], eager[i], f"H={H} member {i}: graph vs eager")
    for i in (0, 2):
        _assert_rows_equal(graph[i], plain[i], f"H={H} member {i}: beside the changed member")
    assert not np.array_equal(graph[1][1], plain[1][1]), "the change did not reach member 1"
    assert not np.array_equal(graph[1][0], plain[1][0]), "member 1's info is that of the old discount"


# ------------------------------------------------------------ 5. exact corners
def _corner_run(name, corner):
    """One injected step of MIXED[name] with member 1 under ``corner`` on top of its own
    values.  Returns (pre-step states, post-step states, counts, leaf table)."""
    specs = MIXED[name]
    hps = [dict(s.kw) for s in specs]
    hps[1] = dict(hps[1], **corner)
    pop = _trained_population(specs, hps)
    pre = [_state(pop, i) for i in range(len(specs))]
    _inject(pop, [trained_member(s) for s in specs], 0)
    post = [_state(pop, i) for i in range(len(specs))]
    counts = [pop.get_count(i) for i in range(len(specs))]
    leaves = pop.leaves
    pop.close()
    return pre, post, counts, leaves


def _leaf_slices(leaves, net):
    return [(slice(o, o + int(np.prod(s))), n.split("/", 1)[1]) for n, o, s in leaves if n.startswith(net + "/")]


@pytest.mark.parametrize("name", ["h64", "h512"])
def test_exact_corners(name):
    _, base, _, leaves = _corner_run(name, {})
    target = np.zeros(base[0][0].shape[0], dtype=bool)
    for sl, _ in _leaf_slices(leaves, "target_critic"):
        target[sl] = True
    critic_at = {leaf: sl for sl, leaf in _leaf_slices(leaves, "critic")}

    def beside(post, tag):
        for i in (0, 2):
            _same(post[i], base[i], f"{name} {tag}: member {i} beside the corner")

    pre, post, counts, _ = _corner_run(name, {"lr": 0.0})
    assert counts == [TRAINED_COUNT + 1] * 3
    assert np.array_equal(post[1][0][~target], pre[1][0][~target]), "lr = 0 moved parameters"
    assert not np.array_equal(post[1][1], pre[1][1]) and not np.array_equal(post[1][2], pre[1][2])
    _same(post[1][1:], base[1][1:], f"{name} lr=0: m and v are the gradients', whatever lr")
    assert np.array_equal(post[1][0][target], base[1][0][target])  # the EMA does not read lr
    beside(post, "lr=0")

    pre, post, _, _ = _corner_run(name, {"tau": 0.0})
    assert np.array_equal(post[1][0][target], pre[1][0][target]), "tau = 0 moved the target critic"
    assert np.array_equal(post[1][0][~target], base[1][0][~target])
    beside(post, "tau=0")

    pre, post, _, _ = _corner_run(name, {"tau": 1.0})
    for sl, leaf in _leaf_slices(leaves, "target_critic"):
        assert np.array_equal(post[1][0][sl], pre[1][0][critic_at[leaf]]), f"tau = 1: {leaf} is not the old critic"
    assert not np.array_equal(post[1][0][target], pre[1][0][target])
    beside(post, "tau=1")


# -------------------------------------------------------------------- 6. clone
def _clone_population(hparams):
    from fqlpop import Population, PopulationConfig
    pc = PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(64,) * 4, batch_size=B)
    alphas, seeds = _alphas_seeds(4)
    pop = Population(pc, alphas, seeds, hparams=hparams)
    pop.set_dataset(synthetic_rows(ROWS, D, A, 5))
    pop.step(2)
    return pop, alphas, seeds


def test_clone_copies_hparams_and_set_member_keeps_them():
    from fqlpop import Population, PopulationConfig
    pop, alphas, seeds = _clone_population(list(CYCLE))
    want = [_f32(hp) if hp else pop.member_hparams(0) for hp in CYCLE]
    assert [pop.member_hparams(i) for i in range(4)] == want
    # dst 0 (cfg values) <- src 2 (HP1), with src's alpha and seed: the same member twice
    pop.clone_members([2], [0], alphas=[alphas[2]], seeds=[seeds[2]])
    assert pop.member_hparams(0) == pop.member_hparams(2) == _f32(HP1)
    # dst 1 <- src 3 under HP0; the twin population sets HP0 by hand after a plain clone
    pop.clone_members([3], [1], alphas=[alphas[3]], seeds=[seeds[3]], hparams=HP0)
    assert pop.member_hparams(1) == _f32(HP0) and pop.member_hparams(3) == _f32(HP2)
    twin, _, _ = _clone_population(list(CYCLE))
    twin.clone_members([3], [1], alphas=[alphas[3]], seeds=[seeds[3]])
    assert twin.member_hparams(1) == _f32(HP2)
    twin.set_member_hparams(1, **HP0)
    pop.step(2)
    twin.step(2)
    _same(_state(pop, 0), _state(pop, 2), "clone without hparams: dst vs src")
    assert np.array_equal(pop.read_info_array("train")[0], pop.read_info_array("train")[2])
    _same(_state(pop, 1), _state(twin, 1), "clone with hparams vs the twin set by hand")
    assert not np.array_equal(_state(pop, 1)[0], _state(pop, 3)[0])
    # set_member leaves the slot's hparams, on the device too: after a reinit member 3 is a fresh
    # member (7.0, 99) under HP2, as slot 3 of a population whose config carries HP2
    pop.set_member(3, 7.0, 99, reinit=False)
    assert pop.member_hparams(3) == _f32(HP2)
    pop.set_member(3, 7.0, 99, reinit=True)
    assert pop.member_hparams(3) == _f32(HP2)
    pop.step(2)
    fresh = Population(PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(64,) * 4, batch_size=B, **HP2),
                       alphas[:3] + [7.0], seeds[:3] + [99])
    fresh.set_dataset(synthetic_rows(ROWS, D, A, 5))
    fresh.step(2)
    _same(_state(pop, 3), _state(fresh, 3), "reinit member under its kept hparams vs a fresh one")
    for p in (pop, twin, fresh):
        p.close()


# ---------------------------------------------------------------------- 7. ABI
def test_abi_argument_checks():
    from fqlpop import Population, PopulationConfig
    from fqlpop._lib import FqlpopError, fptr
    pc = PopulationConfig(obs_dim=D, action_dim=A, hidden_dims=(64,) * 4, batch_size=B, lr=2e-4, discount=0.98, tau=0.01)
    pop = Population(pc, [3.0, 30.0], [1, 2])
    created = _f32({"lr": 2e-4, "discount": 0.98, "tau": 0.01})
    assert pop.member_hparams(0) == pop.member_hparams(1) == created
    pop.set_member_hparams(1, tau=0.5)   # None keeps the current value
    held = [created, dict(created, tau=0.5)]
    nan, inf = float("nan"), float("inf")
    bad = [(-1, {}), (2, {}), (0, {"lr": nan}), (0, {"lr": inf}), (0, {"lr": -inf}), (0, {"lr": -1e-9}),
           (1, {"discount": -1e-6}), (1, {"discount": 1.0 + 1e-6}), (1, {"discount": nan}),
           (0, {"tau": -1e-6}), (0, {"tau": 1.0 + 1e-6}), (0, {"tau": nan})]
    for member, change in bad:
        hp = np.array([dict(created, **change)[k] for k in ("lr", "discount", "tau")], dtype=np.float32)
        rc = pop.lib.fqlpop_set_member_hparams(pop._h, member, fptr(hp))
        assert rc == -1, (member, change, rc)   # FQLPOP_E_ARG
        assert [pop.member_hparams(i) for i in range(2)] == held, (member, change)
    out = np.zeros(3, dtype=np.float32)
    assert pop.lib.fqlpop_get_member_hparams(pop._h, 2, fptr(out)) == -1
    assert pop.lib.fqlpop_set_member_hparams(pop._h, 0, ctypes.POINTER(ctypes.c_float)()) == -1
    with pytest.raises(FqlpopError):
        pop.set_member_hparams(0, lr=-1.0)
    # the ends of the ranges are allowed
    pop.set_member_hparams(0, lr=0.0, discount=1.0, tau=1.0)
    pop.set_member_hparams(0, discount=0.0, tau=0.0)
    assert pop.member_hparams(0) == {"lr": 0.0, "discount": 0.0, "tau": 0.0}
    with pytest.raises(ValueError):
        Population(pc, [3.0, 30.0], [1, 2], hparams=[None])
    pop.close()


# ------------------------------------------------------------------- 8. driver
def _driver_args(tmp_path, *more):
    return [f"--save_directory={tmp_path}", "--steps=200", "--eval_interval=100", "--log_interval=100",
            f"--agent.actor_hidden_dims={SMALL}", f"--agent.value_hidden_dims={SMALL}",
            "--agent.batch_size=64", "--agent.layer_norm", "--eval_episodes=4", "--synthetic_rows=5000",
            "--number_of_seeds=1", "--max_evaluations=100", *more]


def _record_trainers(monkeypatch):
    import tune_alpha
    from trainer.trainer import Trainer
    made = []

    class Recording(Trainer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(tune_alpha, "Trainer", Recording)
    return made


def test_tune_alpha_lr_grid_run_and_resume(tmp_path, monkeypatch):
    import tune_alpha
    made = _record_trainers(monkeypatch)
    grid = ("--number_of_alphas=2", "--lrs", "1e-4", "1e-3")
    args = _driver_args(tmp_path / "a", *grid)
    # four evaluations: one round of the four candidates, which stops the run at step 100
    tune_alpha.main([a for a in args if not a.startswith("--max_evaluations")] + ["--max_evaluations=4"])
    tune_alpha.main(args)   # resumed from checkpoint.pkl: the second hundred steps
    tune_alpha.main(_driver_args(tmp_path / "b", *grid))   # the same run in one piece
    assert len(made) == 3
    # the resumed members trained on under their own lr: bitwise the uninterrupted run's
    for cfg in made[2].experiments:
        a, b = (t.population.get_flat(t.member_of[cfg], 0) for t in (made[1], made[2]))
        assert np.array_equal(a, b), f"{cfg}: resumed and uninterrupted runs differ"
    by_pair = {}
    for cfg in made[1].experiments:
        by_pair.setdefault((cfg.alpha, cfg.seed), []).append(made[1].population.get_flat(made[1].member_of[cfg], 0))
    assert all(len(v) == 2 and not np.array_equal(*v) for v in by_pair.values())
    for trainer, root, step in ((made[0], tmp_path / "a", 100), (made[1], tmp_path / "a", 200),
                                (made[2], tmp_path / "b", 200)):
        assert len(trainer.experiments) == 4 and trainer.population.n == 4
        assert sorted(c.lr for c in trainer.experiments) == [1e-4, 1e-4, 1e-3, 1e-3]
        for cfg, exp in trainer.experiments.items():
            with open(root / ENV / exp.experiment_name / "config.yaml") as f:
                assert float(yaml.safe_load(f)["lr"]) == cfg.lr
            assert f"lr_{cfg.lr}" in exp.experiment_name
            want = _f32({"lr": cfg.lr, "discount": 0.99, "tau": 0.005})
            assert trainer.population.member_hparams(trainer.member_of[cfg]) == want
            assert exp.current_step == step
    assert set(made[0].experiments) == set(made[1].experiments)


def test_tune_alpha_pbt_explores_lr(tmp_path, monkeypatch):
    import tune_alpha
    made = _record_trainers(monkeypatch)
    tune_alpha.main(_driver_args(tmp_path, "--number_of_alphas=4", "--strategy=pbt", "--pbt_explore", "alpha", "lr",
                                 "--pbt_lr_min=1e-5", "--pbt_lr_max=1e-2"))
    trainer = made[0]
    with open(tmp_path / ENV / "pbt_lineage.csv") as f:
        rows = list(csv.DictReader(f))
    assert rows and list(rows[0]) == ["round", "step", "child", "parent", "parent_alpha", "child_alpha",
                                      "parent_score", "parent_lr", "child_lr"]
    by_name = {exp.experiment_name: cfg for cfg, exp in trainer.experiments.items()}
    checked = 0
    for row in rows:
        assert float(row["parent_lr"]) == 3e-4
        assert float(row["child_lr"]) in (3e-4 * 0.8, 3e-4 * 1.25)
        cfg = by_name.get(row["child"])
        if cfg is None:   # (a child replaced later in the run)
            continue
        assert cfg.lr == float(row["child_lr"])
        got = trainer.population.member_hparams(trainer.member_of[cfg])
        assert got == _f32({"lr": cfg.lr, "discount": 0.99, "tau": 0.005})
        checked += 1
    assert checked >= 1
    with open(tmp_path / ENV / "checkpoint.pkl", "rb") as f:
        state = pickle.load(f)
    assert any(c.lr is not None for c in state["trainer"]["experiments"])
