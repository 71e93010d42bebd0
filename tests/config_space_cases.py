"""Cases shared by tests/test_gpu_config_space.py and tests/test_oracle.py (not a test module):
trained-like states across the configuration space fqlpop_create accepts -- depth, num_qs,
input and head widths, flow_steps -- where every other parity test runs four hidden layers, two
Qs, 5 or 8 actions and 26-42 observations.

Every case is one population of two members (alphas 4 and 40, different state seeds), B = 64,
one step on injected batches and noise.  A two-member H = 512 population takes the split plan
by default.  The seeds (and ``head_scale`` where given) are chosen on the CPU so that the
float64 oracle alone meets _helpers.check_member_conditions (tests/test_oracle.py asserts it
for every entry); nothing here comes from a device's output."""
from _helpers import _MIN, Spec

ALPHAS = (4.0, 40.0)


def _case(H, seeds, L=4, D=28, A=5, head_scale=3.0, **kw):
    q_offset = kw.pop("q_offset", -40.0)
    return tuple(Spec(H, 64, s, a, D=D, A=A, q_offset=q_offset, kw=tuple(sorted(kw.items())), L=L,
                      head_scale=head_scale) for s, a in zip(seeds, ALPHAS))


# id -> (what it reaches, the two members)
_TABLE = {
    # ---- H = 512: depth
    "h512_l1": ("nothing splits; zero-size W^T arena", _case(512, (500, 501), L=1)),
    "h512_l2": ("split backward behind unsplit forwards", _case(512, (500, 501), L=2)),
    "h512_l3": ("smallest split forward / Euler", _case(512, (500, 502), L=3)),
    "h512_l8": ("EF_MAX_LAYERS, 8-problem fused dW", _case(512, (500, 501), L=8)),
    "h512_l9": ("per-layer fallback, per-layer dW GEMMs", _case(512, (501, 502), L=9)),
    # ---- H = 512: ensemble size
    "h512_e1": ("leaf layout without ensemble axis", _case(512, (500, 501), num_qs=1)),
    "h512_e3_min": ("three Qs, min", _case(512, (508, 515), num_qs=3, **_MIN)),
    "h512_e4_min": ("full sdq[4]", _case(512, (575, 585), num_qs=4, **_MIN)),
    "h512_e4": ("four Qs, mean", _case(512, (500, 502), num_qs=4)),
    # ---- H = 512: narrow inputs and heads
    "d2_a2": ("critic K0 = 4", _case(512, (500, 501), D=2, A=2)),
    "a1": ("one-output heads", _case(512, (527, 533), D=3, A=1, head_scale=6.0)),
    "a3": ("head width 3", _case(512, (500, 501), D=28, A=3)),
    "a4": ("head width 4: one k-step", _case(512, (500, 503), D=28, A=4)),
    "a6": ("head width 6", _case(512, (501, 503), D=27, A=6)),
    "a7": ("head width 7", _case(512, (501, 502), D=29, A=7)),
    # ---- H = 512: layer-0 width at the streamed kernels' limit
    "k0_64": ("K0bc = 64: last streamed width", _case(512, (500, 502), D=58, A=5)),
    "k0_65": ("K0bc = 65: per-layer fwd + streamed bwd", _case(512, (500, 501), D=59, A=5)),
    "k0_os65": ("K0os = 65 too", _case(512, (500, 501), D=60, A=5)),
    # ---- H = 512: Euler steps
    "s2": ("one Euler step in the persistent kernel", _case(512, (500, 501), flow_steps=2)),
    "s16": ("more than 11 Euler steps", _case(512, (500, 502), flow_steps=16)),
    # ---- H = 64: the per-layer path, unfused Adam, the loss kernels
    "h64_l1": ("per-layer path, one hidden layer", _case(64, (502, 504), L=1)),
    "h64_l2": ("per-layer path, two hidden layers", _case(64, (501, 503), L=2)),
    "h64_l10": ("two-digit leaf names", _case(64, (500, 502), L=10)),
    "h64_e1": ("unfused Adam without ensemble axis", _case(64, (502, 503), num_qs=1)),
    "h64_e4_min": ("loss kernels at four Qs, min", _case(64, (537, 542), num_qs=4, **_MIN)),
    "h64_a1": ("one-output heads, per-layer", _case(64, (509, 527), D=3, A=1)),
    "h64_s2": ("two Euler steps, per-layer", _case(64, (500, 501), flow_steps=2)),
    # ---- the committed argparser golden's (256, 256)
    "h256_l2": ("the golden's hidden_dims", _case(256, (501, 502), L=2)),
}
CASES = {k: v[1] for k, v in _TABLE.items()}

# the H = 512 depth and num_qs cases run a second time with engine option split = 0
UNSPLIT_TOO = ("h512_l1", "h512_l2", "h512_l3", "h512_l8", "h512_l9", "h512_e1", "h512_e3_min", "h512_e4_min",
               "h512_e4")

# (num_qs, num_hidden) at H = 512 around the transpose launch's 32-matrix table:
# (E + 2) * (L - 1) = 42, 36, 35 and 30
TR_CASES = ((4, 8), (4, 7), (3, 8), (4, 6))
_TR_SEEDS = {(4, 8): 503}


def tr_spec(num_qs, num_hidden):
    """The one member of a TR_CASES population."""
    return _case(512, (_TR_SEEDS.get((num_qs, num_hidden), 500),), L=num_hidden, num_qs=num_qs)[0]


# ---- moment bounds at depth ----
# MOMENT_REL was measured at L = 4; at L >= 8 the critic's layer-0 gradient passes through twice
# as many LayerNorm backwards.  depth_factor estimates on the CPU alone how much a correct fp32
# computation loses there: 3.7 and 2.4 for h512_l8's members, 3.3 and 4.1 for h512_l9's, 1.5 to
# 2.9 for the tr_spec members.  No case needs it: on an MI355X the deep cases' worst moment error
# is 0.022 of MOMENT_REL's bound (h512_l9; 0.019 at h512_l8, 0.012 at num_qs 4, L = 8), so every
# case is held to MOMENT_REL itself.
def _worst_f32_grad_error(spec):
    """The worst per-leaf gradient error, relative to the leaf's scale, of the oracle fed
    ``spec``'s state, batch and noise as float32 arrays against the same values in float64.
    numpy then computes in float32 (the oracle upcasts in places: a lower-precision proxy, not
    a true fp32 run)."""
    import numpy as np
    from _helpers import trained_member
    from oracle import fql_oracle as O
    tm = trained_member(spec)
    _, _, g64 = O.loss_and_grads(tm.cfg, tm.params, tm.batches[0], tm.noises[0])
    _, _, g32 = O.loss_and_grads(tm.cfg, O.cast_tree(tm.params, np.float32), O.cast_tree(tm.batches[0], np.float32),
                                 O.cast_tree(tm.noises[0], np.float32))
    worst = 0.0
    for net in O.TRAINABLE:
        for k, want in g64[net].items():
            scale = float(np.abs(want).max())
            if scale > 0:
                worst = max(worst, float(np.abs(g32[net][k].astype(np.float64) - want).max()) / scale)
    return worst


def depth_factor(spec):
    """max(1, error at ``spec``'s depth / error of its L = 4 twin), both as
    _worst_f32_grad_error."""
    return max(1.0, _worst_f32_grad_error(spec) / _worst_f32_grad_error(spec._replace(L=4)))
