"""Cases shared by tests/test_gpu_member_hparams.py and tests/test_member_hparams_cpu.py
(not a test module): the three hyper-parameter sets and the trained-like states of the mixed
populations.  The seeds are chosen so that the float64 oracle alone meets
_helpers.check_member_conditions under each member's OWN discount (the CPU file asserts it);
at H = 64 the seeds 502-505 and 507 do not (clamp share or the 1e-4 margin)."""
from _helpers import Spec

HP0 = {"lr": 1e-4, "discount": 0.9, "tau": 0.001}
HP1 = {"lr": 3e-4, "discount": 0.99, "tau": 0.005}
HP2 = {"lr": 1e-3, "discount": 0.995, "tau": 0.05}
HPS = (HP0, HP1, HP2)
ALPHAS = (4.0, 40.0, 400.0)


def _mixed(H, seeds, n_steps):
    return tuple(Spec(H, 64, s, a, n_steps=n_steps, kw=tuple(sorted(hp.items())))
                 for s, a, hp in zip(seeds, ALPHAS, HPS))


# one mixed population per shape: H = 64 runs adam_kernel, H = 512 the fused dW epilogue with
# the small leaves riding in it
MIXED = {"h64": _mixed(64, (500, 501, 506), 2), "h512": _mixed(512, (500, 502, 504), 1)}
ALL_MIXED_SPECS = MIXED["h64"] + MIXED["h512"]
