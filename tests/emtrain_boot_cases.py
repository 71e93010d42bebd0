"""Shapes and seeds of the bootstrap tests (test infrastructure, not a test module): shared by
tests/test_gpu_emtrain_bootstrap.py, which runs them on the device, and
tests/test_emtrain_bootstrap_cpu.py, which asserts on the restatement alone that no model's
out-of-bag list is empty at these seeds -- at 7 episodes a resample holds every episode with
probability 7!/7^7 = 0.6 %, and an out-of-bag test on such a seed would be vacuous."""

D, A, HIDDEN = 3, 2, (32, 32)
B = 32                      # two 16-row blocks per model
N_ROWS = 203                # state and termination predictor: not a multiple of anything
EP_LEN, N_EP, T = 20, 7, 8  # multistep: 7 episodes of 20 rows, windows of 8
KINDS = ("state", "termination", "multistep")
SEEDS = {1: (11,), 3: (5, 6, 7), 9: tuple(range(100, 109))}
B9 = 16                     # K = 9: one block per model, more models than XCDs


def n_units(kind: str) -> int:
    return N_EP if kind == "multistep" else N_ROWS


def all_cases():
    """(kind, seed) of every model the GPU tests bootstrap."""
    return [(kind, s) for kind in KINDS for seeds in SEEDS.values() for s in seeds]
