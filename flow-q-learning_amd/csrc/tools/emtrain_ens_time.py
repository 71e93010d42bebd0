"""World-model ensemble training time (developer tool): K single trainers one after the other
against ONE K-model trainer (fqlpop_emtrain_create_ensemble), same shapes, at the cube
shapes (obs 28, act 5, hidden (128, 256, 128), B = 256).

  python emtrain_ens_time.py [--kinds sp0,sp1,tp,ms0,ms1] [--K 1,2,5,8,16] [--steps 2000]
                             [--ms_steps 30] [--T 256] [--reps 1] [--single_only] [--train_loop 0]
                             [--root TREE] [--label NAME] [--bootstrap] [--oob N] [--rows N]

kinds: sp0 / sp1 the state predictor with termination_weight 0 / 1, tp the termination
predictor, ms0 / ms1 the multistep model at sequence length T.  Every timed region is
``steps(n)`` (fqlpop_emtrain_step: n asynchronous device-sampled updates) and one sync at its
end, after a warm-up of the same handle, so no host log read hides the kernels.  Paths:

  loop   K single trainers, each created, warmed up, timed and closed in turn; the figure
         is the sum of the K timed regions
  ens0   one K-model trainer under engine option em_ens_xcd = 0 (model-major blocks)
  ens1   the same under em_ens_xcd = 1 (at most ceil(K / 8) models per XCD)

--single_only runs the loop path alone and needs nothing of the ensemble interface, so with
--root it measures another checkout of the project (its package and its libfqlpop.so), e.g.
the parent commit as the baseline.  --train_loop N also times ``train()`` itself (N steps
with the per-step log read and a logger per model) for the loop and for the default
placement at every K asked for.  --bootstrap creates every trainer with ``bootstrap=True`` (each
model draws through its own resample table); --oob N also times, on one K-model trainer, the
one-off table set-up (``what = boot_setup``), ``eval_oob(N)`` (``oob_eval``) and N host-loader
``eval_step``s (``host_eval``); --rows sets the dataset size (200 000).  One JSON line per (kind, K, path, rep) with ms per step,
model-steps/s and the GPU's clocks right after the timed region.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--kinds", default="sp0,sp1,tp,ms0,ms1")
ap.add_argument("--K", default="1,2,5,8,16")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--ms_steps", type=int, default=30)
ap.add_argument("--T", type=int, default=256)
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--single_only", action="store_true")
ap.add_argument("--train_loop", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))))
ap.add_argument("--label", default="")
ap.add_argument("--bootstrap", action="store_true")
ap.add_argument("--oob", type=int, default=0)
ap.add_argument("--rows", type=int, default=200_000)
args = ap.parse_args()
sys.path[:0] = [args.root, os.path.join(args.root, "flow-q-learning_amd")]
import numpy as np  # noqa: E402

import bench  # noqa: E402
import envmodel as em  # noqa: E402
import train_env_model as tem  # noqa: E402
from envmodel import trainer as et  # noqa: E402

D, A, B = 28, 5, 256
data = bench.synthetic_dataset(args.rows, D, A)
BOOT = {"bootstrap": True} if args.bootstrap else {}  # (another checkout's trainers may not take it)
DS = {k: np.asarray(data[k], np.float32) for k in ("observations", "actions", "rewards", "next_observations")}
SPEC = em.EnvModelSpec(D, A)
TP = em.init_termination_predictor(SPEC, 1)


class NullLogger:
    def log(self, row, step):
        pass


def make(kind, seeds, loggers=None, single=False, n=None):
    """A single trainer (single: of seeds[0]) or a K-model trainer of the kind; n: its step count."""
    ms, tw = kind.startswith("ms"), float(kind[-1]) if kind != "tp" else 0.0
    n = n or (args.ms_steps if ms else args.steps)
    cfg = et.EnvModelTrainerConfig(steps=max(n, 1), model="multistep" if ms else "baseline", sequence_length=args.T,
                                   termination_weight=tw, batch_size=B, seed=seeds[0], val_batches=2)
    loaders = (tem.MultistepLoader(DS, args.T), tem.MultistepLoader(DS, args.T)) if ms else \
        (tem.StepLoader(DS), tem.StepLoader(DS))
    if single:
        if kind == "tp":
            return et.TerminationPredictorTrainer(SPEC, em.init_termination_predictor(SPEC, seeds[0]), *loaders, cfg,
                                                  logger=loggers[0] if loggers else None, **BOOT)
        return et.StatePredictorTrainer(SPEC, em.init_state_predictor(SPEC, seeds[0]), *loaders, cfg,
                                        logger=loggers[0] if loggers else None, tp_params=TP if tw > 0 else None,
                                        **BOOT)
    if kind == "tp":
        return et.TerminationPredictorEnsembleTrainer(SPEC, [em.init_termination_predictor(SPEC, s) for s in seeds],
                                                      *loaders, cfg, seeds, loggers=loggers, **BOOT)
    return et.StatePredictorEnsembleTrainer(SPEC, [em.init_state_predictor(SPEC, s) for s in seeds], *loaders, cfg,
                                            seeds, loggers=loggers, tp_params=TP if tw > 0 else None, **BOOT)


def timed_steps(tr, n):
    tr.steps(max(1, n // 10))  # warm-up
    tr.sync()
    t0 = time.perf_counter()
    tr.steps(n)
    tr.sync()
    return time.perf_counter() - t0


def emit(kind, K, path, rep, n, sec, what="steps"):
    print(json.dumps({"label": args.label, "kind": kind, "K": K, "path": path, "rep": rep, "what": what, "steps": n,
                      "ms_per_step": round(1e3 * sec / n, 5), "model_steps_per_s": round(K * n / sec, 1),
                      "gpu_clock": bench.gpu_clock_power(0)}), flush=True)


def set_xcd(v):
    from fqlpop import set_engine_option
    set_engine_option("em_ens_xcd", v)


for kind in args.kinds.split(","):
    n = args.ms_steps if kind.startswith("ms") else args.steps
    for K in [int(k) for k in args.K.split(",")]:
        seeds = list(range(100, 100 + K))
        for rep in range(args.reps):
            sec = 0.0
            for s in seeds:
                tr = make(kind, [s], single=True)
                sec += timed_steps(tr, n)
                tr.close()
            emit(kind, K, "loop", rep, n, sec)
            if args.single_only:
                continue
            for xcd in (0, 1):
                set_xcd(xcd)
                tr = make(kind, seeds)
                sec = timed_steps(tr, n)
                tr.close()
                emit(kind, K, f"ens{xcd}", rep, n, sec)
        if args.oob and not args.single_only:
            # out-of-bag evaluation on the device against the host loader's eval batches
            from fqlpop import reset_engine_options
            reset_engine_options()
            tr = make(kind, seeds)
            tr.steps(2)
            tr.sync()
            t0 = time.perf_counter()
            tr.set_bootstrap(True)  # (synchronises)
            emit(kind, K, "ens", 0, 1, time.perf_counter() - t0, what="boot_setup")
            for what, run in (("oob_eval", lambda: tr.eval_oob(args.oob, 1)),
                              ("host_eval", lambda: [tr.eval_step(None, [tr._sample(tr.val_loader, k) for k in range(K)])
                                                     for _ in range(args.oob)])):
                run()  # warm-up
                t0 = time.perf_counter()
                run()
                emit(kind, K, "ens", 0, args.oob, time.perf_counter() - t0, what=what)
            tr.close()
        if args.train_loop:
            # train() itself: the val passes, one update and one log read per step, K log rows
            for path in ("loop",) if args.single_only else ("loop", "ens"):
                t0 = time.perf_counter()
                if path == "loop":
                    for s in seeds:
                        tr = make(kind, [s], loggers=[NullLogger()], single=True, n=args.train_loop)
                        tr.train()
                        tr.close()
                else:
                    from fqlpop import reset_engine_options
                    reset_engine_options()
                    tr = make(kind, seeds, loggers=[NullLogger() for _ in seeds], n=args.train_loop)
                    tr.train()
                    tr.close()
                emit(kind, K, path, 0, args.train_loop, time.perf_counter() - t0, what="train_loop")
print("emtrain_ens_time done", flush=True)
