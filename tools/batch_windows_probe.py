"""Batches of small GPs (gogp_batch_*): wall time per call against the sequential Observe + Gradient.

    python3 tools/batch_windows_probe.py [--reps R] [--iters ITERS] [--out profiles/batch_windows.txt]
    python3 tools/batch_windows_probe.py --full [--reps R] [--iters ITERS] [--out profiles/batch_windows_full.txt]

1. the 44 windows of the hyperpriors case study (tests/golden/hyperpriors.csv: prefixes of 0 .. 43 rows) -- one
   batch_observe_gradient against 44 x (Observe + Gradient) on one GP;
2. batches of 256 and 1024 members at N = 64 and 128 (evaluations / s);
3. Evaluate on hyperpriors.csv (ITERS = --iters), BATCH off against on.
Medians of R repetitions after one warm-up call.  A kernel trace of the same calls shows one launch per batch call
(rocprofv3 --kernel-trace --stats -- python3 tools/batch_windows_probe.py --trace-only).

--full: the full Observe form (gogp_batch_observe_full_gradient / gogp_batch_produce_full) on the windows of the two
OPTINP case studies -- anynoise (tests/golden/barebones.csv, 20 windows) and warpedtime (tests/golden/events.csv, 43
windows): one batch_observe_full_gradient call against the same windows one at a time through Observe(full x) +
Gradient() on prepared handles (one per window), and Evaluate with OPTINP, BATCH off against on.  With --trace-only: one
call of each kind."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gogp_amd import kernel, priors, tutorial  # noqa: E402
from gogp_amd.gp import GP, Model  # noqa: E402

HYPER = kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))],
                   order=[0, 2, 1, 3, 4])
NOISE = kernel.ScaledNoise(0.01)
DATA = os.path.join(ROOT, "tests", "golden", "hyperpriors.csv")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def full_form(a, say):
    from gogp_amd import _lib
    say("library: %s" % _lib.lib().gogp_version().decode())
    studies = [
        ("anynoise", "barebones.csv", kernel.Scaled(kernel.Matern52), kernel.ConstantNoiseParam(1e-5 ** 0.5),
         lambda g: priors.AnyNoiseModel(Model(g, priors.AnyNoisePriors()))),
        ("warpedtime", "events.csv", kernel.Scaled(kernel.Matern52), kernel.ScaledNoise(0.01),
         lambda g: priors.WarpedTimeModel(Model(g, priors.WarpedTimePriors()))),
    ]
    rng = np.random.default_rng(0)
    for name, data, simil, noise, model in studies:
        path = os.path.join(ROOT, "tests", "golden", data)
        with open(path) as f:
            X, y = tutorial.load(f)
        y = (y - y.mean()) / y.std(ddof=1)
        ends = list(range(len(X)))
        xs = [np.concatenate([0.1 * rng.normal(size=3), X[:e].reshape(-1), y[:e]]) for e in ends]
        g = GP(1, simil, noise, device=0)
        if a.trace_only:
            g.batch_observe_full_gradient(xs)
            g.batch_produce_full(xs, [X[e:e + 1] for e in ends])
            g.close()
            continue
        t_b = timed(lambda: g.batch_observe_full_gradient(xs), a.reps)
        t_p = timed(lambda: g.batch_produce_full(xs, [X[e:e + 1] for e in ends]), a.reps)
        hs = [GP(1, simil, noise, device=0) for _ in ends]

        def seq():
            for hh, x in zip(hs, xs):
                hh.Observe(x)
                hh.Gradient()

        t_s = timed(seq, a.reps)
        for hh in hs:
            hh.close()
        k = len(ends)
        say("%s windows (%d members, n = 0..%d, full form: 3 parameters + 2 n):" % (name, k, k - 1))
        say("  batch_observe_full_gradient, one call        %9.1f us" % (t_b * 1e6))
        say("  batch_produce_full (1 point each), one call  %9.1f us" % (t_p * 1e6))
        say("  %d x (Observe(full x) + Gradient), %d handles %9.1f us  (%.1f us each)  -> %.1fx" %
            (k, k, t_s * 1e6, t_s * 1e6 / k, t_s / t_b))
        for batch in (False, True):
            tutorial.OPTINP, tutorial.BATCH, tutorial.SEED, tutorial.ITERS = True, batch, 7, a.iters
            ge = GP(1, simil, noise, device=0)
            t0 = time.perf_counter()
            with open(path) as f:
                tutorial.Evaluate(ge, model(ge), np.zeros(3), f, io.StringIO(), log=io.StringIO())
            t = time.perf_counter() - t0
            say("  Evaluate %s (OPTINP, ITERS = %d), BATCH %-5s: %8.3f s" % (data, a.iters, batch, t))
            ge.close()
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="one batch call of each kind (for a kernel trace)")
    ap.add_argument("--full", action="store_true", help="the full Observe form on the OPTINP case studies' windows")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.full:
        full_form(a, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    with open(DATA) as f:
        X, y = tutorial.load(f)
    y = (y - y.mean()) / y.std(ddof=1)
    rng = np.random.default_rng(0)
    x0 = np.log([1.0, 0.5, 0.6, 1.3, 0.05, 2.0])
    ends = list(range(len(X)))
    xs = x0 + 0.1 * rng.normal(size=(len(ends), len(x0)))
    g = GP(1, HYPER, NOISE, device=0)
    g.set_batch(X, y, [(0, e) for e in ends])
    if a.trace_only:
        g.batch_observe_gradient(xs)
        g.batch_produce(xs, [X[e:e + 1] for e in ends])
        return
    t_b = timed(lambda: g.batch_observe_gradient(xs), a.reps)
    h = GP(1, HYPER, NOISE, device=0)

    def seq():
        for i, e in enumerate(ends):
            h.X, h.Y = X[:e], y[:e]
            h.Observe(xs[i])
            h.Gradient()

    t_s = timed(seq, max(3, a.reps // 4))
    # the same with the data already on the handle (one handle per window): the evaluation alone
    hs = [GP(1, HYPER, NOISE, X=X[:e], Y=y[:e], device=0) for e in ends]

    def seq_warm():
        for i, hh in enumerate(hs):
            hh.Observe(xs[i])
            hh.Gradient()

    t_w = timed(seq_warm, max(3, a.reps // 4))
    t_p = timed(lambda: g.batch_produce(xs, [X[e:e + 1] for e in ends]), a.reps)
    say("hyperpriors windows (44 members, n = 0..43, 6 parameters):")
    say("  batch_observe_gradient, one call        %9.1f us" % (t_b * 1e6))
    say("  batch_produce (1 point each), one call  %9.1f us" % (t_p * 1e6))
    say("  44 x (set data + Observe + Gradient)    %9.1f us  (%.1f us each)  -> %.1fx" %
        (t_s * 1e6, t_s * 1e6 / len(ends), t_s / t_b))
    say("  44 x (Observe + Gradient), 44 handles   %9.1f us  (%.1f us each)  -> %.1fx" %
        (t_w * 1e6, t_w * 1e6 / len(ends), t_w / t_b))
    for h_ in hs:
        h_.close()
    h.close()
    for n in (64, 128):
        for k in (256, 1024):
            Xb = rng.uniform(-2, 2, (n + k, 1))
            yb = np.sin(3 * Xb[:, 0]) + 0.1 * rng.normal(size=n + k)
            gb = GP(1, HYPER, NOISE, device=0)
            gb.set_batch(Xb, yb, [(i, n) for i in range(k)])
            xk = x0 + 0.1 * rng.normal(size=(k, len(x0)))
            t = timed(lambda: gb.batch_observe_gradient(xk), max(3, a.reps // 2))
            say("batch of %4d members at N = %3d: %9.1f us per call, %9.0f evaluations/s" % (k, n, t * 1e6, k / t))
            gb.close()
    # the forecast harness, BATCH off / on
    for batch in (False, True):
        tutorial.BATCH, tutorial.SEED, tutorial.ITERS = batch, 7, a.iters
        ge = GP(1, HYPER, NOISE, device=0)
        out = io.StringIO()
        t0 = time.perf_counter()
        with open(DATA) as f:
            tutorial.Evaluate(ge, Model(ge, priors.HyperPriors()), np.zeros(6), f, out, log=io.StringIO())
        t = time.perf_counter() - t0
        say("Evaluate hyperpriors.csv (ITERS = %d), BATCH %-5s: %8.3f s" % (a.iters, batch, t))
        ge.close()
    g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
