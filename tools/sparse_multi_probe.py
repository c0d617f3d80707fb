"""Sparse multi-output (GP.SetSparseOutputs, SparseMultiObserve, SparseMultiGradient, SparseMultiGradientInducing,
SparseMultiProduce; gogp_sparse_multi_*): wall time per call beside the single-output calls of the same build.

    python3 tools/sparse_multi_probe.py [--reps R] [--sizes N ..] [--inducing M ..] [--outputs T ..] [--out profiles/sparse_multi.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {65536, 1048576}
with M in {512, 4096} inducing points (a random subset of the inputs) and T in {1, 8, 128} output columns (column 0 is the
workload's y, the others mix it with smooth functions of the inputs), default options.  Per (N, M): the single-output
SparseObserve + SparseGradient, then per T, ms per call, every call ending in the ABI's synchronise:

    observe       SparseMultiObserve: the T bounds and their sum
    obs+grad      SparseMultiObserve + SparseMultiGradient: a whole evaluation, as SparseMultiModel runs it
    obs+grad+dU   SparseMultiObserve + SparseMultiGradientInducing
    produce       SparseMultiProduce at 1024 test points
    x single      obs+grad over the single-output obs+grad
    / T singles   obs+grad over T single-output evaluations: below 1 the multi calls win
    xty share     launch_sparse_xty alone on one chunk (hook gogp_bench_sparse_xty) times the chunks of the data, over observe

and SetSparseOutputs at T = 128.  One warm-up call of each kind, then R rounds (default 5): medians and the spread
(min .. max).  Column 0's bound is checked against the single-output bound and the gradient against a central difference
of the total along one direction, so a fast wrong answer does not make the table."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
MZ = 1024
SIZES = [65536, 1048576]
INDUCING = [512, 4096]
OUTPUTS = [1, 8, 128]
CHUNK = 8192


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def med(t):
    return 1e3 * statistics.median(t)


def fmt(t):
    return "%9.2f (%.2f .. %.2f)" % (med(t), 1e3 * min(t), 1e3 * max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--inducing", type=int, nargs="*", default=INDUCING)
    ap.add_argument("--outputs", type=int, nargs="*", default=OUTPUTS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib, kernel, synth
    from gogp_amd.gp import GP
    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0, sparse_chunk = %d, sparse_jitter_log10 = -8, %d test points; "
        "ms per call: median (min .. max) of %d rounds" % (D, CHUNK, MZ, a.reps))
    names = ("observe", "obs+grad", "obs+grad+dU", "produce")
    say("%8s %5s %4s  %s  %9s %11s %9s  %s" % ("N", "M", "T", " ".join("%-30s" % s for s in names), "x single", "/ T singles",
                                               "xty share", "total, directional derivative: relative error"))
    x = np.log(synth.theta0(D))
    v = np.array([0.6, -0.5, 0.62])
    h = 1e-4
    rng = np.random.default_rng(3)
    tmax = max(a.outputs)
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        Z = rng.uniform(X.min(), X.max(), (MZ, D))
        # column 0: the workload's y; the others: y mixed with smooth functions of the inputs
        W = rng.normal(size=(D, tmax))
        Yall = np.ascontiguousarray(rng.uniform(0.5, 1.0, tmax) * y[:, None] + 0.3 * np.sin(X @ W))
        Yall[:, 0] = y
        for M in a.inducing:
            g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
            U = X[rng.choice(n, M, replace=False)]
            g.SetSparse(X, y, U)

            def single():
                return g.SparseObserve(x), g.SparseGradient()

            bound1 = single()[0]
            t1 = [timed(single) for _ in range(a.reps)]
            say("%8d %5d    -  single-output obs+grad %s" % (n, M, fmt(t1)))
            wins = None
            for T in a.outputs:
                Y = np.ascontiguousarray(Yall[:, :T])
                g.SetSparseOutputs(Y)

                def ev():
                    return g.SparseMultiObserve(x), g.SparseMultiGradient()

                def evu():
                    return g.SparseMultiObserve(x), g.SparseMultiGradientInducing()

                tp, tm = g.SparseMultiObserve(x + h * v)[0], g.SparseMultiObserve(x - h * v)[0]
                (total, bounds), grad = ev()
                e = abs((tp - tm) / (2 * h) - grad @ v) / abs(grad @ v)
                # (a fast wrong answer is off in the first digit: sparse_probe.py has the reasoning)
                assert e < 1e-2, e
                assert abs(bounds[0] - bound1) <= 1e-3 * abs(bound1), (bounds[0], bound1)
                evu()
                g.SparseMultiProduce(Z)
                ts = {k: [] for k in names}
                for _ in range(a.reps):
                    ts["observe"].append(timed(lambda: g.SparseMultiObserve(x)))
                    ts["obs+grad"].append(timed(ev))
                    ts["obs+grad+dU"].append(timed(evu))
                    ts["produce"].append(timed(lambda: g.SparseMultiProduce(Z)))
                ms, tf = ctypes.c_double(0.0), ctypes.c_double(0.0)
                rc = _lib.hooks().gogp_bench_sparse_xty(0, min(CHUNK, n), M, T, 10, ctypes.byref(ms), ctypes.byref(tf))
                assert rc == _lib.GOGP_OK, rc
                share = ms.value * (n / min(CHUNK, n)) / med(ts["observe"])
                ratio = med(ts["obs+grad"]) / med(t1)
                if wins is None and ratio / T < 1.0:
                    wins = T
                say("%8d %5d %4d  %s  %9.3f %11.4f %8.1f%%  %.9e, %.1e" % (n, M, T, " ".join("%-30s" % fmt(ts[k]) for k in names), ratio,
                                                                        ratio / T, 100.0 * share, total, e))
                if T == 128:
                    tso = [timed(lambda: g.SetSparseOutputs(Y)) for _ in range(a.reps)]
                    say("%8d %5d %4d  SetSparseOutputs %s; launch_sparse_xty on one chunk %.3f ms, %.1f TFLOP/s"
                        % (n, M, T, fmt(tso), ms.value, tf.value))
            say("%8d %5d    -  the multi calls win over T single-output evaluations from T = %s (of the T measured)"
                % (n, M, wins if wins is not None else "none"))
            g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
