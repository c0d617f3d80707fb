"""GP.ProduceCovariance and GP.Sample: wall time per call beside GP.Produce (and GP.ProduceGradient, whose forward half
is the same tile route).

    python3 tools/produce_covariance_probe.py [--reps R] [--out profiles/produce_covariance.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/produce_covariance_probe.py --trace

At N in {4096, 16384} and M in {1, 16, 64, 1024} (D = 8, ARD Normal): one Produce(Z), one ProduceCovariance(Z), one
Sample(Z, xi, diag_add = noise variance) with ns = 16 caller-supplied normals, one ProduceGradient(Z).  Every call ends
in a device synchronise (the C ABI copies its results back).  Each shape is warmed up with two calls of every kind; the
kinds are then timed alternately, R rounds (default 9), and the medians and the spread (min .. max) of the rounds are
reported.  sqrt(diag cov) is checked against Produce's sigma at every shape, so a fast wrong answer does not make the
table.  The last column is the SYRK launch's bound for the shape: max(M^2 N / 78.6 TFLOP/s, 8 M N bytes / 8.0 TB/s).

--trace: four ProduceCovariance calls per shape and nothing else, for a kernel trace in a run of its own (the time of
pcov_syrk_kernel per shape is read from the trace's per-launch rows: the shapes run in the order listed)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gogp_amd import _lib, kernel  # noqa: E402
from gogp_amd.gp import GP  # noqa: E402

D = 8
NS = 16
NOISE_STD = 0.3
FP64_MFMA_PEAK = 78.6e12
HBM_PEAK = 8.0e12


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls


def syrk_bound(n, m):
    return max(m * m * n / FP64_MFMA_PEAK, 8.0 * m * n / HBM_PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--points", type=int, nargs="*", default=[1, 16, 64, 1024])
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("library: %s" % _lib.lib().gogp_version().decode())
    if not a.trace:
        say("D = %d, Scaled ARD Normal, noise std %.1f; ms per call: median (min .. max) of %d alternating rounds; "
            "Sample: ns = %d, diag_add = %.2f" % (D, NOISE_STD, a.reps, NS, NOISE_STD ** 2))
        say("%6s %5s  %-24s %-24s %-24s %-24s %6s %6s  %-9s %s" % ("N", "M", "Produce", "ProduceCovariance", "Sample",
                                                                  "ProduceGradient", "PC/P", "S/P", "|ds|/s",
                                                                  "SYRK bound us"))
    rng = np.random.default_rng(0)
    for n in a.sizes:
        X = rng.uniform(-2.0, 2.0, (n, D))
        y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=n)
        g = GP(D, kernel.Scaled(kernel.ARD(kernel.Normal, D)), kernel.UniformNoise,
               ThetaSimil=[1.0] + [2.0 + 0.1 * d for d in range(D)], ThetaNoise=[NOISE_STD], device=0)
        g.Absorb(X, y)
        for m in a.points:
            Z = rng.uniform(-2.5, 2.5, (m, D))
            xi = rng.standard_normal((NS, m))

            def produce():
                return g.Produce(Z)

            def pcov():
                return g.ProduceCovariance(Z)

            def sample():
                return g.Sample(Z, xi=xi, diag_add=NOISE_STD ** 2)

            def pgrad():
                return g.ProduceGradient(Z)

            if a.trace:
                for _ in range(4):
                    pcov()
                say("traced N = %d M = %d: SYRK bound %.2f us" % (n, m, 1e6 * syrk_bound(n, m)))
                continue
            kinds = (produce, pcov, sample, pgrad)
            for fn in kinds:
                fn()
                fn()
            sigma = produce()[1]
            err = np.abs(np.sqrt(np.diag(pcov()[1])) - sigma).max() / sigma.max()
            assert np.isfinite(sample()).all()
            calls = 3 if n >= 16384 or m >= 1024 else 10
            ts = [[] for _ in kinds]
            for _ in range(a.reps):
                for t, fn, mult in zip(ts, kinds, (4, 2, 2, 2)):
                    t.append(window(fn, calls * mult))

            def fmt(v):
                return "%8.3f (%.3f .. %.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
            med = [statistics.median(t) for t in ts]
            say("%6d %5d  %-24s %-24s %-24s %-24s %6.2f %6.2f  %-9.1e %.2f" % (
                n, m, fmt(ts[0]), fmt(ts[1]), fmt(ts[2]), fmt(ts[3]), med[1] / med[0], med[2] / med[0], err,
                1e6 * syrk_bound(n, m)))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
