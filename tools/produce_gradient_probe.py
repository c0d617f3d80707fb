"""GP.ProduceGradient: wall time per call beside GP.Produce and beside the finite-difference route.

    python3 tools/produce_gradient_probe.py [--reps R] [--out profiles/produce_gradient.txt]

At N in {4096, 16384} and M in {1, 16, 64, 1024} (D = 8, ARD Normal): one Produce(Z), one ProduceGradient(Z), and
central differences of Produce -- 2 D + 1 = 17 Produce calls on shifted copies of Z, which is what the derivatives
cost without the call.  Every call ends in a device synchronise (the C ABI copies its results back).  Each shape is
warmed up with two calls of every kind; the three kinds are then timed alternately, R rounds (default 9), at least
three calls per timing, and the medians and the spread (min .. max) of the rounds are reported.  The derivatives are
checked against the differences at every shape, so a fast wrong answer does not make the table."""
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
STEP = 1e-5


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--points", type=int, nargs="*", default=[1, 16, 64, 1024])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled ARD Normal, noise std 0.3; ms per call: median (min .. max) of %d alternating rounds" % (D, a.reps))
    say("%6s %5s  %-24s %-24s %-24s %6s %6s  %s" % ("N", "M", "Produce", "ProduceGradient", "17 x Produce (FD)", "PG/P",
                                                    "FD/PG", "max |dmu - FD| / max |dmu|"))
    rng = np.random.default_rng(0)
    for n in a.sizes:
        X = rng.uniform(-2.0, 2.0, (n, D))
        y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=n)
        g = GP(D, kernel.Scaled(kernel.ARD(kernel.Normal, D)), kernel.UniformNoise,
               ThetaSimil=[1.0] + [2.0 + 0.1 * d for d in range(D)], ThetaNoise=[0.3], device=0)
        g.Absorb(X, y)
        for m in a.points:
            Z = rng.uniform(-2.5, 2.5, (m, D))
            shifted = [Z]
            for d in range(D):
                for sgn in (1.0, -1.0):
                    Zs = Z.copy()
                    Zs[:, d] += sgn * STEP
                    shifted.append(Zs)

            def produce():
                return g.Produce(Z)

            def pgrad():
                return g.ProduceGradient(Z)

            def fd():
                return [g.Produce(Zs) for Zs in shifted]

            for fn in (produce, pgrad, fd):
                fn()
                fn()
            dmu = pgrad()[2]
            r = fd()
            fd_mu = np.stack([(r[1 + 2 * d][0] - r[2 + 2 * d][0]) / (2 * STEP) for d in range(D)], axis=1)
            err = np.abs(dmu - fd_mu).max() / np.abs(fd_mu).max()
            calls = 3 if n >= 16384 or m >= 1024 else 10
            ts = {"p": [], "g": [], "f": []}
            for _ in range(a.reps):
                ts["p"].append(window(produce, calls * 4))
                ts["g"].append(window(pgrad, calls * 2))
                ts["f"].append(window(fd, max(1, calls // 3)))

            def fmt(v):
                return "%8.3f (%.3f .. %.3f)" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
            mp, mg, mf = (statistics.median(ts[k]) for k in "pgf")
            say("%6d %5d  %-24s %-24s %-24s %6.2f %6.2f  %.1e" % (n, m, fmt(ts["p"]), fmt(ts["g"]), fmt(ts["f"]), mg / mp,
                                                                 mf / mg, err))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
