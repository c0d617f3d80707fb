"""Explicit basis functions (GP.SetBasis, BasisLML, BasisGradient, BasisProduce; gogp_basis_*): wall time per call beside
Observe + Gradient and Produce on the same build.

    python3 tools/basis_probe.py [--reps R] [--sizes N ..] [--columns p ..] [--out profiles/basis.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {1024, 4096,
16384} with p in {1, 8, 64} basis columns (the constant plus sqrt(N) times orthonormal random columns, seeded).  Per
(N, p), ms per call, every call ending in a device synchronise:

    OG            Observe + Gradient: one zero-mean evaluation
    eval          Observe + BasisLML + BasisGradient: a whole evaluation with the mean integrated out (BasisModel)
    eval / OG     the headline ratio
    W symm        the first BasisLML behind Observe + Gradient with option basis_symm = 1: W = K^-1 H by the symmetric
                  product with the explicit K^-1, then the Gram sums, the p x p factorisation and the columns
    W subst       the same with basis_symm = 0: W by the two substitutions through the factor
    gradient      BasisGradient with everything in place: the weight pass over K^-1 and the reduction
    produce 1     BasisProduce at 1 test point       beside   Produce 1     (the persistent few-point kernel)
    produce 1024  BasisProduce at 1024 test points   beside   Produce 1024

Two warm-up calls of each kind, then R rounds (default 9): medians and the spread (min .. max).  The value is checked
against the other route's and the gradient against a central difference along one direction, so a fast wrong answer
does not make the table."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
SIZES = [1024, 4096, 16384]
COLUMNS = [1, 8, 64]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def make_gp(n, p):
    from gogp_amd import kernel, synth
    from gogp_amd.gp import GP
    X, y = synth.make_inputs(n, D, 1)
    rng = np.random.default_rng(3)
    Q, R = np.linalg.qr(np.concatenate([np.ones((n, 1)), rng.normal(size=(n, p - 1))], axis=1))
    H = np.ascontiguousarray(Q * np.sign(np.diag(R))[None, :] * np.sqrt(n))
    H[:, 0] = 1.0
    y = y + 10.0 + H @ rng.normal(size=p)
    Z = rng.uniform(X.min(), X.max(), (1024, D))
    Hz = np.concatenate([np.ones((1024, 1)), rng.normal(size=(1024, p - 1))], axis=1)
    g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
    return g, np.log(synth.theta0(D)), H, Z, np.ascontiguousarray(Hz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--columns", type=int, nargs="*", default=COLUMNS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib
    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max) of %d rounds" % (D, a.reps))
    names = ("OG", "eval", "W symm", "W subst", "gradient", "produce 1", "Produce 1", "produce 1024", "Produce 1024")
    say("%6s %3s  %s  %8s  %s" % ("N", "p", " ".join("%-24s" % s for s in names), "eval/OG",
                                  "routes, directional derivative: relative error"))
    for n in a.sizes:
        for p in a.columns:
            g, x, H, Z, Hz = make_gp(n, p)

            def og():
                g.Observe(x)
                return g.Gradient()

            def ev():
                g.Observe(x)
                return g.BasisLML(), g.BasisGradient()

            def first_lml(route):
                g.set_option("basis_symm", route)  # (drops the solved state)
                return g.BasisLML()

            og()
            g.SetBasis(H)
            v = np.array([0.6, -0.5, 0.62])
            h = 1e-4
            sp = (g.Observe(x + h * v), g.BasisLML())[1]
            sm = (g.Observe(x - h * v), g.BasisLML())[1]
            val, grad = ev()
            e1 = abs(first_lml(0) - first_lml(1)) / abs(val)
            e2 = abs((sp - sm) / (2 * h) - grad @ v) / abs(grad @ v)
            assert e1 < 1e-9 and e2 < 1e-3, (e1, e2)
            g.set_option("basis_symm", -1)
            for fn in (og, ev, lambda: g.BasisProduce(Z[:1], Hz[:1]), lambda: g.BasisProduce(Z, Hz),
                       lambda: g.Produce(Z[:1]), lambda: g.Produce(Z)):
                fn()
                fn()
            ts = {k: [] for k in names}
            for _ in range(a.reps):
                ts["OG"].append(timed(og))
                ts["W symm"].append(timed(lambda: first_lml(1)))
                ts["W subst"].append(timed(lambda: first_lml(0)))
                g.set_option("basis_symm", -1)
                g.BasisGradient()  # (its workspace is in place from here on)
                ts["gradient"].append(timed(g.BasisGradient))
                ts["produce 1"].append(timed(lambda: g.BasisProduce(Z[:1], Hz[:1])))
                ts["Produce 1"].append(timed(lambda: g.Produce(Z[:1])))
                ts["produce 1024"].append(timed(lambda: g.BasisProduce(Z, Hz)))
                ts["Produce 1024"].append(timed(lambda: g.Produce(Z)))
                ts["eval"].append(timed(ev))

            def fmt(t):
                return "%8.3f (%.3f .. %.3f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))
            med = {k: statistics.median(t) for k, t in ts.items()}
            say("%6d %3d  %s  %8.4f  %.1e, %.1e" % (n, p, " ".join("%-24s" % fmt(ts[k]) for k in names),
                                                  med["eval"] / med["OG"], e1, e2))
            g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
