"""Multi-output (GP.SetOutputs, MultiLML, MultiGradient, MultiAlpha, MultiProduce; gogp_multi_*): wall time per call
beside Observe + Gradient on the same build.

    python3 tools/multi_output_probe.py [--reps R] [--sizes N ..] [--outputs T ..] [--out profiles/multi_output.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {1024, 4096,
16384} with T in {1, 8, 128} output columns (column 0 the process's own y, the others scaled and shifted sines of the
inputs plus noise).  Per (N, T), ms per call, every call ending in a device synchronise:

    OG            Observe + Gradient: one single-output evaluation
    set           SetOutputs: the transpose on the host and the upload
    solve+LML     the first MultiLML behind an Observe + Gradient: the two substitutions for T right-hand sides, the dots
    LML           MultiLML again (the solutions are kept)
    gradient      MultiGradient with K^-1 in place: the weight pass over K^-1 and the reduction
    alpha         MultiAlpha: the copy and the transpose on the host
    produce       MultiProduce at M = 256 test points: cross-covariance, the means in one tile-kernel launch, the
                  substitution for sigma
    eval          Observe + MultiLML + MultiGradient: a whole multi-output evaluation, as MultiModel runs it
    eval / T*OG   against T separate single-output evaluations

Two warm-up calls of each kind, then R rounds (default 9): medians and the spread (min .. max).  The total is checked
against the sum of the per-output values and the gradient against a central difference of the total along one
direction, so a fast wrong answer does not make the table."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
M = 256
SIZES = [1024, 4096, 16384]
OUTPUTS = [1, 8, 128]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def make_gp(n, T):
    from gogp_amd import kernel, synth
    from gogp_amd.gp import GP
    X, y = synth.make_inputs(n, D, 1)
    rng = np.random.default_rng(3)
    a, phi = rng.uniform(0.5, 1.5, T), rng.uniform(0.0, 2.0 * np.pi, T)
    Y = a[None, :] * np.sin(X.sum(1)[:, None] + phi[None, :]) + 0.1 * rng.normal(size=(n, T))
    Y[:, 0] = y
    Z = rng.uniform(X.min(), X.max(), (M, D))
    g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
    return g, np.log(synth.theta0(D)), np.ascontiguousarray(Y), Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--outputs", type=int, nargs="*", default=OUTPUTS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib
    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0, M = %d test points; ms per call: median (min .. max) of %d "
        "rounds" % (D, M, a.reps))
    names = ("OG", "set", "solve+LML", "LML", "gradient", "alpha", "produce", "eval")
    say("%6s %4s  %s  %10s  %s" % ("N", "T", " ".join("%-24s" % s for s in names), "eval/T*OG",
                                    "total, directional derivative: relative error"))
    for n in a.sizes:
        for T in a.outputs:
            g, x, Y, Z = make_gp(n, T)

            def og():
                g.Observe(x)
                return g.Gradient()

            def ev():
                g.Observe(x)
                return g.MultiLML()[0], g.MultiGradient()

            og()
            g.SetOutputs(Y)
            # checks: the total is the sum of the outputs' values; the gradient matches a central difference along v
            v = np.array([0.6, -0.5, 0.62])
            h = 1e-4
            sp = (g.Observe(x + h * v), g.MultiLML()[0])[1]
            sm = (g.Observe(x - h * v), g.MultiLML()[0])[1]
            total, grad = ev()
            e1 = abs(total - g.MultiLML()[1].sum()) / abs(total)
            e2 = abs((sp - sm) / (2 * h) - grad @ v) / abs(grad @ v)
            assert e1 < 1e-10 and e2 < 1e-3, (e1, e2)
            for fn in (og, ev, lambda: g.SetOutputs(Y), lambda: g.MultiProduce(Z)):
                fn()
                fn()
            ts = {k: [] for k in names}
            for _ in range(a.reps):
                ts["OG"].append(timed(og))
                ts["set"].append(timed(lambda: g.SetOutputs(Y)))
                ts["solve+LML"].append(timed(g.MultiLML))
                ts["LML"].append(timed(g.MultiLML))
                g.MultiGradient()  # (its workspace and K^-1 are in place from here on)
                ts["gradient"].append(timed(g.MultiGradient))
                ts["alpha"].append(timed(lambda: g.MultiAlpha))
                ts["produce"].append(timed(lambda: g.MultiProduce(Z)))
                ts["eval"].append(timed(ev))

            def fmt(t):
                return "%8.3f (%.3f .. %.3f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))
            med = {k: statistics.median(t) for k, t in ts.items()}
            say("%6d %4d  %s  %10.4f  %.1e, %.1e" % (n, T, " ".join("%-24s" % fmt(ts[k]) for k in names),
                                                    med["eval"] / (T * med["OG"]), e1, e2))
            g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
