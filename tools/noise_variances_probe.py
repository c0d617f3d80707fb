"""Per-observation noise variances (GP.SetNoiseVariances, NoiseVariancesGradient, Append with v; gogp_*noise_variances*,
gogp_append_noisy): wall time per call beside the same calls without variances, on the same build.

    python3 tools/noise_variances_probe.py [--reps R] [--sizes N ..] [--small N ..] [--append-n N] [--out profiles/noise_variances.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8), the variances
log-normal around the noise variance with every fifth one exactly 0.  Every call ends in a device synchronise.  The two
arms of a comparison alternate round by round; per arm the median and the spread (min .. max) of R rounds (default 9)
behind two warm-up rounds, and next to every difference the larger of the two arms' spreads.

    1. OG          Observe + Gradient, plain handle | handle with variances, N in --sizes: the hook is two O(N) launches
    2. OG small    the same at N in --small (<= 128): without variances ONE launch (option "tiny"), with them the general
                   sweep -- the known cost of the scoping
    3. dv | LOO    NoiseVariancesGradient | LOO with K^-1 in place (behind Observe + Gradient): one pass over the diagonal
                   of K^-1 each, n doubles | 3 n doubles back
    4. append      Append of 1 and of 64 rows behind Absorb of --append-n rows: plain | with variances on both sides

The LML with variances is checked against a dense numpy evaluation at the smallest size of 1. and dv against a central
difference of it, so a fast wrong answer does not make the table."""
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
SMALL = [64, 128]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def variances(n, s2):
    rng = np.random.default_rng(5 + n)
    v = np.minimum(s2 * np.exp(rng.normal(-0.3, 0.9, size=n)), 4.0 * s2)
    v[1::5] = 0.0
    return v


def make(n, with_v):
    from gogp_amd import kernel, synth
    from gogp_amd.gp import GP
    X, y = synth.make_inputs(n, D, 1)
    th = synth.theta0(D)
    g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
    v = variances(n, th[-1] ** 2)
    if with_v:
        g.SetNoiseVariances(v)
    return g, np.log(th), X, y, v


def alternate(arms, reps, warm=2):
    """arms: name -> callable returning ms.  One call of every arm per round, in turn."""
    out = {k: [] for k in arms}
    for r in range(warm + reps):
        for k, fn in arms.items():
            t = fn()
            if r >= warm:
                out[k].append(t)
    return out


def fmt(ts):
    return "%9.3f (%.3f .. %.3f)" % (statistics.median(ts), min(ts), max(ts))


def diff(a, b):
    """b - a of the medians, and the larger spread of the two arms"""
    return "%+8.3f ms (%+6.2f %%), spread %.3f" % (statistics.median(b) - statistics.median(a),
                                                  100.0 * (statistics.median(b) / statistics.median(a) - 1.0),
                                                  max(max(a) - min(a), max(b) - min(b)))


def dense_check(n, say):
    """LML and one component of dv at n rows against numpy (the model's definition)."""
    gv, x, X, y, v = make(n, True)
    th = np.exp(x)

    def lml(vv):
        d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        K = th[0] * np.exp(-0.5 * d2 / th[1] ** 2) + np.diag(th[2] ** 2 + vv)
        L = np.linalg.cholesky(K)
        a = np.linalg.solve(L.T, np.linalg.solve(L, y))
        return -0.5 * n * np.log(2 * np.pi) - np.log(np.diag(L)).sum() - 0.5 * y @ a

    got = gv.Observe(x)
    want = lml(v)
    dv = gv.NoiseVariancesGradient()
    e = np.zeros(n)
    i = int(np.argmax(np.abs(dv)))
    e[i] = 1e-7
    fd = (lml(v + e) - lml(v - e)) / 2e-7
    say("check at N = %d: LML %.9f against numpy %.9f (relative %.1e); dv[%d] %.6e against a central difference %.6e"
        % (n, got, want, abs(got - want) / abs(want), i, dv[i], fd))
    assert abs(got - want) <= 1e-7 * abs(want) and abs(dv[i] - fd) <= 1e-4 * abs(fd)
    gv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--small", type=int, nargs="*", default=SMALL)
    ap.add_argument("--append-n", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib
    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max) of %d alternating rounds"
        % (D, a.reps))
    if a.sizes:
        dense_check(min(min(a.sizes), 1024), say)
    say("")
    say("1. / 2. Observe + Gradient                plain                          with variances                 difference")
    for n in list(a.small) + list(a.sizes):
        gp_, x, *_ = make(n, False)
        gv, _, *_ = make(n, True)

        def og(g):
            def run():
                g.Observe(x)
                g.Gradient()
            return lambda: timed(run)
        t = alternate({"plain": og(gp_), "v": og(gv)}, a.reps)
        say("  N = %5d%s   %s   %s   %s" % (n, " (tiny | sweep)" if n <= 128 else "               ", fmt(t["plain"]),
                                          fmt(t["v"]), diff(t["plain"], t["v"])))
        if n in a.sizes:
            # 3. with K^-1 in place
            t3 = alternate({"dv": lambda: timed(gv.NoiseVariancesGradient), "loo": lambda: timed(gv.LOO)}, a.reps)
            say("  N = %5d  3. K^-1 in place:  dv %s   LOO %s   dv - LOO %s" % (n, fmt(t3["dv"]), fmt(t3["loo"]),
                                                                              diff(t3["loo"], t3["dv"])))
        gp_.close()
        gv.close()
    if a.append_n > 0:
        say("")
        n = a.append_n
        say("4. Append behind Absorb of N = %d rows     plain                          with variances                 difference" % n)
        from gogp_amd import synth
        gp_, x, X, y, v = make(n, False)
        gv, *_ = make(n, False)
        gp_.ThetaSimil = gv.ThetaSimil = list(np.exp(x[:2]))
        gp_.ThetaNoise = gv.ThetaNoise = list(np.exp(x[2:]))
        X2, y2 = synth.make_inputs(64, D, 2)
        v2 = variances(64, np.exp(x[2]) ** 2)
        for m in (1, 64):
            def plain():
                gp_.Absorb(X, y)
                return timed(lambda: gp_.Append(X2[:m], y2[:m]))

            def noisy():
                gv.Absorb(X, y, v)
                return timed(lambda: gv.Append(X2[:m], y2[:m], v2[:m]))
            t = alternate({"plain": plain, "v": noisy}, a.reps)
            say("  m = %2d                       %s   %s   %s" % (m, fmt(t["plain"]), fmt(t["v"]), diff(t["plain"], t["v"])))
        gp_.close()
        gv.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
