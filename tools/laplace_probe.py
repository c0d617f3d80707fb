"""GP.LaplaceObserve / LaplaceGradient / LaplaceProduce (gogp_laplace_*): wall time per call beside the regression calls
they are built from, on the same build.

    python3 tools/laplace_probe.py [--reps R] [--sizes N ...] [--out profiles/laplace.txt]

The benchmark's inputs (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {1024, 4096,
16384}, for both likelihoods.  The targets are drawn once from the inputs' own smooth signal s (synth's y, centred and
scaled to unit variance): poisson counts with rate exp(s + 1), bernoulli outcomes with P(y = 1) = logistic(2 s).
Per size and likelihood, medians (min .. max) of R rounds (default 7), every call ending in a device synchronise:
  * Absorb: one factorisation of K (what one Newton step is built around);
  * a cold LaplaceObserve (from a = 0), its Newton steps, and the time per factorisation: an observe of s steps factors
    B s + 1 times (once more at the mode), so that figure is the observe's time over s + 1;
  * a warm LaplaceObserve at the same theta (option "laplace_warm": 0 steps, one factorisation at the stored mode);
  * LaplaceGradient on a fresh observe, and a cold observe + gradient beside the regression's Observe + Gradient;
  * LaplaceProduce of 1 and 1024 points beside Produce.
The gradient is checked against a central difference of the objective along one direction, so a fast wrong answer
does not make the table.

Measured on one MI355X (profiles/laplace.txt), N = 1024 / 4096 / 16384, ms:
  Absorb 0.64 / 2.92 / 30.6; Observe + Gradient 0.68 / 3.17 / 70.7; Produce of 1 point 0.09 / 0.15 / 0.43, of 1024 0.18 / 0.63 / 5.2
  bernoulli: 4 / 5 / 5 Newton steps; cold observe 3.5 / 16.9 / 192, i.e. 0.70 / 2.82 / 31.9 per factorisation -- a whole
             Newton iteration: products with K, line search and host round trips are in that figure -- 1.10 / 0.97 / 1.04 of
             an Absorb; warm observe 0.69 / 3.0 / 31.9; gradient 0.36 / 1.85 / 49.7; observe + gradient 3.9 / 18.8 / 241
  poisson:   8 / 8 / 9 Newton steps; cold observe 6.3 / 25.8 / 320, i.e. 0.70 / 2.86 / 32.0 per factorisation (1.10 / 0.98 /
             1.05); warm observe 0.68 / 2.7 / 31.8; gradient 0.36 / 1.87 / 49.6; observe + gradient 6.7 / 27.6 / 370
  LaplaceProduce of 1 point 0.13 / 0.38 / 2.04 (1.4 / 2.5 / 4.7 x Produce: the tile route for every m), of 1024 points
             0.21 / 0.67 / 5.7 (1.14 - 1.18 / 1.05 / 1.10 x)."""
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
LIKS = ("bernoulli", "poisson")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def fmt(t):
    return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))


def targets(lik, s, seed=5):
    rng = np.random.default_rng(seed)
    s = (s - s.mean()) / s.std()
    if lik == "bernoulli":
        return (rng.uniform(size=len(s)) < 1.0 / (1.0 + np.exp(-2.0 * s))).astype(float)
    return rng.poisson(np.exp(s + 1.0)).astype(float)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gogp_amd import _lib, kernel, synth
    from gogp_amd.gp import GP
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max) of %d rounds" % (D, a.reps))
    for n in a.sizes:
        X, s = synth.make_inputs(n, D, 1)
        x = np.log(synth.theta0(D))
        Z = synth.make_inputs(1024, D, 2)[0]
        reg = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=s, device=0)
        ts, tn = np.exp(x[:-1]), np.exp(x[-1:])

        def absorb():
            reg.ThetaSimil, reg.ThetaNoise = list(ts), list(tn)
            reg.Absorb(X, s)

        def og():
            reg.Observe(x)
            return reg.Gradient()

        for fn in (absorb, og, absorb):
            fn()
        t_abs = [timed(absorb)[0] for _ in range(a.reps)]
        t_p1 = [timed(lambda: reg.Produce(Z[:1]))[0] for _ in range(a.reps + 1)][1:]
        t_p1k = [timed(lambda: reg.Produce(Z))[0] for _ in range(a.reps + 1)][1:]
        og()
        t_og = [timed(og)[0] for _ in range(a.reps)]
        say("N = %d  regression: Absorb %s  Observe + Gradient %s  Produce(1) %s  Produce(1024) %s"
            % (n, fmt(t_abs), fmt(t_og), fmt(t_p1), fmt(t_p1k)))
        reg.close()
        for lik in LIKS:
            y = targets(lik, s)
            g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
            g.LaplaceObserve(x, lik)
            g.LaplaceGradient()
            # the gradient against a central difference along v
            v = np.array([0.6, -0.5, 0.62])
            h = 1e-4
            zp, zm = g.LaplaceObserve(x + h * v, lik), g.LaplaceObserve(x - h * v, lik)
            z0 = g.LaplaceObserve(x, lik)
            steps = g.LaplaceMode()[2]
            grad = g.LaplaceGradient()
            e = abs((zp - zm) / (2 * h) - grad @ v) / abs(grad @ v)
            assert e < 1e-3, e
            t_cold, t_grad, t_both, t_warm, t_q1, t_q1k = [], [], [], [], [], []
            for _ in range(a.reps):
                dt, _ = timed(lambda: g.LaplaceObserve(x, lik))
                dg, _ = timed(g.LaplaceGradient)
                t_cold.append(dt)
                t_grad.append(dg)
                t_both.append(dt + dg)
            g.LaplaceProduce(Z[:1])
            g.LaplaceProduce(Z)
            for _ in range(a.reps):
                t_q1.append(timed(lambda: g.LaplaceProduce(Z[:1]))[0])
                t_q1k.append(timed(lambda: g.LaplaceProduce(Z))[0])
            g.set_option("laplace_warm", 1)
            g.LaplaceObserve(x, lik)
            for _ in range(a.reps):
                t_warm.append(timed(lambda: g.LaplaceObserve(x, lik))[0])
            wsteps = g.LaplaceMode()[2]
            per = statistics.median(t_cold) / (steps + 1)
            say("N = %d  %-9s Z = %.6f, %d Newton steps; cold observe %s = %.3f ms per factorisation (%.2f x Absorb); "
                "warm observe (%d steps) %s; gradient %s; observe + gradient %s (%.2f x Observe + Gradient); "
                "produce(1) %s (%.2f x); produce(1024) %s (%.2f x); directional derivative: relative error %.1e"
                % (n, lik, z0, steps, fmt(t_cold), 1e3 * per, per / statistics.median(t_abs), wsteps, fmt(t_warm), fmt(t_grad),
                   fmt(t_both), statistics.median(t_both) / statistics.median(t_og), fmt(t_q1),
                   statistics.median(t_q1) / statistics.median(t_p1), fmt(t_q1k),
                   statistics.median(t_q1k) / statistics.median(t_p1k), e))
            g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
