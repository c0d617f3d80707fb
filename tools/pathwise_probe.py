"""pathwise.draw / Paths (gogp_pathwise_*): wall time per call beside the calls it can be compared with, and the feature
kernel's rate beside the fp64 MFMA roof.

    python3 tools/pathwise_probe.py [--sizes 4096,16384] [--out profiles/pathwise.txt]

Inputs: synth.make_inputs, D = 8, Scaled(Normal) + UniformNoise, R = 1024 features.  Per N: Observe, then draw at S = 1 / 16 /
64 beside Observe on the same build; Paths(Z) and Paths.gradient(Z) (S = 16) at m = 1 / 1024 / 65536 beside GP.Sample (16
draws) at m = 1024 / 4096 and GP.ProduceGradient at m = 1024.  One warm-up call of each, then the median of three; every
call ends in a synchronise (the calls return host arrays).  The feature kernel's rate: 2 R m (ndim + S) flops over the time
of the hook gogp_test_pw_features at m = 16384, S = 64, minus the same call at R = 1 (the hook's copies and allocations),
beside gogp_mfma_f64_peak -- a LOWER bound of the kernel's rate.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, R = 8, 1024


def med3(fn):
    fn()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathwise.txt"))
    a = ap.parse_args()
    from gogp_amd import _lib, kernel, pathwise, synth
    from gogp_amd.gp import GP, mfma_f64_peak
    rng = np.random.default_rng(0)
    lines = ["pathwise_probe: %s, D = %d, R = %d, medians of three, ms" % (_lib.lib().gogp_version().decode(), D, R)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for n in [int(s) for s in a.sizes.split(",")]:
        X, y = synth.make_inputs(n, D, 1)
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
        x = np.log(np.array(synth.theta0(D), float))
        say("N = %5d: Observe %.2f" % (n, med3(lambda: g.Observe(x))))
        feat = pathwise.spectral_features(g, R, rng=rng)
        for S in (1, 16, 64):
            W, Xi = rng.standard_normal((R, S)), rng.standard_normal((S, n))
            say("N = %5d: draw S = %2d %.2f" % (n, S, med3(lambda: pathwise.draw(g, S, features=feat, W=W, Xi=Xi).close())))
        paths = pathwise.draw(g, 16, features=feat, rng=rng)
        for m in (1, 1024, 65536):
            Z = rng.uniform(X.min(), X.max(), (m, D))
            say("N = %5d m = %5d: Paths(Z) %.2f   Paths.gradient(Z) %.2f" % (n, m, med3(lambda: paths(Z)),
                                                                           med3(lambda: paths.gradient(Z))))
        for m in (1024, 4096):
            Z = rng.uniform(X.min(), X.max(), (m, D))
            xi = rng.standard_normal((16, m))
            say("N = %5d m = %5d: Sample (16 draws, jitter 1e-6) %.2f" % (n, m, med3(lambda: g.Sample(Z, xi=xi, diag_add=1e-6))))
        Z = rng.uniform(X.min(), X.max(), (1024, D))
        say("N = %5d m = %5d: ProduceGradient %.2f   Produce %.2f" % (n, 1024, med3(lambda: g.ProduceGradient(Z)),
                                                                     med3(lambda: g.Produce(Z))))
        paths.close()
        g.close()
    m, S = 16384, 64
    Z, W = rng.uniform(-1, 1, (m, D)), rng.standard_normal((R, S))
    Om, ph, am = rng.standard_normal((R, D)), rng.uniform(0, 6, R), np.ones(R)
    for grad in (False, True):
        t = med3(lambda: pathwise.features_check(Om, ph, am, Z, W, grad)) - med3(
            lambda: pathwise.features_check(Om[:1], ph[:1], am[:1], Z, W[:1], grad))
        # (the gradient: D second products; its D / 4 repeated first products are not counted)
        flops = 2.0 * R * m * (D * S if grad else D + S)
        say("feature kernel %s m = %d S = %d: %.2f ms over the empty call, >= %.1f TFLOP/s" %
            ("gradient" if grad else "value", m, S, t, flops / (t * 1e-3) / 1e12))
    say("fp64 MFMA roof %.1f TFLOP/s" % mfma_f64_peak())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
