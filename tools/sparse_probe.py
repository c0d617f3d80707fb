"""Sparse GP (GP.SetSparse, SetInducing, SparseObserve, SparseGradient, SparseGradientInducing, SparseProduce;
gogp_sparse_*): wall time per call, the new SYRK's rate beside the tile kernel's, and the bound beside the dense LML.

    python3 tools/sparse_probe.py [--reps R] [--sizes N ..] [--inducing M ..] [--out profiles/sparse_inducing.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {65536, 262144,
1048576} with M in {512, 2048, 4096} inducing points (a random subset of the inputs), default options.  Per (N, M), ms
per call, every call ending in a device synchronise:

    observe       SparseObserve: the bound
    obs+grad      SparseObserve + SparseGradient: a whole evaluation, as SparseModel runs it
    obs+grad+dU   SparseObserve + SparseGradientInducing: the same with the derivative in the inducing points
    produce       SparseProduce at 1024 test points
    set_inducing  SetInducing: new inducing points, the data stays on the device
    set_data      SetSparse: the only way to move them before SetInducing -- everything again, X and y included

then, per M, sparse_syrk_kernel alone on one chunk (K = 8192 rows) beside the tile kernel's GEMM_LOWER at the same M and
K (hooks gogp_bench_sparse_syrk, gogp_bench_gemm), and at N = 16384, M = 4096 the bound beside the dense LML and the
time beside the dense Observe + Gradient.  One warm-up call of each kind, then R rounds (default 5): medians and the
spread (min .. max).  The gradient is checked against a central difference of the bound along one direction, so a fast
wrong answer does not make the table; so is dU, along one direction of the inducing points.

Measured on one MI355X (profiles/sparse_inducing.txt; DESIGN.md section 4, "Sparse", has the table): obs+grad+dU beside
obs+grad at N = 65536 16.5 / 36.3 / 118.8 ms beside 15.4 / 34.6 / 115.2 (M = 512 / 2048 / 4096), at N = 1048576 244.0 /
494.6 / 1590.2 beside 231.3 / 477.9 / 1557.0: 2 - 7 % more; set_inducing 0.06 - 0.15 ms beside set_data 2.4 - 8.6 ms.  dU
against the central difference: 8e-6 .. 6.7e-3 at a jitter of 1e-6; at the default 1e-8 1e-4 .. 3e-3 up to M = 2048 and
0.09 / 0.5 / 0.9 at M = 4096 (N = 65536 / 262144 / 1048576): the conditioning of Kuu, see DESIGN."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
MZ = 1024
SIZES = [65536, 262144, 1048576]
INDUCING = [512, 2048, 4096]
CHUNK = 8192


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt(t):
    return "%9.2f (%.2f .. %.2f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--inducing", type=int, nargs="*", default=INDUCING)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib, kernel, synth
    from gogp_amd.gp import GP, bench_gemm
    import ctypes
    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0, sparse_chunk = %d, sparse_jitter_log10 = -8, %d test points; "
        "ms per call: median (min .. max) of %d rounds" % (D, CHUNK, MZ, a.reps))
    names = ("observe", "obs+grad", "obs+grad+dU", "produce", "set_inducing", "set_data")
    say("%8s %5s  %s  %s" % ("N", "M", " ".join("%-30s" % s for s in names),
                             "bound, directional derivative: relative error in log theta, in U (in U at a jitter of 1e-6)"))
    x = np.log(synth.theta0(D))
    v = np.array([0.6, -0.5, 0.62])
    h = 1e-4
    rng = np.random.default_rng(3)
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        Z = rng.uniform(X.min(), X.max(), (MZ, D))
        for M in a.inducing:
            g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
            U = X[rng.choice(n, M, replace=False)]
            g.SetSparse(X, y, U)

            def ev():
                return g.SparseObserve(x), g.SparseGradient()

            def evu():
                return g.SparseObserve(x), g.SparseGradientInducing()

            # the derivative in U along its own direction dU / |dU| (along a random one the sum over the M x D
            # coordinates cancels to ~|dU| / sqrt(M D)); every coordinate moves by less than 1e-2.  Asserted at a jitter
            # of 1e-6 and reported at the default 1e-8, where dU presumably carries the rounding of P and G = Y (..) Y^T at
            # cond(Kuu + eps I) ~ 1e10 .. 1e12: measured 1e-2 .. 1e-1 of |dU| at M = 4096, a tenth of it per decade of jitter
            def du_error():
                g.SparseObserve(x)
                dU = g.SparseGradientInducing()[1]
                vu = dU / np.linalg.norm(dU)
                g.SetInducing(U + 1e-2 * vu)
                up = g.SparseObserve(x)
                g.SetInducing(U - 1e-2 * vu)
                um = g.SparseObserve(x)
                g.SetInducing(U)
                return abs((up - um) / 2e-2 - (dU * vu).sum()) / abs((dU * vu).sum())

            g.set_option("sparse_jitter_log10", -6)
            eu6 = du_error()
            assert eu6 < 1e-2, eu6
            g.set_option("sparse_jitter_log10", -8)
            eu = du_error()
            bp, bm = g.SparseObserve(x + h * v), g.SparseObserve(x - h * v)
            bound, grad = ev()
            e = abs((bp - bm) / (2 * h) - grad @ v) / abs(grad @ v)
            # (a fast wrong answer is off in the first digit; the difference itself carries the rounding of two bounds of
            # size ~1e5 at cond(Kuu + eps I) ~ 1e10, divided by 2 h: the tests measure the gradient, not this)
            assert e < 1e-2, e
            g.SparseProduce(Z)
            ts = {k: [] for k in names}
            for _ in range(a.reps):
                ts["observe"].append(timed(lambda: g.SparseObserve(x)))
                ts["obs+grad"].append(timed(ev))
                ts["obs+grad+dU"].append(timed(evu))
                ts["produce"].append(timed(lambda: g.SparseProduce(Z)))
                ts["set_inducing"].append(timed(lambda: g.SetInducing(U)))
                ts["set_data"].append(timed(lambda: g.SetSparse(X, y, U)))
            say("%8d %5d  %s  %.9e, %.1e, %.1e (%.1e)" % (n, M, " ".join("%-30s" % fmt(ts[k]) for k in names), bound, e, eu, eu6))
            g.close()
    say("")
    say("sparse_syrk_kernel alone on one chunk of K = %d rows beside the tile kernel's GEMM_LOWER at the same M and K: "
        "ms per launch, TFLOP/s on the flops launched" % CHUNK)
    for M in a.inducing:
        ms, tf = ctypes.c_double(0.0), ctypes.c_double(0.0)
        rc = _lib.hooks().gogp_bench_sparse_syrk(0, CHUNK, M, 10, ctypes.byref(ms), ctypes.byref(tf))
        assert rc == _lib.GOGP_OK, rc
        tms, ttf = bench_gemm(1, M // 128, M // 128, CHUNK, reps=10, device=0)
        say("M = %5d: sparse_syrk %8.3f ms %6.1f TFLOP/s   GEMM_LOWER %8.3f ms %6.1f TFLOP/s" % (M, ms.value, tf.value, tms, ttf))
    say("")
    n, M = 16384, 4096
    X, y = synth.make_inputs(n, D, 1)
    g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
    g.SetSparse(X, y, X[rng.choice(n, M, replace=False)])

    def dense():
        return g.Observe(x), g.Gradient()

    def sparse():
        return g.SparseObserve(x), g.SparseGradient()

    lml, bound = dense()[0], sparse()[0]
    td, tsp = [], []
    for _ in range(a.reps):
        td.append(timed(dense))
        tsp.append(timed(sparse))
    say("N = %d, M = %d: bound %.6f beside the dense LML %.6f; SparseObserve + SparseGradient %s ms beside the dense "
        "Observe + Gradient %s ms" % (n, M, bound, lml, fmt(tsp), fmt(td)))
    g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
