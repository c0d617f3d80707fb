"""Sparse GP (GP.SetSparse, SparseObserve, SparseGradient, SparseProduce; gogp_sparse_*): wall time per call, the new
SYRK's rate beside the tile kernel's, and the bound beside the dense LML.

    python3 tools/sparse_probe.py [--reps R] [--sizes N ..] [--inducing M ..] [--out profiles/sparse.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {65536, 262144,
1048576} with M in {512, 2048, 4096} inducing points (a random subset of the inputs), default options.  Per (N, M), ms
per call, every call ending in a device synchronise:

    observe       SparseObserve: the bound
    obs+grad      SparseObserve + SparseGradient: a whole evaluation, as SparseModel runs it
    produce       SparseProduce at 1024 test points

then, per M, sparse_syrk_kernel alone on one chunk (K = 8192 rows) beside the tile kernel's GEMM_LOWER at the same M and
K (hooks gogp_bench_sparse_syrk, gogp_bench_gemm), and at N = 16384, M = 4096 the bound beside the dense LML and the
time beside the dense Observe + Gradient.  One warm-up call of each kind, then R rounds (default 5): medians and the
spread (min .. max).  The gradient is checked against a central difference of the bound along one direction, so a fast
wrong answer does not make the table."""
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
    names = ("observe", "obs+grad", "produce")
    say("%8s %5s  %s  %s" % ("N", "M", " ".join("%-30s" % s for s in names), "bound, directional derivative: relative error"))
    x = np.log(synth.theta0(D))
    v = np.array([0.6, -0.5, 0.62])
    h = 1e-4
    rng = np.random.default_rng(3)
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        Z = rng.uniform(X.min(), X.max(), (MZ, D))
        for M in a.inducing:
            g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
            g.SetSparse(X, y, X[rng.choice(n, M, replace=False)])

            def ev():
                return g.SparseObserve(x), g.SparseGradient()

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
                ts["produce"].append(timed(lambda: g.SparseProduce(Z)))
            say("%8d %5d  %s  %.9e, %.1e" % (n, M, " ".join("%-30s" % fmt(ts[k]) for k in names), bound, e))
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
