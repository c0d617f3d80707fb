"""The iterative exact GP with "cg_precision" = 32 (cg_mixed.hip: the product with the similarity evaluated in single
precision; cg_api.hip: restarts on the true fp64 residual) beside the fp64 path of the same build, in one process.

    python3 tools/cg_mixed_probe.py [--reps R] [--sizes N ..] [--big-sizes N ..] [--solve-sizes N ..] [--ranks R ..]
                                    [--solve-reps R] [--kernels normal matern52] [--out profiles/cg_mixed.txt] [--append]

tools/cg_probe.py's workload (synth.make_inputs, UniformNoise at synth.theta0, D = 8) and its method.  Per (kernel, N):

    product    ms per CG iteration at rank 0 for T = 1, 16 and 64 columns -- the difference of two CGSolveColumns calls of 2
               and 6 iterations, divided by 4; median (min .. max) of R such differences after a warm-up -- for three
               operators: the fp64 product (kmm_kernel), the fast instance of kmm32_kernel (one radial term) and its generic
               instance, forced by writing the same kernel as a sum of two terms of half the scale.  An iteration is one
               product and the column-wise kernels; pairs per second and the ratio to the fp64 figure are of T = 1.
    big        (--big-sizes, the first kernel only) T = 1 from ONE difference of runs of 1 and 3 iterations.
    solve      (--solve-sizes) CGSolve at tol = 1e-8 for the ranks given, fp64 and mixed: iterations, rounds, the split of the
               products, wall ms (median of --solve-reps calls), and which of the two won.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 65536, 262144])
    ap.add_argument("--big-sizes", type=int, nargs="*", default=[1048576])
    ap.add_argument("--solve-sizes", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--ranks", type=int, nargs="*", default=[0, 64, 256])
    ap.add_argument("--kernels", nargs="*", default=["normal", "matern52"])
    ap.add_argument("--columns", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--max-iter", type=int, default=4000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()

    if a.out and not a.append:
        open(a.out, "w").close()

    def say(s):  # every line at once: a long run leaves what it measured so far
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    from gogp_amd import _lib, kernel, synth
    from gogp_amd.gp import GP, ConvergenceError
    if not a.append:
        say("library: %s" % _lib.lib().gogp_version().decode())
        say("D = %d, Scaled kernel + UniformNoise at synth.theta0; product: ms per CG iteration at rank 0 (one product + the "
            "column-wise kernels), from differences of runs of 2 and 6 iterations; median (min .. max) of %d" % (D, a.reps))
    theta = synth.theta0(D)
    x1 = np.log(theta)
    x2 = np.log([theta[0] / 2, theta[1], theta[0] / 2, theta[1], theta[2]])  # the same kernel as a sum of two terms
    base = {"normal": kernel.Normal, "matern52": kernel.Matern52}
    rng = np.random.default_rng(11)

    def columns(g, B, iters):
        try:
            g.CGSolveColumns(B, tol=1e-300, max_iter=iters)
        except ConvergenceError:
            pass

    def mmm(ts):
        return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))

    def handle(kname, X, y, two_terms):
        k = [kernel.Scaled(base[kname]) for _ in range(2)]
        g = GP(D, kernel.Sum(k) if two_terms else k[0], kernel.UniformNoise, device=0)
        g.SetCG(X, y)
        try:
            g.CGSolve(x2 if two_terms else x1, rank=0, tol=1e-8, max_iter=1)  # the parameters and the Jacobi preconditioner
        except ConvergenceError:
            pass
        return g

    for kname in a.kernels:
        big = a.big_sizes if kname == a.kernels[0] else []
        for n in sorted(set(a.sizes) | set(a.solve_sizes) | set(big)):
            X, y = synth.make_inputs(n, D, 1)
            g = handle(kname, X, y, False)
            if n in a.sizes or n in big:
                g2 = handle(kname, X, y, True)
                ops = (("fp64", g, 64), ("fast32", g, 32), ("generic32", g2, 32))
                its, div = ((2, 6), 4.0) if n in a.sizes else ((1, 3), 2.0)
                for T in (a.columns if n in a.sizes else [1]):
                    B = rng.standard_normal((T, n))
                    med = {}
                    for name, h, prec in ops:
                        h.set_option("cg_precision", prec)
                        columns(h, B, its[0])  # warm-up: the workspaces
                        ts = []
                        for _ in range(a.reps if n in a.sizes else 1):
                            lo, _ = timed(lambda: columns(h, B, its[0]))
                            hi, _ = timed(lambda: columns(h, B, its[1]))
                            ts.append((hi - lo) / div)
                        med[name] = statistics.median(ts)
                        say("%-8s N %8d  T %2d  %-9s iteration ms %s   pairs/s %.3e   fp64 / this %.2f"
                            % (kname, n, T, name, mmm(ts), n * float(n) / med[name], med["fp64"] / med[name]))
                g2.close()
            if n in a.solve_sizes:
                for rank in a.ranks:
                    res = {}
                    for prec in (64, 32):
                        g.set_option("cg_precision", prec)
                        ts, info = [], None
                        for _ in range(a.solve_reps):
                            try:
                                t, info = timed(lambda: g.CGSolve(x1, rank=rank, tol=1e-8, max_iter=a.max_iter))
                            except ConvergenceError as e:
                                t, info = float("nan"), e.result
                            ts.append(t)
                        res[prec] = (statistics.median(ts), info, g.cg_rounds)
                        say("%-8s N %8d  rank %4d (used %4d)  cg_precision %d: %4d iterations, rounds %d, products32 %d, "
                            "products64 %d, fallbacks %d, %s ms, rel_residual %.2e%s"
                            % (kname, n, rank, info["rank_used"], prec, info["iterations"], res[prec][2]["rounds"],
                               res[prec][2]["products32"], res[prec][2]["products64"], res[prec][2]["fallbacks"], mmm(ts),
                               info["rel_residual"], "" if info["converged"] else " NOT CONVERGED"))
                    say("%-8s N %8d  rank %4d: %s wins, fp64 / mixed wall time %.2f"
                        % (kname, n, rank, "mixed" if res[32][0] < res[64][0] else "fp64", res[64][0] / res[32][0]))
            g.close()


if __name__ == "__main__":
    main()
