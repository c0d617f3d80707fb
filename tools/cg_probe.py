"""The iterative exact GP (GP.SetCG / CGSolve / CGSolveColumns / CGProduce; gogp_cg_*): what one matrix-free product costs
for 1, 16 and 64 right-hand sides, and what a whole solve and a forecast cost.

    python3 tools/cg_probe.py [--reps R] [--sizes N ..] [--big-sizes N ..] [--solve-sizes N ..] [--ranks R ..]
                              [--kernels normal matern52] [--out profiles/cg.txt] [--append]

The sparse section's workload (synth.make_inputs, UniformNoise at synth.theta0, D = 8) with a Scaled Normal and a Scaled
Matern-5/2 kernel.  Per (kernel, N):

    iteration  ms per CG iteration at rank 0 (Jacobi) for T = 1, 16 and 64 columns in lock-step: the difference of two
               CGSolveColumns calls of 2 and 6 iterations, divided by 4 -- uploads, the start-up and the true-residual
               product cancel --, median (min .. max) of R such differences (default 3) after a warm-up.  One iteration is
               one product (kmm_kernel + kmm_finish_kernel) and the column-wise kernels (three two-stage dot products, two
               updates, the Jacobi scaling), whose traffic is ~100 N T bytes.  Beside it the pairs per second of T = 1 and
               the ratio T = 64 / T = 1 of the medians: the claim the design rests on.
    big        (--big-sizes, default 1048576; the first kernel only) the same for T = 1 and 64 from ONE difference of runs
               of 1 and 3 iterations: a product takes seconds there.
    solve      (--solve-sizes, default 16384) CGSolve at tol = 1e-8 for the ranks given: rank used, iterations, total ms
               (the preconditioner's construction included; median (min .. max) of R calls), relative residual; CGProduce,
               one call each: one point, the means of 1024 points, 1024 points with their deviations (16 lock-step blocks).
    dense      (N = 16384 only) Absorb on the same data and the distance between the two alpha.
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 65536, 262144])
    ap.add_argument("--big-sizes", type=int, nargs="*", default=[1048576])
    ap.add_argument("--solve-sizes", type=int, nargs="*", default=[16384])
    ap.add_argument("--ranks", type=int, nargs="*", default=[0, 64, 256, 1024])
    ap.add_argument("--kernels", nargs="*", default=["normal", "matern52"])
    ap.add_argument("--columns", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--max-iter", type=int, default=1000)
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
        say("D = %d, Scaled kernel + UniformNoise at synth.theta0; iteration: ms per CG iteration at rank 0 (one product + the "
            "column-wise kernels), from differences of runs of 2 and 6 iterations; median (min .. max) of %d" % (D, a.reps))
    theta = synth.theta0(D)
    x = np.log(theta)
    simil = {"normal": kernel.Scaled(kernel.Normal), "matern52": kernel.Scaled(kernel.Matern52)}
    rng = np.random.default_rng(11)

    def columns(g, B, iters):
        try:
            g.CGSolveColumns(B, tol=1e-300, max_iter=iters)
        except ConvergenceError:
            pass

    def mmm(ts):
        return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))

    for kname in a.kernels:
        big = a.big_sizes if kname == a.kernels[0] else []
        for n in sorted(set(a.sizes) | set(a.solve_sizes) | set(big)):
            X, y = synth.make_inputs(n, D, 1)
            g = GP(D, simil[kname], kernel.UniformNoise, device=0)
            g.SetCG(X, y)
            try:
                g.CGSolve(x, rank=0, tol=1e-8, max_iter=1)  # the parameters and the Jacobi preconditioner
            except ConvergenceError:
                pass
            if n in a.sizes:
                per = {}
                for T in a.columns:
                    B = rng.standard_normal((T, n))
                    columns(g, B, 2)  # warm-up: the workspaces
                    per[T] = []
                    for _ in range(a.reps):
                        t2, _ = timed(lambda: columns(g, B, 2))
                        t6, _ = timed(lambda: columns(g, B, 6))
                        per[T].append((t6 - t2) / 4.0)
                med = {T: statistics.median(per[T]) for T in per}
                t1 = med.get(1, float("nan"))
                say("%-8s N %8d  iteration ms: %s   pairs/s at T = 1: %.3e   T = 64 / T = 1: %.2f"
                    % (kname, n, "  ".join("T = %d: %s" % (T, mmm(per[T])) for T in a.columns), n * float(n) / t1,
                       med.get(64, float("nan")) / t1))
            elif n in big:
                per = {}
                for T in (1, 64):
                    B = rng.standard_normal((T, n))
                    columns(g, B, 1)  # warm-up: the workspaces
                    t1_, _ = timed(lambda: columns(g, B, 1))
                    t3_, _ = timed(lambda: columns(g, B, 3))
                    per[T] = (t3_ - t1_) / 2.0
                    say("%-8s N %8d  iteration ms, one difference of runs of 1 and 3 iterations: T = %d: %9.1f"
                        % (kname, n, T, 1e3 * per[T]))
                say("%-8s N %8d  pairs/s at T = 1: %.3e   T = 64 / T = 1: %.2f" % (kname, n, n * float(n) / per[1], per[64] / per[1]))
            if n in a.solve_sizes:
                for rank in a.ranks:
                    ts, info = [], None
                    for _ in range(a.reps):
                        try:
                            t, info = timed(lambda: g.CGSolve(x, rank=rank, tol=1e-8, max_iter=a.max_iter))
                        except ConvergenceError as e:
                            t, info = float("nan"), e.result
                        ts.append(t)
                    Z = X[:1024] + 0.01
                    tp1, _ = timed(lambda: g.CGProduce(Z[:1], tol=1e-8, max_iter=a.max_iter))
                    tpm, _ = timed(lambda: g.CGProduce(Z, sigma=False))
                    tps, _ = timed(lambda: g.CGProduce(Z, tol=1e-8, max_iter=a.max_iter))
                    say("%-8s N %8d  rank %4d (used %4d): %4d iterations, %s ms, rel_residual %.2e%s; CGProduce: 1 point "
                        "%8.1f ms, 1024 means %7.1f ms, 1024 with sigma %9.1f ms (%d products)"
                        % (kname, n, rank, info["rank_used"], info["iterations"], mmm(ts), info["rel_residual"],
                           "" if info["converged"] else " NOT CONVERGED", 1e3 * tp1, 1e3 * tpm, 1e3 * tps, g.cg_info["products"]))
                    if n == 16384 and rank == 64:
                        acg = g.CGAlpha()
                        d = GP(D, simil[kname], kernel.UniformNoise, ThetaSimil=list(theta[:-1]), ThetaNoise=[theta[-1]], device=0)
                        d.Absorb(X, y)
                        td, _ = timed(lambda: d.Absorb(X, y))
                        ad = np.array(d.Alpha)
                        d.close()
                        say("%-8s N %8d  dense Absorb %.1f ms; |alpha_cg - alpha_dense| / |alpha_dense| = %.2e"
                            % (kname, n, 1e3 * td, np.linalg.norm(acg - ad) / np.linalg.norm(ad)))
            g.close()


if __name__ == "__main__":
    main()
