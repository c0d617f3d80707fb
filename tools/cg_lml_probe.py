"""The iterative exact GP's LML and gradient (GP.CGObserve / CGGradient; gogp_cg_lml_gradient): what the pair reduction
costs for 1, 16 and 64 rows of weights, and what a whole evaluation costs beside the dense Observe + Gradient.

    python3 tools/cg_lml_probe.py [--reps R] [--sizes N ..] [--eval-sizes N ..] [--kernels normal matern52]
                                  [--out profiles/cg_lml.txt] [--append]

The CG section's workload (synth.make_inputs, UniformNoise at synth.theta0, D = 8) with a Scaled Normal and a Scaled
Matern-5/2 kernel.  Per (kernel, N):

    reduction  ms of ONE pass of cg_grad_kernel (+ its final sum) over all N^2 pairs for S = 1, 16 and 64 rows: the
               difference of two gogp_cg_lml_gradient calls on the same S probes, with and without the gradient (Jacobi,
               max_iter = 1: the solves cancel).  With the gradient the call runs the (alpha, alpha) pass, S = 1, and the
               probes' pass, S rows: the S = 1 figure is half the difference at one probe, the others the difference less
               that figure.  Median (min .. max) of R such differences (default 3) after a warm-up; beside it the pairs per
               second and the ratio S = 64 / S = 1 of the medians -- the matrix cores forming the weights is the claim.
    eval       (--eval-sizes, default 16384 65536) CGObserve (rank 256, 16 probes, tol 1e-8: the solve for alpha, the
               probes' block, the log-determinant, the gradient), median (min .. max) of R calls: the estimate and its
               standard error (1/2 logdet_stderr), iterations, products.  At N = 16384 the dense Observe + Gradient on
               the same data: its time, |LML_cg - LML_dense| in standard errors, and the gradient's relative error.
"""
import argparse
import ctypes
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
    ap.add_argument("--eval-sizes", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--kernels", nargs="*", default=["normal", "matern52"])
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--rank", type=int, default=256)
    ap.add_argument("--probes", type=int, default=16)
    ap.add_argument("--dense-at", type=int, default=16384)
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
        say("D = %d, Scaled kernel + UniformNoise at synth.theta0; reduction: ms of one pass of cg_grad_kernel over N^2 pairs, "
            "from differences of calls with and without the gradient; median (min .. max) of %d" % (D, a.reps))
    theta = synth.theta0(D)
    x = np.log(theta)
    simil = {"normal": kernel.Scaled(kernel.Normal), "matern52": kernel.Scaled(kernel.Matern52)}
    rng = np.random.default_rng(12)
    dp = lambda v: v.ctypes.data_as(_lib._dp)  # noqa: E731

    def mmm(ts):
        return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))

    def lml_call(g, Xi, grad):
        info = _lib.CCgLmlInfo()
        out = np.zeros(len(x))
        rc = _lib.lib().gogp_cg_lml_gradient(g._h, dp(Xi), len(Xi), Xi.shape[1], 1e-300, 1, dp(out) if grad else None, len(x),
                                             None, ctypes.byref(info), None)
        assert rc in (_lib.GOGP_OK, _lib.GOGP_ENOCONV), rc

    for kname in a.kernels:
        for n in sorted(set(a.sizes) | set(a.eval_sizes)):
            X, y = synth.make_inputs(n, D, 1)
            g = GP(D, simil[kname], kernel.UniformNoise, device=0)
            g.SetCG(X, y)
            if n in a.sizes:
                try:
                    g.CGSolve(x, rank=0, tol=1e-8, max_iter=1)  # the parameters and the Jacobi preconditioner
                except ConvergenceError:
                    pass
                per, one = {}, None
                for S in sorted(a.rows):
                    Xi = rng.standard_normal((S, n))
                    lml_call(g, Xi, True)  # warm-up: the workspaces
                    ds = []
                    for _ in range(a.reps):
                        t0, _ = timed(lambda: lml_call(g, Xi, False))
                        t1, _ = timed(lambda: lml_call(g, Xi, True))
                        ds.append(t1 - t0)
                    if S == 1:
                        per[S] = [d / 2.0 for d in ds]
                        one = statistics.median(per[S])
                    else:
                        per[S] = [d - (one if one is not None else 0.0) for d in ds]
                med = {S: statistics.median(per[S]) for S in per}
                t1 = med.get(1, float("nan"))
                say("%-8s N %8d  reduction ms: %s   pairs/s at S = 1: %.3e, at S = 64: %.3e   S = 64 / S = 1: %.2f"
                    % (kname, n, "  ".join("S = %d: %s" % (S, mmm(per[S])) for S in sorted(per)), n * float(n) / t1,
                       n * float(n) / med.get(64, float("nan")), med.get(64, float("nan")) / t1))
            if n in a.eval_sizes:
                def observe():
                    v = g.CGObserve(x, probes=a.probes, seed=1, rank=a.rank, tol=1e-8, max_iter=2000)
                    return v, g.CGGradient()
                g._cg_normals(1, n, a.rank, a.probes)  # the normals are drawn once: not part of an evaluation
                observe()
                ts = []
                for _ in range(a.reps):
                    t, (v, gr) = timed(observe)
                    ts.append(t)
                li, si = g.cg_lml_info, g.cg_info
                say("%-8s N %8d  CGObserve + gradient, rank %d (used %d), %d probes, tol 1e-8: %s ms; LML %.4f +- %.3g; alpha "
                    "in %d iterations, probes in %d .. %d; %d products in the probes' block"
                    % (kname, n, a.rank, si["rank_used"], a.probes, mmm(ts), v, 0.5 * li["logdet_stderr"], si["iterations"],
                       li["iterations"].min(), li["iterations"].max(), li["products"]))
                if n == a.dense_at:
                    d = GP(D, simil[kname], kernel.UniformNoise, ThetaSimil=list(theta[:-1]), ThetaNoise=[theta[-1]], device=0)
                    d.Absorb(X, y)

                    def dense():
                        return d.Observe(x), d.Gradient()
                    dense()
                    td = []
                    for _ in range(a.reps):
                        t, (dv, dg) = timed(dense)
                        td.append(t)
                    d.close()
                    se = 0.5 * li["logdet_stderr"]
                    say("%-8s N %8d  dense Observe + Gradient %s ms; LML %.4f: |LML_cg - LML_dense| = %.3g = %.2f standard errors; "
                        "|grad_cg - grad_dense| / |grad_dense| = %.3g (components: cg %s, dense %s)"
                        % (kname, n, mmm(td), dv, abs(v - dv), abs(v - dv) / se if se > 0 else float("nan"),
                           np.linalg.norm(gr - dg) / np.linalg.norm(dg), np.array2string(gr, precision=4),
                           np.array2string(dg, precision=4)))
            g.close()


if __name__ == "__main__":
    main()
