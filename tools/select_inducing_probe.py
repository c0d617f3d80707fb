"""Greedy selection of the inducing points (GP.SelectInducing; gogp_sparse_select_inducing*): wall time per selection
beside its byte model, and what the selected points buy against a random subset of the same size.

    python3 tools/select_inducing_probe.py [--reps R] [--sizes N ..] [--inducing M ..] [--out profiles/select_inducing.txt]
                                           [--append]

The sparse section's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {65536,
262144, 1048576} with M in {512, 2048, 4096}, tol = 0 so that m = M.  Per (N, M):

    select    ms of the resident form (the rows of SetSparse, nothing uploaded): one warm-up, then the median (min .. max)
              of R rounds (default 5); beside it one call of the explicit form, which also checks and uploads X
    model     the factor's traffic, 4 N M^2 bytes (step j reads j columns of N doubles), divided by the median: TB/s,
              beside the ~6.3 TB/s a streaming kernel reaches on HBM; "L3" marks the cells whose factor (8 N M bytes) is
              within the 256 MiB Infinity Cache
    effect    greedy against rng.choice(N, M) at the same theta, default jitter 1e-8: (max L_ii / min L_ii)^2 of the
              factor of Kuu + eps I (numpy, fp64; "not PD" where it fails), the bound (SparseObserve) and, at M = 4096,
              d bound / dU along its own direction against a central difference -- the case DESIGN.md records as failing
              for a random subset

The N = 1048576, M = 4096 cell takes a 34 GB factor and by the byte model about ten seconds per selection: run it on
its own (--sizes 1048576 --inducing 4096 --append) under a time limit of its own.

Measured on one MI355X (profiles/select_inducing.txt; DESIGN.md section 4, "Sparse: choosing the inducing points", has
the table): 13.8 / 202 / 785 ms at N = 65536, 218 / 3040 / 11581 ms at N = 1048576 (M = 512 / 2048 / 4096), 5.0 .. 6.1 TB/s
of the byte model; the pivot ratio falls by a factor of 50 .. 400 and dU at M = 4096 agrees with the central difference
to 7e-5 .. 4e-4 where the random subset is off by 0.09 .. 0.9; the bound at this theta is lower for the greedy points in
every cell."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
SIZES = [65536, 262144, 1048576]
INDUCING = [512, 2048, 4096]
HBM_TBS = 6.3
L3_BYTES = 256 << 20


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def pivot_ratio(U, theta, eps):
    """(max L_ii / min L_ii)^2 of chol(k(U, U) + eps I) for the Scaled Normal kernel at theta = (scale, length, ..)."""
    c, ell = theta[0], theta[1]
    sq = (U * U).sum(1)
    r2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * U @ U.T, 0.0) / (ell * ell)
    K = c * np.exp(-0.5 * r2)
    K[np.diag_indices_from(K)] = c + eps
    try:
        dg = np.diag(np.linalg.cholesky(K))
    except np.linalg.LinAlgError:
        return float("nan")
    return float((dg.max() / dg.min()) ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--inducing", type=int, nargs="*", default=INDUCING)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of replacing it (no header)")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib, kernel, synth
    from gogp_amd.gp import GP
    if not a.append:
        say("library: %s" % _lib.lib().gogp_version().decode())
        say("D = %d, Scaled Normal + UniformNoise at synth.theta0, tol = 0 (m = M), sparse_jitter_log10 = -8; select: ms of the "
            "resident form, median (min .. max) of %d rounds after a warm-up, and one call of the explicit form; model: "
            "4 N M^2 bytes / median beside ~%.1f TB/s of HBM (L3: the factor fits the Infinity Cache); effect: greedy / "
            "random subset" % (D, a.reps, HBM_TBS))
        say("%8s %5s  %-34s %9s  %-14s  %-25s %-35s %s"
            % ("N", "M", "select (resident)", "explicit", "model TB/s", "(max Lii / min Lii)^2", "bound",
               "dU rel. error (M = 4096)"))
    theta = synth.theta0(D)
    x = np.log(theta)
    rng = np.random.default_rng(3)
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        for M in a.inducing:
            g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
            Ur = X[rng.choice(n, M, replace=False)]
            g.SetSparse(X, y, Ur)
            idx, Ug, pv, trace = g.SelectInducing(x, M, tol=0.0)  # warm-up
            assert len(set(idx.tolist())) == len(idx) and np.array_equal(Ug, X[idx])
            if len(idx) < M:  # (the residuals reached zero: SetInducing keeps M, so there is nothing to compare)
                say("%8d %5d  the selection stopped at m = %d (last pivot %.3e): no timing, no comparison" % (n, M, len(idx), pv[-1]))
                g.close()
                continue
            ts = [timed(lambda: g.SelectInducing(x, M, tol=0.0)) for _ in range(a.reps)]
            te = timed(lambda: g.SelectInducing(x, M, X=X, tol=0.0))
            med = statistics.median(ts)
            tbs = 4.0 * n * M * M / med * 1e-12
            where = "L3" if 8.0 * n * M <= L3_BYTES else "HBM"

            def du_error(U):
                g.SetInducing(U)
                g.SparseObserve(x)
                dU = g.SparseGradientInducing()[1]
                vu = dU / np.linalg.norm(dU)
                g.SetInducing(U + 1e-2 * vu)
                up = g.SparseObserve(x)
                g.SetInducing(U - 1e-2 * vu)
                um = g.SparseObserve(x)
                return abs((up - um) / 2e-2 - (dU * vu).sum()) / abs((dU * vu).sum())

            bounds, ratios, dus = [], [], []
            for U in (Ug, Ur):
                g.SetInducing(U)
                bounds.append(g.SparseObserve(x))
                ratios.append(pivot_ratio(U, theta, 1e-8))
                dus.append(du_error(U) if M == 4096 else float("nan"))
            say("%8d %5d  %-34s %9.2f  %5.2f %-8s  %-25s %-35s %s"
                % (n, M, "%9.2f (%.2f .. %.2f)" % (1e3 * med, 1e3 * min(ts), 1e3 * max(ts)), 1e3 * te, tbs, where,
                   "%.3g / %s" % (ratios[0], "not PD" if np.isnan(ratios[1]) else "%.3g" % ratios[1]),
                   "%.9e / %.9e" % tuple(bounds), "-" if M != 4096 else "%.1e / %.1e" % tuple(dus)))
            say("%14s  greedy: pivots %.3e .. %.3e, trace term t0 - tr Qff %.6e" % ("", pv[0], pv[-1], trace))
            g.close()
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
