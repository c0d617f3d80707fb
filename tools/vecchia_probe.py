"""Vecchia's approximation (GP.SetVecchia, VecchiaObserve, VecchiaGradient, VecchiaProduce; gogp_vecchia_*): wall time per
call, the pair rate, the sparse bound's time beside it, and the approximation itself beside the dense LML.

    python3 tools/vecchia_probe.py [--reps R] [--sizes N ..] [--neighbours m ..] [--out profiles/vecchia.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {65536, 262144,
1048576} with m in {15, 31, 63} conditioning rows.  A nearest-neighbour table at these sizes needs a spatial index, which
is not this library's business (vecchia.nearest is O(N^2 D)); the TIMING tables hold, per row, m distinct earlier rows
scattered over the 65536 rows before it -- the gather a real table causes, not its values.  Per (N, m), ms per call,
every call ending in a device synchronise:

    observe      VecchiaObserve without the terms' copy: the value
    obs+terms    VecchiaObserve as GP.VecchiaObserve runs it (N x 3 doubles come back)
    obs+grad     value + VecchiaGradient: a whole evaluation, as VecchiaModel runs it
    produce      VecchiaProduce at 1024 test points

pairs/s counts the (m + 1)(m + 2) / 2 similarity evaluations of a full block (the first rows have shorter ones): once
for observe, twice for the gradient's own pass.  Beside them SparseObserve + SparseGradient at M = 512 from the same
build and, with --cg, one iteration of the iterative exact GP (CGSolve at rank 0: the difference of a run of three
iterations and a run of one, per product).  Then, at N = 16384 where the dense LML exists, nearest tables (lengths = the kernel's): |Vecchia - dense| in the
LML and the angle between the two gradients.  One warm-up call of each kind, then R rounds (default 3): medians and the
spread.  The gradient is checked against a central difference of the value along one direction."""
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
MZ = 1024
SIZES = [65536, 262144, 1048576]
NEIGHBOURS = [15, 31, 63]
WINDOW = 65536


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt(t):
    return "%9.2f (%.2f .. %.2f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))


def scattered_table(rng, rows, m, n, causal=True):
    """Per row m distinct rows: causal, among the WINDOW rows before it (1 + (a + k b) mod WINDOW back, b odd); else anywhere."""
    if not causal:
        pw = 1 << (int(n).bit_length() - 1)  # b odd and a power-of-two modulus: m <= pw distinct values
        a, b = rng.integers(0, pw, rows), 2 * rng.integers(0, pw // 2, rows) + 1
        return np.ascontiguousarray((a[:, None] + np.arange(m)[None, :] * b[:, None]) % pw, dtype=np.int32)
    a, b = rng.integers(0, WINDOW, rows), 2 * rng.integers(0, WINDOW // 2, rows) + 1
    t = np.arange(rows)[:, None] - 1 - ((a[:, None] + np.arange(m)[None, :] * b[:, None]) % WINDOW)
    head = min(rows, WINDOW)
    h = t[:head]
    h[h < 0] = -1
    order = np.argsort(h < 0, axis=1, kind="stable")  # the padding goes behind
    t[:head] = np.take_along_axis(h, order, axis=1)
    return np.ascontiguousarray(t, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--neighbours", type=int, nargs="*", default=NEIGHBOURS)
    ap.add_argument("--dense", type=int, default=16384, help="N of the comparison with the dense LML (0: skip)")
    ap.add_argument("--cg", action="store_true", help="time one CG iteration per size as well (seconds each at N = 1048576)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib, kernel, synth, vecchia
    from gogp_amd.gp import GP
    L = _lib.lib()
    say("library: %s" % L.gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0, %d test points; ms per call: median (min .. max) of %d rounds"
        % (D, MZ, a.reps))
    names = ("observe", "obs+terms", "obs+grad", "produce")
    say("%8s %3s  %s  %-22s %-22s %s" % ("N", "m", " ".join("%-30s" % s for s in names), "pairs/s observe", "pairs/s gradient pass",
                                         "value, directional derivative: relative error"))
    x = np.log(synth.theta0(D))
    v = np.array([0.6, -0.5, 0.62])
    h = 1e-4
    rng = np.random.default_rng(3)
    dp = lambda arr: arr.ctypes.data_as(_lib._dp)  # noqa: E731
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        Z = rng.uniform(X.min(), X.max(), (MZ, D))
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
        for m in a.neighbours:
            t, tz = scattered_table(rng, n, m, n), scattered_table(rng, MZ, m, n, causal=False)
            assert L.gogp_vecchia_check(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, m, n, 1) == 0
            g.SetVecchia(X, y, t)
            val = ctypes.c_double(0.0)

            def observe():
                g._check(L.gogp_vecchia_observe(g._h, dp(x), x.size, ctypes.byref(val), None))

            def ev():
                observe()
                return g.VecchiaGradient()

            vp, vm = g.VecchiaObserve(x + h * v), g.VecchiaObserve(x - h * v)
            value, grad = g.VecchiaObserve(x), ev()
            e = abs((vp - vm) / (2 * h) - grad @ v) / abs(grad @ v)
            assert e < 1e-4, e
            g.VecchiaProduce(Z, tz)
            ts = {k: [] for k in names}
            for _ in range(a.reps):
                ts["observe"].append(timed(observe))
                ts["obs+terms"].append(timed(lambda: g.VecchiaObserve(x)))
                ts["obs+grad"].append(timed(ev))
                ts["produce"].append(timed(lambda: g.VecchiaProduce(Z, tz)))
            pairs = n * (m + 1) * (m + 2) / 2.0
            to = statistics.median(ts["observe"])
            tg = statistics.median(ts["obs+grad"]) - to
            say("%8d %3d  %s  %-22.3e %-22.3e %.9e, %.1e" % (n, m, " ".join("%-30s" % fmt(ts[k]) for k in names), pairs / to,
                                                           2 * pairs / tg, value, e))
        g.SetVecchia(None, None, None)
        M = 512
        g.SetSparse(X, y, X[rng.choice(n, M, replace=False)])

        def sparse():
            return g.SparseObserve(x), g.SparseGradient()

        sparse()
        tsp = [timed(sparse) for _ in range(a.reps)]
        say("%8d      SparseObserve + SparseGradient at M = %d: %s ms" % (n, M, fmt(tsp)))
        if a.cg:
            from gogp_amd.gp import ConvergenceError
            g.SetCG(X, y)

            def solve(iters):  # tol is out of reach: the run stops at max_iter
                t0 = time.perf_counter()
                try:
                    g.CGSolve(x, rank=0, tol=1e-14, max_iter=iters)
                except ConvergenceError:
                    pass
                return time.perf_counter() - t0, g.cg_info["products"]

            solve(1)
            (t1, p1), (t3, p3) = solve(1), solve(3)
            say("%8d      one CG iteration at rank 0 (runs of %d and %d products): %.1f ms" % (n, p1, p3, 1e3 * (t3 - t1) / (p3 - p1)))
            g.SetCG(None, None)
        g.close()
    if a.dense:
        say("")
        n = a.dense
        X, y = synth.make_inputs(n, D, 1)
        th = synth.theta0(D)
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)

        def dense():
            return g.Observe(x), g.Gradient()

        lml, dgrad = dense()
        td = [timed(dense) for _ in range(a.reps)]
        say("N = %d: dense LML %.6f, Observe + Gradient %s ms; nearest tables under the kernel's length scale %.4g"
            % (n, lml, fmt(td), th[1]))
        t0 = time.perf_counter()
        full = vecchia.nearest(X, max(a.neighbours), th[1])
        say("vecchia.nearest(m = %d) on the host: %.1f s" % (max(a.neighbours), time.perf_counter() - t0))
        for m in a.neighbours:
            g.SetVecchia(X, y, np.ascontiguousarray(full[:, :m]))  # nearest first: a prefix is the table of a smaller m

            def ev():
                return g.VecchiaObserve(x), g.VecchiaGradient()

            value, grad = ev()
            tv = [timed(ev) for _ in range(a.reps)]
            cos = float(grad @ dgrad / (np.linalg.norm(grad) * np.linalg.norm(dgrad)))
            say("m = %2d: value %.6f, |Vecchia - dense| %.4g (%.3g per observation), angle between the gradients %.4g degrees, "
                "|gradient| %.4g beside %.4g; VecchiaObserve + VecchiaGradient %s ms"
                % (m, value, abs(value - lml), abs(value - lml) / n, np.degrees(np.arccos(min(1.0, cos))), np.linalg.norm(grad),
                   np.linalg.norm(dgrad), fmt(tv)))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
