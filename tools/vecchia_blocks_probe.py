"""Vecchia on blocks of targets (GP.SetVecchiaBlocks, VecchiaBlockObserve, VecchiaBlockGradient; gogp_vecchia_blocks_*):
wall time per call beside the single-target kernel at m = 63 on the same table, and the approximation beside the dense LML.

    python3 tools/vecchia_blocks_probe.py [--reps R] [--sizes N ..] [--dense N] [--out profiles/vecchia_blocks.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {65536, 262144,
1048576} with (c, t) in {(63, 1), (127, 1), (96, 32), (64, 64), (0, 128)}: consecutive targets, the conditioning rows
scattered over the 65536 rows before the block (the gather a real table causes, not its values; tools/vecchia_probe.py
times the single-target kernel the same way).  Per (N, c, t), ms per call, every call ending in a device synchronise:

    observe      gogp_vecchia_blocks_observe without the terms' copy: the value
    obs+terms    GP.VecchiaBlockObserve (N x 3 doubles come back)
    obs+grad     value + VecchiaBlockGradient: a whole evaluation, as VecchiaBlockModel runs it

(63, 1) runs beside GP.VecchiaObserve / VecchiaGradient on the SAME rows in the same process: that kernel's figure is the
yardstick.  Then, at N = 16384 where the dense LML exists, vecchia.block_nearest under the kernel's length scale: |value -
dense| per observation and the angle between the two gradients.  One warm-up call of each kind, then R rounds (default 3):
medians and the spread."""
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
SIZES = [65536, 262144, 1048576]
SHAPES = [(63, 1), (127, 1), (96, 32), (64, 64), (0, 128)]
WINDOW = 65536


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt(t):
    return "%9.2f (%.2f .. %.2f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))


def scattered_blocks(rng, n, c, t):
    """Consecutive blocks of t targets; per block c distinct rows among the WINDOW rows before its first target (1 + (a + k b)
    mod WINDOW back, b odd), those that exist first."""
    starts = np.arange(0, n, t)
    nb = len(starts)
    a, b = rng.integers(0, WINDOW, nb), 2 * rng.integers(0, WINDOW // 2, nb) + 1
    cond = starts[:, None] - 1 - ((a[:, None] + np.arange(c)[None, :] * b[:, None]) % WINDOW)
    cond[cond < 0] = -1
    cond = np.take_along_axis(cond, np.argsort(cond < 0, axis=1, kind="stable"), axis=1)
    nc = (cond >= 0).sum(1).astype(np.int32)
    nt = np.minimum(t, n - starts).astype(np.int32)
    tbl = np.full((nb, c + t), -1, np.int32)
    targ = starts[:, None] + np.arange(t)[None, :]
    targ[targ >= n] = -1
    for k in np.flatnonzero(nc < c):  # the head of the data: shorter conditioning sets, the targets move up
        tbl[k, :nc[k]] = cond[k, :nc[k]]
        tbl[k, nc[k]:nc[k] + nt[k]] = targ[k, :nt[k]]
    full = nc == c
    tbl[full, :c] = cond[full]
    tbl[full, c:] = targ[full]
    return tbl, nc, nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--dense", type=int, default=16384, help="N of the comparison with the dense LML (0: skip)")
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
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max) of %d rounds" % (D, a.reps))
    names = ("observe", "obs+terms", "obs+grad")
    say("%8s %9s  %s  %s" % ("N", "(c, t)", " ".join("%-30s" % s for s in names), "value, directional derivative: relative error"))
    x = np.log(synth.theta0(D))
    v = np.array([0.6, -0.5, 0.62])
    h = 1e-4
    rng = np.random.default_rng(3)
    dp = lambda arr: arr.ctypes.data_as(_lib._dp)  # noqa: E731
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
        for c, t in SHAPES:
            blocks = scattered_blocks(rng, n, c, t)
            g.SetVecchiaBlocks(X, y, blocks)
            val = ctypes.c_double(0.0)

            def observe():
                g._check(L.gogp_vecchia_blocks_observe(g._h, dp(x), x.size, ctypes.byref(val), None))

            def ev():
                observe()
                return g.VecchiaBlockGradient()

            vp, vm = g.VecchiaBlockObserve(x + h * v), g.VecchiaBlockObserve(x - h * v)
            value, grad = g.VecchiaBlockObserve(x), ev()
            e = abs((vp - vm) / (2 * h) - grad @ v) / abs(grad @ v)
            ts = {k: [] for k in names}
            for _ in range(a.reps):
                ts["observe"].append(timed(observe))
                ts["obs+terms"].append(timed(lambda: g.VecchiaBlockObserve(x)))
                ts["obs+grad"].append(timed(ev))
            say("%8d %9s  %s  %.9e, %.1e" % (n, "(%d, %d)" % (c, t), " ".join("%-30s" % fmt(ts[k]) for k in names), value, e))
            if (c, t) == (63, 1):  # the single-target kernel on the same rows
                table = np.ascontiguousarray(np.where(np.arange(c)[None, :] < blocks[1][:, None], blocks[0][:, :c], -1), np.int32)
                g.SetVecchia(X, y, table)

                def ev1():
                    return g.VecchiaObserve(x), g.VecchiaGradient()

                one = ev1()
                t1 = [timed(ev1) for _ in range(a.reps)]
                say("%8d   m = 63    VecchiaObserve + VecchiaGradient on the same table: %s ms; value %.9e (difference %.2e)"
                    % (n, fmt(t1), one[0], abs(one[0] - value)))
                g.SetVecchia(None, None, None)
        g.close()
    if a.dense:
        say("")
        n = a.dense
        X, y = synth.make_inputs(n, D, 1)
        th = synth.theta0(D)
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
        lml, dgrad = g.Observe(x), g.Gradient()
        say("N = %d: dense LML %.6f; vecchia.block_nearest under the kernel's length scale %.4g" % (n, lml, th[1]))
        for c, t in SHAPES:
            g.SetVecchiaBlocks(X, y, vecchia.block_nearest(X, t, c, th[1]))
            value, grad = g.VecchiaBlockObserve(x), g.VecchiaBlockGradient()
            cos = float(grad @ dgrad / (np.linalg.norm(grad) * np.linalg.norm(dgrad)))
            say("(c, t) = (%3d, %3d): value %.6f, |value - dense| %.4g (%.3g per observation), angle between the gradients %.4g "
                "degrees" % (c, t, value, abs(value - lml), abs(value - lml) / n, np.degrees(np.arccos(min(1.0, cos)))))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
