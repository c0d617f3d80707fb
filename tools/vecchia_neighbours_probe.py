"""Neighbour tables built on the device (GP.SetVecchiaNearest, VecchiaReneighbour, VecchiaProduceNearest;
gogp_amd/csrc/vecchia_knn.hip): wall time per call and the pair rate.

    python3 tools/vecchia_neighbours_probe.py [--reps R] [--sizes N ..] [--neighbours m ..] [--host N]
                                              [--out profiles/vecchia_neighbours.txt]

The benchmark's inputs (synth.make_inputs, D = 8) at N in {65536, 262144, 1048576} with m in {15, 31, 63}, lengths = the
kernel's length scale.  Per (N, m), ms per call, every call ending in a device synchronise:

    set nearest    SetVecchiaNearest: upload of X, y and the causal search
    reneighbour    VecchiaReneighbour: the causal search on the resident rows (N (N - 1) / 2 pairs)
    nearest 1      VecchiaProduceNearest of one test point (N pairs), beside `produce 1`: VecchiaProduce with a ready table
    nearest 1024   ... of 1024 test points (1024 N pairs), beside `produce 1024`

pairs/s is N (N - 1) / 2 over the reneighbour's time.  Beside it the count bound: a pair costs 3 D fp64 vector
instructions (a subtraction, a multiplication and an addition per dimension, unfused), and a CU retires 64 fp64 lanes a
clock -- FP64_LANE_RATE lanes a second at the peak clock.  One warm-up call of each kind, then R rounds (default 3):
medians and the spread.  --host N times gogp_amd.vecchia.nearest at m = 63 on the host and checks the device's table
against it."""
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
NEIGHBOURS = [15, 31, 63]
FP64_LANE_RATE = 256 * 64 * 2.4e9  # CUs x fp64 lanes per clock x peak clock: 78.6 Tflop/s counted as fused pairs


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt(t):
    return "%10.2f (%.2f .. %.2f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--neighbours", type=int, nargs="*", default=NEIGHBOURS)
    ap.add_argument("--host", type=int, default=16384, help="N of the host helper's timing at m = 63 (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from gogp_amd import _lib, kernel, synth, vecchia
    from gogp_amd.gp import GP
    say("library: %s" % _lib.lib().gogp_version().decode())
    th = synth.theta0(D)
    x = np.log(th)
    ln = float(th[1])
    bound = FP64_LANE_RATE / (3 * D)
    say("D = %d, lengths = %.4g; ms per call: median (min .. max) of %d rounds; count bound %.3e pairs/s (3 D fp64 vector "
        "instructions a pair at %.3e lanes/s)" % (D, ln, a.reps, bound, FP64_LANE_RATE))
    names = ("set nearest", "reneighbour", "nearest 1", "produce 1", "nearest 1024", "produce 1024")
    say("%8s %3s  %s  %-12s %s" % ("N", "m", " ".join("%-32s" % s for s in names), "pairs/s", "of the count bound"))
    rng = np.random.default_rng(5)
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        Z = rng.uniform(X.min(), X.max(), (1024, D))
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
        for m in a.neighbours:
            ts = {k: [] for k in names}
            g.SetVecchiaNearest(X, y, m, ln)
            g.VecchiaObserve(x)
            tz = g.VecchiaProduceNearest(Z, table=True)[2]
            g.VecchiaProduce(Z[:1], tz[:1])
            for _ in range(a.reps):
                ts["set nearest"].append(timed(lambda: g.SetVecchiaNearest(X, y, m, ln)))
                ts["reneighbour"].append(timed(lambda: g.VecchiaReneighbour(ln)))
                g.VecchiaObserve(x)
                ts["nearest 1"].append(timed(lambda: g.VecchiaProduceNearest(Z[:1])))
                ts["produce 1"].append(timed(lambda: g.VecchiaProduce(Z[:1], tz[:1])))
                ts["nearest 1024"].append(timed(lambda: g.VecchiaProduceNearest(Z)))
                ts["produce 1024"].append(timed(lambda: g.VecchiaProduce(Z, tz)))
            rate = n * (n - 1) / 2.0 / statistics.median(ts["reneighbour"])
            say("%8d %3d  %s  %-12.3e %.3f" % (n, m, " ".join("%-32s" % fmt(ts[k]) for k in names), rate, rate / bound))
        g.close()
    if a.host:
        n = a.host
        X, _ = synth.make_inputs(n, D, 1)
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
        g.VecchiaNeighbours(X[:256], 63, ln)
        td = [timed(lambda: g.VecchiaNeighbours(X, 63, ln)) for _ in range(a.reps)]
        t0 = time.perf_counter()
        want = vecchia.nearest(X, 63, ln)
        th_ = time.perf_counter() - t0
        same = np.array_equal(g.VecchiaNeighbours(X, 63, ln), want)
        say("")
        say("N = %d, m = 63: vecchia.nearest on the host %.1f s; VecchiaNeighbours (upload, search, table back) %s ms; "
            "tables equal: %s" % (n, th_, fmt(td), same))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
