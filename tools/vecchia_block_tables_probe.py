"""Block tables built on the device (GP.SetVecchiaBlocksNearest, VecchiaBlockReneighbour, VecchiaBlockProduceNearest;
gogp_amd/csrc/vecchia_bknn.hip): wall time per call beside what it replaces and what it feeds.

    python3 tools/vecchia_block_tables_probe.py [--reps R] [--sizes N ..] [--host N] [--out profiles/vecchia_block_tables.txt]

Per N and (t, c), ms, median (min .. max) of R calls (one call where a call takes more than 5 s):
    rebuild      VecchiaBlockReneighbour: the resident table rebuilt from the resident X, nothing crosses the bus
    obs+grad     VecchiaBlockObserve + VecchiaBlockGradient on that table: the evaluation the table feeds
    knn m=63     (t = 1 only) GP.VecchiaNeighbours at m = 63, upload and download included
and, at --host N, vecchia.block_nearest on the CPU.  Then VecchiaBlockProduceNearest for 1 and 1024 test points against
VecchiaBlockProduce on a ready table.  Wall clock around synchronous calls; see DESIGN.md section 4."""
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
SHAPES = [(64, 64), (16, 48), (1, 63)]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if ts[-1] > 5.0:
            break
    return "%9.2f (%.2f .. %.2f; %d)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="t c t c ...")
    ap.add_argument("--host", type=int, default=65536, help="N of the host helper's timing (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = SHAPES if not a.shapes else list(zip(a.shapes[::2], a.shapes[1::2]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    from gogp_amd import _lib, kernel, synth, vecchia
    from gogp_amd.gp import GP
    say("library: %s" % _lib.lib().gogp_version().decode())
    say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max; calls)" % D)
    x = np.log(synth.theta0(D))
    lengths = np.linspace(0.5, 2.0, D)
    for n in a.sizes:
        X, y = synth.make_inputs(n, D, 1)
        g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, device=0)
        for t, c in shapes:
            g.SetVecchiaBlocksNearest(X, y, t, c, lengths)
            row = "N %8d (t, c) = (%3d, %3d)  rebuild %s" % (n, t, c, timed(lambda: g.VecchiaBlockReneighbour(lengths), a.reps))
            row += "  obs+grad %s" % timed(lambda: (g.VecchiaBlockObserve(x), g.VecchiaBlockGradient()), a.reps)
            if t == 1:
                row += "  knn m=63 %s" % timed(lambda: g.VecchiaNeighbours(X, 63, lengths), a.reps)
            if n == a.host:
                row += "  host block_nearest %s" % timed(lambda: vecchia.block_nearest(X, t, c, lengths), 1)
            say(row)
        t, c = shapes[0]
        g.SetVecchiaBlocksNearest(X, y, t, c, lengths)
        g.VecchiaBlockObserve(x)
        for mz in (1, 1024):
            Z = synth.make_inputs(mz, D, 2)[0]
            gsz = min(mz, 16)
            off, groups = vecchia.group_nearest_to(X, Z, gsz, c, lengths) if n <= 262144 else (None, None)
            row = "N %8d produce %4d points in groups of %2d, c = %d: nearest %s" % (
                n, mz, gsz, c, timed(lambda: g.VecchiaBlockProduceNearest(Z, gsz), a.reps))
            if off is not None:
                row += "  ready table %s" % timed(lambda: g.VecchiaBlockProduce(Z, off, groups), a.reps)
            say(row)
        g.close()


if __name__ == "__main__":
    main()
