"""GP.BlockCV and GP.BlockCVGradient (gogp_blockcv, gogp_blockcv_gradient): wall time per call beside GP.LOO,
GP.LOOGradient and Observe + Gradient of the same build, and the time of the two new launches alone.

    python3 tools/blockcv_probe.py [--reps R] [--out profiles/blockcv.txt]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o blockcv -- python3 tools/blockcv_probe.py --trace
    python3 tools/blockcv_probe.py --parse DIR [--append profiles/blockcv.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {1024, 4096,
16384}, equal blocks of 1, 16 and 128 rows.  Per size one Observe + Gradient leaves K^-1 on the device; the calls are
then timed on that state (none changes it, none is cached).  Every call ends in the ABI's synchronise.  Two warm-up
calls of each kind, then R alternating rounds (default 5): medians and the spread (min .. max).  Per block length the
score is checked against the sum of the returned log densities and the gradient against a central difference of the
score along one direction; with blocks of one row the values and the gradient are compared with LOO's on the same
handle, and the differences go into the table.

--trace: per size and block length one Observe + Gradient and four BlockCVGradient calls, for a kernel trace in a run of
its own.  --parse: reads that trace (the *kernel_trace.csv under DIR) and prints, per BlockCVGradient call, the time of
the group kernel, of the block multiply and of the product Bm Bm^T behind it (the launches between the multiply and the
rank-2 correction)."""
import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
SIZES = [1024, 4096, 16384]
LENGTHS = [1, 16, 128]
TRACE_CALLS = 4


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls


def make_gp(n):
    from gogp_amd import kernel, synth
    from gogp_amd.gp import GP
    X, y = synth.make_inputs(n, D, 1)
    g = GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y, device=0)
    return g, np.log(synth.theta0(D))


def parse(trace_dir, sizes):
    rows = []
    for base, _, files in os.walk(trace_dir):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                with open(os.path.join(base, f)) as fh:
                    for r in csv.DictReader(fh):
                        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls, cur = [], None
    for t0, t1, name in rows:
        us = (t1 - t0) / 1e3
        if "blockcv_groups_kernel" in name:
            cur = {"groups": us, "apply": 0.0, "syrk": 0.0, "stage": "groups"}
            calls.append(cur)
        elif cur is None:
            continue
        elif "blockcv_apply_kernel" in name:
            cur["apply"] = us
            cur["stage"] = "syrk"
        elif "loo_rank2_kernel" in name:
            cur = None
        elif cur["stage"] == "syrk":
            cur["syrk"] += us
    calls = [c for c in calls if c["syrk"] > 0.0]  # (BlockCV() alone launches the group kernel only)
    out = ["rocprofv3 --kernel-trace, a run of its own (tools/blockcv_probe.py --trace: %d BlockCVGradient calls per size and "
           "block length); us per launch, per call in launch order:" % TRACE_CALLS,
           "%6s %6s  %12s %14s %12s  %s" % ("N", "block", "group kernel", "block multiply", "Bm Bm^T", "multiply / product")]
    cases = [(n, b) for n in sizes for b in LENGTHS]
    for i, c in enumerate(calls):
        n, b = cases[i // TRACE_CALLS] if i // TRACE_CALLS < len(cases) else (0, 0)
        out.append("%6d %6d  %12.2f %14.2f %12.2f  %.4f" % (n, b, c["groups"], c["apply"], c["syrk"], c["apply"] / c["syrk"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parse", default=None)
    ap.add_argument("--append", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.parse:
        for s in parse(a.parse, a.sizes):
            say(s)
        if a.append:
            with open(a.append, "a") as f:
                f.write("\n" + "\n".join(lines) + "\n")
        return
    from gogp_amd import _lib
    from gogp_amd.gp import blocks
    say("library: %s" % _lib.lib().gogp_version().decode())
    if not a.trace:
        say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max) of %d alternating rounds"
            % (D, a.reps))
        say("%6s %6s  %-26s %-26s %-26s %-26s %-26s  %s"
            % ("N", "block", "Observe + Gradient", "LOO", "LOOGradient", "BlockCV", "BlockCVGradient",
               "score, directional derivative: relative error"))
    for n in a.sizes:
        g, x = make_gp(n)

        def og():
            g.Observe(x)
            return g.Gradient()

        og()
        for length in LENGTHS:
            start = blocks(n, length)
            bcv = lambda: g.BlockCV(start)  # noqa: E731
            bcvg = lambda: g.BlockCVGradient(start)  # noqa: E731
            if a.trace:
                for _ in range(TRACE_CALLS):
                    bcvg()
                say("traced N = %d, blocks of %d" % (n, length))
                continue
            kinds = (og, g.LOO, g.LOOGradient, bcv, bcvg)
            for fn in kinds:
                fn()
                fn()
            # checks: the score is the sum of the log densities; the gradient matches a central difference along v
            v = np.array([0.6, -0.5, 0.62])
            h = 1e-4
            sp = (g.Observe(x + h * v), g.BlockCVScore(start))[1]
            sm = (g.Observe(x - h * v), g.BlockCVScore(start))[1]
            og()
            score, grad = g.BlockCVScore(start), bcvg()
            e1 = abs(score - bcv()[2].sum()) / abs(score)
            e2 = abs((sp - sm) / (2 * h) - grad @ v) / abs(grad @ v)
            assert e1 < 1e-10 and e2 < 1e-3, (e1, e2)
            note = "%.1e, %.1e" % (e1, e2)
            if length == 1:
                loo, lg = g.LOO(), g.LOOGradient()
                dv = max(np.abs(p - q).max() for p, q in zip(bcv(), loo))
                dg = np.abs(grad - lg).max() / np.abs(lg).max()
                note += "; against LOO on the same handle: values max |diff| %.1e, gradient %.1e of its largest component" \
                    % (dv, dg)
            calls = 2 if n >= 16384 else 10
            ts = [[] for _ in kinds]
            for _ in range(a.reps):
                og()  # the cross-validation calls are timed on a finished Observe + Gradient
                for t, fn, mult in zip(ts, kinds, (1, 10, 1, 10, 1)):
                    t.append(window(fn, calls * mult))

            def fmt(t):
                return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))
            say("%6d %6d  %-26s %-26s %-26s %-26s %-26s  %s" % ((n, length) + tuple(fmt(t) for t in ts) + (note,)))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
