"""GP.LOO and GP.LOOGradient (gogp_loo, gogp_loo_gradient): wall time per call beside Observe + Gradient, and the
time of each launch behind them.

    python3 tools/loo_probe.py [--reps R] [--out profiles/loo.txt]
    rocprofv3 --kernel-trace -d DIR -o loo -- python3 tools/loo_probe.py --trace
    python3 tools/loo_probe.py --parse DIR [--append profiles/loo.txt]

The benchmark's workload (synth.make_inputs, Scaled Normal + UniformNoise at synth.theta0, D = 8) at N in {1024, 4096,
16384}.  Per size one Observe + Gradient leaves K^-1 on the device; LOO() and LOOGradient() are then timed on that
state (neither changes it, neither is cached), and Observe + Gradient itself beside them on the same build.  Every
call ends in a device synchronise.  Two warm-up calls of each kind, then R alternating rounds (default 9): medians and
the spread (min .. max).  The score is checked against the sum of the returned log densities and the gradient against a
central difference of the score along one direction, so a fast wrong answer does not make the table.

--trace: per size one Observe + Gradient and four LOOGradient calls, for a kernel trace in a run of its own.
--parse: reads that trace (the *kernel_trace.csv under DIR) and prints, per LOOGradient call, the time of each launch:
statistics, scale + symv pass (with the final sum of u), the product B B^T on the tile kernel (the launch between the
sum of u and the rank-2 correction) with its rate, the rank-2 correction, the gradient reduction (all launches between
the correction and the next call)."""
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


def syrk_flops(n):
    nblk = (n + 255) // 256 * 2  # 128-tiles of the padded size
    return 2.0 * (nblk * (nblk + 1) // 2) * 128.0 * 128.0 * (nblk * 128.0)


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
        if "loo_stats_kernel" in name:
            cur = {"stats": us, "symv": 0.0, "syrk": 0.0, "rank2": 0.0, "reduce": 0.0, "stage": "stats"}
            calls.append(cur)
        elif cur is None:
            continue
        elif "loo_scale_symv_kernel" in name or "loo_u_final_kernel" in name:
            cur["symv"] += us
            cur["stage"] = "symv"
        elif "loo_rank2_kernel" in name:
            cur["rank2"] = us
            cur["stage"] = "reduce"
        elif cur["stage"] == "symv":
            cur["syrk"] += us
        elif cur["stage"] == "reduce":
            cur["reduce"] += us
            if "grad_final_kernel" in name:
                cur = None
    calls = [c for c in calls if c["syrk"] > 0.0]  # (LOO() alone launches the statistics only)
    out = ["rocprofv3 --kernel-trace, a run of its own (tools/loo_probe.py --trace: %d LOOGradient calls per size); us per "
           "launch, per call in launch order:" % TRACE_CALLS,
           "%6s  %8s %12s %12s %8s %10s  %s" % ("N", "stats", "scale+symv", "B B^T", "rank-2", "reduction", "B B^T TFLOP/s")]
    for i, c in enumerate(calls):
        n = sizes[i // TRACE_CALLS] if i // TRACE_CALLS < len(sizes) else 0
        out.append("%6d  %8.2f %12.2f %12.2f %8.2f %10.2f  %.1f" % (n, c["stats"], c["symv"], c["syrk"], c["rank2"],
                                                                  c["reduce"], syrk_flops(n) / c["syrk"] / 1e6 if n else 0.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
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
    say("library: %s" % _lib.lib().gogp_version().decode())
    if not a.trace:
        say("D = %d, Scaled Normal + UniformNoise at synth.theta0; ms per call: median (min .. max) of %d alternating rounds"
            % (D, a.reps))
        say("%6s  %-26s %-26s %-26s %8s %8s  %s" % ("N", "Observe + Gradient", "LOO", "LOOGradient", "LOO/OG", "LG/OG",
                                                    "score, directional derivative: relative error"))
    for n in a.sizes:
        g, x = make_gp(n)

        def og():
            g.Observe(x)
            return g.Gradient()

        og()
        if a.trace:
            for _ in range(TRACE_CALLS):
                g.LOOGradient()
            say("traced N = %d" % n)
            g.close()
            continue
        kinds = (og, g.LOO, g.LOOGradient)
        for fn in kinds:
            fn()
            fn()
        # checks: the score is the sum of the log densities; the gradient matches a central difference along v
        v = np.array([0.6, -0.5, 0.62])
        h = 1e-4
        sp = (g.Observe(x + h * v), g.LOOScore())[1]
        sm = (g.Observe(x - h * v), g.LOOScore())[1]
        og()
        score, grad = g.LOOScore(), g.LOOGradient()
        e1 = abs(score - g.LOO()[2].sum()) / abs(score)
        e2 = abs((sp - sm) / (2 * h) - grad @ v) / abs(grad @ v)
        assert e1 < 1e-10 and e2 < 1e-3, (e1, e2)
        calls = 2 if n >= 16384 else 10
        ts = [[] for _ in kinds]
        for _ in range(a.reps):
            og()  # LOO and LOOGradient are timed on a finished Observe + Gradient
            for t, fn, mult in zip(ts, kinds, (1, 10, 1)):
                t.append(window(fn, calls * mult))

        def fmt(t):
            return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t))
        med = [statistics.median(t) for t in ts]
        say("%6d  %-26s %-26s %-26s %8.4f %8.3f  %.1e, %.1e" % (n, fmt(ts[0]), fmt(ts[1]), fmt(ts[2]), med[1] / med[0],
                                                              med[2] / med[0], e1, e2))
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
