"""GP.Remove (gogp_remove) against gogp_set_data + gogp_absorb of the kept rows, on one GPU and the same build: wall time
per call, warm, median of 20.  Every Remove starts from the same factored N rows (the handle is put back by Absorb(N
rows), which is not timed).  Also one sliding step, Remove([0]) + Append(1 row).  Writes profiles/remove.txt.
usage: python3 tools/remove_probe.py [N,N,...] [out]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gogp_amd import _lib, gp as G, kernel, synth
Ns = [int(a) for a in (sys.argv[1] if len(sys.argv) > 1 else "4096,16384").split(",")]
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "remove.txt")
D, REPS = 8, 20
lines = ["# %s; D = %d, Scaled(Normal) + UniformNoise at synth.theta0; ms per call, warm, median of %d"
         % (_lib.lib().gogp_version().decode(), D, REPS),
         "#     N  removed     remove_ms   set_data+absorb_ms   ratio   max|alpha - alpha_absorb| / max|alpha|"]
for N in Ns:
    X, y = synth.make_inputs(N + 1, D, 20251114 + 3)
    th = synth.theta0(D)
    g = G.GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, ThetaSimil=list(th[:2]), ThetaNoise=list(th[2:]))
    cases = [("first1", [0]), ("first16", list(range(16))), ("first64", list(range(64))), ("middle1", [N // 2]),
             ("last1", [N - 1])]
    for name, idx in cases:
        keep = np.ones(N, dtype=bool)
        keep[idx] = False
        Xk, yk = np.ascontiguousarray(X[:N][keep]), np.ascontiguousarray(y[:N][keep])
        ta, tb = [], []
        for rep in range(REPS + 2):  # two warm-up rounds
            g.Absorb(X[:N], y[:N])
            t = time.perf_counter()
            g.Remove(idx)
            ta.append(time.perf_counter() - t)
        alpha_a = g.Alpha
        for rep in range(REPS + 2):
            g.Absorb(X[:N], y[:N])
            t = time.perf_counter()
            g.Absorb(Xk, yk)  # gogp_set_data + gogp_absorb of the kept rows
            tb.append(time.perf_counter() - t)
        alpha_b = g.Alpha
        a, b = statistics.median(ta[2:]) * 1e3, statistics.median(tb[2:]) * 1e3
        lines.append("%7d %8s %13.3f %20.3f %7.2f   %.2e" % (N, name, a, b, b / a,
                                                              np.abs(alpha_a - alpha_b).max() / np.abs(alpha_b).max()))
        print(lines[-1], flush=True)
    # one sliding step on a window of N rows: the oldest row leaves, a new one joins
    g.Absorb(X[:N], y[:N])
    ts = []
    for rep in range(REPS + 2):
        t = time.perf_counter()
        g.Remove([0])
        g.Append(X[N:N + 1], y[N:N + 1])
        ts.append(time.perf_counter() - t)
    lines.append("%7d %8s %13.3f   (Remove([0]) + Append(1 row), the window kept at N)" % (N, "slide", statistics.median(ts[2:]) * 1e3))
    print(lines[-1], flush=True)
    g.close()
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
