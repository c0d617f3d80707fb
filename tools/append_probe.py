"""GP.Append (gogp_append) against gogp_set_data + gogp_absorb of the same n + m rows, on one GPU and the same build:
wall time per call, warm, median of 20.  Every Append starts from the same factored N rows (the handle is put back by
Absorb(N rows), which is not timed).  Writes profiles/append.txt.
usage: python3 tools/append_probe.py [N,N,...] [m,m,...] [out]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gogp_amd import _lib, gp as G, kernel, synth
Ns = [int(a) for a in (sys.argv[1] if len(sys.argv) > 1 else "4096,16384").split(",")]
Ms = [int(a) for a in (sys.argv[2] if len(sys.argv) > 2 else "1,16,64").split(",")]
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "append.txt")
D, REPS = 8, 20
lines = ["# %s; D = %d, Scaled(Normal) + UniformNoise at synth.theta0; ms per call, warm, median of %d"
         % (_lib.lib().gogp_version().decode(), D, REPS),
         "#     N    m   append_ms   set_data+absorb_ms   ratio   max|alpha - alpha_absorb| / max|alpha|"]
for N in Ns:
    X, y = synth.make_inputs(N + max(Ms), D, 20251114 + 2)
    th = synth.theta0(D)
    g = G.GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, ThetaSimil=list(th[:2]), ThetaNoise=list(th[2:]))
    for m in Ms:
        ta, tb = [], []
        for rep in range(REPS + 2):  # two warm-up rounds
            g.Absorb(X[:N], y[:N])
            t = time.perf_counter()
            g.Append(X[N:N + m], y[N:N + m])
            ta.append(time.perf_counter() - t)
        alpha_a = g.Alpha
        for rep in range(REPS + 2):
            g.Absorb(X[:N], y[:N])
            t = time.perf_counter()
            g.Absorb(X[:N + m], y[:N + m])  # gogp_set_data + gogp_absorb of the n + m rows
            tb.append(time.perf_counter() - t)
        alpha_b = g.Alpha
        a, b = statistics.median(ta[2:]) * 1e3, statistics.median(tb[2:]) * 1e3
        lines.append("%7d %4d %11.3f %20.3f %7.2f   %.2e" % (N, m, a, b, b / a,
                                                             np.abs(alpha_a - alpha_b).max() / np.abs(alpha_b).max()))
        print(lines[-1], flush=True)
    g.close()
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
