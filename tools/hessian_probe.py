"""hessian.lml_hessian (gogp_lml_hessian): wall time per call beside the 2 P evaluations of Observe + Gradient that
central differences of the gradient take, and the rate of hess_kmm_kernel alone beside the tile kernel's.

    python3 tools/hessian_probe.py [--reps R] [--sizes 1024,4096,16384] [--out profiles/hessian.txt]

Inputs: synth.make_inputs, D = 8, at N in {1024, 4096, 16384}.  P = 3: Scaled(Normal) + UniformNoise (2 slots, one
group); P = 10: Scaled(ARD(Normal, 8)) + UniformNoise (9 slots, three groups, 9 matrices of 8 npad^2 bytes).  Per case one
Observe + Gradient leaves K^-1 on the device; lml_hessian is then timed on that state (it neither changes nor caches
it), and Observe + Gradient beside it on the same build, every call ending in a synchronise.  Two warm-up calls of each,
then R alternating rounds (default 5): medians and the spread.  The Hessian's row of the first parameter is checked
against a central difference of the gradient, so a fast wrong answer does not make the table.

hess_kmm_kernel alone: the call with profiling events around it is not separated here; its share is reported as the
N^3-flop rate 2 S npad^3 / (time of the whole call), a LOWER bound of the kernel's rate (S: slots), beside GEMM_LOWER of
the tile kernel at the same size (gogp_bench_gemm).
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
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian.txt"))
    a = ap.parse_args()
    from gogp_amd import _lib, kernel, synth
    from gogp_amd.gp import GP
    from gogp_amd.hessian import lml_hessian
    lines = ["hessian_probe: %s, D = %d, medians of %d rounds (min .. max), ms" % (_lib.lib().gogp_version().decode(), D, a.reps)]
    for n in [int(s) for s in a.sizes.split(",")]:
        X, y = synth.make_inputs(n, D, 1)
        t0 = synth.theta0(D)
        for P, simil, theta in ((3, kernel.Scaled(kernel.Normal), t0),
                                (10, kernel.Scaled(kernel.ARD(kernel.Normal, D)), [t0[0]] + [t0[1]] * D + [t0[-1]])):
            g = GP(D, simil, kernel.UniformNoise, X=X, Y=y, device=0)
            x = np.log(np.array(theta, float))

            def evalgrad(xx=x):
                g.Observe(xx)
                return g.Gradient()

            for _ in range(2):
                evalgrad()
                H = lml_hessian(g)
            e = np.zeros(P)
            e[0] = 1e-4
            fd = (evalgrad(x + e) - evalgrad(x - e)) / 2e-4
            evalgrad()
            err = np.abs(fd - H[0]).max() / np.abs(H).max()
            assert err < 1e-5, (n, P, err)
            th, te = [], []
            for _ in range(a.reps):
                te.append(timed(evalgrad))
                th.append(timed(lambda: lml_hessian(g)))
            S, npad = P - 1, (n + 255) // 256 * 256
            mh, me = statistics.median(th), statistics.median(te)
            lines.append("N = %5d P = %2d: lml_hessian %9.2f (%.2f .. %.2f)   Observe + Gradient %8.2f (%.2f .. %.2f)   "
                         "2 P of them %9.2f   ratio %.2f   products >= %.1f TFLOP/s   row 0 vs difference %.1e"
                         % (n, P, mh, min(th), max(th), me, min(te), max(te), 2 * P * me, mh / (2 * P * me),
                            2.0 * S * npad ** 3 / (mh * 1e-3) / 1e12, err))
            print(lines[-1], flush=True)
            del g
        tf = ctypes.c_double(0.0)
        ms = ctypes.c_double(0.0)
        try:  # GEMM_LOWER (mode 1) of the tile kernel at the same size, K = npad
            rc = _lib.hooks().gogp_bench_gemm(0, 1, npad // 128, npad // 128, npad, 5, ctypes.byref(ms), ctypes.byref(tf))
            lines.append("N = %5d: tile kernel GEMM_LOWER %.1f TFLOP/s (rc %d)" % (n, tf.value, rc))
            print(lines[-1], flush=True)
        except Exception as ex:  # the figure is a comparison, not a result
            lines.append("N = %5d: tile kernel GEMM_LOWER not measured (%s)" % (n, ex))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
