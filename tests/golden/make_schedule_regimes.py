"""Generate tests/golden/schedule_regimes.json: how far two independent CPU restatements of the same evaluation
disagree at the sizes of tests/test_schedule_regimes_gpu.py, and how close LAPACK's own factor sits to Higham's bound.

The GPU test compares the HIP path with oracle.FastOracle() at ragged N on each side of every size-selected schedule
switch (tests/cases.py: REGIME_SIZES).  Its fp64 tolerances are not chosen there: per case they are 100 x what the two
oracle variants

    FastOracle()                                                LAPACK potrf / potri, the C pair loops
    FastOracle(use_c=False, potrf="blocked", potri="blocked")   dgemm-based blocked factor / inverse, numpy pair loops

differ by -- two summation orders under the same cond x u error law, the GPU being a third -- capped by the suite's
bounds (1e-9 relative on the LML, 1e-7 on the gradient).  The gradient is recorded per component, relative to that
component: a component that partly cancels gets the room the variants themselves need.  rho_ref is the factor residual
ratio (cases.factor_residual_ratio) of the LAPACK factor; the GPU factor is held to min(1, 8 rho_ref).

Like oracle_vectors.json these are NOT outputs of the reference.  CPU only:

    python tests/golden/make_schedule_regimes.py            # every case (minutes)
    python tests/golden/make_schedule_regimes.py 4400       # only the cases of that N, printed, nothing written
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cases import REGIME_CASES, REGIME_FAMILIES, REGIME_M, factor_residual_ratio, regime_inputs  # noqa: E402
from oracle.oracle import FastOracle  # noqa: E402

#: a gradient component below this fraction of the largest is a cancellation: its own value is the wrong scale
MIN_COMPONENT_RATIO = 1e-4


def checksums(family, n):
    X, y, Z, x = regime_inputs(family, n)
    return {"family": family, "n": n, "ndim": X.shape[1], "m": REGIME_M, "log_theta": x.tolist(),
            "x_sum": float(X.sum()), "y_sum": float(y.sum()), "z_sum": float(Z.sum())}


def record(family, n):
    D, simil, noise, _, _, _ = REGIME_FAMILIES[family]
    X, y, Z, x = regime_inputs(family, n)
    a = FastOracle(D, simil, noise)
    b = FastOracle(D, simil, noise, use_c=False, potrf="blocked", potri="blocked")
    a.set_data(X, y)
    b.set_data(X, y)
    lml_a, lml_b = a.Observe(x), b.Observe(x)
    d = np.diag(a.Lc)
    cond_diag = float((d.max() / d.min()) ** 2)
    K = a._gram(a.ts, a.tn)
    rho, at = factor_residual_ratio(np.tril(a.Lc), K)
    del K
    g_a, g_b = a.Gradient(), b.Gradient()
    ratio = float(np.abs(g_a).min() / np.abs(g_a).max())
    assert ratio >= MIN_COMPONENT_RATIO, (family, n, g_a)  # change theta or the seed, not the condition
    v = checksums(family, n)
    v.update({"lml": float(lml_a), "grad": g_a.tolist(),
              "lml_disagreement": float(abs(lml_a - lml_b) / abs(lml_a)),
              "grad_disagreement": (np.abs(g_a - g_b) / np.abs(g_a)).tolist(),
              "min_component_ratio": ratio, "cond_diag": cond_diag, "rho_ref": rho, "rho_ref_at": list(at)})
    return v


def main():
    only = [int(a) for a in sys.argv[1:]]
    out = []
    for family, n in REGIME_CASES:
        if only and n not in only:
            continue
        v = record(family, n)
        out.append(v)
        print("%-12s n=%-6d lml=%.6f dlml=%.1e dgrad=%.1e ratio=%.1e cond=%.0f rho_ref=%.4f" % (
            family, n, v["lml"], v["lml_disagreement"], max(v["grad_disagreement"]), v["min_component_ratio"],
            v["cond_diag"], v["rho_ref"]), flush=True)
    if only:
        return
    doc = {"_comment": "Disagreement of two CPU oracle variants and LAPACK's factor residual ratio per case -- see "
                       "make_schedule_regimes.py (NOT reference outputs).  Inputs: cases.regime_inputs(family, n).",
           "cases": out}
    with open(os.path.join(HERE, "schedule_regimes.json"), "w") as fh:
        json.dump(doc, fh, indent=0)
    print("wrote %d cases" % len(out))


if __name__ == "__main__":
    main()
