#!/usr/bin/env python3
"""Writes tests/golden/vecchia.json: per golden case of tests/vecchia_ref.py (GOLDEN) and quantity -- the value, the
gradient, mu and sigma of the test points -- the float64 results of the reference and its float64-minus-long-double
difference (per component for the gradient, the largest for mu and sigma).  The N x 3 terms themselves are NOT recorded:
21600 numbers would make the file half a megabyte.  The file holds their largest magnitude and their largest
float64-minus-long-double difference per column (the tolerance needs nothing else); the tests recompute the float64
terms with the reference (no gradient: a second at the largest case) and the recorded value, their sum, ties them to the
file.  CPU only; the inputs are generated from seeds by vecchia_ref.golden_problem, in the tests as here.  The tool
refuses to write a case on which the reference meets a pivot that is not positive.

    python tools/make_vecchia_golden.py            # rewrites the file
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import vecchia_ref as V  # noqa: E402

F64 = np.float64


def case(name):
    p = V.golden_problem(name)
    out = {}
    runs = {mode: V.observe(p["kp"], p["X"], p["y"], p["v"], p["t"], mode) for mode in ("f64", "ld")}
    prods = {mode: V.produce(p["kp"], p["X"], p["y"], p["v"], p["Z"], p["tz"], mode) for mode in ("f64", "ld")}
    for r in runs.values():
        if r["failed"]:
            raise SystemExit("%s: pivot at targets %r" % (name, r["failed"]))
    for r in prods.values():
        if r[2]:
            raise SystemExit("%s: pivot at test points %r" % (name, r[2]))
    f, l = runs["f64"], runs["ld"]
    diff = lambda a, b: np.abs(np.asarray(a, V.LD) - b).astype(F64)  # noqa: E731
    out["value"] = float(f["value"])
    out["value_diff"] = float(diff(f["value"], l["value"]))
    out["terms_norm"] = [float(x) for x in np.abs(f["terms"]).max(0)]
    out["terms_diff"] = [float(x) for x in diff(f["terms"], l["terms"]).max(0)]
    gf, gl = V.gradient_of(p, f["slots"]), V.gradient_of(p, l["slots"])
    out["grad"] = [float(x) for x in gf]
    out["grad_diff"] = [float(x) for x in diff(gf, gl)]
    if "-N200-" in name:  # the test points are judged on the six cases of N = 200: the file stays small
        for k, q in enumerate(("mu", "sigma")):
            out[q] = [float(x) for x in prods["f64"][k]]
            out[q + "_diff"] = float(diff(prods["f64"][k], prods["ld"][k]).max())
    return out


def main():
    gold = {"noise_std": V.GOLDEN_NOISE_STD, "cases": {}}
    for name in V.GOLDEN:
        gold["cases"][name] = case(name)
        c = gold["cases"][name]
        print("%-22s value %.12g (diff %.2g), grad diff %.2g, terms diff %s" % (name, c["value"], c["value_diff"],
                                                                               max(c["grad_diff"]), c["terms_diff"]))
    path = os.path.join(ROOT, "tests", "golden", "vecchia.json")
    with open(path, "w") as fh:
        json.dump(gold, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
