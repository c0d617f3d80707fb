#!/usr/bin/env python3
"""Writes tests/golden/cg_lml.json: the REFERENCE's own errors of the iterative exact GP's LML and gradient
(tests/cg_lml_ref.py), which tests/test_cg_lml_gpu.py turns into the device's tolerances.  Runs on the CPU (numpy only;
under a minute, most of it the long-double runs), needs no library build:

    python3 tools/make_cg_lml_golden.py

  ortho   the orthogonal-probe cases (cg_lml_ref.ORTHO; t = N + rank_used, Xi = sqrt(t) Q): the float64 reference against
          the dense numpy values (slogdet, solve, 1/2 tr((alpha alpha^T - K^^-1) dK^)): |lml - dense|, |logdet - dense|,
          |grad - dense| per component, and max |W - (alpha alpha^T - K^^-1)| / max |K^^-1|.
  random  the SMALL cases of cg_ref.CASES with t = 16 probes of numpy.random.default_rng(seed): the difference between the
          reference's float64 and long-double runs of quad (largest over the probes), logdet, lml and the gradient
          (per component), both runs' iteration counts, the float64 run's results themselves, and (logdet - exact) / logdet_stderr of the float64 run, which
          this script REFUSES to write unless it is within 3 (the seed is then changed here, by hand)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

import cg_lml_ref as L  # noqa: E402
import cg_ref as C  # noqa: E402

ORTHO_TOL, RANDOM_TOL, RANDOM_RANK, RANDOM_T, PIV_TOL = 1e-10, 1e-8, 64, 16, 1e-8
SEEDS = {name: 0 for name in C.SMALL}


def ortho_entry(key):
    name, N, rank = L.ORTHO[key]
    p = L.small_problem(name, N)
    _, used = C.precond_of(p["K"], p["d"], rank, PIV_TOL)
    Xi = L.orthogonal_xi(N + used, 0)
    e, d = L.estimate(p, rank, ORTHO_TOL, Xi, piv_tol=PIV_TOL), L.dense(p)
    Wd = np.outer(d["alpha"], d["alpha"]) - d["Kinv"]
    return dict(N=N, rank=rank, rank_used=int(used), tol=ORTHO_TOL, cond=p["cond"], lml_err=abs(e["lml"] - d["lml"]),
                logdet_err=abs(e["logdet"] - d["logdet"]), grad_err=np.abs(e["grad"] - d["grad"]).tolist(),
                w_err=float(np.abs(e["W"] - Wd).max() / np.abs(d["Kinv"]).max()), iterations_max=int(e["iterations"].max()))


def random_entry(name):
    p = C.problem(name)
    seed = SEEDS[name]
    Xi = np.random.default_rng(seed).standard_normal((RANDOM_T, p["N"] + RANDOM_RANK))
    f = L.estimate(p, RANDOM_RANK, RANDOM_TOL, Xi, piv_tol=PIV_TOL, mode="f64")
    g = L.estimate(p, RANDOM_RANK, RANDOM_TOL, Xi, piv_tol=PIV_TOL, mode="ld")
    exact = float(np.linalg.slogdet(p["Kh"])[1])
    sig = (f["logdet"] - exact) / f["logdet_stderr"]
    assert abs(sig) <= 3.0, "%s seed %d: the reference is %.2f standard errors off; choose another seed" % (name, seed, sig)
    return dict(seed=seed, rank=RANDOM_RANK, rank_used=int(f["rank_used"]), tol=RANDOM_TOL, t=RANDOM_T,
                quad_diff=float(np.abs(f["quad"] - g["quad"]).max()), logdet_diff=abs(f["logdet"] - g["logdet"]),
                lml_diff=abs(f["lml"] - g["lml"]), grad_diff=np.abs(f["grad"] - g["grad"]).tolist(),
                iterations_f64=[int(v) for v in f["iterations"]], iterations_ld=[int(v) for v in g["iterations"]],
                logdet_exact=exact, ref_sigmas=float(sig), logdet_stderr=f["logdet_stderr"],
                # the float64 run itself: the tests compare the device with these recorded results, so that their verdict
                # does not move with the summation order of the numpy build that happens to run them
                quad=f["quad"].tolist(), logdet=f["logdet"], logdet_precond=f["logdet_precond"], lml=f["lml"],
                grad=f["grad"].tolist())


def main():
    out = dict(piv_tol=PIV_TOL, ortho={}, random={})
    for key in L.ORTHO:
        out["ortho"][key] = ortho_entry(key)
        print("ortho", key, json.dumps(out["ortho"][key]), flush=True)
    for name in C.SMALL:
        out["random"][name] = random_entry(name)
        print("random", name, json.dumps(out["random"][name]), flush=True)
    path = os.path.join(HERE, "..", "tests", "golden", "cg_lml.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
