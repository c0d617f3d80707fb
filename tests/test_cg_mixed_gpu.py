"""The iterative exact GP with "cg_precision" = 32 (iterations on the float-evaluated product, restarted on the true fp64
residual; include/gogp_hip.h) on the GPU, against the fp64 path and the dense references of tests/cg_ref.py.

  1  the seven end-to-end cases, rank 0 and 64, tol 1e-8: converged; rel_residual <= tol, also recomputed in long double
     from alpha; |alpha32 - alpha64| <= 2 tol cond |alpha*| (both solves within tol); cg_rounds: >= 1 round, float products,
     no fallback; back at 64 the solve returns the bits it returned before the option was touched;
  2  CGSolveColumns with 3 and 65 columns and CGProduce with sigma against their fp64 results, within the same bound;
  3  inputs with a common offset of 1e7: centring makes the float operator harmless -- converged, no fallback;
  4  256 near-duplicate points under a noise variance of 1e-6, where the float operator is too coarse: the call still
     returns with rel_residual <= tol (the fallback count measured on an MI355X is recorded in tests/golden/cg_mixed.json,
     not asserted);
  5  the option's refusals."""
import numpy as np
import pytest

import cg_ref as C
import gram_ref as R
from gogp_amd import _lib, kernel

pytestmark = pytest.mark.gpu

TOL = 1e-8
COLS_CASE = "matern52_2d"


def _gp(p, noise=C.NOISE, **kw):
    from gogp_amd.gp import GP
    return GP(p["D"], p["simil"], noise, ThetaSimil=list(p["theta"]), device=0, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("rank", [0, 64])
@pytest.mark.parametrize("name", list(C.CASES))
def test_solve(name, rank):
    p = C.problem(name)
    g = _gp(p)
    g.SetCG(p["X"], p["y"], p["v"])
    kw = dict(rank=rank, tol=TOL, max_iter=4000)
    i64 = g.CGSolve(p["x"], **kw)
    a64, r64 = g.CGAlpha(), g.cg_rounds
    assert r64 == dict(rounds=1, products32=0, products64=i64["products"], fallbacks=0)
    g.set_option("cg_precision", 32)
    i32 = g.CGSolve(p["x"], **kw)
    a32, r32 = g.CGAlpha(), g.cg_rounds
    ld, _ = C.true_residual_ld(p, a32)
    err = float(np.linalg.norm(a32 - a64))
    bound = 2 * TOL * p["cond"] * float(np.linalg.norm(p["alpha"]))
    print("%s rank %d: fp64 %d iterations, %d products; mixed %d iterations, %s; rel_residual %.3g (long double %.3g); "
          "|a32 - a64| / bound %.3g" % (name, rank, i64["iterations"], i64["products"], i32["iterations"], r32,
                                        i32["rel_residual"], ld, err / bound))
    assert i32["converged"] and i32["rel_residual"] <= TOL and ld <= TOL
    assert err <= bound
    assert r32["rounds"] >= 1 and r32["products32"] > 0 and r32["fallbacks"] == 0
    assert r32["products32"] + r32["products64"] == i32["products"] and r32["products64"] == r32["rounds"]
    g.set_option("cg_precision", 64)
    j64 = g.CGSolve(p["x"], **kw)
    assert np.array_equal(bits(g.CGAlpha()), bits(a64)) and j64 == i64
    g.close()


def test_columns_and_produce():
    p = C.problem(COLS_CASE)
    g = _gp(p)
    g.SetCG(p["X"], p["y"], p["v"])
    g.CGSolve(p["x"], rank=64, tol=TOL)
    rng = np.random.default_rng([98])
    B = {T: rng.standard_normal((T, p["N"])) for T in (3, 65)}
    Z = rng.uniform(0.0, 4.0, (5, p["D"]))
    S64 = {T: g.CGSolveColumns(B[T], tol=TOL)[0] for T in B}
    mu64, sg64 = g.CGProduce(Z, tol=TOL)
    g.set_option("cg_precision", 32)
    for T in B:
        S32, cols = g.CGSolveColumns(B[T], tol=TOL)
        assert cols["converged"].all() and (cols["rel_residual"] <= TOL).all()
        assert g.cg_rounds["products32"] > 0 and g.cg_info["blocks"] == -(-T // 64)
        assert (np.linalg.norm(S32 - S64[T], axis=1) <= 2 * TOL * p["cond"] * np.linalg.norm(S64[T], axis=1)).all()
        one, _ = g.CGSolveColumns(B[T][T - 1:], tol=TOL)  # alone: the same bits (no fallback happened)
        assert g.cg_rounds["fallbacks"] == 0 and np.array_equal(bits(one[0]), bits(S32[T - 1]))
    mu32, sg32 = g.CGProduce(Z, tol=TOL)
    Ks = R._f64(R.pair_values(p["kp"], Z, p["X"], "f64")[0])
    Sstar = np.linalg.solve(p["Kh"], Ks.T).T
    qb = np.linalg.norm(Ks, axis=1) * 2 * TOL * p["cond"] * np.linalg.norm(Sstar, axis=1)
    assert np.array_equal(bits(mu32), bits(mu64)), "the mean stays on the fp64 product"
    assert (np.abs(sg32 * sg32 - sg64 * sg64) <= qb).all() and g.cg_cols["converged"].all()
    g.close()


def _special(which):
    """(problem-like dict, noise) of the two safeguard cases: D = 1, Scaled Normal, N = 256."""
    rng = np.random.default_rng([99, len(which)])
    N = 256
    if which == "offset":  # a common offset of 1e7, unit spacing, l = 0.5
        X, std = 1e7 + np.arange(N) + rng.uniform(-0.25, 0.25, N), 0.1
    else:                  # 32 sites, eight near-duplicates each
        X, std = np.repeat(rng.uniform(0.0, 10.0, 32), 8) + 1e-7 * rng.standard_normal(N), 1e-3
    theta = [1.5, 0.5]
    kp = C.KP(1, [dict(kind=R.K_NORMAL, c=1.5, inv_len=2.0)], noise_var=std * std)
    Kh = R._f64(R.pair_values(kp, X[:, None], X[:, None], "f64")[0]) + std * std * np.eye(N)
    y = Kh @ rng.standard_normal(N)
    return dict(D=1, N=N, simil=kernel.Scaled(kernel.Normal), theta=theta, x=np.log(theta), X=X[:, None], y=y, Kh=Kh), \
        kernel.ConstantNoise(std)


@pytest.mark.parametrize("which", ["offset", "near_duplicates"])
def test_safeguards(which):
    p, noise = _special(which)
    g = _gp(p, noise)
    g.SetCG(p["X"], p["y"])
    g.set_option("cg_precision", 32)
    info = g.CGSolve(p["x"], rank=64, tol=TOL, max_iter=4000)
    a, r = g.CGAlpha(), g.cg_rounds
    res = float(np.linalg.norm(p["y"] - p["Kh"] @ a) / np.linalg.norm(p["y"]))
    print("%s: %d iterations, %s, rel_residual %.3g (host fp64 %.3g)" % (which, info["iterations"], r, info["rel_residual"], res))
    assert info["converged"] and info["rel_residual"] <= TOL
    if which == "offset":
        assert r["fallbacks"] == 0 and res <= 2 * TOL
    g.close()


def test_option_refusals():
    p = C.problem("normal_1d")
    g = _gp(p)
    L = _lib.lib()
    for val in (0, 16, 33, 128):
        assert L.gogp_set_option(g._h, b"cg_precision", val) == _lib.GOGP_EARG
    assert L.gogp_set_option(g._h, b"cg_precision", 32) == _lib.GOGP_OK
    g.SetCG(p["X"], p["y"])
    g.SetCG(None, None)  # the option survives the release of the data
    g.SetCG(p["X"], p["y"])
    g.CGSolve(p["x"], rank=8, tol=TOL)
    assert g.cg_rounds["products32"] > 0
    g.close()
    g32 = _gp(p, precision=32)
    assert L.gogp_set_option(g32._h, b"cg_precision", 32) == _lib.GOGP_EARG and b"precision = 32" in L.gogp_last_error(g32._h)
    g32.close()
