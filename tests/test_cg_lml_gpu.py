"""The iterative exact GP's LML and gradient on the GPU (GP.CGObserve / CGGradient / CGModel; gogp_cg_lml_gradient), through
the C ABI, against tests/cg_lml_ref.py and dense numpy linear algebra.  Every figure is printed before it is asserted (-s).

  1  ORTHOGONAL PROBES make the estimator exact (t = N + rank_used, Xi = sqrt(t) Q, tol = 1e-10; cg_lml_ref.ORTHO: Normal
     1-d N = 96 rank 8 -- two blocks, the second ragged --, Matern-3/2 N = 96 rank 0, ARD 8-d N = 120 rank 16, periodic +
     Matern N = 100): lml, logdet and the gradient against slogdet, solve and the explicit 1/2 tr((alpha alpha^T - K^^-1)
     dK^).  Tolerance: the REFERENCE's own error on the same inputs (tests/golden/cg_lml.json, written by
     tools/make_cg_lml_golden.py on the CPU) times 8 -- the device adds in another order --, the gradient with the floor
     (cond tol + cond N u) max |grad| that cg_ref.alpha_bound forms for alpha.  A noise kernel WITH a parameter (the trace
     slot) goes against the same library's dense Observe + Gradient, both within that floor of the exact values.
  2  RANDOM PROBES, t = 16, rank 64, tol = 1e-8, on the SMALL cases of cg_ref.CASES with the seeds of the golden file
     (chosen so that the reference alone is within 3 standard errors of the exact log-determinant; the tool refuses
     to write otherwise): quad, logdet, lml and every gradient component against the reference running the same
     algorithm on the same Xi in float64 (its results are recorded in the golden file, so that the verdict does not move
     with the summation order of the numpy build that runs the test), margin 8 x |float64 run - long-double run| of
     that case from the same file, one margin per quantity and case (the largest over the probes for quad, over the
     components for the gradient); |logdet - exact| <= 4 logdet_stderr.  Iteration counts: test_cg_gpu.py holds the
     device's counts to the reference's by inequalities only; here they lie within max(1, ceil(count / 16)) of the
     reference's.  The reference's own two runs differ by 1 at 50 .. 90 iterations: behind a few dozen iterations the
     recurrences of two roundings are different trajectories of the same rate, and |r| <= tol |b| is crossed where a
     plateau of the residual ends.
  3  identical calls, identical bits; a probe alone has the quad bits it has inside a block of 64; t = 1, 64, 65;
     grad = NULL leaves lml and quad unchanged; CGAlpha / CGProduce / gogp_cg_last_info before and after return the same
     bits; CGSolve and CGSolveColumns still meet cg_ref's conditions; every error code; GOGP_ENOCONV at max_iter = 3
     writes finite outputs; CGModel.
Every device result is computed once per case and shared, read only."""
import ctypes
import json
import os

import numpy as np
import pytest

import cg_lml_ref as L
import cg_ref as C
from gogp_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "cg_lml.json")) as _f:
    GOLD = json.load(_f)
PIV = GOLD["piv_tol"]
KEPT = "periodic_matern_1d"  # N = 500: the case the bit, size and state checks run on


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _gp(p):
    from gogp_amd.gp import GP
    g = GP(p["D"], p["simil"], C.NOISE, ThetaSimil=list(p["theta"]), device=0)
    g.SetCG(p["X"], p["y"], p["v"])
    return g


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(L.ORTHO))
def test_orthogonal_probes_are_exact(key):
    name, N, rank = L.ORTHO[key]
    gold = GOLD["ortho"][key]
    p = L.small_problem(name, N)
    t = N + gold["rank_used"]
    Xi = L.orthogonal_xi(t, 0)
    g = _gp(p)
    lml = g.CGObserve(p["x"], probes=t, rank=rank, tol=gold["tol"], max_iter=1000, piv_tol=PIV,
                      xi=np.hstack([Xi, np.zeros((t, rank - gold["rank_used"]))]))
    info, grad = g.cg_lml_info, g.CGGradient()
    used = g.cg_info["rank_used"]
    g.close()
    d = L.dense(p)
    floor = (gold["cond"] * gold["tol"] + gold["cond"] * N * C.U) * float(np.abs(d["grad"]).max())
    gerr = np.abs(grad - d["grad"])
    print("%s: t %d, blocks %d, lanczos_max %d; |lml - dense| %.3g (reference %.3g), |logdet - dense| %.3g (reference %.3g), "
          "gradient errors %s (reference %s, floor %.3g)" % (key, t, info["blocks"], info["lanczos_max"], abs(lml - d["lml"]),
                                                             gold["lml_err"], abs(info["logdet"] - d["logdet"]),
                                                             gold["logdet_err"], gerr, gold["grad_err"], floor))
    assert used == gold["rank_used"] and info["probes"] == t and info["blocks"] == -(-t // 64)
    assert info["converged"].all() and info["lml"] == lml
    assert abs(info["logdet"] - d["logdet"]) <= 8 * gold["logdet_err"]
    assert abs(lml - d["lml"]) <= 8 * gold["lml_err"]
    assert (gerr <= 8 * np.array(gold["grad_err"]) + floor).all()


def test_noise_parameter_against_the_dense_handle():
    """A noise kernel with a parameter (UniformNoise; no per-observation variances): the trace slot goes through the
    finishing code of the dense path, d noise_var / d log(std) = 2 noise_var.  Orthogonal probes at tol = 1e-10 against
    the SAME library's dense Observe + Gradient on the same data: both lie within (cond tol + cond N u) max |grad| of the
    exact gradient, as cg_ref.alpha_bound forms it, so within twice that of each other; the LML likewise with |LML|."""
    from gogp_amd import kernel as GK
    from gogp_amd.gp import GP
    p = L.small_problem("matern52_2d", 96)
    theta, std = [1.5, 0.7], 0.25
    x = np.log(np.array(theta + [std]))
    Kh = p["K"] + std * std * np.eye(96)
    cond = float(np.linalg.cond(Kh))
    g = GP(2, p["simil"], GK.UniformNoise, device=0)
    g.SetCG(p["X"], p["y"])
    t, tol = 96 + 8, 1e-10
    lml = g.CGObserve(x, probes=t, rank=8, tol=tol, piv_tol=PIV, xi=L.orthogonal_xi(t, 1))
    grad, used = g.CGGradient(), g.cg_info["rank_used"]
    g.close()
    d = GP(2, p["simil"], GK.UniformNoise, ThetaSimil=theta, ThetaNoise=[std], device=0)
    d.Absorb(p["X"], p["y"])
    dl, dg = d.Observe(x), d.Gradient()
    d.close()
    floor = cond * tol + cond * 96 * C.U
    print("noise parameter: cond %.3g; |lml - dense| %.3g, gradient %s, dense %s, difference %s, floor %.3g x %.3g"
          % (cond, abs(lml - dl), grad, dg, np.abs(grad - dg), floor, np.abs(dg).max()))
    assert used == 8 and len(grad) == 3
    assert abs(lml - dl) <= 2 * floor * abs(dl)
    assert (np.abs(grad - dg) <= 2 * floor * np.abs(dg).max()).all()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
_RUN = {}


def _observed(name):
    """(info, gradient, alpha, solve info) of CGObserve with the golden file's seed: one per case, shared, read only."""
    if name not in _RUN:
        gold = GOLD["random"][name]
        p = C.problem(name)
        g = _gp(p)
        lml = g.CGObserve(p["x"], probes=gold["t"], seed=gold["seed"], rank=gold["rank"], tol=gold["tol"], piv_tol=PIV)
        info = dict(g.cg_lml_info, solve=dict(g.cg_info))
        assert info["lml"] == lml
        _RUN[name] = (g if name == KEPT else None, info, g.CGGradient(), g.CGAlpha())
        if name != KEPT:
            g.close()
    return _RUN[name]


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_handles():
    yield
    for g, _, _, _ in _RUN.values():
        if g is not None:
            g.close()
    _RUN.clear()


@pytest.mark.parametrize("name", C.SMALL)
def test_random_probes_against_the_reference(name):
    gold = GOLD["random"][name]
    p = C.problem(name)
    _, info, grad, _ = _observed(name)
    ref = dict(quad=np.array(gold["quad"]), grad=np.array(gold["grad"]), logdet=gold["logdet"], lml=gold["lml"],
               logdet_precond=gold["logdet_precond"], iterations=np.array(gold["iterations_f64"]), rank_used=gold["rank_used"])
    dq = float(np.abs(info["quad"] - ref["quad"]).max())
    dg = np.abs(grad - ref["grad"])
    sig = (info["logdet"] - gold["logdet_exact"]) / info["logdet_stderr"]
    print("%s: rank %d; |quad - ref| %.3g (f64 - ld %.3g), |logdet - ref| %.3g (%.3g), |lml - ref| %.3g (%.3g), gradient %s (%s); "
          "iterations %s, reference %s; logdet %.6f +- %.3g, exact %.6f: %.2f standard errors"
          % (name, info["solve"]["rank_used"], dq, gold["quad_diff"], abs(info["logdet"] - ref["logdet"]), gold["logdet_diff"],
             abs(info["lml"] - ref["lml"]), gold["lml_diff"], dg, gold["grad_diff"], info["iterations"].tolist(),
             ref["iterations"].tolist(), info["logdet"], info["logdet_stderr"], gold["logdet_exact"], sig))
    assert info["solve"]["rank_used"] == ref["rank_used"] == gold["rank_used"]
    assert info["converged"].all() and info["probes"] == gold["t"] and info["blocks"] == 1
    assert (np.abs(info["iterations"] - ref["iterations"]) <= np.maximum(1, -(-ref["iterations"] // 16))).all()
    assert info["lanczos_max"] == info["iterations"].max()
    assert abs(info["logdet_precond"] - ref["logdet_precond"]) <= 1e-12 * abs(ref["logdet_precond"])
    assert abs(sig) <= 4.0
    assert dq <= 8 * gold["quad_diff"]
    assert abs(info["logdet"] - ref["logdet"]) <= 8 * gold["logdet_diff"]
    assert abs(info["lml"] - ref["lml"]) <= 8 * gold["lml_diff"]
    assert (dg <= 8 * max(gold["grad_diff"])).all()
    q = info["quad"]
    assert info["logdet_stderr"] == pytest.approx(q.std(ddof=1) / np.sqrt(len(q)), rel=1e-12)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _call(g, Xi, tol=1e-8, max_iter=1000, want_grad=True, want_quad=True, want_cols=True, ldxi=None, t=None, plen=None):
    """gogp_cg_lml_gradient itself: (rc, info struct, grad, quad, cols)."""
    Xi = np.ascontiguousarray(Xi, dtype=np.float64)
    t = len(Xi) if t is None else t
    p = g._ns + g._nn
    grad, quad = np.full(max(p, 1), np.nan), np.full(max(t, 1), np.nan)
    info, cols = _lib.CCgLmlInfo(), (_lib.CCgCol * max(t, 1))()
    dp = lambda a: a.ctypes.data_as(_lib._dp)  # noqa: E731
    rc = _lib.lib().gogp_cg_lml_gradient(g._h, dp(Xi), t, Xi.shape[1] if ldxi is None else ldxi, tol, max_iter,
                                         dp(grad) if want_grad else None, p if plen is None else plen,
                                         dp(quad) if want_quad else None, ctypes.byref(info), cols if want_cols else None)
    return rc, info, grad[:p], quad[:t], cols


def _kept():
    g, info, grad, alpha = _observed(KEPT)
    p = C.problem(KEPT)
    gold = GOLD["random"][KEPT]
    Xi = np.random.default_rng(gold["seed"]).standard_normal((gold["t"], p["N"] + gold["rank"]))
    return g, p, info, grad, alpha, Xi


def test_same_bits_and_state_left_as_found():
    g, p, info, grad, alpha, Xi = _kept()
    z = np.linspace(0.0, 10.0, 7)[:, None]
    mu0, sg0 = g.CGProduce(z)
    last0 = g._cg_info()
    rc, i1, g1, q1, c1 = _call(g, Xi)
    assert rc == _lib.GOGP_OK
    assert np.array_equal(bits(q1), bits(info["quad"])) and np.array_equal(bits(g1), bits(grad))
    assert i1.lml == info["lml"] and i1.logdet == info["logdet"] and i1.logdet_stderr == info["logdet_stderr"]
    assert i1.logdet_precond == info["logdet_precond"] and i1.yt_alpha == info["yt_alpha"] == info["solve"]["yt_alpha"]
    assert [c1[s].iterations for s in range(len(Xi))] == info["iterations"].tolist()
    assert g._cg_info() == last0, "gogp_cg_last_info keeps the figures of the call before"
    assert np.array_equal(bits(g.CGAlpha()), bits(alpha))
    mu1, sg1 = g.CGProduce(z)
    assert np.array_equal(bits(mu1), bits(mu0)) and np.array_equal(bits(sg1), bits(sg0))
    # grad = NULL, quad = NULL, cols = NULL: the other outputs keep their bits
    rc, i2, g2, q2, _ = _call(g, Xi, want_grad=False)
    assert rc == _lib.GOGP_OK and i2.lml == i1.lml and np.array_equal(bits(q2), bits(q1)) and np.isnan(g2).all()
    rc, i3, g3, q3, _ = _call(g, Xi, want_quad=False, want_cols=False)
    assert rc == _lib.GOGP_OK and i3.lml == i1.lml and np.array_equal(bits(g3), bits(g1)) and np.isnan(q3).all()
    # a padded leading dimension reads the same numbers
    wide = np.hstack([Xi, np.full((len(Xi), 5), np.nan)])
    rc, i4, g4, q4, _ = _call(g, wide)
    assert rc == _lib.GOGP_OK and np.array_equal(bits(q4), bits(q1)) and np.array_equal(bits(g4), bits(g1))


def test_a_probe_alone_and_the_block_sizes():
    g, p, info, _, _, _ = _kept()
    rng = np.random.default_rng(77)
    Xi = rng.standard_normal((65, p["N"] + 64))
    rc, i65, g65, q65, c65 = _call(g, Xi)
    assert rc == _lib.GOGP_OK and i65.blocks == 2 and i65.probes == 65 and np.isfinite(q65).all()
    rc, i64, g64, q64, _ = _call(g, Xi[:64])
    assert rc == _lib.GOGP_OK and i64.blocks == 1 and np.array_equal(bits(q64), bits(q65[:64]))
    for s in (0, 17, 64):
        rc, i1, g1, q1, c1 = _call(g, Xi[s:s + 1])
        assert rc == _lib.GOGP_OK and i1.blocks == 1 and i1.logdet_stderr == 0.0
        assert np.array_equal(bits(q1), bits(q65[s:s + 1])), "probe %d alone" % s
        assert c1[0].iterations == c65[s].iterations and i1.logdet == i1.logdet_precond + q1[0]
    # the estimate of 65 probes is the mean of their values, and lies with the 16-probe one inside the standard errors
    assert i65.logdet == pytest.approx(i65.logdet_precond + q65.mean(), rel=1e-14)
    assert abs(i65.logdet - info["logdet"]) <= 4 * np.hypot(i65.logdet_stderr, info["logdet_stderr"])
    assert np.isfinite(g65).all() and np.isfinite(g64).all()


def test_solve_and_columns_still_meet_cg_refs_conditions():
    g, p, info, _, alpha, _ = _kept()
    s = info["solve"]
    assert s["converged"] and np.linalg.norm(alpha - p["alpha"]) <= C.alpha_bound(p, s["rel_residual"])
    B = np.random.default_rng(5).standard_normal((3, p["N"]))
    S, cols = g.CGSolveColumns(B, tol=1e-8)
    want = np.linalg.solve(p["Kh"], B.T).T
    for t in range(3):
        assert np.linalg.norm(S[t] - want[t]) <= (p["cond"] * cols["rel_residual"][t] + p["cond"] * p["N"] * C.U) * np.linalg.norm(want[t])
    S1, _ = g.CGSolveColumns(B[1:2], tol=1e-8)
    assert np.array_equal(bits(S1[0]), bits(S[1]))


def test_error_codes():
    from gogp_amd.gp import GP
    g, p, _, _, _, Xi = _kept()
    EARG, ESTATE = _lib.GOGP_EARG, _lib.GOGP_ESTATE
    one = Xi[:1]
    assert _call(g, one, t=0)[0] == EARG
    assert _call(g, one, ldxi=p["N"] + 63)[0] == EARG
    assert _call(g, one, plen=1)[0] == EARG
    assert _call(g, one, tol=0.0)[0] == EARG and _call(g, one, tol=float("nan"))[0] == EARG
    assert _call(g, one, max_iter=0)[0] == EARG
    bad = one.copy()
    bad[0, p["N"] + 63] = np.inf
    assert _call(g, bad)[0] == EARG
    bad = np.hstack([one, [[np.nan]]])  # behind N + rank_used: not read
    assert _call(g, bad)[0] == _lib.GOGP_OK
    dp = one.ctypes.data_as(_lib._dp)
    info = _lib.CCgLmlInfo()
    assert _lib.lib().gogp_cg_lml_gradient(g._h, None, 1, one.shape[1], 1e-8, 10, None, 0, None, ctypes.byref(info), None) == EARG
    assert _lib.lib().gogp_cg_lml_gradient(g._h, dp, 1, one.shape[1], 1e-8, 10, None, 0, None, None, None) == EARG
    # before a solve, and without data
    h = GP(p["D"], p["simil"], C.NOISE, ThetaSimil=list(p["theta"]), device=0)
    assert _call(h, one)[0] == ESTATE
    h.SetCG(p["X"], p["y"], p["v"])
    assert _call(h, one)[0] == ESTATE
    with pytest.raises(Exception):
        h.CGGradient()
    h.close()
    # the kinds of handle the family refuses
    f = GP(p["D"], p["simil"], C.NOISE, ThetaSimil=list(p["theta"]), device=0, precision=32)
    assert _call(f, one)[0] == EARG
    f.close()


def test_not_converged_writes_every_output():
    p = C.problem("matern52_2d")
    g = _gp(p)
    g.CGSolve(p["x"], rank=64, tol=1e-8, piv_tol=PIV)
    Xi = np.random.default_rng(9).standard_normal((3, p["N"] + 64))
    Xi[1] = 0.0  # a zero probe: frozen from the start, quad 0
    rc, info, grad, quad, cols = _call(g, Xi, max_iter=3)
    assert rc == _lib.GOGP_ENOCONV and b"did not reach" in _lib.lib().gogp_last_error(g._h)
    assert np.isfinite(grad).all() and np.isfinite(quad).all() and np.isfinite([info.lml, info.logdet, info.logdet_stderr]).all()
    assert [cols[s].iterations for s in range(3)] == [3, 0, 3] and [cols[s].converged for s in range(3)] == [0, 1, 0]
    assert quad[1] == 0.0 and info.lanczos_max == 3
    from gogp_amd.gp import ConvergenceError
    with pytest.raises(ConvergenceError) as e:
        g.CGObserve(p["x"], probes=4, rank=64, tol=1e-8, max_iter=3, piv_tol=PIV)
    assert np.isfinite(e.value.result) and np.isfinite(g.CGGradient()).all()
    # not positive definite: a negative output scale is refused by the solve; the probes' own refusal names the column
    g.close()


def test_cg_model_and_adam():
    from gogp_amd import CGModel, optimize
    p = L.small_problem("matern52_2d", 300)
    g = _gp(p)
    m = CGModel(g, probes=16, seed=3, rank=32, tol=1e-8)
    f, gr = optimize.func_grad(m)
    v = g.CGObserve(p["x"], probes=16, seed=3, rank=32, tol=1e-8)
    dg = g.CGGradient()
    assert f(p["x"]) == -v and np.array_equal(bits(gr(p["x"])), bits(-dg))
    assert m.Observe(p["x"]) == v and np.array_equal(bits(m.Gradient()), bits(dg))
    with pytest.raises(ValueError):
        m.Observe(np.zeros(len(p["x"]) + 1))
    d = L.dense(p)
    print("CGModel at the true theta: estimate %.6f +- %.3g, dense %.6f; gradient %s, dense %s"
          % (v, 0.5 * g.cg_lml_info["logdet_stderr"], d["lml"], dg, d["grad"]))
    assert abs(v - d["lml"]) <= 4 * 0.5 * g.cg_lml_info["logdet_stderr"] + 1e-6 * abs(d["lml"])
    x = p["x"] + np.array([0.6, -0.5])
    first = m.Observe(x)
    adam = optimize.Adam(Rate=0.05)
    for _ in range(10):
        adam.Step(m, x)
    last = m.Observe(x)
    print("ten Adam steps from a perturbed theta: %.4f -> %.4f" % (first, last))
    assert last >= first
    g.close()
