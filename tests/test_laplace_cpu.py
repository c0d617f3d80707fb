"""The Laplace approximation without a GPU: the numpy restatement of tests/laplace_ref.py (what gogp_laplace_* evaluate)
pinned against definitions, the host-only gogp_laplace_check, and the binding of the symbols.

Z: against its definition -1/2 f^T K^-1 f + sum log p - 1/2 log det(I + K W) with numpy's solve and slogdet, rtol 1e-9
(n = 40, cond(K) ~ 1e3: both sides carry ~1e-13 relative).

Mode: |a - g(f)|_inf <= 1e-10 max(1, |a|_inf) at the returned iterate, and f = K a.

Gradient: against the central difference D(h) = (Z(x + h e_p) - Z(x - h e_p)) / (2 h) in x = log theta, h = 2.5e-4 (the
period of the periodic term, 0.05, curves Z too much for the 1e-3 of tests/test_loo_cpu.py to keep its teeth), with
the error-bound tolerance of tests/test_loo_cpu.py, taken from the reference itself: the measured truncation
|D(2 h) - D(h)| (three times the truncation error of D(h)) plus the rounding 4 eps cond(K) |Z| / h.  (Z at a mode found
to 1e-10 is off by the square of that: nothing.)  The same gradient with the sign of s as printed in Rasmussen &
Williams (eq. 5.23, Alg. 5.1) must FAIL that check: it is tens of percent off.

Bernoulli mean: the 32-point Gauss-Hermite rule against numpy.polynomial.hermite.hermgauss(200) on mu in [-6, 6],
sigma in [0, 3].  Measured there: 1.81e-5 absolute at the worst (sigma = 3; 1.3e-7 at sigma = 2, 1.1e-13 at sigma = 1);
the bound is four times that, 7.3e-5."""
import ctypes
import os
import re

import numpy as np
import pytest

import laplace_ref as LP
from gogp_amd import _lib, kernel

N = 40
H = 2.5e-4
EPS = np.finfo(float).eps
GH_BOUND = 4 * 1.81e-5

#: name -> (NDim, Simil, theta_simil, events); UniformNoise with std 0.3 throughout (one noise parameter)
CASES = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8], None),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8], None),
    "ard_rbf3": LP.FAMILIES["ard_rbf3"] + (None,),
    "sum_periodic": LP.FAMILIES["hyperpriors"] + (None,),
    "events": LP.FAMILIES["matern52"] + (LP.EVENTS,),
}
LIKS = [LP.BERNOULLI, LP.POISSON]
IDS = ["bernoulli", "poisson"]


def _case(name, lik):
    D, simil, ts, events = CASES[name]
    X, _, _ = LP.inputs(N, 1, D)
    x = np.log(np.array(list(ts) + LP.TN))
    y = LP.draw(lik, LP.gram(D, simil, x, X, events))
    return D, simil, x, X, y, events


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_z_and_mode_against_their_definitions(name, lik):
    D, simil, x, X, y, events = _case(name, lik)
    assert LP.valid(lik, y)
    K = LP.gram(D, simil, x, X, events)
    fit = LP.mode(lik, K, y)
    assert fit.converged and fit.iterations <= 8
    lp, g, W, _ = LP.sites(lik, fit.f, y)
    res = np.abs(fit.a - g).max()
    print("%s %d: %d steps, |a - g| = %.3e, |f - K a| = %.3e" % (name, lik, fit.iterations, res, np.abs(fit.f - K @ fit.a).max()))
    assert res <= 1e-10 * max(1.0, np.abs(fit.a).max())
    np.testing.assert_allclose(fit.f, K @ fit.a, rtol=1e-12, atol=1e-12)
    want = -0.5 * fit.f @ np.linalg.solve(K, fit.f) + lp.sum() - 0.5 * np.linalg.slogdet(np.eye(N) + K * W[None, :])[1]
    print("%s %d: Z = %.12e, definition %.12e" % (name, lik, fit.Z, want))
    np.testing.assert_allclose(fit.Z, want, rtol=1e-9)
    # a warm start from the mode takes no step and returns the same numbers
    again = LP.mode(lik, K, y, a0=fit.a)
    assert again.iterations == 0 and again.converged
    np.testing.assert_allclose(again.Z, fit.Z, rtol=1e-12)


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_against_central_differences_and_the_printed_sign_fails(name, lik):
    D, simil, x, X, y, events = _case(name, lik)
    K, dK = LP.gram(D, simil, x, X, events, want_grad=True)
    fit = LP.mode(lik, K, y)
    grad = LP.gradient(fit, K, dK)
    printed = LP.gradient(fit, K, dK, sign=-1.0)
    assert grad.shape == x.shape

    def z(xx):
        return LP.mode(lik, LP.gram(D, simil, xx, X, events), y).Z

    cond = np.linalg.cond(K)
    printed_fails = False
    for p in range(len(x)):
        e = np.zeros(len(x))
        e[p] = 1.0
        d1 = (z(x + H * e) - z(x - H * e)) / (2 * H)
        d2 = (z(x + 2 * H * e) - z(x - 2 * H * e)) / (4 * H)
        tol = abs(d2 - d1) + 4.0 * EPS * cond * abs(fit.Z) / H
        print("%s %d grad[%d] = %.9e, central difference %.9e, |diff| = %.3e, tolerance %.3e; printed sign: |diff| = %.3e"
              % (name, lik, p, grad[p], d1, abs(grad[p] - d1), tol, abs(printed[p] - d1)))
        assert abs(grad[p] - d1) <= tol, (name, p, grad[p], d1, tol)
        assert tol < 1e-3 * max(1.0, np.abs(grad).max())  # the check has teeth
        printed_fails = printed_fails or abs(printed[p] - d1) > tol
    assert printed_fails, "a reference carrying the printed sign passes: the check cannot tell them apart"


def test_a_strict_increase_of_psi_rejects_converged_steps():
    """Why a step is accepted when psi drops by no more than the rounding of its sums (1e-12 max(1, |psi|)): near the
    mode a Newton step gains ~|a - g|^2, far below the last bits of psi ~ 1e2, so whether psi_t > psi holds there is
    decided by rounding.  Over the cases of this file at the tolerances 1e-10 and 1e-12 the rule with the slack
    converges every time; the strict rule halves a good step twenty times and gives up on some of them (measured: 1 of
    10 at 1e-10, 3 of 10 at 1e-12) although its iterate has the same Z to 1e-9 relative."""
    strict_failures = 0
    for tol in (1e-10, 1e-12):
        for name in sorted(CASES):
            for lik in LIKS:
                D, simil, x, X, y, events = _case(name, lik)
                K = LP.gram(D, simil, x, X, events)
                slack, strict = LP.mode(lik, K, y, tol=tol), LP.mode(lik, K, y, tol=tol, strict=True)
                assert slack.converged, (name, lik, tol)
                np.testing.assert_allclose(strict.Z, slack.Z, rtol=1e-9)
                if not strict.converged:
                    strict_failures += 1
                    print("strict rule gives up: %s %d tol %.0e after %d steps, |a - g| = %.3e"
                          % (name, lik, tol, strict.iterations, np.abs(strict.a - strict.g).max()))
    assert strict_failures >= 1


def test_bernoulli_mean_rule():
    mu, sg = np.meshgrid(np.linspace(-6, 6, 49), np.linspace(0, 3, 25))
    mu, sg = mu.ravel(), sg.ravel()
    a, b = LP.gh_mean(LP.BERNOULLI, mu, sg), LP.gh_mean(LP.BERNOULLI, mu, sg, points=200)
    print("32-point rule against 200 points: max |diff| = %.3e (bound %.3e)" % (np.abs(a - b).max(), GH_BOUND))
    assert np.abs(a - b).max() <= GH_BOUND
    assert np.all((a > 0) & (a < 1))
    np.testing.assert_allclose(LP.gh_mean(LP.BERNOULLI, np.array([0.7]), np.array([0.0])), LP.logistic(np.array([0.7])),
                               rtol=1e-14)
    np.testing.assert_allclose(LP.gh_mean(LP.POISSON, np.array([0.3]), np.array([0.5])), np.exp(0.3 + 0.125), rtol=1e-15)


def test_site_functions_do_not_overflow():
    f = np.array([-700.0, -40.0, 0.0, 40.0, 700.0])
    for lik, y in ((LP.BERNOULLI, np.array([0.0, 1.0, 1.0, 0.0, 1.0])), (LP.POISSON, np.array([0.0, 3.0, 1.0, 7.0, 2.0]))):
        for v in LP.sites(lik, f, y):
            assert np.all(np.isfinite(v))
    lp, g, W, rho = LP.sites(LP.BERNOULLI, f, np.array([0.0, 1.0, 1.0, 0.0, 1.0]))
    assert W[0] > 0 and W[-1] > 0 and W[2] == 0.25 and rho[2] == 0.0
    np.testing.assert_allclose(lp[[0, 4]], [0.0, 0.0], atol=1e-300)
    np.testing.assert_allclose(lp[[1, 3]], [-40.0, -40.0], rtol=1e-15)


def test_laplace_check():
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    good = {LP.BERNOULLI: np.array([0.0, 1.0, 1.0, 0.0]), LP.POISSON: np.array([0.0, 3.0, 41.0, 1.0])}
    bad = {LP.BERNOULLI: [0.5, 2.0, -1.0, np.nan], LP.POISSON: [-1.0, 0.5, np.inf, np.nan]}
    for lik in LIKS:
        assert L.gogp_laplace_check(lik, dp(good[lik]), 4) == _lib.GOGP_OK
        assert LP.valid(lik, good[lik])
        assert L.gogp_laplace_check(lik, None, 0) == _lib.GOGP_OK
        assert L.gogp_laplace_check(lik, None, 3) == _lib.GOGP_EARG
        for v in bad[lik]:
            y = good[lik].copy()
            y[2] = v
            assert L.gogp_laplace_check(lik, dp(y), 4) == _lib.GOGP_EARG, (lik, v)
            assert not LP.valid(lik, y)
    assert L.gogp_laplace_check(2, dp(good[0]), 4) == _lib.GOGP_EARG
    assert L.gogp_laplace_check(-1, dp(good[0]), 4) == _lib.GOGP_EARG


def test_symbols_bound_and_declared():
    """Fails on the parent commit: the five calls are in the binding's table with their argument counts, and
    include/gogp_hip.h declares them, the status code and the likelihood kinds."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    counts = {"gogp_laplace_check": 3, "gogp_laplace_observe": 5, "gogp_laplace_gradient": 3, "gogp_laplace_get_mode": 4,
              "gogp_laplace_produce": 6}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gogp_hip.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name, k in counts.items():
        assert name in table and len(table[name][1]) == k
        m = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == k, name
        assert getattr(L, name)
    assert re.search(r"#define GOGP_ENOCONV 7\b", header) and _lib.GOGP_ENOCONV == 7
    assert re.search(r"GOGP_LIK_BERNOULLI_LOGIT = 0, GOGP_LIK_POISSON_LOG = 1", header)
    assert (_lib.GOGP_LIK_BERNOULLI_LOGIT, _lib.GOGP_LIK_POISSON_LOG) == (LP.BERNOULLI, LP.POISSON)
    hooks = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    assert {"gogp_test_" + k for k in _lib.LAPLACE_HOOKS} <= hooks


def test_model_and_errors_exist():
    from gogp_amd import gp
    assert issubclass(gp.ConvergenceError, gp.GogpError)
    assert gp.ConvergenceError("x").code == _lib.GOGP_ENOCONV
    for name in ("LaplaceObserve", "LaplaceGradient", "LaplaceMode", "LaplaceProduce"):
        assert callable(getattr(gp.GP, name))
    assert gp.LIKELIHOODS == {"bernoulli": LP.BERNOULLI, "poisson": LP.POISSON}
    assert callable(gp.LaplaceModel)
