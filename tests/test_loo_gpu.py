"""GP.LOO / GP.LOOGradient (gogp_loo, gogp_loo_gradient) on the GPU against the dense closed form of tests/loo_ref.py
(np.linalg.inv in fp64; tests/test_loo_cpu.py pins that closed form to n refits and to central differences).

Tolerances (the header of tests/test_gpu_parity.py): mu, sigma, log p and their sum rtol = 1e-6, atol = 1e-8; every
component of the gradient within 1e-6 of the largest absolute component (the suite's rule for gradients).  The inputs
keep the reference far inside that: prior variances 0.9 - 2.3 and noise variance 0.09 with n <= 1100 give
cond(K) <~ (1100 * 2.3 + 0.09) / 0.09 ~ 3e4, so np.linalg.inv and the solve carry ~3e4 * 2.2e-16 ~ 1e-11 relative; the
entries of K^-1 are at most 1 / 0.09, kappa_i >= 1 / 2.4, and the sums of the gradient run over n^2 <= 1.2e6 terms of
mixed sign whose rounding (~1e-13 relative each) stays six orders below the bound.  The optimiser's end point has a
smaller noise (std ~0.1 at n = 200: cond(K) <~ 200 * 1.5 / 0.01 = 3e4), the same regime.

Shapes (TILE = 128, PANEL = 256; the LOO passes and the reduction work on 64 x 64 tiles): n = 1 one observation; 20 the
one-launch `tiny` path; 128 its limit; 129 the first size on the general sweep, two 128-tiles in one padded panel; 300
two panels, ragged; 1100 npad = 1280: off-diagonal tile pairs in the product B B^T, several 64-tiles per workgroup in
the reduction.  Each after Absorb and after Observe.

Reference counterpart: none (the reference's forecast harness refits per prefix)."""
import ctypes

import numpy as np
import pytest

import loo_ref as LR
from gogp_amd import _lib, kernel, optimize, synth

pytestmark = pytest.mark.gpu

SHAPE_FAMILY = "ard_rbf3"
SHAPES = (1, 20, 128, 129, 300, 1100)
#: name -> (NDim, Simil, theta_simil): the four radial kinds next to the shared families
RADIAL = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8]),
    "matern52": (2, kernel.Scaled(kernel.Matern52), [1.2, 0.9]),
    "matern52textbook": (2, kernel.Scaled(kernel.Matern52Textbook), [0.9, 1.1]),
}
FAMILIES = dict(LR.FAMILIES, **RADIAL)
_REF = {}


def _x(fam):
    return np.log(np.array(list(FAMILIES[fam][2]) + LR.TN))


def _ref(fam, n, events=None):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, n, bool(events))
    if key not in _REF:
        D, simil, _ = FAMILIES[fam]
        X, y, _ = LR.inputs(n, 1, D)
        _REF[key] = (X, y) + LR.reference(D, simil, _x(fam), X, y, events)
    return _REF[key]


def _gp(fam, simil=None, **kw):
    from gogp_amd.gp import GP
    D, s, ts = FAMILIES[fam]
    return GP(D, simil or s, LR.NOISE, ThetaSimil=ts, ThetaNoise=LR.TN, device=0, **kw)


def _fit(g, fam, X, y, state):
    if state == "absorb":
        g.Absorb(X, y)
    else:
        g.X, g.Y = X, y
        g.Observe(_x(fam))


def _check(g, want, tag, gradient=True):
    """LOO values, score and gradient against the reference, every figure printed first; a second call: the same bits"""
    mu_o, sigma_o, logp_o, grad_o = want
    mu, sigma, logp = g.LOO()
    score = g.LOOScore()
    grad = g.LOOGradient() if gradient else None
    crit = lambda a, b: (np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))).max() if len(b) else 0.0  # noqa: E731
    print("%s: mu %.3e sigma %.3e logp %.3e of the rtol 1e-6 + atol 1e-8 criterion; score %.12e (reference %.12e)"
          % (tag, crit(mu, mu_o), crit(sigma, sigma_o), crit(logp, logp_o), score, logp_o.sum()))
    if gradient:
        scale = np.abs(grad_o).max()
        print("%s: gradient max |err| = %.3e of largest component %.3e (%.2e relative)"
              % (tag, np.abs(grad - grad_o).max(), scale, np.abs(grad - grad_o).max() / scale))
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(sigma, sigma_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(logp, logp_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(score, logp_o.sum(), rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(score, logp.sum(), rtol=1e-12, atol=1e-12)  # the device's sum of the same numbers
    for a, b in zip(g.LOO(), (mu, sigma, logp)):
        np.testing.assert_array_equal(a, b)
    assert g.LOOScore() == score
    if gradient:
        assert grad.shape == grad_o.shape
        assert np.abs(grad - grad_o).max() <= 1e-6 * scale, (tag, grad, grad_o)
        np.testing.assert_array_equal(g.LOOGradient(), grad)
    return grad


@pytest.mark.parametrize("state", ["absorb", "observe"])
@pytest.mark.parametrize("n", SHAPES)
def test_shapes(n, state):
    X, y, *want = _ref(SHAPE_FAMILY, n)
    g = _gp(SHAPE_FAMILY)
    _fit(g, SHAPE_FAMILY, X, y, state)
    _check(g, want, (n, state))
    g.close()


@pytest.mark.parametrize("fam", sorted(RADIAL) + ["ard_rbf3", "ard_rbf64", "hyperpriors"])
def test_kernel_families(fam):
    X, y, *want = _ref(fam, 300)
    g = _gp(fam)
    _fit(g, fam, X, y, "observe")
    _check(g, want, fam)
    g.close()


def test_events():
    fam = "matern52"
    D, simil, ts = FAMILIES[fam]
    X, y, *want = _ref(fam, 300, LR.EVENTS)
    plain = _ref(fam, 300)
    assert np.abs(want[2] - plain[4]).max() > 1e-3  # the discounts change log p ...
    assert np.abs(want[3] - plain[5]).max() > 1e-3 * np.abs(plain[5]).max()  # ... and the gradient
    g = _gp(fam, simil=kernel.Events(simil, LR.EVENTS, 0))
    _fit(g, fam, X, y, "observe")
    _check(g, want, "events")
    g.close()


@pytest.mark.parametrize("option,value,n", [("eager", 0, 300), ("kinv_fused", 0, 300), ("kinv_fused", 1, 300),
                                            ("tiny", 0, 100)])
def test_options(option, value, n):
    X, y, *want = _ref(SHAPE_FAMILY, n)
    g = _gp(SHAPE_FAMILY)
    g.set_option(option, value)
    _fit(g, SHAPE_FAMILY, X, y, "observe")
    _check(g, want, (option, value, n))
    g.close()


@pytest.mark.parametrize("n", [100, 300])
def test_state_is_preserved(n):
    """Gradient, Produce, the factor and a later Append return the bits they return without the LOO calls between"""
    fam = SHAPE_FAMILY
    D = FAMILIES[fam][0]
    X, y, *_ = _ref(fam, n)
    Z = LR.inputs(1, 33, D)[2]
    X2, y2, _ = LR.inputs(5, 1, D, seed=11)

    def run(loo):
        g = _gp(fam)
        _fit(g, fam, X, y, "observe")
        if loo == "first":  # the LOO calls form K^-1, the gradient finds it
            g.LOOGradient()
            g.LOO()
        first = (g.Gradient(), *g.Produce(Z))
        if loo == "between":
            g.LOO()
            g.LOOGradient()
        out = first + (g.Gradient(), *g.Produce(Z), g.L)
        if loo:
            g.LOOGradient()
        g.Append(X2, y2)
        out += (g.L, g.Alpha, *g.Produce(Z))
        g.close()
        return out

    a = run(None)
    for b in (run("between"), run("first")):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
        for k in range(3):  # before and after, on the same handle
            np.testing.assert_array_equal(b[k], b[3 + k])


def test_after_absorb_gradient_is_still_refused():
    from gogp_amd.gp import GogpError
    X, y, *want = _ref(SHAPE_FAMILY, 300)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    _check(g, want, "absorb, then Gradient")
    with pytest.raises(GogpError) as e:  # no gradient after Absorb (gp/gp.go:85-86): the LOO calls do not change that
        g.Gradient()
    assert e.value.code == _lib.GOGP_ESTATE
    g.close()


def test_after_append_remove_and_restore():
    fam = SHAPE_FAMILY
    D, simil, _ = FAMILIES[fam]
    X, y, *want = _ref(fam, 300)
    X2, y2, _ = LR.inputs(5, 1, D, seed=11)
    g = _gp(fam)
    _fit(g, fam, X, y, "observe")
    g.LOOGradient()  # the workspaces exist before the data grow
    g.Append(X2, y2)
    Xa, ya = np.concatenate([X, X2]), np.concatenate([y, y2])
    _check(g, LR.reference(D, simil, _x(fam), Xa, ya), "append 5")
    g.Remove([0, 7])
    keep = np.ones(len(ya), dtype=bool)
    keep[[0, 7]] = False
    _check(g, LR.reference(D, simil, _x(fam), Xa[keep], ya[keep]), "remove [0, 7]")
    L, alpha = g.L, g.Alpha
    r = _gp(fam)  # set_factor on a fresh handle
    r.X, r.Y = Xa[keep], ya[keep]
    r.restore(L, alpha)
    _check(r, LR.reference(D, simil, _x(fam), Xa[keep], ya[keep]), "restore")
    r.close()
    # ... and on a handle whose last sweep left a partial K^-1 behind
    _fit(g, fam, X, y, "observe")
    g.restore(np.linalg.cholesky(LR.gram(D, simil, _x(fam), X)), np.linalg.solve(LR.gram(D, simil, _x(fam), X), y))
    _check(g, want, "restore over an Observe")
    g.close()


def test_contract():
    from gogp_amd.gp import GP, GogpError
    fam = SHAPE_FAMILY
    D, simil, ts = FAMILIES[fam]
    X, y, *want = _ref(fam, 300)
    P = len(ts) + 1
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    g = _gp(fam)
    g.X, g.Y = X, y
    g._push_data()
    grad, total = np.zeros(P), ctypes.c_double(-1.0)
    assert L.gogp_loo(g._h, None, None, None, ctypes.byref(total)) == _lib.GOGP_ESTATE  # nothing factored yet
    assert L.gogp_loo_gradient(g._h, dp(grad), P) == _lib.GOGP_ESTATE
    g.Absorb(X, y)
    assert L.gogp_loo_gradient(g._h, dp(grad), P + 1) == _lib.GOGP_EARG
    assert L.gogp_loo_gradient(g._h, dp(grad), P - 1) == _lib.GOGP_EARG
    # NULL arrays: any subset
    logp = np.zeros(300)
    assert L.gogp_loo(g._h, None, None, None, None) == _lib.GOGP_OK
    assert L.gogp_loo(g._h, None, None, dp(logp), ctypes.byref(total)) == _lib.GOGP_OK
    np.testing.assert_allclose(logp, want[2], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(total.value, want[2].sum(), rtol=1e-6, atol=1e-8)
    sigma = np.zeros(300)
    assert L.gogp_loo(g._h, None, dp(sigma), None, None) == _lib.GOGP_OK
    np.testing.assert_allclose(sigma, want[1], rtol=1e-6, atol=1e-8)
    # gradient_precision = 32: K^-1 is float
    g.set_option("gradient_precision", 32)
    g.Observe(_x(fam))
    for call in (g.LOO, g.LOOGradient):
        with pytest.raises(GogpError) as e:
            call()
        assert e.value.code == _lib.GOGP_EARG
    g.close()
    g32 = GP(D, simil, LR.NOISE, ThetaSimil=ts, ThetaNoise=LR.TN, device=0, precision=32)
    g32.Absorb(X, y)
    for call in (g32.LOO, g32.LOOGradient):
        with pytest.raises(GogpError) as e:
            call()
        assert e.value.code == _lib.GOGP_EARG
    g32.close()


def test_empty_process():
    fam = SHAPE_FAMILY
    D, _, ts = FAMILIES[fam]
    g = _gp(fam)
    g.Absorb(np.zeros((0, D)), np.zeros(0))
    mu, sigma, logp = g.LOO()
    assert mu.shape == sigma.shape == logp.shape == (0,)
    assert g.LOOScore() == 0.0
    grad = g.LOOGradient()
    assert grad.shape == (len(ts) + 1,) and not grad.any()
    g.Observe(_x(fam))
    assert g.LOOScore() == 0.0 and not g.LOOGradient().any()
    g.close()


def test_optimiser_on_the_loo_objective():
    from gogp_amd.gp import GP, LOOModel
    n, D, threshold = 200, 2, 1e-3
    X, y = synth.make_inputs(n, D, 5)
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, LR.NOISE, X=X, Y=y, device=0)
    m = LOOModel(g)
    x0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    start = m.Observe(x0)
    res = optimize.lbfgs(m, x0, gradient_threshold=threshold)
    want = LR.reference(D, simil, res.x, X, y)
    print("LOO objective: start %.9f, end %.9f (reference %.9f) after %d iterations, %d evaluations; theta = %s, "
          "max |gradient| = %.3e (reference %.3e)"
          % (start, res.lml, want[2].sum(), res.iterations, res.evaluations, np.exp(res.x), np.abs(res.grad).max(),
             np.abs(want[3]).max()))
    assert res.lml >= start
    assert res.converged and np.abs(res.grad).max() <= threshold
    np.testing.assert_allclose(res.lml, want[2].sum(), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.Observe(res.x), res.lml, rtol=1e-12, atol=0)  # the model ends at the returned point
    g.close()


def test_loo_model_adds_the_priors():
    from gogp_amd.gp import GP, LOOModel
    fam = "matern52"
    D, simil, ts = FAMILIES[fam]
    X, y, *want = _ref(fam, 129)
    pri = optimize.NormalLogPriors(np.zeros(len(ts) + 1), np.ones(len(ts) + 1))
    g = GP(D, simil, LR.NOISE, X=X, Y=y, device=0)
    x = _x(fam)
    v = LOOModel(g, pri).Observe(x)
    m = LOOModel(g, pri)
    assert m.Observe(x) == v
    np.testing.assert_allclose(v, want[2].sum() + pri.Observe(x), rtol=1e-6, atol=1e-8)
    gr = m.Gradient()
    want_g = want[3] + np.asarray(pri.Gradient())
    assert np.abs(gr - want_g).max() <= 1e-6 * np.abs(want_g).max()
    g.close()
