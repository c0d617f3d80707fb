"""GP.LaplaceObserve / LaplaceGradient / LaplaceMode / LaplaceProduce (gogp_laplace_*) on the GPU against the numpy
restatement of tests/laplace_ref.py (tests/test_laplace_cpu.py pins it to the definitions and to central differences).

Tolerances (the header of tests/test_gpu_parity.py): values -- Z, the mode's f and a, mu, sigma, mean -- rtol = 1e-6,
atol = 1e-8; every component of the gradient within 1e-6 of the largest absolute component.  Inputs: X of
tests/loo_ref.py; y drawn once with a fixed seed from the model itself (laplace_ref.draw: poisson rate exp(f + 1),
bernoulli P(y = 1) = logistic(f)).  There the reference converges in <= 8 Newton steps and cond(B) <~ 1e3 (asserted on
the reference below against 1e5, so that the tolerance is not what hides a failure): both sides solve to ~1e-12
relative, and a mode found to 1e-10 moves Z by the square of that.

Shapes (TILE = 128, PANEL = 256; the passes work on 64 x 64 tiles): n = 1; 20 and 128, where the regression path takes
the one-launch `tiny` route that the Laplace calls bypass; 129; 300 two panels, ragged; 1100 npad = 1280.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

import laplace_ref as LP
from gogp_amd import _lib, kernel, optimize

pytestmark = pytest.mark.gpu

SHAPE_FAMILY = "ard_rbf3"
SHAPES = (1, 20, 128, 129, 300, 1100)
LIKS = [LP.BERNOULLI, LP.POISSON]
IDS = ["bernoulli", "poisson"]
RADIAL = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8]),
    "matern52": (2, kernel.Scaled(kernel.Matern52), [1.2, 0.9]),
    "matern52textbook": (2, kernel.Scaled(kernel.Matern52Textbook), [0.9, 1.1]),
}
FAMILIES = dict(LP.FAMILIES, **RADIAL)
_REF = {}
dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731


def _x(fam):
    return np.log(np.array(list(FAMILIES[fam][2]) + LP.TN))


def _ref(fam, n, lik, events=None):
    """Inputs and reference of one case: computed once, shared, read only.  y is drawn from the model WITHOUT the
    discounts, so that the case with events shares its data with the case without."""
    key = (fam, n, lik, bool(events))
    if key not in _REF:
        D, simil, _ = FAMILIES[fam]
        X = LP.inputs(n, 1, D)[0]
        y = LP.draw(lik, LP.gram(D, simil, _x(fam), X))
        fit, grad = LP.reference(lik, D, simil, _x(fam), X, y, events)
        assert fit.converged and fit.iterations <= 8, (key, fit.iterations)
        assert np.linalg.cond(fit.B) <= 1e5, key
        _REF[key] = (X, y, fit, grad)
    return _REF[key]


def _gp(fam, simil=None, **kw):
    from gogp_amd.gp import GP
    D, s, ts = FAMILIES[fam]
    return GP(D, simil or s, LP.NOISE, ThetaSimil=ts, ThetaNoise=LP.TN, device=0, **kw)


def _check(g, fam, lik, fit, grad_o, tag):
    """Z, the mode and the gradient against the reference, every figure printed first; a second call: the same bits"""
    z = g.LaplaceObserve(_x(fam), lik)
    f, a, its = g.LaplaceMode()
    grad = g.LaplaceGradient()
    crit = lambda u, v: (np.abs(u - v) / (1e-8 + 1e-6 * np.abs(v))).max() if len(v) else 0.0  # noqa: E731
    scale = np.abs(grad_o).max()
    print("%s: Z %.12e (reference %.12e), %d steps (reference %d); f %.3e a %.3e of the rtol 1e-6 + atol 1e-8 criterion; "
          "gradient max |err| = %.3e of largest component %.3e (%.2e relative)"
          % (tag, z, fit.Z, its, fit.iterations, crit(f, fit.f), crit(a, fit.a), np.abs(grad - grad_o).max(), scale,
             np.abs(grad - grad_o).max() / scale))
    np.testing.assert_allclose(z, fit.Z, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(f, fit.f, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(a, fit.a, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    assert abs(its - fit.iterations) <= 1, tag  # (a residual at the tolerance's edge may round either way)
    assert grad.shape == grad_o.shape
    assert np.abs(grad - grad_o).max() <= 1e-6 * scale, (tag, grad, grad_o)
    np.testing.assert_array_equal(g.LaplaceGradient(), grad)
    assert g.LaplaceObserve(_x(fam), lik) == z
    f2, a2, its2 = g.LaplaceMode()
    np.testing.assert_array_equal(f2, f)
    np.testing.assert_array_equal(a2, a)
    np.testing.assert_array_equal(g.LaplaceGradient(), grad)
    assert its2 == its
    return z, f, a, grad


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
@pytest.mark.parametrize("n", SHAPES)
def test_shapes(n, lik):
    X, y, fit, grad = _ref(SHAPE_FAMILY, n, lik)
    g = _gp(SHAPE_FAMILY)
    g.X, g.Y = X, y
    _check(g, SHAPE_FAMILY, lik, fit, grad, (n, lik))
    g.close()


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
@pytest.mark.parametrize("fam", sorted(RADIAL) + ["ard_rbf3", "ard_rbf64", "hyperpriors"])
def test_kernel_families(fam, lik):
    X, y, fit, grad = _ref(fam, 300, lik)
    g = _gp(fam)
    g.X, g.Y = X, y
    _check(g, fam, lik, fit, grad, (fam, lik))
    g.close()


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
def test_events(lik):
    fam = "matern52"
    D, simil, ts = FAMILIES[fam]
    X, y, fit, grad = _ref(fam, 300, lik, LP.EVENTS)
    _, y0, plain, grad0 = _ref(fam, 300, lik)
    np.testing.assert_array_equal(y, y0)
    assert abs(fit.Z - plain.Z) > 1e-3  # the discounts change Z ...
    assert np.abs(grad - grad0).max() > 1e-3 * np.abs(grad0).max()  # ... and the gradient
    g = _gp(fam, simil=kernel.Events(simil, LP.EVENTS, 0))
    g.X, g.Y = X, y
    _check(g, fam, lik, fit, grad, ("events", lik))
    Z = LP.inputs(1, 65, D)[2]
    Ks, prior = LP.cross(D, simil, _x(fam), X, Z, LP.EVENTS)
    for got, want in zip(g.LaplaceProduce(Z), LP.predict(lik, fit, Ks, prior)):
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8)
    g.close()


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
def test_produce(lik):
    fam = SHAPE_FAMILY
    D, simil, _ = FAMILIES[fam]
    X, y, fit, _ = _ref(fam, 300, lik)
    g = _gp(fam)
    g.X, g.Y = X, y
    g.LaplaceObserve(_x(fam), lik)
    for m in (1, 64, 65, 300):
        Z = LP.inputs(1, m, D)[2]
        Ks, prior = LP.cross(D, simil, _x(fam), X, Z)
        want = LP.predict(lik, fit, Ks, prior)
        got = g.LaplaceProduce(Z)
        crit = lambda u, v: (np.abs(u - v) / (1e-8 + 1e-6 * np.abs(v))).max()  # noqa: E731
        print("produce m = %d: mu %.3e sigma %.3e mean %.3e of the rtol 1e-6 + atol 1e-8 criterion"
              % ((m,) + tuple(crit(u, v) for u, v in zip(got, want))))
        for u, v in zip(got, want):
            np.testing.assert_allclose(u, v, rtol=1e-6, atol=1e-8)
        again = g.LaplaceProduce(Z, mean=False)  # mean == NULL
        assert again[2] is None
        np.testing.assert_array_equal(again[0], got[0])
        np.testing.assert_array_equal(again[1], got[1])
    # after the gradient turned B^-1 into its weight matrix: the factor is untouched
    g.LaplaceGradient()
    for u, v in zip(g.LaplaceProduce(Z), got):
        np.testing.assert_array_equal(u, v)
    mu, sigma, mean = g.LaplaceProduce(np.zeros((0, D)))  # m == 0
    assert mu.shape == sigma.shape == mean.shape == (0,)
    g.close()


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
def test_empty_process(lik):
    fam = SHAPE_FAMILY
    D, simil, ts = FAMILIES[fam]
    g = _gp(fam)
    g.X, g.Y = np.zeros((0, D)), np.zeros(0)
    assert g.LaplaceObserve(_x(fam), lik) == 0.0
    grad = g.LaplaceGradient()
    assert grad.shape == (len(ts) + 1,) and not grad.any()
    f, a, its = g.LaplaceMode()
    assert f.shape == a.shape == (0,) and its == 0
    Z = LP.inputs(1, 5, D)[2]
    _, prior = LP.cross(D, simil, _x(fam), np.zeros((0, D)), Z)
    mu, sigma, mean = g.LaplaceProduce(Z)
    assert not mu.any()
    np.testing.assert_allclose(sigma, np.sqrt(prior), rtol=1e-12)
    np.testing.assert_allclose(mean, LP.gh_mean(lik, np.zeros(5), np.sqrt(prior)), rtol=1e-6, atol=1e-8)
    g.close()


def test_regression_after_laplace_returns_a_fresh_handles_bits():
    from gogp_amd.gp import GogpError
    fam = SHAPE_FAMILY
    D = FAMILIES[fam][0]
    X, yc, *_ = _ref(fam, 300, LP.POISSON)
    Z = LP.inputs(1, 33, D)[2]
    yr = LP.inputs(300, 1, D)[1]

    def regression(g):
        g.X, g.Y = X, yr
        return (np.array(g.Observe(_x(fam))), g.Gradient(), *g.Produce(Z))

    fresh = _gp(fam)
    want = regression(fresh)
    fresh.close()
    g = _gp(fam)
    g.X, g.Y = X, yc
    g.LaplaceObserve(_x(fam), LP.POISSON)
    g.LaplaceGradient()
    g.LaplaceProduce(Z)
    for call in (g.Gradient, lambda: g.Produce(Z), g.LOOScore):  # the regression state is gone
        with pytest.raises(GogpError) as e:
            call()
        assert e.value.code == _lib.GOGP_ESTATE
    for u, v in zip(regression(g), want):
        np.testing.assert_array_equal(u, v)
    # ... and the factorisation of a regression call drops the Laplace state
    g.Absorb(X, yr)
    for call in (g.LaplaceGradient, g.LaplaceMode, lambda: g.LaplaceProduce(Z)):
        with pytest.raises(GogpError) as e:
            call()
        assert e.value.code == _lib.GOGP_ESTATE
    g.close()
    g = _gp(fam)  # before any Laplace observe
    g.X, g.Y = X, yc
    g._push_data()
    with pytest.raises(GogpError) as e:
        g.LaplaceGradient()
    assert e.value.code == _lib.GOGP_ESTATE
    g.close()


def test_sparse_and_multi_output_states_survive():
    fam = SHAPE_FAMILY
    D = FAMILIES[fam][0]
    X, yc, *_ = _ref(fam, 300, LP.POISSON)
    yr = LP.inputs(300, 1, D)[1]
    Y2 = np.stack([yr, yr * yr], axis=1)
    L = _lib.lib()

    def run(laplace):
        g = _gp(fam)
        g.X, g.Y = X, yc
        g._push_data()
        x = _x(fam)
        assert L.gogp_sparse_set_data(g._h, dp(X), dp(yr), 300, dp(np.ascontiguousarray(X[:32])), 32) == _lib.GOGP_OK
        assert L.gogp_multi_set_outputs(g._h, dp(np.ascontiguousarray(Y2)), 300, 2) == _lib.GOGP_OK
        b = ctypes.c_double()
        assert L.gogp_sparse_observe(g._h, dp(x), x.size, ctypes.byref(b)) == _lib.GOGP_OK
        if laplace:
            g.LaplaceObserve(x, LP.POISSON)
            g.LaplaceGradient()
        sg = np.zeros(x.size)
        assert L.gogp_sparse_gradient(g._h, dp(sg), x.size) == _lib.GOGP_OK  # the sparse observe is still in place
        g.Observe(x)
        tot, lml = ctypes.c_double(), np.zeros(2)
        assert L.gogp_multi_lml(g._h, ctypes.byref(tot), dp(lml)) == _lib.GOGP_OK  # the outputs are still set
        g.close()
        return b.value, sg, tot.value, lml

    for u, v in zip(run(False), run(True)):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
def test_warm_start(lik):
    fam = "matern52"
    X, y, fit, grad = _ref(fam, 300, lik)
    g = _gp(fam)
    g.X, g.Y = X, y
    x = _x(fam)
    cold = g.LaplaceObserve(x, lik)
    its_cold = g.LaplaceMode()[2]
    g.set_option("laplace_warm", 1)
    warm = g.LaplaceObserve(x, lik)
    f, a, its_warm = g.LaplaceMode()
    print("warm start: %d steps against %d cold; Z %.12e against %.12e" % (its_warm, its_cold, warm, cold))
    np.testing.assert_allclose(warm, cold, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(f, fit.f, rtol=1e-6, atol=1e-8)
    assert its_warm <= its_cold
    gw = g.LaplaceGradient()
    assert np.abs(gw - grad).max() <= 1e-6 * np.abs(grad).max()
    # a nearby theta from the stored mode
    x2 = x + 0.05
    D, simil, _ = FAMILIES[fam]
    fit2, _ = LP.reference(lik, D, simil, x2, X, y)
    np.testing.assert_allclose(g.LaplaceObserve(x2, lik), fit2.Z, rtol=1e-6, atol=1e-8)
    assert g.LaplaceMode()[2] <= fit2.iterations
    # with the option off again an observe does not depend on the earlier ones
    g.set_option("laplace_warm", 0)
    assert g.LaplaceObserve(x, lik) == cold
    g.close()


def test_refusals():
    from gogp_amd.gp import GP, ConvergenceError, GogpError
    fam = SHAPE_FAMILY
    D, simil, ts = FAMILIES[fam]
    X, y, fit, _ = _ref(fam, 300, LP.POISSON)
    yb = _ref(fam, 300, LP.BERNOULLI)[1]
    x = _x(fam)
    P = x.size
    L = _lib.lib()
    g = _gp(fam)
    z = ctypes.c_double()
    assert L.gogp_laplace_observe(g._h, LP.POISSON, dp(x), P, ctypes.byref(z)) == _lib.GOGP_ESTATE  # no data
    for lik, good, bad in ((LP.BERNOULLI, yb, 0.5), (LP.BERNOULLI, yb, 2.0), (LP.POISSON, y, -1.0)):
        yy = good.copy()
        yy[137] = bad
        g.X, g.Y = X, yy
        with pytest.raises(GogpError) as e:
            g.LaplaceObserve(x, lik)
        assert e.value.code == _lib.GOGP_EARG and "137" in str(e.value)
    g.X, g.Y = X, y  # the handle stays usable
    np.testing.assert_allclose(g.LaplaceObserve(x, LP.POISSON), fit.Z, rtol=1e-6, atol=1e-8)
    assert L.gogp_laplace_observe(g._h, LP.POISSON, dp(x), P + 1, ctypes.byref(z)) == _lib.GOGP_EARG
    assert L.gogp_laplace_observe(g._h, 2, dp(x), P, ctypes.byref(z)) == _lib.GOGP_EARG
    assert L.gogp_laplace_observe(g._h, LP.POISSON, None, P, ctypes.byref(z)) == _lib.GOGP_EARG
    xb = x.copy()
    xb[0] = np.nan
    assert L.gogp_laplace_observe(g._h, LP.POISSON, dp(xb), P, ctypes.byref(z)) == _lib.GOGP_EARG
    grad = np.zeros(P)
    g.LaplaceObserve(x, LP.POISSON)
    assert L.gogp_laplace_gradient(g._h, dp(grad), P + 1) == _lib.GOGP_EARG
    assert L.gogp_laplace_gradient(g._h, None, P) == _lib.GOGP_EARG
    assert L.gogp_laplace_get_mode(g._h, None, None, None) == _lib.GOGP_OK
    # one Newton step is not enough: GOGP_ENOCONV with finite values, and gradient and produce work on the iterate
    g.set_option("laplace_max_iter", 1)
    with pytest.raises(ConvergenceError) as e:
        g.LaplaceObserve(x, LP.POISSON)
    assert e.value.code == _lib.GOGP_ENOCONV and np.isfinite(e.value.lml)
    f, a, its = g.LaplaceMode()
    assert its == 1 and np.all(np.isfinite(f)) and np.all(np.isfinite(a))
    assert np.all(np.isfinite(g.LaplaceGradient()))
    assert all(np.all(np.isfinite(v)) for v in g.LaplaceProduce(LP.inputs(1, 3, D)[2]))
    for name, bad in (("laplace_max_iter", 0), ("laplace_max_iter", 201), ("laplace_tol_log10", -15),
                      ("laplace_tol_log10", -3), ("laplace_warm", 2)):
        with pytest.raises(GogpError):
            g.set_option(name, bad)
    # the refused kinds of handle
    g.set_option("laplace_max_iter", 50)
    g.set_option("gradient_precision", 32)
    with pytest.raises(GogpError) as e:
        g.LaplaceObserve(x, LP.POISSON)
    assert e.value.code == _lib.GOGP_EARG
    g.close()
    g32 = GP(D, simil, LP.NOISE, ThetaSimil=ts, ThetaNoise=LP.TN, device=0, precision=32)
    g32.X, g32.Y = X, y
    with pytest.raises(GogpError) as e:
        g32.LaplaceObserve(x, LP.POISSON)
    assert e.value.code == _lib.GOGP_EARG
    g32.close()


def test_sharded_handles_are_refused():
    import loopback
    from gogp_amd.sharded import ShardedGP
    fam = "matern52"
    D, simil, _ = FAMILIES[fam]
    x = _x(fam)
    P = x.size
    Z = np.ascontiguousarray(LP.inputs(1, 3, D)[2])

    def rank_fn(r, lb):
        sh = ShardedGP(D, simil, LP.NOISE, device=0, grid=(1, 2), rank=r, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        L = _lib.lib()
        z, grad, mu, sigma, mean = ctypes.c_double(), np.zeros(P), np.zeros(3), np.zeros(3), np.zeros(3)
        rcs, msgs = [], []
        for call in (lambda: L.gogp_laplace_observe(sh._h, LP.POISSON, dp(x), P, ctypes.byref(z)),
                     lambda: L.gogp_laplace_gradient(sh._h, dp(grad), P),
                     lambda: L.gogp_laplace_produce(sh._h, dp(Z), 3, dp(mu), dp(sigma), dp(mean))):
            rcs.append(call())
            msgs.append(L.gogp_last_error(sh._h))
        sh.close()  # the handle still closes cleanly
        return rcs, msgs

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rcs, msgs in outs:
        assert rcs == [_lib.GOGP_EARG] * 3
        assert all(b"sharded" in m for m in msgs), msgs


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
def test_optimiser_on_the_laplace_objective(lik):
    from gogp_amd.gp import GP, LaplaceModel
    n, D = 200, 2
    simil = kernel.Scaled(kernel.Normal)
    X = LP.inputs(n, 1, D)[0]
    x_true = np.log(np.array([1.1, 0.8] + LP.TN))
    y = LP.draw(lik, LP.gram(D, simil, x_true, X))
    g = GP(D, simil, LP.NOISE, X=X, Y=y, device=0)
    m = LaplaceModel(g, "bernoulli" if lik == LP.BERNOULLI else "poisson")
    x0 = np.log(np.array([0.7, 1.3, 0.3]))
    start = m.Observe(x0)
    res = optimize.lbfgs(m, x0, major_iterations=30)
    fit, grad = LP.reference(lik, D, simil, res.x, X, y)
    print("Laplace objective: start %.9f, end %.9f (reference %.9f) after %d iterations, %d evaluations; theta = %s, "
          "max |gradient| = %.3e (reference %.3e)"
          % (start, res.lml, fit.Z, res.iterations, res.evaluations, np.exp(res.x), np.abs(res.grad).max(),
             np.abs(grad).max()))
    assert res.iterations <= 30
    assert res.lml >= start
    np.testing.assert_allclose(res.lml, fit.Z, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.Observe(res.x), fit.Z, rtol=1e-6, atol=1e-8)
    g.close()
