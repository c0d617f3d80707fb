"""GP.ProduceCovariance / GP.Sample (gogp_produce_covariance, gogp_produce_samples) on the GPU against the dense numpy
reference of tests/produce_cov_ref.py.

Tolerances (the header of tests/test_gpu_parity.py): mu, every entry of cov and every sample rtol = 1e-6, atol = 1e-8
against the reference.  The entries are O(1) (prior variances 1.0 - 1.2); with noise variance 0.09 and n <= 1100,
cond(K) <~ 1.5e4, so the rounding of V^T V is ~1e-12 and the reference sits far inside that.  mu and sqrt(diag cov)
against Produce on the same handle rtol = 1e-9, atol = 1e-12 (equivalent Produce paths; every sigma > 0.05 with these
inputs, asserted).  Samples are drawn at diag_add = 0.09 (noisy observations): cov + 0.09 I has cond <~ 15, so its
Cholesky factor is as well determined as cov itself.

Shapes (TILE = 128, PANEL = 256, SYRK output tile 64 x 64, a slab >= 256 columns): n = 20 below one tile, one slab;
129 two tiles in one padded panel; 300 two panels; 1100 a ragged last panel (npad = 1280) with at least two slabs;
m = 1 one point, 17 a partial 16-row MFMA tile, 65 the first size past one 64-row tile, 130 three tile rows with
off-diagonal tile pairs and two substitution groups; samples m = 300: the factorisation of the covariance crosses a
256-panel.

Reference counterpart: none (gp.GP.Produce keeps the diagonal of Kstar^T K^-1 Kstar only)."""
import ctypes

import numpy as np
import pytest

import produce_cov_ref as PC
from gogp_amd import _lib, kernel

pytestmark = pytest.mark.gpu

SHAPES = [(n, m) for n in (20, 129, 300, 1100) for m in (1, 65)] + [(1100, 17), (1100, 130)]
SHAPE_FAMILY = "ard_rbf3"
DIAG_ADD = 0.09
_REF = {}


def _ref(fam, n, m):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, n, m)
    if key not in _REF:
        D, simil, ts = PC.FAMILIES[fam]
        X, y, Z = PC.inputs(n, m, D)
        _REF[key] = (X, y, Z) + PC.reference(D, simil, ts, X, y, Z)
    return _REF[key]


def _gp(fam, simil=None, **kw):
    from gogp_amd.gp import GP
    D, s, ts = PC.FAMILIES[fam]
    return GP(D, simil or s, PC.NOISE, ThetaSimil=ts, ThetaNoise=PC.TN, device=0, **kw)


def _report(tag, what, got, want):
    err = np.abs(np.asarray(got) - want)
    print("%s %s: max |err| = %.3e (largest entry %.3e)" % (tag, what, err.max() if err.size else 0.0,
                                                            np.abs(want).max() if err.size else 0.0))


def _check(g, Z, want, tag):
    """mu, cov against the reference and against Produce; symmetry; a second call returns the same bits"""
    mu_o, cov_o = want
    m = len(Z)
    mu, cov = g.ProduceCovariance(Z)
    assert mu.shape == (m,) and cov.shape == (m, m)
    _report(tag, "mu", mu, mu_o)
    _report(tag, "cov", cov, cov_o)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(cov, cov_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_array_equal(cov, cov.T)
    mu_p, sigma_p = g.Produce(Z)
    assert sigma_p.min() > 0.05, sigma_p.min()
    _report(tag, "sqrt(diag cov) against Produce", np.sqrt(np.diag(cov)), sigma_p)
    np.testing.assert_allclose(mu, mu_p, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), sigma_p, rtol=1e-9, atol=1e-12)
    mu2, cov2 = g.ProduceCovariance(Z)
    np.testing.assert_array_equal(mu, mu2)
    np.testing.assert_array_equal(cov, cov2)
    return mu, cov


@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes(n, m):
    X, y, Z, *want = _ref(SHAPE_FAMILY, n, m)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    _check(g, Z, want, (n, m))
    g.close()


@pytest.mark.parametrize("fam,n,m", [(f, 300, 33) for f in PC.FOUR] + [("ard_rbf64", 129, 5)])
def test_kernel_families(fam, n, m):
    X, y, Z, *want = _ref(fam, n, m)
    g = _gp(fam)
    g.Absorb(X, y)
    _check(g, Z, want, (fam, n, m))
    g.close()


def test_events():
    D, simil, ts = PC.FAMILIES["matern52"]
    X, y, Z, bounds = PC.event_inputs(129, 33)
    assert np.abs(Z - bounds[None, :]).min() >= 1e-3  # no test point on (or within 1e-3 of) a boundary
    assert (Z[:, 0] < 1.0).any() and (Z[:, 0] > 1.0).any() and (X[:, 0] < 1.0).any() and (X[:, 0] > 1.0).any()
    want = PC.reference(D, simil, ts, X, y, Z, events=PC.EVENTS)
    assert np.abs(want[1] - PC.reference(D, simil, ts, X, y, Z)[1]).max() > 1e-3  # the discounts matter here
    g = _gp("matern52", simil=kernel.Events(simil, PC.EVENTS, 0))
    g.Absorb(X, y)
    mu, cov = _check(g, Z, want, "events")
    xi = np.random.default_rng(5).standard_normal((3, 33))
    want_s = want[0] + xi @ np.linalg.cholesky(want[1] + DIAG_ADD * np.eye(33)).T
    np.testing.assert_allclose(g.Sample(Z, xi=xi, diag_add=DIAG_ADD), want_s, rtol=1e-6, atol=1e-8)
    g.close()


def test_empty_process():
    D, simil, ts = PC.FAMILIES[SHAPE_FAMILY]
    Z = PC.inputs(1, 70, D)[2]
    want = PC.reference(D, simil, ts, np.zeros((0, D)), np.zeros(0), Z)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(np.zeros((0, D)), np.zeros(0))  # no observations; the parameters are the handle's from here on
    mu, cov = g.ProduceCovariance(Z)
    assert not mu.any()
    np.testing.assert_allclose(cov, want[1], rtol=1e-6, atol=1e-8)
    np.testing.assert_array_equal(cov, cov.T)
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), g.Produce(Z)[1], rtol=1e-9, atol=1e-12)
    xi = np.random.default_rng(3).standard_normal((4, 70))  # draws from the prior
    want_s = xi @ np.linalg.cholesky(want[1] + DIAG_ADD * np.eye(70)).T
    np.testing.assert_allclose(g.Sample(Z, xi=xi, diag_add=DIAG_ADD), want_s, rtol=1e-6, atol=1e-8)
    mu0, cov0 = g.ProduceCovariance(np.zeros((0, D)))
    assert mu0.shape == (0,) and cov0.shape == (0, 0)
    assert g.Sample(np.zeros((0, D)), ns=3).shape == (3, 0)
    g.close()


def test_states():
    fam, n, m = SHAPE_FAMILY, 300, 33
    D, simil, ts = PC.FAMILIES[fam]
    X, y, Z, *want = _ref(fam, n, m)
    x = np.log(np.array(list(ts) + PC.TN))
    absorbed = _gp(fam)
    absorbed.Absorb(X, y)
    _check(absorbed, Z, want, "absorb")
    restored = _gp(fam)  # set_factor on a fresh handle
    restored.X, restored.Y = X, y
    restored.restore(absorbed.L, absorbed.Alpha)
    _check(restored, Z, want, "restore")
    appended = _gp(fam)
    appended.Absorb(X[:295], y[:295])
    appended.Append(X[295:], y[295:])
    _check(appended, Z, want, "append")
    removed = _gp(fam)
    removed.Absorb(X, y)
    gone = [0, 7, 150, 299]
    keep = np.setdiff1d(np.arange(n), gone)
    removed.Remove(gone)
    _check(removed, Z, PC.reference(D, simil, ts, X[keep], y[keep], Z), "remove")
    for g in (absorbed, restored, appended, removed):
        g.close()
    ns0 = _gp(fam)
    ns0.Absorb(X, y)
    assert ns0.Sample(Z, ns=0).shape == (0, m)
    ns0.close()
    # nothing absorbed: the state error of Produce
    from gogp_amd.gp import GogpError
    g = _gp(fam, X=X, Y=y)
    g._push_data()
    for call in (g.ProduceCovariance, g.Sample):
        with pytest.raises(GogpError) as ei:
            call(Z)
        assert ei.value.code == _lib.GOGP_ESTATE
    g.close()


def test_behind_an_eager_observe_and_gradient_unchanged():
    fam, n, m = SHAPE_FAMILY, 1100, 65
    D, simil, ts = PC.FAMILIES[fam]
    X, y, Z, *want = _ref(fam, n, m)
    x = np.log(np.array(list(ts) + PC.TN))
    g = _gp(fam, X=X, Y=y)
    g.Observe(x)
    grad_alone = g.Gradient()
    g.Observe(x)  # eager: the triangular inverse is still running when the call starts
    mu, cov = g.ProduceCovariance(Z)
    g.Observe(x)
    xi = np.random.default_rng(11).standard_normal((2, m))
    smp = g.Sample(Z, xi=xi, diag_add=DIAG_ADD)
    grad = g.Gradient()
    np.testing.assert_allclose(mu, want[0], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(cov, want[1], rtol=1e-6, atol=1e-8)
    want_s = want[0] + xi @ np.linalg.cholesky(want[1] + DIAG_ADD * np.eye(m)).T
    np.testing.assert_allclose(smp, want_s, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(grad, grad_alone, rtol=1e-12, atol=0)
    g.close()


def test_the_handle_is_left_as_found():
    X, y, Z, *_ = _ref(SHAPE_FAMILY, 1100, 130)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    before = g.Produce(Z) + (g.L, g.Alpha, g.LML())
    g.ProduceCovariance(Z)
    g.Sample(Z, ns=2, rng=np.random.default_rng(1), diag_add=DIAG_ADD)
    after = g.Produce(Z) + (g.L, g.Alpha, g.LML())
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    g.close()


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("m", [1, 65, 130, 300])
def test_samples(m, ns):
    X, y, Z, mu_o, cov_o = _ref(SHAPE_FAMILY, 300, m)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    xi = np.random.default_rng(100 * m + ns).standard_normal((ns, m))
    smp = g.Sample(Z, xi=xi, diag_add=DIAG_ADD)
    assert smp.shape == (ns, m)
    want = mu_o + xi @ np.linalg.cholesky(cov_o + DIAG_ADD * np.eye(m)).T
    _report((m, ns), "samples", smp, want)
    np.testing.assert_allclose(smp, want, rtol=1e-6, atol=1e-8)
    np.testing.assert_array_equal(smp, g.Sample(Z, xi=xi, diag_add=DIAG_ADD))  # the same bits again
    # the mean the C call returns is ProduceCovariance's
    mu_c, out = np.zeros(m), np.zeros((ns, m))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    Zc, xic = np.ascontiguousarray(Z), np.ascontiguousarray(xi)
    assert _lib.lib().gogp_produce_samples(g._h, dp(Zc), m, dp(xic), ns, DIAG_ADD, dp(mu_c), dp(out)) == _lib.GOGP_OK
    np.testing.assert_array_equal(mu_c, g.ProduceCovariance(Z)[0])
    np.testing.assert_array_equal(out, smp)
    # ns == 0 still fills mu
    mu_z = np.full(m, np.nan)
    assert _lib.lib().gogp_produce_samples(g._h, dp(Zc), m, None, 0, DIAG_ADD, dp(mu_z), None) == _lib.GOGP_OK
    np.testing.assert_array_equal(mu_z, mu_c)
    g.close()


def test_sample_draws_its_own_normals_from_the_rng():
    X, y, Z, mu_o, cov_o = _ref(SHAPE_FAMILY, 300, 65)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    a = g.Sample(Z, ns=3, rng=np.random.default_rng(42), diag_add=DIAG_ADD)
    xi = np.random.default_rng(42).standard_normal((3, 65))
    np.testing.assert_array_equal(a, g.Sample(Z, xi=xi, diag_add=DIAG_ADD))
    assert g.Sample(Z, diag_add=DIAG_ADD).shape == (1, 65)
    g.close()


def test_the_factor_itself():
    """xi = I returns the factor's columns: independent of the conditioning of cov"""
    m, jitter = 300, 1e-6
    X, y, Z, *_ = _ref(SHAPE_FAMILY, 300, m)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    mu, cov = g.ProduceCovariance(Z)
    smp = g.Sample(Z, xi=np.eye(m), diag_add=jitter)
    C = (smp - mu).T
    assert not np.triu(C, 1).any()  # exact zeros above the diagonal
    assert (np.diag(C) > 0).all()
    want = cov + jitter * np.eye(m)
    _report("factor", "C C^T", C @ C.T, want)
    np.testing.assert_allclose(C @ C.T, want, rtol=1e-6, atol=1e-8)
    g.close()


def test_argument_errors():
    from gogp_amd.gp import GogpError
    D, simil, ts = PC.FAMILIES[SHAPE_FAMILY]
    X, y, Z = PC.inputs(40, 3, D)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    xi = np.zeros((2, 3))
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(GogpError) as ei:
            g.Sample(Z, xi=xi, diag_add=bad)
        assert ei.value.code == _lib.GOGP_EARG and "diag_add" in str(ei.value)
    for bad in (float("nan"), float("inf")):
        xib = xi.copy()
        xib[1, 2] = bad
        with pytest.raises(GogpError) as ei:
            g.Sample(Z, xi=xib)
        assert ei.value.code == _lib.GOGP_EARG and "xi" in str(ei.value)
    # m > GOGP_COV_MAX_M is refused before anything is read or written: the output arrays may be tiny
    big = _lib.GOGP_COV_MAX_M + 1
    Zb = np.ascontiguousarray(np.resize(Z, (big, D)))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    one = np.full(1, 7.0)
    L = _lib.lib()
    assert L.gogp_produce_covariance(g._h, dp(Zb), big, dp(one), dp(one)) == _lib.GOGP_EARG
    assert b"GOGP_COV_MAX_M" in L.gogp_last_error(g._h)
    assert L.gogp_produce_samples(g._h, dp(Zb), big, dp(one), 1, 0.0, dp(one), dp(one)) == _lib.GOGP_EARG
    assert one[0] == 7.0
    assert L.gogp_produce_covariance(g._h, None, 3, dp(one), dp(one)) == _lib.GOGP_EARG
    assert L.gogp_produce_samples(g._h, dp(Zb), 3, None, 1, 0.0, dp(one), dp(one)) == _lib.GOGP_EARG
    mu, cov = g.ProduceCovariance(Z)  # ... and the handle still works
    assert np.isfinite(cov).all()
    g.close()
    g32 = _gp(SHAPE_FAMILY, precision=32)
    g32.Absorb(X, y)
    for call in (g32.ProduceCovariance, g32.Sample):
        with pytest.raises(GogpError) as ei:
            call(Z)
        assert ei.value.code == _lib.GOGP_EARG and "precision" in str(ei.value)
    g32.close()


def test_not_positive_definite_covariance():
    """One test point eight times, no jitter: cov has rank m - 7 in exact arithmetic.  Whether a pivot of the factorisation
    comes out non-positive or as a tiny positive number rests on rounding and cannot be fixed in advance: both outcomes
    are accepted -- the error (with the pivot's index among the test points) or finite samples -- and in both the fitted
    process must be untouched."""
    from gogp_amd.gp import FactorizeError
    m = 20
    X, y, Z, *_ = _ref(SHAPE_FAMILY, 300, 33)
    Z = Z[:m].copy()
    Z[5:13] = Z[5]
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    before = g.Produce(Z) + (g.L, g.Alpha)
    xi = np.random.default_rng(9).standard_normal((2, m))
    try:
        smp = g.Sample(Z, xi=xi, diag_add=0.0)
        print("outcome: finite samples")
        assert smp.shape == (2, m) and np.isfinite(smp).all()
    except FactorizeError as e:
        print("outcome: not positive definite, pivot %d: %s" % (e.pivot, e))
        assert 1 <= e.pivot < m  # the first copy of the point has a positive pivot
        assert e.pivot == _lib.lib().gogp_notpd_index(g._h)
        assert "predictive covariance" in str(e)
    after = g.Produce(Z) + (g.L, g.Alpha)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    smp = g.Sample(Z, xi=xi, diag_add=DIAG_ADD)  # ... and with the noise on the diagonal it draws
    assert np.isfinite(smp).all()
    g.close()
