"""GP.ProduceGradient (gogp_produce_gradient) on the GPU against the dense numpy reference of tests/produce_grad_ref.py.

Tolerances (the header of tests/test_gpu_parity.py): mu and sigma rtol = 1e-6, atol = 1e-8 against the reference; each
derivative array within 1e-6 of its largest absolute component; mu and sigma against Produce on the same handle
rtol = 1e-9, atol = 1e-12 (equivalent Produce paths).

Shapes (TILE = 128, PANEL = 256, a super-panel of the substitution = 4 panels = 1024 columns): n = 20 below one tile,
129 two tiles in one padded panel, 300 two panels, 1100 two super-panels with a ragged last panel; m = 1 one point,
33 both few-point launches of Produce, 65 the first size past produce_small_max, 130 two tile rows = two substitution
groups (and three row groups of the backward kernel).

Reference counterpart: none (gp.GP.Produce returns mu and sigma only)."""
import numpy as np
import pytest

import produce_grad_ref as PG
from gogp_amd import _lib, kernel

pytestmark = pytest.mark.gpu

SHAPES = [(n, m) for n in (20, 129, 300, 1100) for m in (1, 65)] + [(1100, 33), (1100, 130)]
SHAPE_FAMILY = "ard_rbf3"
_REF = {}


def _ref(fam, n, m):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, n, m)
    if key not in _REF:
        D, simil, ts = PG.FAMILIES[fam]
        X, y, Z = PG.inputs(n, m, D)
        _REF[key] = (X, y, Z) + PG.reference(D, simil, ts, X, y, Z)
    return _REF[key]


def _gp(fam, simil=None, **kw):
    from gogp_amd.gp import GP
    D, s, ts = PG.FAMILIES[fam]
    return GP(D, simil or s, PG.NOISE, ThetaSimil=ts, ThetaNoise=PG.TN, device=0, **kw)


def _check(got, want, tag):
    mu, sigma, dmu, dsigma = got
    mu_o, sigma_o, dmu_o, dsigma_o = want
    assert dmu.shape == dmu_o.shape and dsigma.shape == dsigma_o.shape
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(sigma, sigma_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    PG.assert_derivative(dmu, dmu_o, "%s dmu" % (tag,))
    PG.assert_derivative(dsigma, dsigma_o, "%s dsigma" % (tag,))


def _same_as_produce(g, Z, got):
    mu, sigma = g.Produce(Z)
    np.testing.assert_allclose(got[0], mu, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got[1], sigma, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes(n, m):
    X, y, Z, *want = _ref(SHAPE_FAMILY, n, m)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    got = g.ProduceGradient(Z)
    _check(got, want, (n, m))
    _same_as_produce(g, Z, got)
    g.close()


@pytest.mark.parametrize("fam,n,m", [(f, 300, 33) for f in PG.FOUR] + [("ard_rbf64", 129, 1)])
def test_kernel_families(fam, n, m):
    X, y, Z, *want = _ref(fam, n, m)
    g = _gp(fam)
    g.Absorb(X, y)
    got = g.ProduceGradient(Z)
    _check(got, want, (fam, n, m))
    _same_as_produce(g, Z, got)
    g.close()


def test_events():
    D, simil, ts = PG.FAMILIES["matern52"]
    X, y, Z, bounds = PG.event_inputs(129, 33)
    assert np.abs(Z - bounds[None, :]).min() >= 1e-3  # no test point on (or within 1e-3 of) a boundary
    assert (Z[:, 0] < 1.0).any() and (Z[:, 0] > 1.0).any() and (X[:, 0] < 1.0).any() and (X[:, 0] > 1.0).any()
    want = PG.reference(D, simil, ts, X, y, Z, events=PG.EVENTS)
    g = _gp("matern52", simil=kernel.Events(simil, PG.EVENTS, 0))
    g.Absorb(X, y)
    got = g.ProduceGradient(Z)
    _check(got, want, "events")
    _same_as_produce(g, Z, got)
    g.close()


def test_states():
    fam, n, m = SHAPE_FAMILY, 300, 33
    D, simil, ts = PG.FAMILIES[fam]
    X, y, Z, *want = _ref(fam, n, m)
    x = np.log(np.array(list(ts) + PG.TN))
    absorbed = _gp(fam)
    absorbed.Absorb(X, y)
    ref_state = absorbed.ProduceGradient(Z)
    _check(ref_state, want, "absorb")
    observed = _gp(fam, X=X, Y=y)
    observed.Observe(x)
    _check(observed.ProduceGradient(Z), want, "observe")
    full = _gp(fam)
    full.Observe(np.concatenate([x, X.reshape(-1), y]))
    _check(full.ProduceGradient(Z), want, "observe, full form")
    restored = _gp(fam)
    restored.X, restored.Y = X, y
    restored.restore(absorbed.L, absorbed.Alpha)
    _check(restored.ProduceGradient(Z), want, "restore")
    appended = _gp(fam)
    appended.Absorb(X[:295], y[:295])
    appended.Append(X[295:], y[295:])
    got = appended.ProduceGradient(Z)
    _check(got, want, "append")
    for a, b in zip(got, ref_state):  # ... and equals the GP that absorbed all 300 rows
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
    for g in (absorbed, observed, full, restored, appended):
        g.close()


def test_behind_an_eager_observe_and_gradient_unchanged():
    fam, n, m = SHAPE_FAMILY, 1100, 65
    D, simil, ts = PG.FAMILIES[fam]
    X, y, Z, *want = _ref(fam, n, m)
    x = np.log(np.array(list(ts) + PG.TN))
    g = _gp(fam, X=X, Y=y)
    g.Observe(x)
    grad_alone = g.Gradient()
    g.Observe(x)  # eager: the triangular inverse is still running when the call starts
    got = g.ProduceGradient(Z)
    grad = g.Gradient()
    _check(got, want, "busy")
    np.testing.assert_allclose(grad, grad_alone, rtol=1e-12, atol=0)
    g.close()


@pytest.mark.parametrize("m", [33, 130])
def test_produce_is_not_disturbed_and_calls_are_deterministic(m):
    X, y, Z, *_ = _ref(SHAPE_FAMILY, 1100, m)
    g = _gp(SHAPE_FAMILY)
    g.Absorb(X, y)
    before = g.Produce(Z)
    first = g.ProduceGradient(Z)
    after = g.Produce(Z)
    second = g.ProduceGradient(Z)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    g.close()


def test_duplicate_point():
    fam, n, m = "matern32_2d", 129, 5
    D, simil, ts = PG.FAMILIES[fam]
    X, y, Z = PG.inputs(n, m, D)
    Z = Z.copy()
    Z[2] = X[40]  # a test point on a training point: the pair contributes exact zeros
    want = PG.reference(D, simil, ts, X, y, Z)
    g = _gp(fam)
    g.Absorb(X, y)
    got = g.ProduceGradient(Z)
    assert all(np.isfinite(a).all() for a in got)
    _check(got, want, "duplicate")
    g.close()


def test_empty_process():
    D, simil, ts = PG.FAMILIES[SHAPE_FAMILY]
    Z = PG.inputs(1, 6, D)[2]
    g = _gp(SHAPE_FAMILY)
    mu, sigma, dmu, dsigma = g.ProduceGradient(Z)
    mu_p, sigma_p = g.Produce(Z)
    np.testing.assert_array_equal(mu, mu_p)
    np.testing.assert_array_equal(sigma, sigma_p)
    assert dmu.shape == (6, D) and dsigma.shape == (6, D)
    assert not dmu.any() and not dsigma.any()
    assert all(a.shape == (0, D) for a in g.ProduceGradient(np.zeros((0, D)))[2:])
    g.close()


def test_refusals():
    from gogp_amd.gp import GogpError
    D, simil, ts = PG.FAMILIES[SHAPE_FAMILY]
    X, y, Z = PG.inputs(40, 3, D)
    g32 = _gp(SHAPE_FAMILY, precision=32)
    g32.Absorb(X, y)
    with pytest.raises(GogpError) as ei:
        g32.ProduceGradient(Z)
    assert ei.value.code == _lib.GOGP_EARG and "precision" in str(ei.value)
    g32.close()
    g = _gp(SHAPE_FAMILY, X=X, Y=y)
    g._push_data()  # data set, nothing absorbed
    for call in (g.Produce, g.ProduceGradient):
        with pytest.raises(GogpError) as ei:
            call(Z)
        assert ei.value.code == _lib.GOGP_ESTATE
    g.close()
