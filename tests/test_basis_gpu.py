"""GP.SetBasis / BasisLML / BasisGradient / BasisBeta / BasisAlpha / BasisProduce (gogp_basis_*) on the GPU against the
dense reference of tests/basis_ref.py (numpy Cholesky in fp64; tests/test_basis_cpu.py pins it to the restricted
likelihood, the universal-kriging system, a proper prior in its limit and central differences, and holds every case
run here to cond(H^T K^-1 H) <= 1e6).

Tolerances (the header of tests/test_gpu_parity.py): LML <= 1e-8 relative; beta, alpha~, mu, sigma rtol = 1e-6,
atol = 1e-8; every component of the gradient within 1e-6 of the largest absolute component.  The reference sits far
inside them: cond(K) <~ 3e4 (tests/test_multi_output_gpu.py) and cond(A) <= 1e6 give beta ~2e-10 relative.

Shapes (n, p): (2, 1) the smallest process a basis fits; (20, 3) the one-launch `tiny` path; (128, 4) its limit;
(129, 5) the first size on the general sweep; (300, 33) two ragged panels and a second LDS pass over p; (1100, 64)
npad = 1280, the limit of p, tile pairs on both sides of the diagonal.  After Absorb W comes from the factor (two
substitutions), after Observe from the explicit K^-1 (basis_symm_kernel): both states run every shape.

Reference counterpart: none (gp.GP has mean zero)."""
import ctypes

import numpy as np
import pytest

import basis_ref as BR
from gogp_amd import _lib, basis, kernel, optimize, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    _lib.build()


def _gp(fam, simil=None, **kw):
    from gogp_amd.gp import GP
    D, s, ts = BR.FAMILIES[fam]
    return GP(D, simil or s, BR.NOISE, ThetaSimil=ts, ThetaNoise=BR.TN, device=0, **kw)


def _fit(g, r, state):
    if state == "absorb":
        g.Absorb(r["X"], r["y"])
    else:
        g.X, g.Y = r["X"], r["y"]
        g.Observe(r["lt"])


crit = lambda a, b: (np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))).max() if b.size else 0.0  # noqa: E731


def _calls(g, r, ms):
    lml, (beta, cov), at, grad = g.BasisLML(), g.BasisBeta(), g.BasisAlpha, g.BasisGradient()
    outs = [g.BasisProduce(r["Z"][:m], r["Hz"][:m]) for m in ms]
    return lml, beta, cov, at, grad, outs


def _check(g, r, tag, ms=BR.MS):
    """Every basis call against the reference, every figure printed first; a second round: the same bits"""
    lml, beta, cov, at, grad, outs = _calls(g, r, ms)
    scale = np.abs(r["grad"]).max()
    print("%s: lml %.12e (reference %.12e, rel err %.3e); beta %.3e cov %.3e alpha~ %.3e of the rtol 1e-6 + atol 1e-8 "
          "criterion; gradient max |err| = %.3e of largest component %.3e (%.2e relative); cond(A) = %.2e"
          % (tag, lml, r["lml"], abs(lml - r["lml"]) / abs(r["lml"]), crit(beta, r["beta"]), crit(cov, r["cov"]),
             crit(at, r["alpha"]), np.abs(grad - r["grad"]).max(), scale, np.abs(grad - r["grad"]).max() / scale,
             r["condA"]))
    for m, (mu, sigma) in zip(ms, outs):
        print("%s: m = %d: mu %.3e sigma %.3e of the criterion" % (tag, m, crit(mu, r["mu"][:m]), crit(sigma, r["sigma"][:m])))
    assert beta.shape == r["beta"].shape and cov.shape == r["cov"].shape and at.shape == r["alpha"].shape
    assert grad.shape == r["grad"].shape
    assert abs(lml - r["lml"]) <= 1e-8 * abs(r["lml"]), (tag, lml, r["lml"])
    np.testing.assert_allclose(beta, r["beta"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(cov, r["cov"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(at, r["alpha"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    assert np.abs(grad - r["grad"]).max() <= 1e-6 * scale, (tag, grad, r["grad"])
    for m, (mu, sigma) in zip(ms, outs):
        assert mu.shape == (m,) and sigma.shape == (m,)
        np.testing.assert_allclose(mu, r["mu"][:m], rtol=1e-6, atol=1e-8, err_msg=str((tag, m)))
        np.testing.assert_allclose(sigma, r["sigma"][:m], rtol=1e-6, atol=1e-8, err_msg=str((tag, m)))
    again = _calls(g, r, ms)
    assert again[0] == lml
    for u, v in zip(again[1:5], (beta, cov, at, grad)):
        np.testing.assert_array_equal(u, v)
    for (mu2, sigma2), (mu, sigma) in zip(again[5], outs):
        np.testing.assert_array_equal(mu2, mu)
        np.testing.assert_array_equal(sigma2, sigma)
    return lml, beta, cov, at, grad, outs


@pytest.mark.parametrize("state", ["absorb", "observe"])
@pytest.mark.parametrize("n,p", BR.SHAPES)
def test_shapes(n, p, state):
    r = BR.case(BR.SHAPE_FAMILY, n, p)
    g = _gp(BR.SHAPE_FAMILY)
    _fit(g, r, state)
    g.SetBasis(r["H"])
    _check(g, r, (n, p, state))
    g.close()


@pytest.mark.parametrize("p", BR.COUNTS)
def test_column_counts(p):
    r = BR.case(BR.SHAPE_FAMILY, 300, p)
    g = _gp(BR.SHAPE_FAMILY)
    _fit(g, r, "observe")
    g.SetBasis(r["H"])
    _check(g, r, ("p", p))
    g.close()


@pytest.mark.parametrize("fam", sorted(BR.FAMILIES))
def test_kernel_families(fam):
    r = BR.case(fam, 300, 3)
    g = _gp(fam)
    _fit(g, r, "observe")
    g.SetBasis(r["H"])
    _check(g, r, fam)
    g.close()


def test_events():
    fam = BR.EVENT_FAMILY
    simil = BR.FAMILIES[fam][1]
    r, plain = BR.case(fam, 300, 3, True), BR.case(fam, 300, 3)
    assert abs(r["lml"] - plain["lml"]) > 1e-3  # the discounts change the LML ...
    assert np.abs(r["grad"] - plain["grad"]).max() > 1e-3 * np.abs(plain["grad"]).max()  # ... and the gradient
    g = _gp(fam, simil=kernel.Events(simil, BR.EVENTS, 0))
    _fit(g, r, "observe")
    g.SetBasis(r["H"])
    _check(g, r, "events")
    g.close()


def _modes(g):
    _, _, _, tag = g.profile_read_launches()
    return tag // 100000000  # common.h: GemmMode; 2 = GEMM_LAUUM, the product K^-1 = Y Y^T


@pytest.mark.parametrize("n,p", [(300, 33), (1100, 64)])
def test_both_routes_to_w_agree(n, p):
    """W from the factor (option basis_symm = 0) and from the explicit K^-1 (1), each against the reference; after
    Absorb alone BasisProduce takes the factor's route and launches no inverse: the launch record holds no
    K^-1 = Y Y^T product (mode 2), and does once the option forces the symmetric product."""
    r = BR.case(BR.SHAPE_FAMILY, n, p)
    res = {}
    for route in (0, 1):
        g = _gp(BR.SHAPE_FAMILY)
        g.set_option("basis_symm", route)
        _fit(g, r, "observe")
        g.SetBasis(r["H"])
        res[route] = _check(g, r, (n, p, "basis_symm", route), ms=(70,))
        g.close()
    a, b = res[0], res[1]
    print("routes: lml %.15e / %.15e; beta max |diff| %.3e; alpha~ max |diff| %.3e"
          % (a[0], b[0], np.abs(a[1] - b[1]).max(), np.abs(a[3] - b[3]).max()))
    assert abs(a[0] - b[0]) <= 1e-8 * abs(b[0])
    np.testing.assert_allclose(a[1], b[1], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-6, atol=1e-8)
    assert np.abs(a[4] - b[4]).max() <= 1e-6 * np.abs(b[4]).max()
    g = _gp(BR.SHAPE_FAMILY)
    _fit(g, r, "absorb")
    g.SetBasis(r["H"])
    g.profile_enable(True)
    mu, sigma = g.BasisProduce(r["Z"][:70], r["Hz"][:70])
    modes = _modes(g)
    assert len(modes) > 0 and not (modes == 2).any(), modes
    np.testing.assert_allclose(mu, r["mu"][:70], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(sigma, r["sigma"][:70], rtol=1e-6, atol=1e-8)
    g.profile_read()  # resets the record
    g.set_option("basis_symm", 1)
    mu1, sigma1 = g.BasisProduce(r["Z"][:70], r["Hz"][:70])
    assert (_modes(g) == 2).any()
    g.profile_enable(False)
    np.testing.assert_allclose(mu1, r["mu"][:70], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(sigma1, r["sigma"][:70], rtol=1e-6, atol=1e-8)
    g.close()


def test_the_forecast_returns_to_the_estimated_level():
    """p = 1, a constant column, data with a large offset: far from the data Produce falls back to 0, BasisProduce to
    beta, with the deviation of the prior widened by beta's"""
    fam = "matern52"
    D, simil, ts = BR.FAMILIES[fam]
    X, y, _ = BR.inputs(129, 1, D)
    y = y + 1000.0
    H = basis.polynomial(X, 0)
    lt = BR.log_theta(fam)
    K, d = BR.reference(D, simil, lt, X, y, H)
    Z = np.array([[60.0] * D, [-75.0] * D])
    Hz = basis.polynomial(Z, 0)
    g = _gp(fam)
    g.Absorb(X, y)
    g.SetBasis(H)
    beta, cov = g.BasisBeta()
    mu, sigma = g.BasisProduce(Z, Hz)
    mu0, sigma0 = g.Produce(Z)
    print("level: beta %.9f (reference %.9f, mean of y %.6f); far forecast %s (zero-mean: %s); sigma %s (zero-mean %s)"
          % (beta[0], d["beta"][0], y.mean(), mu, mu0, sigma, sigma0))
    np.testing.assert_allclose(beta, d["beta"], rtol=1e-6, atol=1e-8)
    assert abs(beta[0] - 1000.0) < 3.0  # the level, up to the process's own spread
    assert np.abs(mu0).max() < 1e-6
    np.testing.assert_allclose(mu, beta[0], rtol=1e-9)
    np.testing.assert_allclose(sigma, np.sqrt(sigma0 ** 2 + cov[0, 0]), rtol=1e-9)
    g.close()


@pytest.mark.parametrize("state", ["absorb", "observe"])
def test_handle_is_left_as_found(state):
    """One of two twins makes every basis call; Observe, Gradient, Produce, L, Alpha, LOOScore, MultiLML and a following
    Append + Produce are bit-equal between them."""
    fam, n = BR.SHAPE_FAMILY, 300
    D = BR.FAMILIES[fam][0]
    r = BR.case(fam, n, 5)
    Z = r["Z"][:33]
    X2, y2, _ = BR.inputs(5, 1, D, seed=11)
    Y = np.stack([r["y"], r["y"] ** 2], axis=1)

    def run(with_basis):
        g = _gp(fam)
        _fit(g, r, state)
        if with_basis:
            g.SetBasis(r["H"])
            _calls(g, r, (33, 200))
        out = (g.Gradient(),) if state == "observe" else ()
        out += (*g.Produce(Z), g.L, g.Alpha, np.array([g.LOOScore(), g.LML()]))
        g.SetOutputs(Y)
        out += (np.array(g.MultiLML()[0]), g.MultiLML()[1], g.MultiGradient())
        if with_basis:
            g.BasisGradient()
        out += (np.array(g.Observe(r["lt"] + 0.1)), g.Gradient())
        if with_basis:
            g.BasisLML()
        g.Append(X2, y2)
        out += (g.L, g.Alpha, *g.Produce(Z))
        g.close()
        return out

    for u, v in zip(run(False), run(True)):
        np.testing.assert_array_equal(u, v)


def test_lifecycle_and_refusals():
    from gogp_amd.gp import GP, GogpError
    fam = BR.SHAPE_FAMILY
    D, simil, ts = BR.FAMILIES[fam]
    r = BR.case(fam, 300, 5)
    X, y, H = r["X"], r["y"], r["H"]
    n, p, P = 300, 5, len(ts) + 1
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    lml, grad, beta, at = ctypes.c_double(0.0), np.zeros(P), np.zeros(64), np.zeros(400)
    mu, Z, Hz = np.zeros(3), np.ascontiguousarray(r["Z"][:3]), np.ascontiguousarray(r["Hz"][:3])

    def five(h):
        return (L.gogp_basis_lml(h, ctypes.byref(lml)), L.gogp_basis_gradient(h, dp(grad), P),
                L.gogp_basis_get_beta(h, dp(beta), None), L.gogp_basis_get_alpha(h, dp(at)),
                L.gogp_basis_produce(h, dp(Z), dp(Hz), 3, dp(mu), None))

    g = _gp(fam)
    assert L.gogp_basis_set(g._h, dp(H), n, p) == _lib.GOGP_ESTATE  # no data
    g.Absorb(X, y)
    assert five(g._h) == (_lib.GOGP_ESTATE,) * 5  # factored, but no basis
    for args in ((dp(H), 299, p), (dp(H), n, 0), (dp(H), n, 65), (None, n, p)):
        assert L.gogp_basis_set(g._h, *args) == _lib.GOGP_EARG, args[1:]
    bad = H.copy()
    bad[17, 2] = np.inf
    assert L.gogp_basis_set(g._h, dp(bad), n, p) == _lib.GOGP_EARG
    assert five(g._h) == (_lib.GOGP_ESTATE,) * 5  # a refused set sets nothing
    g.SetBasis(H)
    assert L.gogp_basis_gradient(g._h, dp(grad), P + 1) == _lib.GOGP_EARG
    assert L.gogp_basis_produce(g._h, None, None, 0, None, None) == _lib.GOGP_OK  # m = 0
    badz = Hz.copy()
    badz[1, 1] = np.nan
    assert L.gogp_basis_produce(g._h, dp(Z), dp(badz), 3, dp(mu), None) == _lib.GOGP_EARG
    _check(g, r, "after Absorb", ms=(3,))
    # a duplicated column: A is singular
    dup = H.copy()
    dup[:, 4] = dup[:, 1]
    g.SetBasis(dup)
    with pytest.raises(GogpError) as e:
        g.BasisLML()
    print("duplicated column:", e.value)
    assert e.value.code == _lib.GOGP_ECOND and "basis" in str(e.value)
    assert L.gogp_basis_get_beta(g._h, dp(beta), None) == _lib.GOGP_ECOND
    g.SetBasis(H)
    _check(g, r, "a good basis after a dependent one", ms=(3,))
    g.SetBasis(None)  # cleared
    assert five(g._h) == (_lib.GOGP_ESTATE,) * 5
    # n <= p
    small = _gp(fam)
    small.Absorb(X[:5], y[:5])
    assert L.gogp_basis_set(small._h, dp(np.ascontiguousarray(H[:5])), 5, 5) == _lib.GOGP_EARG
    assert L.gogp_basis_set(small._h, dp(np.ascontiguousarray(H[:5, :4])), 5, 4) == _lib.GOGP_OK
    small.close()
    # a basis set before anything is factored: ESTATE until a factorisation; it follows a new theta
    h = _gp(fam)
    h.X, h.Y = X, y
    h.SetBasis(H)
    assert five(h._h) == (_lib.GOGP_ESTATE,) * 5
    h.Observe(r["lt"])
    _check(h, r, "basis first, then Observe", ms=(3,))
    x2 = r["lt"] + 0.2
    h.Observe(x2)
    K2, d2 = BR.reference(D, simil, x2, X, y, H)
    Ks2, prior2 = BR.cross(D, simil, x2, X, r["Z"])
    mu2, sigma2, _, _ = BR.produce_dense(K2, Ks2, prior2, d2, r["Hz"])
    _check(h, dict(r, **d2, mu=mu2, sigma=sigma2), "another theta", ms=(3,))
    # dropped by Append, Remove, set_data and the full Observe form; usable again after a new SetBasis
    X2, y2, _ = BR.inputs(5, 1, D, seed=11)
    h.Append(X2, y2 + 25.0)
    assert five(h._h) == (_lib.GOGP_ESTATE,) * 5
    Xa, ya = np.concatenate([X, X2]), np.concatenate([y, y2 + 25.0])
    c, s = basis.polynomial_frame(X, [0, 1])
    Ha = basis.polynomial(Xa, 2, [0, 1], c, s)
    h.SetBasis(Ha)
    Ka, da = BR.reference(D, simil, x2, Xa, ya, Ha)
    Ksa, _ = BR.cross(D, simil, x2, Xa, r["Z"])
    mua, sigmaa, _, _ = BR.produce_dense(Ka, Ksa, prior2, da, r["Hz"])
    _check(h, dict(r, **da, mu=mua, sigma=sigmaa), "after Append", ms=(3,))
    h.Remove([0, 7])
    assert five(h._h) == (_lib.GOGP_ESTATE,) * 5
    keep = np.ones(len(ya), dtype=bool)
    keep[[0, 7]] = False
    h.SetBasis(Ha[keep])
    Kr, dr = BR.reference(D, simil, x2, Xa[keep], ya[keep], Ha[keep])
    Ksr, _ = BR.cross(D, simil, x2, Xa[keep], r["Z"])
    mur, sigmar, _, _ = BR.produce_dense(Kr, Ksr, prior2, dr, r["Hz"])
    _check(h, dict(r, **dr, mu=mur, sigma=sigmar), "after Remove", ms=(3,))
    h.Absorb(X, y)  # set_data (at the parameters of the last Observe)
    assert five(h._h) == (_lib.GOGP_ESTATE,) * 5
    h.SetBasis(H)
    _check(h, dict(r, **d2, mu=mu2, sigma=sigma2), "after set_data", ms=(3,))
    h.Observe(np.concatenate([r["lt"], X.ravel(), y]))  # the full Observe form: drops the basis, and refuses the gradient
    assert five(h._h) == (_lib.GOGP_ESTATE,) * 5
    h.SetBasis(H)
    got = five(h._h)
    assert got == (_lib.GOGP_OK, _lib.GOGP_EARG, _lib.GOGP_OK, _lib.GOGP_OK, _lib.GOGP_OK), got
    assert abs(lml.value - r["lml"]) <= 1e-8 * abs(r["lml"])
    h.close()
    # gradient_precision = 32: K^-1 is float
    g.SetBasis(H)
    g.set_option("gradient_precision", 32)
    g.Observe(r["lt"])
    assert five(g._h) == (_lib.GOGP_EARG,) * 5
    with pytest.raises(GogpError) as e:
        g.BasisLML()
    assert e.value.code == _lib.GOGP_EARG and "gradient_precision = 32" in str(e.value)
    g.close()
    g32 = GP(D, simil, BR.NOISE, ThetaSimil=ts, ThetaNoise=BR.TN, device=0, precision=32)
    g32.Absorb(X, y)
    assert L.gogp_basis_set(g32._h, dp(H), n, p) == _lib.GOGP_EARG
    assert five(g32._h) == (_lib.GOGP_EARG,) * 5
    g32.close()


def test_sharded_handles_are_refused():
    import loopback
    from gogp_amd.sharded import ShardedGP
    fam = BR.SHAPE_FAMILY
    D, simil, ts = BR.FAMILIES[fam]
    H = BR.case(fam, 300, 5)["H"]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def rank_fn(r, lb):
        sh = ShardedGP(D, simil, BR.NOISE, device=0, grid=(1, 2), rank=r, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        L = _lib.lib()
        v, grad = ctypes.c_double(), np.zeros(len(ts) + 1)
        rcs, msgs = [], []
        for call in (lambda: L.gogp_basis_set(sh._h, dp(H), 300, 5), lambda: L.gogp_basis_lml(sh._h, ctypes.byref(v)),
                     lambda: L.gogp_basis_gradient(sh._h, dp(grad), grad.size)):
            rcs.append(call())
            msgs.append(L.gogp_last_error(sh._h))
        sh.close()  # the handle still closes cleanly
        return rcs, msgs

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rcs, msgs in outs:
        assert rcs == [_lib.GOGP_EARG] * 3
        assert all(b"sharded" in m for m in msgs), msgs


# ---- BasisModel -----------------------------------------------------------------------------------------------------------
def test_optimiser_on_the_basis_objective():
    from gogp_amd.gp import GP, BasisModel
    n, D, threshold = 200, 2, 1e-3
    X, y = synth.make_inputs(n, D, 5)
    c, s = basis.polynomial_frame(X)
    H = basis.polynomial(X, 1, None, c, s)
    y = y + 40.0 + H @ np.array([0.0, 3.0, -2.0])
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, BR.NOISE, X=X, Y=y, device=0)
    g.SetBasis(H)
    m = BasisModel(g)
    x0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    start = m.Observe(x0)
    res = optimize.lbfgs(m, x0, gradient_threshold=threshold)
    K, d = BR.reference(D, simil, res.x, X, y, H)
    print("basis objective: start %.9f, end %.9f (reference %.9f) after %d iterations, %d evaluations; theta = %s; beta = %s"
          % (start, res.lml, d["lml"], res.iterations, res.evaluations, np.exp(res.x), g.BasisBeta()[0]))
    assert res.lml >= start
    assert abs(res.lml - d["lml"]) <= 1e-8 * abs(d["lml"])
    # the gradient at the end against central differences of the reference
    m.Observe(res.x)
    grad = m.Gradient()
    fd, hstep = np.zeros_like(res.x), 1e-5
    for k in range(len(res.x)):
        e = np.zeros_like(res.x)
        e[k] = hstep
        fd[k] = (BR.reference(D, simil, res.x + e, X, y, H, want_grad=False)[1]["lml"]
                 - BR.reference(D, simil, res.x - e, X, y, H, want_grad=False)[1]["lml"]) / (2 * hstep)
    # At the optimum the two halves of every component, 1/2 tr((alpha~ alpha~^T + Q Q^T) dK_p) and 1/2 tr(K^-1 dK_p),
    # cancel: the error of their difference is measured against the size of the halves (the suite's 1e-6 of the
    # largest component, taken over the terms instead of their vanishing sum).
    import loo_ref as LR
    Kd, dK = LR.gram(D, simil, res.x, X, want_grad=True)
    Kinv = np.linalg.inv(Kd)
    scale = max(0.5 * abs((Kinv * dk).sum()) for dk in dK)
    print("at the end: gradient %s, central differences %s, reference %s; size of the cancelling halves %.3e"
          % (grad, fd, d["grad"], scale))
    assert np.abs(grad).max() <= 10 * threshold * max(1.0, abs(res.lml))  # the optimiser stopped near a stationary point
    assert np.abs(grad - d["grad"]).max() <= 1e-6 * scale
    assert np.abs(grad - fd).max() <= 1e-6 * scale
    with pytest.raises(ValueError):
        m.Observe(np.concatenate([res.x, [0.0]]))
    g.close()
