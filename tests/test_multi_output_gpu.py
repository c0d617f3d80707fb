"""GP.SetOutputs / MultiLML / MultiGradient / MultiAlpha / MultiProduce (gogp_multi_*) on the GPU against the dense
reference of tests/multi_output_ref.py (numpy Cholesky in fp64; tests/test_multi_output_cpu.py pins it to the oracle
column by column and to central differences), and multi_weight_kernel in isolation through its test hook.

Tolerances (the header of tests/test_gpu_parity.py): LML <= 1e-8 relative; alpha, mu, sigma rtol = 1e-6, atol = 1e-8;
every component of the gradient within 1e-6 of the largest absolute component.  The inputs keep the reference far inside
that: prior variances 0.9 - 2.3 and noise variance 0.09 with n <= 1100 give cond(K) <~ (1100 * 2.3 + 0.09) / 0.09 ~ 3e4, so
the dense solves carry ~3e4 * 2.2e-16 ~ 1e-11 relative (as argued in tests/test_loo_gpu.py).

The kernel in isolation: integer-valued A^T in [-8, 8] and an integer symmetric Kinv in [-1000, 1000] -- T Kinv - A A^T is
at most 128 * 1000 + 128 * 64 in magnitude and every partial sum an integer below 2^53: exact in fp64 whatever the order,
so the comparison is assert_array_equal.  With normal deviates each of the T products rounds once (fused multiply-add
on the matrix core) at a partial sum of size <~ a few * sqrt(T): 1e-12 per unit of K = T is the bound
tests/test_tile_kernels.py::test_dgemm_tile_kernel holds the tile kernel to.

Shapes (TILE = 128, PANEL = 256; the weight pass and the reduction work on 64 x 64 tiles): n = 1 one observation; 20 the
one-launch `tiny` path; 128 its limit; 129 the first size on the general sweep; 300 two ragged panels; 1100 npad = 1280:
off-diagonal tile pairs.  T = 1, 3 (padded to 4), 4, 33 (a second LDS pass of one step), 128 (the limit).

Reference counterpart: none (gp.GP holds one output vector)."""
import ctypes

import numpy as np
import pytest

import multi_output_ref as MR
from gogp_amd import _lib, kernel, optimize, synth

pytestmark = pytest.mark.gpu

SHAPE_FAMILY = "ard_rbf3"
SHAPES = (1, 20, 128, 129, 300, 1100)
MS = (1, 70, 200)
RADIAL = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8]),
    "matern52": (2, kernel.Scaled(kernel.Matern52), [1.2, 0.9]),
    "matern52textbook": (2, kernel.Scaled(kernel.Matern52Textbook), [0.9, 1.1]),
}
FAMILIES = dict(MR.FAMILIES, **RADIAL)
_REF = {}
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


# ---- multi_weight_kernel in isolation ---------------------------------------------------------------------------------
def _weight_case(gpm, n, npad, T, At, Kl, tol=None, tag=""):
    """At: T x npad; Kl: n x n symmetric.  Kinv handed in: Kl on j <= i < n, NaN elsewhere; G preset to a sentinel."""
    ld = npad
    Kinv = np.full((npad, ld), np.nan)
    Kinv[:n, :n] = np.where(np.tril(np.ones((n, n), bool)), Kl, np.nan)
    G0 = np.full((npad, ld), SENTINEL)
    G = gpm.multi_weight_check(np.ascontiguousarray(At), npad, T, Kinv, ld, n, npad, G0).reshape(npad, ld)
    assert not np.isnan(G).any(), tag
    A = At[:, :n].T
    want = T * Kl - A @ A.T
    low = np.tril(np.ones((n, n), bool))
    if tol is None:
        np.testing.assert_array_equal(G[:n, :n][low], want[low], err_msg=str(tag))
    else:
        err = np.abs(G[:n, :n][low] - want[low]).max()
        print("%s: max |err| = %.3e, bound %.3e" % (tag, err, tol))
        assert err <= tol, (tag, err, tol)
    # the lower 64 x 64 tiles: everything but j <= i < n is an exact zero; outside them the sentinel is untouched
    i, j = np.indices((npad, ld))
    tiles = (j // 64) <= (i // 64)
    live = (j <= i) & (i < n)
    rest = G[tiles & ~live]
    assert rest.size == 0 or (not rest.any() and not np.signbit(rest).any()), tag
    np.testing.assert_array_equal(G[~tiles], SENTINEL, err_msg=str(tag))


def _int_inputs(n, npad, T, seed):
    rng = np.random.default_rng(seed)
    At = np.zeros((T, npad))
    At[:, :n] = rng.integers(-8, 9, (T, n)).astype(float)
    At[:, n:] = 7.0  # columns >= n of A^T must not reach j <= i < n (the product keeps zeros there)
    Kl = rng.integers(-1000, 1001, (n, n)).astype(float)
    Kl = np.tril(Kl) + np.tril(Kl, -1).T
    return At, Kl


@pytest.mark.parametrize("n,npad,T", [(1, 256, 1), (64, 256, 3), (65, 256, 4), (129, 256, 5), (300, 512, 33),
                                      (1100, 1280, 128)])
def test_weight_kernel_exact(gpm, n, npad, T):
    At, Kl = _int_inputs(n, npad, T, 100 + n + T)
    _weight_case(gpm, n, npad, T, At, Kl, tag=(n, npad, T))


def test_weight_kernel_fragment_layout_asymmetric(gpm):
    """Columns of A with one or two non-zero entries each, placed asymmetrically over the tile pairs: A A^T has a handful
    of non-zero elements that a transposed fragment map moves, and Kinv[i][j] = 1000 i + j (j <= i) tells a transposed
    epilogue apart."""
    n, npad, T = 200, 256, 8
    At = np.zeros((T, npad))
    hits = [(0, 3), (1, 70), (2, 3), (2, 150), (3, 199), (4, 64), (5, 65), (5, 1), (6, 130), (7, 17), (7, 180)]
    for t, i in hits:
        At[t, i] = 1.0 + t  # (A A^T)[i][j] = sum_t At[t][i] At[t][j]: off the diagonal only (150, 3), (65, 1), (180, 17)
    i, j = np.indices((n, n))
    Kl = np.where(j <= i, 1000.0 * i + j, 1000.0 * j + i)
    _weight_case(gpm, n, npad, T, At, Kl, tag="unit columns")


def test_weight_kernel_normal_deviates(gpm):
    n, npad, T = 300, 512, 33
    rng = np.random.default_rng(5)
    At = np.zeros((T, npad))
    At[:, :n] = rng.normal(size=(T, n))
    Kl = rng.normal(size=(n, n))
    Kl = np.tril(Kl) + np.tril(Kl, -1).T
    _weight_case(gpm, n, npad, T, At, Kl, tol=1e-12 * T, tag="normal deviates")


# ---- the calls against the dense reference ----------------------------------------------------------------------------
def _x(fam):
    return np.log(np.array(list(FAMILIES[fam][2]) + MR.TN))


def _ref(fam, n, T, events=None):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, n, T, bool(events))
    if key not in _REF:
        D, simil, _ = FAMILIES[fam]
        X, y, _ = MR.inputs(n, 1, D)
        Z = MR.inputs(1, max(MS), D)[2]
        Y = MR.outputs(X, T, y)
        A, lml, grad = MR.reference(D, simil, _x(fam), X, Y, events)
        mu, sigma = MR.produce(D, simil, _x(fam), X, A, Z, events)
        _REF[key] = dict(X=X, y=y, Y=Y, Z=Z, A=A, lml=lml, grad=grad, mu=mu, sigma=sigma)
    return _REF[key]


def _gp(fam, simil=None, **kw):
    from gogp_amd.gp import GP
    D, s, ts = FAMILIES[fam]
    return GP(D, simil or s, MR.NOISE, ThetaSimil=ts, ThetaNoise=MR.TN, device=0, **kw)


def _fit(g, fam, X, y, state):
    if state == "absorb":
        g.Absorb(X, y)
    else:
        g.X, g.Y = X, y
        g.Observe(_x(fam))


def _check(g, r, tag, ms=MS):
    """Every multi call against the reference, every figure printed first; a second call: the same bits"""
    total, lml = g.MultiLML()
    A = g.MultiAlpha
    grad = g.MultiGradient()
    crit = lambda a, b: (np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))).max() if b.size else 0.0  # noqa: E731
    scale = np.abs(r["grad"]).max()
    print("%s: lml max rel err %.3e; total %.12e (reference %.12e); alpha %.3e of the rtol 1e-6 + atol 1e-8 criterion; "
          "gradient max |err| = %.3e of largest component %.3e (%.2e relative)"
          % (tag, (np.abs(lml - r["lml"]) / np.abs(r["lml"])).max(), total, r["lml"].sum(), crit(A, r["A"]),
             np.abs(grad - r["grad"]).max(), scale, np.abs(grad - r["grad"]).max() / scale))
    outs = []
    for m in ms:
        mu, sigma = g.MultiProduce(r["Z"][:m])
        print("%s: m = %d: mu %.3e sigma %.3e of the criterion" % (tag, m, crit(mu, r["mu"][:m]), crit(sigma, r["sigma"][:m])))
        outs.append((mu, sigma))
    assert lml.shape == r["lml"].shape and A.shape == r["A"].shape and grad.shape == r["grad"].shape
    assert (np.abs(lml - r["lml"]) <= 1e-8 * np.abs(r["lml"])).all(), (tag, lml, r["lml"])
    assert abs(total - r["lml"].sum()) <= 1e-8 * np.abs(r["lml"]).sum(), (tag, total)
    np.testing.assert_allclose(A, r["A"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    assert np.abs(grad - r["grad"]).max() <= 1e-6 * scale, (tag, grad, r["grad"])
    for m, (mu, sigma) in zip(ms, outs):
        assert mu.shape == (m, r["A"].shape[1]) and sigma.shape == (m,)
        np.testing.assert_allclose(mu, r["mu"][:m], rtol=1e-6, atol=1e-8, err_msg=str((tag, m)))
        np.testing.assert_allclose(sigma, r["sigma"][:m], rtol=1e-6, atol=1e-8, err_msg=str((tag, m)))
    # a second call: the same bits
    total2, lml2 = g.MultiLML()
    assert total2 == total
    np.testing.assert_array_equal(lml2, lml)
    np.testing.assert_array_equal(g.MultiAlpha, A)
    np.testing.assert_array_equal(g.MultiGradient(), grad)
    for m, (mu, sigma) in zip(ms, outs):
        mu2, sigma2 = g.MultiProduce(r["Z"][:m])
        np.testing.assert_array_equal(mu2, mu)
        np.testing.assert_array_equal(sigma2, sigma)
    return total, lml, A, grad, outs


@pytest.mark.parametrize("state", ["absorb", "observe"])
@pytest.mark.parametrize("n", SHAPES)
def test_shapes(n, state):
    r = _ref(SHAPE_FAMILY, n, 5)
    g = _gp(SHAPE_FAMILY)
    _fit(g, SHAPE_FAMILY, r["X"], r["y"], state)
    g.SetOutputs(r["Y"])
    _check(g, r, (n, state))
    g.close()


@pytest.mark.parametrize("T", [1, 3, 4, 33, 128])
def test_output_counts(T):
    r = _ref(SHAPE_FAMILY, 300, T)
    g = _gp(SHAPE_FAMILY)
    _fit(g, SHAPE_FAMILY, r["X"], r["y"], "observe")
    g.SetOutputs(r["Y"])
    _check(g, r, ("T", T))
    g.close()


@pytest.mark.parametrize("fam", sorted(RADIAL) + ["ard_rbf64", "hyperpriors"])
def test_kernel_families(fam):
    r = _ref(fam, 300, 3)
    g = _gp(fam)
    _fit(g, fam, r["X"], r["y"], "observe")
    g.SetOutputs(r["Y"])
    _check(g, r, fam)
    g.close()


def test_events():
    fam = "matern52"
    D, simil, ts = FAMILIES[fam]
    r, plain = _ref(fam, 300, 3, MR.EVENTS), _ref(fam, 300, 3)
    assert np.abs(r["lml"] - plain["lml"]).max() > 1e-3  # the discounts change the LML ...
    assert np.abs(r["grad"] - plain["grad"]).max() > 1e-3 * np.abs(plain["grad"]).max()  # ... and the gradient
    g = _gp(fam, simil=kernel.Events(simil, MR.EVENTS, 0))
    _fit(g, fam, r["X"], r["y"], "observe")
    g.SetOutputs(r["Y"])
    _check(g, r, "events")
    g.close()


@pytest.mark.parametrize("n", [300, 1100])
def test_against_the_single_output_path(n):
    """Column t through the multi calls = a handle holding column t through Observe / Alpha / Produce / Gradient"""
    fam, T = SHAPE_FAMILY, 3
    r = _ref(fam, n, T)
    Z = r["Z"][:70]
    g = _gp(fam)
    _fit(g, fam, r["X"], r["y"], "observe")
    g.SetOutputs(r["Y"])
    total, lml = g.MultiLML()
    A, grad, (mu, sigma) = g.MultiAlpha, g.MultiGradient(), g.MultiProduce(Z)
    print("n = %d: lml[0] %.15e, GP.LML() %.15e" % (n, lml[0], g.LML()))
    assert abs(lml[0] - g.LML()) <= 1e-8 * abs(g.LML())
    gsum = np.zeros_like(grad)
    for t in range(T):
        s = _gp(fam)
        s.X, s.Y = r["X"], r["Y"][:, t].copy()
        l = s.Observe(_x(fam))
        gsum += s.Gradient()
        mu_t, sigma_t = s.Produce(Z)
        print("n = %d column %d: lml %.15e single %.15e; alpha max |diff| %.3e; mu max |diff| %.3e"
              % (n, t, lml[t], l, np.abs(A[:, t] - s.Alpha).max(), np.abs(mu[:, t] - mu_t).max()))
        assert abs(lml[t] - l) <= 1e-8 * abs(l)
        np.testing.assert_allclose(A[:, t], s.Alpha, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(mu[:, t], mu_t, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(sigma, sigma_t, rtol=1e-6, atol=1e-8)
        s.close()
    print("n = %d: gradient max |diff| %.3e of %.3e" % (n, np.abs(grad - gsum).max(), np.abs(gsum).max()))
    assert np.abs(grad - gsum).max() <= 1e-6 * np.abs(gsum).max()
    g.close()


@pytest.mark.parametrize("state", ["absorb", "observe"])
def test_handle_is_left_as_found(state):
    """One of two twins makes every multi call; Gradient, Produce, L, LOOScore and a following Append + Produce are
    bit-equal between them.  After Absorb K^-1 is formed lazily (by MultiGradient here, by LOOScore on the twin)."""
    fam, n = SHAPE_FAMILY, 300
    D = FAMILIES[fam][0]
    r = _ref(fam, n, 5)
    Z = r["Z"][:33]
    X2, y2, _ = MR.inputs(5, 1, D, seed=11)

    def run(multi):
        g = _gp(fam)
        _fit(g, fam, r["X"], r["y"], state)
        if multi:
            g.SetOutputs(r["Y"])
            g.MultiLML()
            g.MultiGradient()
            g.MultiAlpha
            g.MultiProduce(Z)
            g.MultiProduce(r["Z"][:200])
        out = (g.Gradient(),) if state == "observe" else ()
        out += (*g.Produce(Z), g.L, g.Alpha, np.array([g.LOOScore(), g.LML()]))
        if multi:
            g.MultiGradient()
        g.Append(X2, y2)
        out += (g.L, g.Alpha, *g.Produce(Z))
        g.close()
        return out

    for u, v in zip(run(False), run(True)):
        np.testing.assert_array_equal(u, v)


def test_lifecycle_and_refusals():
    from gogp_amd.gp import GP, GogpError
    fam = SHAPE_FAMILY
    D, simil, ts = FAMILIES[fam]
    r = _ref(fam, 300, 5)
    X, y, Y = r["X"], r["y"], r["Y"]
    P = len(ts) + 1
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    total, grad, A = ctypes.c_double(0.0), np.zeros(P), np.zeros((300, 5))
    mu, Z = np.zeros((3, 5)), np.ascontiguousarray(r["Z"][:3])

    def four(h):
        return (L.gogp_multi_lml(h, ctypes.byref(total), None), L.gogp_multi_gradient(h, dp(grad), P),
                L.gogp_multi_get_alpha(h, dp(A)), L.gogp_multi_produce(h, dp(Z), 3, dp(mu), None))

    g = _gp(fam)
    assert L.gogp_multi_set_outputs(g._h, dp(Y), 300, 5) == _lib.GOGP_ESTATE  # no data
    g.Absorb(X, y)
    assert four(g._h) == (_lib.GOGP_ESTATE,) * 4  # factored, but no outputs
    for args in ((dp(Y), 299, 5), (dp(Y), 300, 0), (dp(Y), 300, 129), (None, 300, 5)):
        assert L.gogp_multi_set_outputs(g._h, *args) == _lib.GOGP_EARG, args[1:]
    bad = Y.copy()
    bad[17, 2] = np.nan
    assert L.gogp_multi_set_outputs(g._h, dp(bad), 300, 5) == _lib.GOGP_EARG
    assert four(g._h) == (_lib.GOGP_ESTATE,) * 4  # a refused set_outputs sets nothing
    g.SetOutputs(Y)
    assert L.gogp_multi_gradient(g._h, dp(grad), P + 1) == _lib.GOGP_EARG
    assert L.gogp_multi_produce(g._h, None, 0, None, None) == _lib.GOGP_OK  # m = 0
    _check(g, r, "after Absorb", ms=(3,))
    g.SetOutputs(None)  # cleared
    assert four(g._h) == (_lib.GOGP_ESTATE,) * 4
    # outputs set before anything is factored: ESTATE until a factorisation
    h = _gp(fam)
    h.X, h.Y = X, y
    h.SetOutputs(Y)
    assert four(h._h) == (_lib.GOGP_ESTATE,) * 4
    h.Observe(_x(fam))
    _check(h, r, "outputs first, then Observe", ms=(3,))
    # the solutions follow a new Observe at another theta
    x2 = _x(fam) + 0.2
    h.Observe(x2)
    A2, lml2, grad2 = MR.reference(D, simil, x2, X, Y)
    mu2, sigma2 = MR.produce(D, simil, x2, X, A2, r["Z"])
    r2 = dict(r, A=A2, lml=lml2, grad=grad2, mu=mu2, sigma=sigma2)
    _check(h, r2, "another theta", ms=(3,))
    # dropped by Append, Remove, set_data and the full Observe form; usable again after a new SetOutputs
    X2, y2, _ = MR.inputs(5, 1, D, seed=11)
    h.Append(X2, y2)
    assert four(h._h) == (_lib.GOGP_ESTATE,) * 4
    Xa, ya = np.concatenate([X, X2]), np.concatenate([y, y2])
    Ya = MR.outputs(Xa, 5, ya, seed=9)
    h.SetOutputs(Ya)
    Aa, lmla, grada = MR.reference(D, simil, x2, Xa, Ya)
    mua, sigmaa = MR.produce(D, simil, x2, Xa, Aa, r["Z"])
    _check(h, dict(r, A=Aa, lml=lmla, grad=grada, mu=mua, sigma=sigmaa), "after Append", ms=(3,))
    h.Remove([0, 7])
    assert four(h._h) == (_lib.GOGP_ESTATE,) * 4
    keep = np.ones(len(ya), dtype=bool)
    keep[[0, 7]] = False
    h.SetOutputs(Ya[keep])
    Ar, lmlr, gradr = MR.reference(D, simil, x2, Xa[keep], Ya[keep])
    mur, sigmar = MR.produce(D, simil, x2, Xa[keep], Ar, r["Z"])
    _check(h, dict(r, A=Ar, lml=lmlr, grad=gradr, mu=mur, sigma=sigmar), "after Remove", ms=(3,))
    h.Absorb(X, y)  # set_data (at the parameters of the last Observe)
    assert four(h._h) == (_lib.GOGP_ESTATE,) * 4
    h.SetOutputs(Y)
    _check(h, r2, "after set_data", ms=(3,))
    h.Observe(np.concatenate([_x(fam), X.ravel(), y]))  # the full Observe form
    assert four(h._h) == (_lib.GOGP_ESTATE,) * 4
    h.SetOutputs(Y)
    _check(h, r, "after the full Observe form", ms=(3,))
    h.close()
    # gradient_precision = 32: K^-1 is float
    g.SetOutputs(Y)
    g.set_option("gradient_precision", 32)
    g.Observe(_x(fam))
    assert four(g._h) == (_lib.GOGP_EARG,) * 4
    with pytest.raises(GogpError) as e:
        g.MultiLML()
    assert e.value.code == _lib.GOGP_EARG and "gradient_precision = 32" in str(e.value)
    g.close()
    g32 = GP(D, simil, MR.NOISE, ThetaSimil=ts, ThetaNoise=MR.TN, device=0, precision=32)
    g32.Absorb(X, y)
    assert L.gogp_multi_set_outputs(g32._h, dp(Y), 300, 5) == _lib.GOGP_EARG
    assert four(g32._h) == (_lib.GOGP_EARG,) * 4
    g32.close()


def test_empty_process():
    fam = SHAPE_FAMILY
    D, simil, ts = FAMILIES[fam]
    g = _gp(fam)
    g.Absorb(np.zeros((0, D)), np.zeros(0))
    g.SetOutputs(np.zeros((0, 3)))
    total, lml = g.MultiLML()
    assert total == 0.0 and lml.shape == (3,) and not lml.any()
    grad = g.MultiGradient()
    assert grad.shape == (len(ts) + 1,) and not grad.any()
    assert g.MultiAlpha.shape == (0, 3)
    Z = MR.inputs(1, 4, D)[2]
    mu, sigma = g.MultiProduce(Z)
    assert mu.shape == (4, 3) and not mu.any()
    np.testing.assert_array_equal(sigma, g.Produce(Z)[1])  # the prior, as Produce returns it
    want = MR.produce(D, simil, _x(fam), np.zeros((0, D)), np.zeros((0, 3)), Z)[1]
    np.testing.assert_allclose(sigma, want, rtol=1e-6, atol=1e-8)
    g.close()


# ---- MultiModel ---------------------------------------------------------------------------------------------------------
def test_multi_model_is_the_sum_of_single_output_models():
    from gogp_amd.gp import GP, Model, MultiModel
    fam, T = "matern52", 3
    D, simil, ts = FAMILIES[fam]
    r = _ref(fam, 129, T)
    pri = optimize.NormalLogPriors(np.zeros(len(ts) + 1), np.ones(len(ts) + 1))
    g = GP(D, simil, MR.NOISE, X=r["X"], Y=r["y"], device=0)
    g.SetOutputs(r["Y"])
    m = MultiModel(g, pri)
    singles = [Model(GP(D, simil, MR.NOISE, X=r["X"], Y=r["Y"][:, t].copy(), device=0), pri) for t in range(T)]
    for dx in (0.0, 0.3, -0.25):
        x = _x(fam) + dx
        v, gr = m.Observe(x), m.Gradient()
        want_v = sum(s.Observe(x) for s in singles) - (T - 1) * pri.Observe(x)
        want_g = sum(s.Gradient() for s in singles) - (T - 1) * np.asarray(pri.Gradient())
        print("x + %.2f: value %.12e, want %.12e; gradient max |diff| %.3e of %.3e"
              % (dx, v, want_v, np.abs(gr - want_g).max(), np.abs(want_g).max()))
        assert abs(v - want_v) <= 1e-8 * abs(want_v)
        assert np.abs(gr - want_g).max() <= 1e-6 * np.abs(want_g).max()
    for s in singles:
        s.GP.close()
    g.close()


def test_optimiser_on_the_multi_output_objective():
    from gogp_amd.gp import GP, MultiModel
    n, D, T, threshold = 200, 2, 3, 1e-3
    X, y = synth.make_inputs(n, D, 5)
    Y = MR.outputs(X, T, y)
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, MR.NOISE, X=X, Y=y, device=0)
    g.SetOutputs(Y)
    m = MultiModel(g)
    x0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    start = m.Observe(x0)
    res = optimize.lbfgs(m, x0, gradient_threshold=threshold)
    want = MR.reference(D, simil, res.x, X, Y)
    print("multi-output objective: start %.9f, end %.9f (reference %.9f) after %d iterations, %d evaluations; theta = %s"
          % (start, res.lml, want[1].sum(), res.iterations, res.evaluations, np.exp(res.x)))
    assert res.lml >= start
    assert abs(res.lml - want[1].sum()) <= 1e-8 * abs(want[1].sum())
    g.close()
