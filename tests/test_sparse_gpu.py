"""GP.SetSparse / SparseObserve / SparseGradient / SparseProduce (gogp_sparse_*) on the GPU against the numpy reference
of tests/sparse_ref.py (tests/test_sparse_cpu.py pins it to the oracle, to the unwhitened form and to central
differences), and the two new kernels in isolation through their test hooks.

sparse_syrk_kernel alone: the inputs are small integers in [-8, 8], at most 300 rows -- every partial sum is an integer
below 2^53, exact in fp64 whatever the order, so the comparison is assert_array_equal.  Padding columns of Vt hold NaN,
rows behind the live ones too: whatever leaks shows.

sparse_grad_kernel alone: against the numpy pair sum sum_fu W_fu dk(x_f, u_u)/dlog theta over gram_np's derivative
matrices, every component within 1e-6 of the largest (produce_grad_ref.assert_derivative, the suite's gradient rule).

Through the C ABI.  The tolerances are computed in the test from the reference and printed, by the rule of the
multi-output tests: a dense fp64 solve carries about cond * 2.2e-16 relative, over a few hundred operations, so
    rel = 300 * cond(Kuu + eps I) * 2.2e-16
bounds the relative error of the bound; the cases take eps = 1e-2 (option "sparse_jitter_log10" = -2), which keeps
cond(Kuu + eps I) <= (M * sum of the output scales + eps) / eps <~ 5e4 for M <= 512 and rel below 1e-8 -- asserted
per case, on the reference.  mu and sigma: rtol = 1e-6, atol = 1e-8; gradient: 1e-6 of the largest component.

Shapes: N = 700 with "sparse_chunk" = 256 is three chunks with a ragged last one (188 rows: two 128-tiles, the second
ragged); M = 48 is one 256-panel of inducing points, M = 300 two (Mp = 512: the panel loops of the M x M work take their
second step).  N = 20000 at the default chunk is two full chunks and a ragged one.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

import grad_reduce_ref as GR
import sparse_ref as SR
from gogp_amd import _lib, kernel, optimize, synth
from oracle.oracle import gram_np
from produce_grad_ref import assert_derivative

pytestmark = pytest.mark.gpu

EPSM = np.finfo(float).eps
JIT = -2
EPS = 10.0 ** JIT
N0 = 700
_REF = {}


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- sparse_syrk_kernel in isolation ------------------------------------------------------------------------------------
def _syrk(Vt, ld, rows, M, Mp, y, B, r):
    Vt, y = np.ascontiguousarray(Vt, float).reshape(-1), np.ascontiguousarray(y, float)
    B, r = np.ascontiguousarray(B, float).copy(), np.ascontiguousarray(r, float).copy()
    rc = _lib.hooks().gogp_test_sparse_syrk(0, _dp(Vt), Vt.size, ld, rows, M, Mp, _dp(y), y.size, _dp(B), B.size, Mp, _dp(r),
                                            r.size)
    assert rc == _lib.GOGP_OK
    return B.reshape(Mp, Mp), r


def _syrk_case(M, Mp, rows, seed, extra_rows=3):
    rng = np.random.default_rng(seed)
    ld = Mp + 8
    Vt = np.full((rows + extra_rows, ld), np.nan)  # columns >= M, the slack behind Mp and the rows behind `rows`: NaN
    Vt[:rows, :M] = rng.integers(-8, 9, (rows, M)).astype(float)
    y = np.full(rows + extra_rows, np.nan)
    y[:rows] = rng.integers(-8, 9, rows).astype(float)
    B0 = rng.integers(-50, 51, (Mp, Mp)).astype(float)  # accumulation onto a non-zero B and r
    r0 = rng.integers(-50, 51, Mp).astype(float)
    B, r = _syrk(Vt, ld, rows, M, Mp, y, B0, r0)
    V = np.zeros((rows, Mp))
    V[:, :M] = Vt[:rows, :M]
    i, j = np.indices((Mp, Mp))
    tiles = (j // 64) <= (i // 64)  # the lower 64-tiles, whole (a diagonal tile's upper half included)
    want = B0 + np.where(tiles, V.T @ V, 0.0)
    np.testing.assert_array_equal(B, want, err_msg=str((M, Mp, rows)))
    np.testing.assert_array_equal(r, r0 + V.T @ y[:rows], err_msg=str((M, Mp, rows)))


@pytest.mark.parametrize("M,Mp", [(256, 256), (512, 512), (200, 256), (300, 512), (1, 256)])
@pytest.mark.parametrize("rows", [1, 37, 256, 300])
def test_syrk_kernel_exact(gpm, M, Mp, rows):
    _syrk_case(M, Mp, rows, 1000 * M + rows)


def test_syrk_kernel_fragment_layout_asymmetric(gpm):
    """Rows of Vt with one or two non-zero entries each, placed asymmetrically over the tile pairs: Vt^T Vt has a handful
    of non-zero elements that a transposed fragment map or a transposed epilogue moves."""
    M, Mp, rows = 300, 512, 12
    Vt = np.zeros((rows, Mp))
    hits = [(0, 3), (1, 70), (2, 3), (2, 150), (3, 299), (4, 64), (5, 65), (5, 1), (6, 130), (7, 17), (7, 280), (9, 257),
            (9, 2), (11, 190), (11, 191)]
    for k, u in hits:
        Vt[k, u] = 1.0 + k
    y = np.arange(1.0, rows + 1.0)
    B, r = _syrk(Vt, Mp, rows, M, Mp, y, np.zeros((Mp, Mp)), np.zeros(Mp))
    i, j = np.indices((Mp, Mp))
    np.testing.assert_array_equal(B, np.where((j // 64) <= (i // 64), Vt.T @ Vt, 0.0))
    np.testing.assert_array_equal(r, Vt.T @ y)
    assert B[150, 3] == 9.0 and B[65, 1] == 36.0 and B[280, 17] == 64.0 and B[257, 2] == 100.0 and B[191, 190] == 144.0


# ---- sparse_grad_kernel in isolation ------------------------------------------------------------------------------------
def _grad_hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4, accumulate=False, out0=None):
    X, U, Wt = (np.ascontiguousarray(a, float).reshape(-1) for a in (X, U, Wt))
    y, mvec = np.ascontiguousarray(y, float), np.ascontiguousarray(mvec, float)
    out = np.zeros(_lib.GOGP_TEST_NACC) if out0 is None else np.array(out0, float)
    rc = _lib.hooks().gogp_test_sparse_grad(0, kp.hook(gpm), _dp(X), X.size, len(y), _dp(U), U.size, len(mvec), _dp(Wt),
                                            Wt.size, ldw, _dp(y), y.size, _dp(mvec), mvec.size, s4, int(accumulate), _dp(out))
    assert rc == _lib.GOGP_OK
    return out


def _grad_case(gpm, fam, rows, M, seed=3):
    D, simil, ts = SR.FAMILIES[fam]
    desc = kernel.build_desc(D, simil, SR.NOISE)
    ths = np.asarray(ts, float)
    kp = GR.kp_from_desc(desc, ths, SR.TN)
    rng = np.random.default_rng(seed + rows + M)
    X = SR.inputs(rows, 1, D)[0]
    U = SR.inputs(M, 1, D, seed=11)[0]
    ldw = M + 5
    Wt = np.full((rows, ldw), np.nan)
    Wt[:, :M] = rng.normal(size=(rows, M))  # mixed sign
    y, mvec, s4 = rng.normal(size=rows), rng.normal(size=M), 1.0 / 0.09 ** 2
    slots = _grad_hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4)
    W = Wt[:, :M] + np.outer(y, mvec) * s4
    _, dK = gram_np(desc, ths, X, U, want_grad=True)
    want = np.array([(W * d).sum() for d in dK])
    got = GR.assemble(desc, 2.0 * slots, 0.0)[:len(ths)]
    assert slots[GR.ACC_TRACE] == 0.0
    assert_derivative(got, want, "%s rows %d M %d" % (fam, rows, M))
    return kp, X, U, Wt, ldw, y, mvec, s4, slots


@pytest.mark.parametrize("fam", SR.FOUR + ["ard_rbf64"])
def test_grad_kernel_against_the_pair_sum(gpm, fam):
    _grad_case(gpm, fam, 130, 70)


@pytest.mark.parametrize("rows,M", [(1, 70), (130, 1), (1, 1), (64, 64), (65, 129)])
def test_grad_kernel_edge_shapes(gpm, rows, M):
    _grad_case(gpm, "ard_rbf3", rows, M)
    _grad_case(gpm, "hyperpriors", rows, M)


def test_grad_kernel_accumulates_and_repeats(gpm):
    kp, X, U, Wt, ldw, y, mvec, s4, slots = _grad_case(gpm, "ard_rbf64", 130, 70)
    again = _grad_hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4)
    np.testing.assert_array_equal(again, slots)  # fixed order: the same bits
    base = np.arange(1.0, _lib.GOGP_TEST_NACC + 1.0)
    acc = _grad_hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4, accumulate=True, out0=base)
    np.testing.assert_array_equal(acc, base + slots)
    over = _grad_hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4, accumulate=False, out0=base)
    np.testing.assert_array_equal(over, slots)


# ---- through the C ABI --------------------------------------------------------------------------------------------------
def _x(fam):
    return np.log(np.array(list(SR.FAMILIES[fam][2]) + SR.TN))


def _inducing(X, M, seed=5):
    """M inducing points: a subset of X where it has that many rows, else X and uniform points of its box."""
    rng = np.random.default_rng(seed)
    if M <= len(X):
        return X[rng.choice(len(X), M, replace=False)].copy()
    return np.vstack([X, rng.uniform(-2.0, 2.0, (M - len(X), X.shape[1]))])


def _ref(fam, N, M, eps=EPS):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, N, M, eps)
    if key not in _REF:
        D, simil, _ = SR.FAMILIES[fam]
        X, y, Z = SR.inputs(N, 7, D)
        U = _inducing(X, M)
        F, grad, st = SR.reference(D, simil, _x(fam), X, y, U, eps)
        mu, sigma = SR.produce(D, simil, _x(fam), st, U, Z)
        cond = np.linalg.cond(st.Kuu + eps * np.eye(M))
        _REF[key] = dict(X=X, y=y, Z=Z, U=U, F=F, grad=grad, mu=mu, sigma=sigma, rel=300.0 * cond * EPSM, cond=cond)
    return _REF[key]


def _gp(fam, jit=JIT, chunk=256, **kw):
    from gogp_amd.gp import GP
    D, s, ts = SR.FAMILIES[fam]
    g = GP(D, s, SR.NOISE, ThetaSimil=ts, ThetaNoise=SR.TN, device=0, **kw)
    if kw.get("precision", 64) == 64:
        g.set_option("sparse_jitter_log10", jit)
        g.set_option("sparse_chunk", chunk)
    return g


def _check(g, r, x, tag, need_1e8=True):
    F = g.SparseObserve(x)
    grad = g.SparseGradient()
    mu, sigma = g.SparseProduce(r["Z"])
    scale = np.abs(r["grad"]).max()
    crit = lambda a, b: (np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))).max()  # noqa: E731
    print("%s: bound %.12e (reference %.12e), rel err %.3e, allowed %.3e (cond(Kuu + eps I) = %.3e); gradient max |err| = "
          "%.3e of largest component %.3e (%.2e relative); mu %.3e sigma %.3e of the rtol 1e-6 + atol 1e-8 criterion"
          % (tag, F, r["F"], abs(F - r["F"]) / abs(r["F"]), r["rel"], r["cond"], np.abs(grad - r["grad"]).max(), scale,
             np.abs(grad - r["grad"]).max() / scale, crit(mu, r["mu"]), crit(sigma, r["sigma"])))
    if need_1e8:
        assert r["rel"] < 1e-8, (tag, r["rel"])  # the case is conditioned well enough for the rule to have teeth
    assert abs(F - r["F"]) <= r["rel"] * abs(r["F"]), (tag, F, r["F"])
    assert grad.shape == r["grad"].shape
    assert np.abs(grad - r["grad"]).max() <= 1e-6 * scale, (tag, grad, r["grad"])
    np.testing.assert_allclose(mu, r["mu"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(sigma, r["sigma"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    return F, grad, mu, sigma


@pytest.mark.parametrize("M", [48, 300])
@pytest.mark.parametrize("fam", SR.FOUR)
def test_values_against_the_reference(fam, M):
    r = _ref(fam, N0, M)
    g = _gp(fam)
    g.SetSparse(r["X"], r["y"], r["U"])
    first = _check(g, r, _x(fam), (fam, M))
    # the same calls again: the same bits
    again = (g.SparseObserve(_x(fam)), g.SparseGradient(), *g.SparseProduce(r["Z"]))
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    g.close()


@pytest.mark.parametrize("M", [48, 300])
def test_chunk_sizes_agree(M):
    fam = "ard_rbf3"
    r = _ref(fam, N0, M)
    outs = []
    for chunk in (256, 1024):
        g = _gp(fam, chunk=chunk)
        g.SetSparse(r["X"], r["y"], r["U"])
        outs.append((np.array([g.SparseObserve(_x(fam))]), g.SparseGradient(), *g.SparseProduce(r["Z"])))
        g.close()
    for what, a, b in zip(("bound", "gradient", "mu", "sigma"), *outs):
        d = np.abs(a - b).max() / np.abs(b).max()
        print("M = %d %s: chunk 256 against 1024: %.3e of the largest" % (M, what, d))
        assert d <= 1e-11, (what, d)


def test_u_equal_x_against_the_dense_observe():
    """U = X at N = 300: the bound against this handle's own dense Observe, within the eps bound of the CPU test."""
    fam, N, jit = "matern32_2d", 300, -10
    D, simil, _ = SR.FAMILIES[fam]
    X, y, _ = SR.inputs(N, 1, D)
    g = _gp(fam, jit=jit)
    g.X, g.Y = X, y
    lml = g.Observe(_x(fam))
    g.SetSparse(X, y, X)
    F = g.SparseObserve(_x(fam))
    Kn = SR.LR.gram(D, simil, _x(fam), X)
    alpha = np.linalg.solve(Kn, y)
    first = 0.5 * 10.0 ** jit * abs(np.trace(np.linalg.inv(Kn)) - alpha @ alpha)
    bound = first + 1e-9 * abs(lml) + 1e-11
    print("U = X: bound %.12e, dense LML %.12e, |diff| = %.3e, allowed %.3e (eps term %.3e)" % (F, lml, abs(F - lml), bound, first))
    assert abs(F - lml) <= bound
    g.close()


def test_no_observations():
    fam = "ard_rbf3"
    D, simil, ts = SR.FAMILIES[fam]
    X, _, Z = SR.inputs(30, 7, D)
    g = _gp(fam)
    g.SetSparse(np.zeros((0, D)), np.zeros(0), X)
    assert g.SparseObserve(_x(fam)) == 0.0
    grad = g.SparseGradient()
    assert grad.shape == (len(ts) + 1,) and not grad.any()
    mu, sigma = g.SparseProduce(Z)
    assert not mu.any()
    np.testing.assert_allclose(sigma, SR.produce(D, simil, _x(fam), None, X, Z)[1], rtol=1e-6, atol=1e-8)
    g.close()


def test_more_inducing_points_than_observations():
    fam = "matern32_2d"
    r = _ref(fam, 20, 48)
    g = _gp(fam)
    g.SetSparse(r["X"], r["y"], r["U"])
    _check(g, r, _x(fam), "M = 48 > N = 20")
    g.close()


def _duplicated(fam):
    D, simil, _ = SR.FAMILIES[fam]
    X, y, Z = SR.inputs(200, 7, D)
    U = np.vstack([X[:24], X[:24]])
    return D, simil, X, y, Z, U


def test_duplicated_inducing_points():
    """The jitter carries them: Kuu alone is singular."""
    fam = "matern32_2d"
    D, simil, X, y, Z, U = _duplicated(fam)
    F, grad, st = SR.reference(D, simil, _x(fam), X, y, U, EPS)
    mu, sigma = SR.produce(D, simil, _x(fam), st, U, Z)
    cond = np.linalg.cond(st.Kuu + EPS * np.eye(len(U)))
    r = dict(X=X, y=y, Z=Z, U=U, F=F, grad=grad, mu=mu, sigma=sigma, rel=300.0 * cond * EPSM, cond=cond)
    g = _gp(fam)
    g.SetSparse(X, y, U)
    _check(g, r, _x(fam), "duplicated inducing points")
    g.close()


def test_not_positive_definite_without_jitter():
    from gogp_amd.gp import FactorizeError
    fam = "matern32_2d"
    D, simil, X, y, Z, U = _duplicated(fam)
    g = _gp(fam, jit=-14)
    g.SetSparse(X, y, U)
    try:
        F = g.SparseObserve(_x(fam))
    except FactorizeError as e:
        print("jitter 1e-14 on duplicated points: GOGP_ENOTPD at inducing point %d" % e.pivot)
        assert 0 <= e.pivot < len(U)
        v = ctypes.c_double(0.0)
        x = _x(fam)
        assert _lib.lib().gogp_sparse_observe(g._h, _dp(x), x.size, ctypes.byref(v)) == _lib.GOGP_ENOTPD and np.isnan(v.value)
        grad = np.zeros(x.size)
        assert _lib.lib().gogp_sparse_gradient(g._h, _dp(grad), x.size) == _lib.GOGP_ESTATE  # nothing was observed
    else:
        print("jitter 1e-14 on duplicated points: the factorisation went through (bound %.6e): GOGP_ENOTPD did not occur, "
              "its assertion is skipped" % F)
    g.close()


# ---- state --------------------------------------------------------------------------------------------------------------
def test_dense_state_is_untouched_and_the_sparse_state_survives():
    """One of two twins interleaves sparse calls with the dense ones: Produce, Gradient, LOO and MultiLML return the
    same bits.  The sparse data survives a dense set_data."""
    fam = "ard_rbf3"
    D, simil, _ = SR.FAMILIES[fam]
    r = _ref(fam, N0, 48)
    Xd, yd, Zd = SR.inputs(300, 33, D, seed=21)
    Yd = np.stack([yd, yd ** 2, np.cos(yd)], axis=1)

    def run(sparse):
        g = _gp(fam)
        sp = []
        if sparse:
            g.SetSparse(r["X"], r["y"], r["U"])
            sp.append(g.SparseObserve(_x(fam)))
        g.X, g.Y = Xd, yd
        out = [np.array([g.Observe(_x(fam))])]
        if sparse:
            sp.append(g.SparseObserve(_x(fam)))  # survives the dense set_data
            g.SparseGradient()
        out += [g.Gradient(), *g.Produce(Zd)]
        if sparse:
            g.SparseProduce(r["Z"])
        out += [*g.LOO(), g.LOOGradient()]
        g.SetOutputs(Yd)
        if sparse:
            sp.append(g.SparseObserve(_x(fam) + 0.1))
            g.SparseGradient()
        out += [np.array([g.MultiLML()[0]]), g.MultiGradient(), *g.Produce(Zd), g.L, g.Alpha]
        if sparse:
            sp.append(g.SparseObserve(_x(fam)))
            assert sp[0] == sp[1] == sp[3] and sp[2] != sp[0]
        g.close()
        return out

    for u, v in zip(run(False), run(True)):
        np.testing.assert_array_equal(u, v)


def test_lifecycle_and_refusals():
    from gogp_amd.gp import GP, GogpError
    fam = "matern52"
    D, simil, ts = SR.FAMILIES[fam]
    r = _ref(fam, N0, 48)
    X, y, U, Z = r["X"], r["y"], r["U"], np.ascontiguousarray(r["Z"][:3])
    x = _x(fam)
    P = x.size
    L = _lib.lib()
    v, grad, mu, sg = ctypes.c_double(0.0), np.zeros(P), np.zeros(3), np.zeros(3)

    def three(h):
        return (L.gogp_sparse_observe(h, _dp(x), P, ctypes.byref(v)), L.gogp_sparse_gradient(h, _dp(grad), P),
                L.gogp_sparse_produce(h, _dp(Z), 3, _dp(mu), _dp(sg)))

    g = _gp(fam)
    assert three(g._h) == (_lib.GOGP_ESTATE,) * 3  # before gogp_sparse_set_data
    for args in ((_dp(X), _dp(y), N0, _dp(U), 0), (_dp(X), _dp(y), N0, _dp(U), 4097), (_dp(X), _dp(y), N0, None, 48),
                 (None, _dp(y), N0, _dp(U), 48), (_dp(X), None, N0, _dp(U), 48), (_dp(X), _dp(y), -1, _dp(U), 48)):
        assert L.gogp_sparse_set_data(g._h, *args) == _lib.GOGP_EARG, args[2::2]
    for i in range(3):  # a non-finite value in X, y, U
        b = [a.copy() for a in (X, y, U)]
        b[i].reshape(-1)[5] = np.inf
        assert L.gogp_sparse_set_data(g._h, _dp(b[0]), _dp(b[1]), N0, _dp(b[2]), 48) == _lib.GOGP_EARG
    assert three(g._h) == (_lib.GOGP_ESTATE,) * 3  # a refused set_data sets nothing
    g.SetSparse(X, y, U)
    assert L.gogp_sparse_gradient(g._h, _dp(grad), P) == _lib.GOGP_ESTATE  # before observe
    assert L.gogp_sparse_produce(g._h, _dp(Z), 3, _dp(mu), _dp(sg)) == _lib.GOGP_ESTATE
    assert L.gogp_sparse_observe(g._h, _dp(x), P + 1, ctypes.byref(v)) == _lib.GOGP_EARG
    xb = x.copy()
    xb[0] = np.nan
    assert L.gogp_sparse_observe(g._h, _dp(xb), P, ctypes.byref(v)) == _lib.GOGP_EARG
    assert L.gogp_sparse_observe(g._h, None, P, ctypes.byref(v)) == _lib.GOGP_EARG
    _check(g, r, x, "lifecycle")
    assert L.gogp_sparse_gradient(g._h, _dp(grad), P - 1) == _lib.GOGP_EARG
    assert L.gogp_sparse_produce(g._h, None, 0, None, None) == _lib.GOGP_OK  # m = 0
    for name, val in (("sparse_jitter_log10", -15), ("sparse_jitter_log10", -1), ("sparse_chunk", 128), ("sparse_chunk", 300),
                      ("sparse_chunk", 65536 + 256)):
        assert L.gogp_set_option(g._h, name.encode(), val) == _lib.GOGP_EARG, (name, val)
    # event discounts are out of scope: refused, by name
    ev = np.array([0.0, 1.0, 0.5])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == _lib.GOGP_OK
    assert three(g._h) == (_lib.GOGP_EARG,) * 3
    assert L.gogp_sparse_set_data(g._h, _dp(X), _dp(y), N0, _dp(U), 48) == _lib.GOGP_EARG
    assert b"event" in L.gogp_last_error(g._h)
    assert L.gogp_set_events(g._h, None, 0, 0) == _lib.GOGP_OK
    _check(g, r, x, "events cleared again")
    g.SetSparse(None, None, None)  # cleared
    assert three(g._h) == (_lib.GOGP_ESTATE,) * 3
    g.close()
    g32 = GP(D, simil, SR.NOISE, ThetaSimil=ts, ThetaNoise=SR.TN, device=0, precision=32)
    assert L.gogp_sparse_set_data(g32._h, _dp(X), _dp(y), N0, _dp(U), 48) == _lib.GOGP_EARG
    assert three(g32._h) == (_lib.GOGP_EARG,) * 3
    with pytest.raises(GogpError) as e:
        g32.SparseObserve(x)
    assert e.value.code == _lib.GOGP_EARG and "precision = 32" in str(e.value)
    g32.close()
    # destroy with the sparse state allocated and observed
    h = _gp(fam)
    h.SetSparse(X, y, U)
    h.SparseObserve(x)
    h.close()


# ---- one larger case ----------------------------------------------------------------------------------------------------
def test_larger_than_a_dense_handle_was_given():
    """N = 20000, M = 512, D = 2 at the default chunk: two full chunks and a ragged one, against the chunked reference."""
    fam, N, M = "matern32_2d", 20000, 512
    D, simil, _ = SR.FAMILIES[fam]
    X, y, Z = SR.inputs(N, 7, D)
    U = _inducing(X, M)
    x = _x(fam)
    F, grad, st = SR.reference_chunked(D, simil, x, X, y, U, EPS, 4096)
    mu, sigma = SR.produce(D, simil, x, st, U, Z)
    cond = np.linalg.cond(st.Kuu + EPS * np.eye(M))
    r = dict(Z=Z, F=F, grad=grad, mu=mu, sigma=sigma, rel=300.0 * cond * EPSM, cond=cond)
    g = _gp(fam, chunk=8192)
    g.SetSparse(X, y, U)
    _check(g, r, x, "N = 20000, M = 512")
    g.close()


# ---- SparseModel --------------------------------------------------------------------------------------------------------
def test_optimiser_raises_the_bound():
    from gogp_amd.gp import GP, SparseModel
    n, D, M = 600, 2, 40
    X, y = synth.make_inputs(n, D, 5)
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, SR.NOISE, device=0)
    g.set_option("sparse_jitter_log10", -6)
    g.SetSparse(X, y, _inducing(X, M))
    m = SparseModel(g)
    x0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    start = m.Observe(x0)
    g0 = np.linalg.norm(m.Gradient())
    res = optimize.lbfgs(m, x0, gradient_threshold=1e-3)
    end = m.Observe(res.x)
    g1 = np.linalg.norm(m.Gradient())
    print("sparse objective: start %.9f, end %.9f after %d iterations, %d evaluations; |grad| %.3e -> %.3e; theta = %s"
          % (start, end, res.iterations, res.evaluations, g0, g1, np.exp(res.x)))
    assert end > start
    assert g1 < g0
    g.close()
