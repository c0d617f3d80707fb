"""GP.SetSparseOutputs / SparseMultiObserve / SparseMultiGradient / SparseMultiGradientInducing / SparseMultiProduce
(gogp_sparse_multi_*) on the GPU against the numpy matrix form of tests/sparse_multi_ref.py (tests/test_sparse_multi_cpu.py
pins it to the column-wise sum of the single-output reference), and sparse_xty_kernel in isolation through its hook.

sparse_xty_kernel alone: the inputs are small integers in [-8, 8], at most a few hundred rows -- every partial sum is
an integer below 2^53, exact in fp64 whatever the order, so the comparison is assert_array_equal.  The padding of Vt
(ld = Mp + 8: columns >= M, rows behind the live ones) and of Y (ld = T + 3) holds NaN: whatever leaks shows.  R starts
non-zero: the launch accumulates.

Through the C ABI: the rules of tests/test_sparse_gpu.py, computed in the test from the reference and printed --
    rel = 300 * cond(Kuu + eps I) * 2.2e-16, asserted < 1e-8 on the reference (eps = 1e-2: "sparse_jitter_log10" = -2),
every bounds[t] within rel |ref_t|, the total within rel sum_t |ref_t|, gradient and dU within 1e-6 of the largest
component (produce_grad_ref.assert_derivative), mu and sigma rtol = 1e-6, atol = 1e-8.

Shapes: N = 700 with "sparse_chunk" = 256 is three chunks with a ragged last one; M = 48 is one 256-panel of inducing
points, M = 300 two; T = 3 / 65 / 128 are one ragged 64-tile of outputs, two with a ragged second and two whole.
N = 20000 at the default chunk is two full chunks and a ragged one.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

import sparse_inducing_ref as SI
import sparse_multi_ref as SM
import sparse_ref as SR
from gogp_amd import _lib, kernel, optimize, synth
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


# ---- sparse_xty_kernel in isolation -------------------------------------------------------------------------------------
def _xty(Vt, ld, rows, M, Mp, Y, ldy, T, R, ldr):
    Vt, Y = np.ascontiguousarray(Vt, float).reshape(-1), np.ascontiguousarray(Y, float).reshape(-1)
    R = np.ascontiguousarray(R, float).copy()
    rc = _lib.hooks().gogp_test_sparse_xty(0, _dp(Vt), Vt.size, ld, rows, M, Mp, _dp(Y), Y.size, ldy, T, _dp(R), R.size, ldr)
    assert rc == _lib.GOGP_OK
    return R


def _xty_case(M, Mp, T, rows, seed, extra_rows=3):
    rng = np.random.default_rng(seed)
    ld, ldy = Mp + 8, T + 3
    Vt = np.full((rows + extra_rows, ld), np.nan)  # columns >= M, the slack behind Mp and the rows behind `rows`: NaN
    Vt[:rows, :M] = rng.integers(-8, 9, (rows, M)).astype(float)
    Y = np.full((rows + extra_rows, ldy), np.nan)
    Y[:rows, :T] = rng.integers(-8, 9, (rows, T)).astype(float)
    R0 = rng.integers(-50, 51, (128, Mp)).astype(float)  # accumulation onto a non-zero R
    R = _xty(Vt, ld, rows, M, Mp, Y, ldy, T, R0, Mp)
    want = R0.copy()
    want[:T, :M] += Y[:rows, :T].T @ Vt[:rows, :M]  # (the padded elements receive += exact zeros)
    np.testing.assert_array_equal(R, want, err_msg=str((M, Mp, T, rows)))


@pytest.mark.parametrize("M,Mp", [(256, 256), (200, 256), (300, 512), (1, 256)])
@pytest.mark.parametrize("rows", [1, 37, 256, 300])
def test_xty_kernel_exact(gpm, M, Mp, rows):
    for T in (1, 3, 64, 65, 128):
        _xty_case(M, Mp, T, rows, 1000 * M + 10 * rows + T)


@pytest.mark.parametrize("M,Mp,T", [(200, 256, 3), (300, 512, 65), (4096, 4096, 128)])
def test_xty_kernel_short_last_slab(gpm, M, Mp, T):
    """The first row count at which the launch's own slab function gives more than one slab with a short last one."""
    hk = _lib.hooks()
    rps = ctypes.c_int64(0)
    rows = next(r for r in range(1, 1 << 16) if hk.gogp_test_sparse_xty_slabs(r, M, T, ctypes.byref(rps)) > 1 and r % rps.value)
    slabs = hk.gogp_test_sparse_xty_slabs(rows, M, T, ctypes.byref(rps))
    print("M = %d, T = %d: %d rows are %d slabs of %d rows, the last of %d" % (M, T, rows, slabs, rps.value, rows % rps.value))
    assert slabs > 1 and 0 < rows % rps.value < rps.value and (slabs - 1) * rps.value < rows
    assert slabs <= hk.gogp_test_sparse_xty_slabs_bound(rows, M, T)
    _xty_case(M, Mp, T, rows, 77)


def test_xty_kernel_fragment_layout_asymmetric(gpm):
    """A handful of non-zeros placed asymmetrically over the (output, inducing point) tiles: Y^T Vt has a few non-zero
    elements that a transposed fragment map or a transposed epilogue moves."""
    M, Mp, T, rows = 300, 512, 100, 12
    Vt, Y = np.zeros((rows, Mp)), np.zeros((rows, T))
    vhits = [(0, 3), (1, 70), (2, 150), (3, 299), (4, 64), (5, 65), (6, 130), (7, 17), (9, 257), (11, 190)]
    yhits = [(0, 1), (1, 0), (2, 99), (3, 2), (4, 65), (5, 63), (6, 64), (7, 30), (9, 5), (11, 77)]
    for k, u in vhits:
        Vt[k, u] = 1.0 + k
    for k, t in yhits:
        Y[k, t] = 2.0 + k
    R = _xty(Vt, Mp, rows, M, Mp, Y, T, T, np.zeros((128, Mp)), Mp)
    want = np.zeros((128, Mp))
    want[:T] = Y.T @ Vt
    np.testing.assert_array_equal(R, want)
    assert np.count_nonzero(R) == len(vhits)
    assert R[1, 3] == 2.0 and R[0, 70] == 6.0 and R[99, 150] == 12.0 and R[2, 299] == 20.0 and R[65, 64] == 30.0
    assert R[63, 65] == 42.0 and R[64, 130] == 56.0 and R[77, 190] == 156.0


# ---- through the C ABI --------------------------------------------------------------------------------------------------
def _x(fam):
    return np.log(np.array(list(SR.FAMILIES[fam][2]) + SR.TN))


def _ref(fam, N, M, T, eps=EPS):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, N, M, T, eps)
    if key not in _REF:
        D, simil, _ = SR.FAMILIES[fam]
        X, _, Z = SR.inputs(N, 7, D)
        U = SI.displaced_subset(X, M) if M <= N else np.vstack([X, np.random.default_rng(5).uniform(-2.0, 2.0, (M - N, D))])
        Y = SM.outputs(X, T)
        total, bounds, grad, dU, st = SM.reference(D, simil, _x(fam), X, Y, U, eps)
        mu, sigma = SM.produce(D, simil, _x(fam), st, U, Z)
        cond = np.linalg.cond(st.Kuu + eps * np.eye(M))
        _REF[key] = dict(X=X, Y=Y, Z=Z, U=U, total=total, bounds=bounds, grad=grad, dU=dU, mu=mu, sigma=sigma,
                         rel=300.0 * cond * EPSM, cond=cond)
    return _REF[key]


def _gp(fam, jit=JIT, chunk=256, **kw):
    from gogp_amd.gp import GP
    D, s, ts = SR.FAMILIES[fam]
    g = GP(D, s, SR.NOISE, ThetaSimil=ts, ThetaNoise=SR.TN, device=0, **kw)
    if kw.get("precision", 64) == 64:
        g.set_option("sparse_jitter_log10", jit)
        if chunk is not None:
            g.set_option("sparse_chunk", chunk)
    return g


def _set(g, r):
    g.SetSparse(r["X"], np.zeros(len(r["X"])), r["U"])  # (the y of SetSparse does not enter the multi calls)
    g.SetSparseOutputs(r["Y"])


def _all(g, r, x):
    total, bounds = g.SparseMultiObserve(x)
    grad = g.SparseMultiGradient()
    grad2, dU = g.SparseMultiGradientInducing()
    np.testing.assert_array_equal(grad2, grad)
    mu, sigma = g.SparseMultiProduce(r["Z"])
    return np.array([total]), bounds, grad, dU, mu, sigma


def _check(g, r, x, tag, need_1e8=True):
    out = _all(g, r, x)
    total, bounds, grad, dU, mu, sigma = out
    total = total[0]
    crit = lambda a, b: (np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))).max()  # noqa: E731
    sabs = np.abs(r["bounds"]).sum()
    print("%s: total %.12e (reference %.12e), err %.3e of sum |ref_t|, bounds max rel err %.3e, allowed %.3e (cond(Kuu + eps I)"
          " = %.3e); mu %.3e sigma %.3e of the rtol 1e-6 + atol 1e-8 criterion"
          % (tag, total, r["total"], abs(total - r["total"]) / sabs, (np.abs(bounds - r["bounds"]) / np.abs(r["bounds"])).max(),
             r["rel"], r["cond"], crit(mu, r["mu"]), crit(sigma, r["sigma"])))
    if need_1e8:
        assert r["rel"] < 1e-8, (tag, r["rel"])  # the case is conditioned well enough for the rule to have teeth
    assert bounds.shape == r["bounds"].shape and grad.shape == r["grad"].shape and dU.shape == r["dU"].shape
    assert (np.abs(bounds - r["bounds"]) <= r["rel"] * np.abs(r["bounds"])).all(), (tag, bounds, r["bounds"])
    assert abs(total - r["total"]) <= r["rel"] * sabs, (tag, total, r["total"])
    assert_derivative(grad, r["grad"], "%s gradient" % (tag,))
    assert_derivative(dU, r["dU"], "%s dU" % (tag,))
    assert mu.shape == r["mu"].shape
    np.testing.assert_allclose(mu, r["mu"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(sigma, r["sigma"], rtol=1e-6, atol=1e-8, err_msg=str(tag))
    return out


@pytest.mark.parametrize("M", [48, 300])
@pytest.mark.parametrize("fam", SR.FOUR)
def test_values_against_the_reference(fam, M):
    r = _ref(fam, N0, M, 3)
    g = _gp(fam)
    _set(g, r)
    first = _check(g, r, _x(fam), (fam, M, 3))
    for a, b in zip(first, _all(g, r, _x(fam))):  # the same calls again: the same bits
        np.testing.assert_array_equal(a, b)
    g.close()


@pytest.mark.parametrize("T", [1, 65, 128])
def test_output_counts(T):
    fam = "matern52"
    r = _ref(fam, N0, 300, T)
    g = _gp(fam)
    _set(g, r)
    _check(g, r, _x(fam), (fam, 300, T))
    g.close()


def test_one_output_agrees_with_the_single_output_calls():
    """T = 1 against gogp_sparse_observe / gradient / gradient_inducing / produce on the same handle, by the tolerances
    of _check (the sums run in another order: bits are not required)."""
    fam = "ard_rbf3"
    r = _ref(fam, N0, 300, 1)
    g = _gp(fam)
    g.SetSparse(r["X"], r["Y"][:, 0], r["U"])
    g.SetSparseOutputs(r["Y"])
    x = _x(fam)
    F = g.SparseObserve(x)
    grad, dU = g.SparseGradientInducing()
    mu, sigma = g.SparseProduce(r["Z"])
    total, bounds, mgrad, mdU, mmu, msigma = _all(g, r, x)
    print("T = 1: bound %.12e, multi total %.12e, rel diff %.3e (allowed %.3e)" % (F, total[0], abs(F - total[0]) / abs(F), r["rel"]))
    assert r["rel"] < 1e-8
    assert abs(total[0] - F) <= r["rel"] * abs(F) and abs(bounds[0] - F) <= r["rel"] * abs(F)
    assert_derivative(mgrad, grad, "T = 1 gradient")
    assert_derivative(mdU, dU, "T = 1 dU")
    np.testing.assert_allclose(mmu[:, 0], mu, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(msigma, sigma, rtol=1e-6, atol=1e-8)
    g.close()


def test_chunk_sizes_agree():
    fam = "ard_rbf3"
    r = _ref(fam, N0, 300, 3)
    outs = []
    for chunk in (256, None):  # None: the default
        g = _gp(fam, chunk=chunk)
        _set(g, r)
        outs.append(_all(g, r, _x(fam)))
        g.close()
    for what, a, b in zip(("total", "bounds", "gradient", "dU", "mu", "sigma"), *outs):
        d = np.abs(a - b).max() / np.abs(b).max()
        print("%s: chunk 256 against the default: %.3e of the largest" % (what, d))
        assert d <= 1e-11, (what, d)


def test_u_equal_x_against_the_dense_multi_lml():
    """U = X at N = M = 200: the total against this handle's own dense MultiLML total.  Allowed: the eps-perturbation of
    every column's LML, 1/2 eps |tr(Kn^-1) - alpha_t^T alpha_t| (tests/test_sparse_cpu.py), plus rel sum_t |LML_t|."""
    fam, N, jit = "matern32_2d", 200, -10
    D, simil, _ = SR.FAMILIES[fam]
    X, y, _ = SR.inputs(N, 1, D)
    Y = SM.outputs(X, 3)
    g = _gp(fam, jit=jit)
    g.X, g.Y = X, y
    g.Observe(_x(fam))
    g.SetOutputs(Y)
    lml, per = g.MultiLML()
    g.SetSparse(X, y, X)
    g.SetSparseOutputs(Y)
    total, bounds = g.SparseMultiObserve(_x(fam))
    Kn = SR.LR.gram(D, simil, _x(fam), X)
    Kuu = Kn - np.exp(2.0 * _x(fam)[-1]) * np.eye(N)
    rel = 300.0 * np.linalg.cond(Kuu + 10.0 ** jit * np.eye(N)) * EPSM
    A = np.linalg.solve(Kn, Y)
    first = sum(0.5 * 10.0 ** jit * abs(np.trace(np.linalg.inv(Kn)) - A[:, t] @ A[:, t]) for t in range(3))
    allowed = first + rel * np.abs(per).sum()
    print("U = X: total %.12e, dense MultiLML %.12e, |diff| = %.3e, allowed %.3e (eps term %.3e, rel %.3e)"
          % (total, lml, abs(total - lml), allowed, first, rel))
    assert abs(total - lml) <= allowed
    assert total <= lml + allowed  # a lower bound
    g.close()


def test_no_observations_and_no_test_points():
    fam = "ard_rbf3"
    D, simil, ts = SR.FAMILIES[fam]
    X, _, Z = SR.inputs(30, 7, D)
    g = _gp(fam)
    g.SetSparse(np.zeros((0, D)), np.zeros(0), X)
    g.SetSparseOutputs(np.zeros((0, 4)))
    total, bounds = g.SparseMultiObserve(_x(fam))
    assert total == 0.0 and bounds.shape == (4,) and not bounds.any()
    grad, dU = g.SparseMultiGradientInducing()
    assert grad.shape == (len(ts) + 1,) and not grad.any() and dU.shape == X.shape and not dU.any()
    assert not g.SparseMultiGradient().any()
    mu, sigma = g.SparseMultiProduce(Z)
    assert mu.shape == (len(Z), 4) and not mu.any()
    np.testing.assert_allclose(sigma, SR.produce(D, simil, _x(fam), None, X, Z)[1], rtol=1e-6, atol=1e-8)
    mu, sigma = g.SparseMultiProduce(np.zeros((0, D)))  # m == 0
    assert mu.shape == (0, 4) and sigma.shape == (0,)
    g.close()


def test_two_identical_sequences_return_identical_bits():
    fam = "hyperpriors"
    r = _ref(fam, N0, 300, 3)
    outs = []
    for _ in range(2):
        g = _gp(fam)
        _set(g, r)
        a = _all(g, r, _x(fam))
        b = _all(g, r, _x(fam) + 0.05)
        outs.append(a + b)
        g.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


# ---- state --------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    from gogp_amd.gp import GP, GogpError
    fam = "matern52"
    D, simil, ts = SR.FAMILIES[fam]
    r = _ref(fam, N0, 48, 3)
    X, Y, U, Z = r["X"], np.ascontiguousarray(r["Y"]), r["U"], np.ascontiguousarray(r["Z"][:3])
    y = np.ascontiguousarray(Y[:, 0])
    x = _x(fam)
    P, T = x.size, 3
    L = _lib.lib()
    OK, EARG, ESTATE = _lib.GOGP_OK, _lib.GOGP_EARG, _lib.GOGP_ESTATE
    v, bs, grad, dU, mu, sg = ctypes.c_double(0.0), np.zeros(T), np.zeros(P), np.zeros(U.shape), np.zeros((3, T)), np.zeros(3)
    mu1 = np.zeros(3)

    def obs(h):
        return L.gogp_sparse_multi_observe(h, _dp(x), P, ctypes.byref(v), _dp(bs))

    def rest(h):
        return (L.gogp_sparse_multi_gradient(h, _dp(grad), P), L.gogp_sparse_multi_gradient_inducing(h, _dp(grad), P, _dp(dU)),
                L.gogp_sparse_multi_produce(h, _dp(Z), 3, _dp(mu), _dp(sg)))

    def single(h):
        return (L.gogp_sparse_gradient(h, _dp(grad), P), L.gogp_sparse_produce(h, _dp(Z), 3, _dp(mu1), _dp(sg)))

    g = _gp(fam)
    # before gogp_sparse_set_data
    assert L.gogp_sparse_multi_set_outputs(g._h, _dp(Y), N0, T) == ESTATE
    assert obs(g._h) == ESTATE and rest(g._h) == (ESTATE,) * 3
    g.SetSparse(X, y, U)
    # before the outputs
    assert obs(g._h) == ESTATE and rest(g._h) == (ESTATE,) * 3
    for args in ((_dp(Y), N0, 0), (_dp(Y), N0, 129), (_dp(Y), N0, -1), (_dp(Y), N0 - 1, T), (None, N0, T)):
        assert L.gogp_sparse_multi_set_outputs(g._h, *args) == EARG, args[1:]
    bad = Y.copy()
    bad[5, 1] = np.inf
    assert L.gogp_sparse_multi_set_outputs(g._h, _dp(bad), N0, T) == EARG
    assert obs(g._h) == ESTATE  # a refused set_outputs sets nothing
    g.SetSparseOutputs(Y)
    assert rest(g._h) == (ESTATE,) * 3  # before the multi observe
    assert L.gogp_sparse_multi_observe(g._h, _dp(x), P + 1, ctypes.byref(v), _dp(bs)) == EARG
    xb = x.copy()
    xb[0] = np.nan
    assert L.gogp_sparse_multi_observe(g._h, _dp(xb), P, ctypes.byref(v), _dp(bs)) == EARG
    assert L.gogp_sparse_multi_observe(g._h, None, P, ctypes.byref(v), _dp(bs)) == EARG
    assert L.gogp_sparse_multi_observe(g._h, _dp(x), P, None, _dp(bs)) == EARG
    assert L.gogp_sparse_multi_observe(g._h, _dp(x), P, ctypes.byref(v), None) == OK  # bounds may be NULL
    assert abs(v.value - r["total"]) <= r["rel"] * np.abs(r["bounds"]).sum()
    _check(g, r, x, "lifecycle")
    assert L.gogp_sparse_multi_gradient(g._h, _dp(grad), P - 1) == EARG
    assert L.gogp_sparse_multi_gradient(g._h, None, P) == EARG
    assert L.gogp_sparse_multi_gradient_inducing(g._h, _dp(grad), P, None) == EARG
    assert L.gogp_sparse_multi_produce(g._h, None, 0, None, None) == OK  # m = 0
    assert L.gogp_sparse_multi_produce(g._h, None, 3, _dp(mu), _dp(sg)) == EARG
    zb = Z.copy()
    zb[1, 0] = np.nan
    assert L.gogp_sparse_multi_produce(g._h, _dp(zb), 3, _dp(mu), _dp(sg)) == EARG
    # the last observe of either flavour owns the workspace
    assert single(g._h) == (ESTATE,) * 2
    assert L.gogp_sparse_observe(g._h, _dp(x), P, ctypes.byref(v)) == OK
    assert single(g._h) == (OK,) * 2 and rest(g._h) == (ESTATE,) * 3
    assert obs(g._h) == OK and rest(g._h) == (OK,) * 3 and single(g._h) == (ESTATE,) * 2
    # gogp_sparse_set_inducing keeps the outputs; both flavours wait for their observe
    g.SetInducing(U)
    assert rest(g._h) == (ESTATE,) * 3 and single(g._h) == (ESTATE,) * 2
    _check(g, r, x, "after set_inducing")
    # a change of the jitter asks for a new observe
    assert L.gogp_set_option(g._h, b"sparse_jitter_log10", JIT) == OK
    assert rest(g._h) == (ESTATE,) * 3
    # event discounts are out of scope: refused, by name
    ev = np.array([0.0, 1.0, 0.5])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == OK
    assert obs(g._h) == EARG and rest(g._h) == (EARG,) * 3
    assert L.gogp_sparse_multi_set_outputs(g._h, _dp(Y), N0, T) == EARG
    assert b"event" in L.gogp_last_error(g._h)
    assert L.gogp_set_events(g._h, None, 0, 0) == OK
    _check(g, r, x, "events cleared again")
    # T = 0 with Y = NULL clears the outputs, gogp_sparse_set_data drops them
    g.SetSparseOutputs(None)
    assert obs(g._h) == ESTATE and rest(g._h) == (ESTATE,) * 3
    g.SetSparseOutputs(Y)
    assert obs(g._h) == OK
    g.SetSparse(X, y, U)
    assert obs(g._h) == ESTATE and rest(g._h) == (ESTATE,) * 3
    g.SetSparseOutputs(Y)
    _check(g, r, x, "outputs set again")
    g.SetSparse(None, None, None)  # cleared
    assert obs(g._h) == ESTATE and L.gogp_sparse_multi_set_outputs(g._h, _dp(Y), N0, T) == ESTATE
    g.close()
    g32 = GP(D, simil, SR.NOISE, ThetaSimil=ts, ThetaNoise=SR.TN, device=0, precision=32)
    assert L.gogp_sparse_multi_set_outputs(g32._h, _dp(Y), N0, T) == EARG
    assert obs(g32._h) == EARG and rest(g32._h) == (EARG,) * 3
    with pytest.raises(GogpError) as e:
        g32.SparseMultiObserve(x)
    assert e.value.code == EARG and "precision = 32" in str(e.value)
    g32.close()
    # destroy with the multi state allocated and observed
    h = _gp(fam)
    _set(h, r)
    h.SparseMultiObserve(x)
    h.close()


def test_not_positive_definite_gives_nan():
    from gogp_amd.gp import FactorizeError
    fam = "matern32_2d"
    D, simil, _ = SR.FAMILIES[fam]
    X, _, _ = SR.inputs(200, 7, D)
    U = np.vstack([X[:24], X[:24]])
    g = _gp(fam, jit=-14)
    g.SetSparse(X, np.zeros(200), U)
    g.SetSparseOutputs(SM.outputs(X, 2))
    x = _x(fam)
    try:
        total = g.SparseMultiObserve(x)[0]
    except FactorizeError as e:
        assert 0 <= e.pivot < len(U)
        v, bs = ctypes.c_double(0.0), np.zeros(2)
        assert _lib.lib().gogp_sparse_multi_observe(g._h, _dp(x), x.size, ctypes.byref(v), _dp(bs)) == _lib.GOGP_ENOTPD
        assert np.isnan(v.value) and np.isnan(bs).all()
        grad = np.zeros(x.size)
        assert _lib.lib().gogp_sparse_multi_gradient(g._h, _dp(grad), x.size) == _lib.GOGP_ESTATE
    else:
        print("jitter 1e-14 on duplicated points: the factorisation went through (total %.6e): GOGP_ENOTPD did not occur, "
              "its assertion is skipped" % total)
    g.close()


def test_dense_state_is_untouched():
    """One of two twins interleaves multi calls with the dense ones: Gradient, Produce and the dense multi-output calls
    return the same bits."""
    fam = "ard_rbf3"
    D, simil, _ = SR.FAMILIES[fam]
    r = _ref(fam, N0, 48, 3)
    Xd, yd, Zd = SR.inputs(300, 33, D, seed=21)
    Yd = np.stack([yd, yd ** 2, np.cos(yd)], axis=1)

    def run(sparse):
        g = _gp(fam)
        if sparse:
            _set(g, r)
            g.SparseMultiObserve(_x(fam))
        g.X, g.Y = Xd, yd
        out = [np.array([g.Observe(_x(fam))])]
        if sparse:
            g.SparseMultiObserve(_x(fam))  # survives the dense set_data
            g.SparseMultiGradientInducing()
        out += [g.Gradient(), *g.Produce(Zd)]
        if sparse:
            g.SparseMultiProduce(r["Z"])
        g.SetOutputs(Yd)
        if sparse:
            g.SparseMultiObserve(_x(fam) + 0.1)
            g.SparseMultiGradient()
        out += [np.array([g.MultiLML()[0]]), g.MultiGradient(), *g.MultiProduce(Zd), *g.Produce(Zd), g.L, g.Alpha]
        g.close()
        return out

    for u, v in zip(run(False), run(True)):
        np.testing.assert_array_equal(u, v)


def test_single_output_calls_after_a_multi_sequence_return_fresh_bits():
    fam = "ard_rbf3"
    r = _ref(fam, N0, 300, 3)
    y = np.ascontiguousarray(r["Y"][:, 1])
    x = _x(fam)

    def single(g):
        return [np.array([g.SparseObserve(x)]), *g.SparseGradientInducing(), *g.SparseProduce(r["Z"])]

    fresh = _gp(fam)
    fresh.SetSparse(r["X"], y, r["U"])
    want = single(fresh)
    fresh.close()
    g = _gp(fam)
    g.SetSparse(r["X"], y, r["U"])
    g.SetSparseOutputs(r["Y"])
    _all(g, r, x + 0.1)
    _all(g, r, x)
    for a, b in zip(single(g), want):
        np.testing.assert_array_equal(a, b)
    g.close()


# ---- one larger case ----------------------------------------------------------------------------------------------------
def test_larger_than_a_dense_handle_was_given():
    """N = 20000, M = 300, T = 8, D = 2 at the default chunk: two full chunks and a ragged one, against the chunked form."""
    fam, N, M, T = "matern32_2d", 20000, 300, 8
    D, simil, _ = SR.FAMILIES[fam]
    X, _, Z = SR.inputs(N, 7, D)
    U = SI.displaced_subset(X, M)
    Y = SM.outputs(X, T)
    x = _x(fam)
    total, bounds, grad, dU, st = SM.reference_chunked(D, simil, x, X, Y, U, EPS, 4096)
    mu, sigma = SM.produce(D, simil, x, st, U, Z)
    cond = np.linalg.cond(st.Kuu + EPS * np.eye(M))
    r = dict(X=X, Y=Y, U=U, Z=Z, total=total, bounds=bounds, grad=grad, dU=dU, mu=mu, sigma=sigma, rel=300.0 * cond * EPSM,
             cond=cond)
    g = _gp(fam, chunk=None)
    _set(g, r)
    _check(g, r, x, "N = 20000, M = 300, T = 8")
    g.close()


# ---- SparseMultiModel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inducing", [False, True])
def test_optimiser_raises_the_total(inducing):
    from gogp_amd.gp import GP, SparseMultiModel
    n, D, M = 600, 2, 40
    X, y = synth.make_inputs(n, D, 5)
    Y = np.stack([y, 0.5 * y + 0.1 * np.sin(3.0 * X[:, 0]), -y + 0.2 * X[:, 1]], axis=1)
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, SR.NOISE, device=0)
    g.set_option("sparse_jitter_log10", -6)
    U0 = X[np.random.default_rng(5).choice(n, M, replace=False)].copy()
    g.SetSparse(X, y, U0)
    g.SetSparseOutputs(Y)
    m = SparseMultiModel(g, inducing=inducing)
    x0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    if inducing:
        x0 = np.concatenate([x0, U0.reshape(-1)])
    start = m.Observe(x0)
    g0 = m.Gradient()
    assert g0.shape == x0.shape
    res = optimize.lbfgs(m, x0, major_iterations=10, gradient_threshold=1e-3)
    end = m.Observe(res.x)
    print("sparse multi-output objective (inducing = %s): start %.9f, end %.9f after %d iterations, %d evaluations"
          % (inducing, start, end, res.iterations, res.evaluations))
    assert end > start
    if inducing:
        assert np.abs(res.x[3:] - x0[3:]).max() > 0.0
    g.close()
