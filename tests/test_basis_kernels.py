"""The kernels of basis.hip in isolation, through their test hooks (include/gogp_testhooks.h).

basis_symm_kernel, W^T = (K^-1 H)^T from the symmetric K^-1 of which only j <= i < n is stored.  Exact cases: K^-1
integer-valued in [-1000, 1000], H in [-8, 8]: every partial sum is an integer below 1100 * 8000 < 2^53, exact in fp64
whatever the order, so the comparison is assert_array_equal.  K^-1 is handed in with NaN everywhere outside j <= i < n,
H^T with a non-zero filler in its columns >= n, the output preset to a sentinel: columns >= n and rows >= p (up to a
multiple of 4) must be exact zeros, nothing else may be touched.  Shapes (n, npad, p): (2, 256, 1) one tile;
(64, 256, 3) a full tile; (65, 256, 4) the first second tile; (129, 256, 5) a ragged third; (300, 512, 33) a second
LDS pass over p; (1100, 1280, 64) the limit, tile pairs on both sides of the diagonal and more than one slab.
With normal deviates each of the n products rounds once at a partial sum of size <~ a few sqrt(n): 1e-12 per unit of
the summed length n, the bound tests/test_tile_kernels.py holds the tile kernel to.

The other four: integer or small-rational inputs, assert_array_equal where the arithmetic is exact (the Gram sums, a
factor with powers of two on its diagonal, alpha~, the predictive mean), 1e-12 relative against numpy otherwise.
"""
import numpy as np
import pytest

from gogp_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


# ---- basis_symm_kernel ----------------------------------------------------------------------------------------------------
def _symm(gpm, n, npad, p, H, Kl):
    ld, p4 = npad, (p + 3) // 4 * 4
    Kinv = np.full((npad, ld), np.nan)
    Kinv[:n, :n] = np.where(np.tril(np.ones((n, n), bool)), Kl, np.nan)
    Ht = np.full((p, ld), 7.0)  # the filler of the columns >= n must not reach the result
    Ht[:, :n] = H.T
    nslab = gpm.basis_slabs(n)[0]
    assert 1 <= nslab <= 16
    part0 = np.full(nslab * p4 * ld, SENTINEL)
    Wt0 = np.full((p4 + 2, ld), SENTINEL)
    _, Wt = gpm.basis_kernel_check("basis_symm", Kinv=Kinv, ldk=ld, n=n, npad=npad, Ht=Ht, ld=ld, p=p, part=part0, Wt=Wt0)
    return Wt.reshape(p4 + 2, ld)


def _symm_case(gpm, n, npad, p, H, Kl, tol=None, tag=""):
    p4 = (p + 3) // 4 * 4
    Wt = _symm(gpm, n, npad, p, H, Kl)
    assert not np.isnan(Wt).any(), tag
    want = (Kl @ H).T
    if tol is None:
        bad = Wt[:p, :n] != want
        if bad.any():
            print("%s: wrong rows %s, wrong columns %s" % (tag, np.flatnonzero(bad.any(1)), np.flatnonzero(bad.any(0))))
        np.testing.assert_array_equal(Wt[:p, :n], want, err_msg=str(tag))
    else:
        err = np.abs(Wt[:p, :n] - want).max()
        print("%s: max |err| = %.3e, bound %.3e" % (tag, err, tol))
        assert err <= tol, (tag, err, tol)
    for rest in (Wt[:p4, n:], Wt[p:p4, :]):
        assert rest.size == 0 or (not rest.any() and not np.signbit(rest).any()), tag
    np.testing.assert_array_equal(Wt[p4:], SENTINEL, err_msg=str(tag))
    return Wt


def _int_inputs(n, p, seed):
    rng = np.random.default_rng(seed)
    H = rng.integers(-8, 9, (n, p)).astype(float)
    Kl = rng.integers(-1000, 1001, (n, n)).astype(float)
    return H, np.tril(Kl) + np.tril(Kl, -1).T


@pytest.mark.parametrize("n,npad,p", [(2, 256, 1), (64, 256, 3), (65, 256, 4), (129, 256, 5), (300, 512, 33),
                                      (1100, 1280, 64)])
def test_symm_exact(gpm, n, npad, p):
    H, Kl = _int_inputs(n, p, 200 + n + p)
    _symm_case(gpm, n, npad, p, H, Kl, tag=(n, npad, p))


def test_symm_fragment_layout_asymmetric(gpm):
    """K^-1[i][j] = 1000 i + j (j <= i) tells a transposed read apart; columns of H with one or two non-zeros placed
    asymmetrically over the tile pairs pick single elements of it: a swapped fragment map moves them."""
    n, npad, p = 200, 256, 8
    H = np.zeros((n, p))
    for c, i in [(0, 3), (1, 70), (2, 3), (2, 150), (3, 199), (4, 64), (5, 65), (5, 1), (6, 130), (7, 17), (7, 180)]:
        H[i, c] = 1.0 + c
    i, j = np.indices((n, n))
    Kl = np.where(j <= i, 1000.0 * i + j, 1000.0 * j + i)
    _symm_case(gpm, n, npad, p, H, Kl, tag="unit columns")


def test_symm_normal_deviates_and_same_bits(gpm):
    n, npad, p = 300, 512, 33
    rng = np.random.default_rng(5)
    H = rng.normal(size=(n, p))
    Kl = rng.normal(size=(n, n))
    Kl = np.tril(Kl) + np.tril(Kl, -1).T
    W1 = _symm_case(gpm, n, npad, p, H, Kl, tol=1e-12 * n, tag="normal deviates")
    W2 = _symm(gpm, n, npad, p, H, Kl)
    np.testing.assert_array_equal(W1, W2)


def test_symm_refuses_what_it_cannot_honour(gpm):
    from gogp_amd.gp import GogpError
    H, Kl = _int_inputs(10, 2, 1)
    ok = dict(Kinv=np.zeros(256 * 256), ldk=256, n=10, npad=256, Ht=np.zeros(2 * 256), ld=256, p=2,
              part=np.zeros(gpm.basis_slabs(10)[0] * 4 * 256), Wt=np.zeros(4 * 256))
    for bad in (dict(p=0), dict(p=65), dict(n=0), dict(n=257), dict(npad=200), dict(Wt=np.zeros(4 * 256 - 1)),
                dict(part=np.zeros(4 * 256 - 1)), dict(Ht=np.zeros(2 * 256 - 1)), dict(ld=128)):
        with pytest.raises(GogpError) as e:
            gpm.basis_kernel_check("basis_symm", **dict(ok, **bad))
        assert e.value.code == _lib.GOGP_EARG, bad


# ---- basis_gram_kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld,p", [(2, 256, 1), (65, 256, 3), (300, 512, 33), (1100, 1280, 64)])
def test_gram_exact(gpm, n, ld, p):
    rng = np.random.default_rng(300 + n)
    Ht, Wt = np.full((p, ld), 7.0), np.full((p, ld), -3.0)  # fillers in the columns >= n
    Ht[:, :n] = rng.integers(-8, 9, (p, n))
    Wt[:, :n] = rng.integers(-100, 101, (p, n))
    alpha = np.full(ld, 5.0)
    alpha[:n] = rng.integers(-50, 51, n)
    nslab = gpm.basis_slabs(n)[1]
    assert nslab == min(64, (n + 255) // 256)
    total = p * (p + 1)
    _, Ag = gpm.basis_kernel_check("basis_gram", Ht=Ht, Wt=Wt, ld=ld, alpha=alpha, n=n, p=p,
                                   part=np.full(nslab * total, SENTINEL), Ag=np.full(total + 3, SENTINEL))
    want = Ht[:, :n] @ np.concatenate([Wt[:, :n].T, alpha[:n, None]], axis=1)
    np.testing.assert_array_equal(Ag[:total].reshape(p, p + 1), want)
    np.testing.assert_array_equal(Ag[total:], SENTINEL)


def _factor(rng, p):
    """A lower factor whose Cholesky arithmetic is exact: entries -1, 0, 1 below a diagonal of powers of two.  Beyond
    p = 5 the diagonal is 4 and only two sub-diagonals are filled, so that L = 4 (I + N / 4) with |N / 4| <= 1/2 has a
    bounded inverse (a full unit-lower factor of order 64 has one of size ~1.6^64)."""
    low = np.tril(rng.integers(-1, 2, (p, p)).astype(float), -1)
    if p <= 5:
        return low + np.diag(rng.choice([1.0, 2.0, 4.0], p))
    return low - np.tril(low, -3) + 4.0 * np.eye(p)


# ---- basis_finish_kernel --------------------------------------------------------------------------------------------------
def _finish(gpm, Ag, p):
    pp = p * p
    LA, Ainv, beta, scal, info = gpm.basis_kernel_check(
        "basis_finish", Ag=Ag, p=p, LA=np.full(pp, SENTINEL), Ainv=np.full(pp, SENTINEL), beta=np.full(p, SENTINEL),
        scal=np.full(2, SENTINEL), info=np.full(1, SENTINEL))
    return LA.reshape(p, p), Ainv.reshape(p, p), beta, scal, int(info[0])


@pytest.mark.parametrize("p", [1, 5, 33, 64])
def test_finish(gpm, p):
    """A = L L^T with _factor's L: the factor comes back exactly; the rest against numpy"""
    rng = np.random.default_rng(400 + p)
    L = _factor(rng, p)
    A = L @ L.T
    g = rng.integers(-9, 10, p).astype(float)
    Ag = np.concatenate([np.where(np.tril(np.ones((p, p), bool)), A, np.nan), g[:, None]], axis=1)  # the upper half is not read
    LA, Ainv, beta, scal, info = _finish(gpm, Ag, p)
    assert info == 0
    np.testing.assert_array_equal(LA, L)
    want_inv = np.linalg.inv(A)
    want_beta = want_inv @ g
    err = lambda a, b: np.abs(a - b).max() / np.abs(b).max()  # noqa: E731
    print("p = %d: Ainv %.3e, beta %.3e, log|A| %.3e, g^T beta %.3e relative; cond(A) = %.2e"
          % (p, err(Ainv, want_inv), err(beta, want_beta), abs(scal[0] - np.linalg.slogdet(A)[1]),
             abs(scal[1] - g @ want_beta) / abs(g @ want_beta), np.linalg.cond(A)))
    # (the inverse of this A is L^-T L^-1 with an integer-over-power-of-two L^-1: numpy's own error ~ cond(A) * 2.2e-16)
    tol = max(1e-12, 4.0 * np.linalg.cond(A) * 2.2e-16)
    assert err(Ainv, want_inv) <= tol and err(beta, want_beta) <= tol
    np.testing.assert_array_equal(Ainv, Ainv.T)
    assert abs(scal[0] - 2.0 * np.log(np.diag(L)).sum()) <= 1e-12 * max(1.0, abs(scal[0]))
    assert abs(scal[1] - g @ want_beta) <= tol * abs(g @ want_beta)


@pytest.mark.parametrize("A,want", [([[1.0, 1.0], [1.0, 1.0]], 2), ([[1.0, 2.0], [2.0, 1.0]], 2), ([[-1.0, 0.0], [0.0, 1.0]], 1),
                                    ([[0.0, 0.0], [0.0, 1.0]], 1), ([[4.0, 2.0], [2.0, np.nan]], 2),
                                    ([[1.0, 0.0], [0.0, np.inf]], 2)])
def test_finish_reports_a_bad_pivot(gpm, A, want):
    """A zero, negative or non-finite pivot is a status, not a fault: info = pivot + 1, nothing else is written"""
    Ag = np.concatenate([np.array(A), np.ones((2, 1))], axis=1)
    LA, Ainv, beta, scal, info = _finish(gpm, Ag, 2)
    assert info == want
    for out in (LA, Ainv, beta, scal):
        np.testing.assert_array_equal(out, SENTINEL)


# ---- basis_cols_kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld,p", [(2, 256, 1), (65, 256, 3), (300, 512, 33), (1100, 1280, 64)])
def test_cols(gpm, n, ld, p):
    rng = np.random.default_rng(500 + n)
    rows = (p + 1 + 3) // 4 * 4
    Wt = np.full((p, ld), 7.0)
    Wt[:, :n] = rng.integers(-8, 9, (p, n))
    L = _factor(rng, p)
    beta = rng.integers(-5, 6, p).astype(float)
    alpha = np.full(ld, 9.0)
    alpha[:n] = rng.integers(-50, 51, n)
    Ct = gpm.basis_kernel_check("basis_cols", Wt=Wt, ld=ld, n=n, p=p, LA=L, beta=beta, alpha=alpha,
                                Ct=np.full((rows + 1, ld), SENTINEL)).reshape(rows + 1, ld)
    np.testing.assert_array_equal(Ct[p, :n], alpha[:n] - Wt[:, :n].T @ beta)  # integers: exact
    want = np.linalg.solve(L, Wt[:, :n])
    scale = np.abs(want).max()
    print("n = %d p = %d: Q^T max |err| %.3e of %.3e" % (n, p, np.abs(Ct[:p, :n] - want).max(), scale))
    if p <= 3:
        np.testing.assert_array_equal(Ct[:p, :n], want)  # small integers over powers of two: exact
    assert np.abs(Ct[:p, :n] - want).max() <= 1e-12 * scale
    for rest in (Ct[:rows, n:], Ct[p + 1:rows, :]):
        assert rest.size == 0 or (not rest.any() and not np.signbit(rest).any())
    np.testing.assert_array_equal(Ct[rows:], SENTINEL)


# ---- basis_predict_kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,p", [(1, 1), (70, 5), (200, 64)])
def test_predict(gpm, m, p):
    rng = np.random.default_rng(600 + m)
    ldkw = 128
    Hz = rng.integers(-4, 5, (m, p)).astype(float)
    KW = np.full((m, ldkw), 11.0)
    KW[:, :p] = rng.integers(-4, 5, (m, p))
    beta = rng.integers(-5, 6, p).astype(float)
    B = rng.integers(-2, 3, (p, p)).astype(float)
    Ainv = B @ B.T + np.eye(p)
    mu0, q = rng.integers(-20, 21, m).astype(float), rng.integers(0, 5, m).astype(float)
    prior = q + rng.integers(1, 4, m)
    mu, sigma = gpm.basis_kernel_check("basis_predict", Hz=Hz, KW=KW, ldkw=ldkw, m=m, p=p, beta=beta, Ainv=Ainv, mu0=mu0,
                                       prior=prior, q=q, mu=np.full(m + 1, SENTINEL), sigma=np.full(m + 1, SENTINEL))
    Rm = Hz - KW[:, :p]
    np.testing.assert_array_equal(mu[:m], mu0 + Rm @ beta)
    np.testing.assert_allclose(sigma[:m], np.sqrt(prior - q + ((Rm @ Ainv) * Rm).sum(1)), rtol=1e-12, atol=0.0)
    assert mu[m] == SENTINEL and sigma[m] == SENTINEL


def test_predict_does_not_clamp_the_variance(gpm):
    """As Produce (solve.hip: sigma_kernel): a negative variance shows as NaN instead of a silent zero"""
    one = np.ones(1)
    mu, sigma = gpm.basis_kernel_check("basis_predict", Hz=one, KW=np.ones(128), ldkw=128, m=1, p=1, beta=one, Ainv=one,
                                       mu0=one, prior=one, q=2.0 * one, mu=np.zeros(1), sigma=np.zeros(1))
    assert mu[0] == 1.0 and np.isnan(sigma[0])
