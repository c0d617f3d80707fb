"""Explicit basis functions (gogp_basis_*): a mean h(x)^T beta with beta integrated out under a flat prior (Rasmussen &
Williams section 2.7, eq. 2.41 - 2.45 in the limit B^-1 -> 0).  The numpy fp64 reference its tests share, built on
loo_ref.gram (K with the noise on its diagonal, and the list dK / d log theta_p).  Families, events, noise and inputs:
those of tests/produce_grad_ref.py.

    W = K^-1 H,  A = H^T W,  g = H^T alpha,  beta = A^-1 g,  alpha~ = alpha - W beta,
    lml_b = lml_0 + 1/2 g^T beta - 1/2 log|A| + p/2 log 2 pi,
    grad_p = 1/2 sum_ab (alpha~ alpha~^T + W A^-1 W^T - K^-1)_ab (dK_p)_ab,
    R = Hz - Ks^T W,  mu_b = Ks^T alpha + R beta,  sigma_b^2 = k(z, z) - diag(Ks^T K^-1 Ks) + diag(R A^-1 R^T).

The cases of tests/test_basis_gpu.py are listed here (GPU_CASES) so that tests/test_basis_cpu.py can hold the reference
of every one of them to cond(A) <= 1e6.
"""
import numpy as np

import events_ref as R
import loo_ref as LR
from gogp_amd import basis, kernel
from oracle.oracle import gram_np
from produce_grad_ref import EVENTS, FAMILIES as PG_FAMILIES, NOISE, TN, inputs  # noqa: F401  (shared with the tests)

LOG_2PI = float(np.log(2.0 * np.pi))

RADIAL = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8]),
    "matern52": (2, kernel.Scaled(kernel.Matern52), [1.2, 0.9]),
    "matern52textbook": (2, kernel.Scaled(kernel.Matern52Textbook), [0.9, 1.1]),
}
#: the families of multi_output_ref.FAMILIES (= produce_grad_ref.FAMILIES) plus the four radial kinds, as
#: tests/test_multi_output_gpu.py combines them; "events" is produce_grad_ref's matern52 under EVENTS
FAMILIES = dict(PG_FAMILIES, **RADIAL)
SHAPE_FAMILY = "ard_rbf3"
#: (n, p) of the shape cases, (p) of the column-count cases at n = 300, the test-point counts
SHAPES = ((2, 1), (20, 3), (128, 4), (129, 5), (300, 33), (1100, 64))
COUNTS = (1, 3, 4, 5, 33, 64)
MS = (1, 70, 200)
EVENT_FAMILY = "matern52"
#: every (family, n, p, events) the GPU file runs against this reference
GPU_CASES = ([(SHAPE_FAMILY, n, p, False) for n, p in SHAPES] + [(SHAPE_FAMILY, 300, p, False) for p in COUNTS]
             + [(f, 300, 3, False) for f in sorted(FAMILIES)] + [(EVENT_FAMILY, 300, 3, True)]
             + [("matern52", 129, 3, False)])


def log_theta(fam):
    return np.log(np.array(list(FAMILIES[fam][2]) + TN))


def case_basis(X, Z, p, seed=17):
    """(H, Hz) with p columns: a polynomial of degree <= 2 in coordinates scaled to [-1, 1] for small p (1: the
    constant; 3: degree 2 in x_0; 4: degree 3 in x_0 where D < 3, degree 1 in x_0 .. x_2 otherwise; 5: degree 2 in
    x_0, x_1 where D >= 2, degree 4 in x_0 otherwise), the constant plus sqrt(n) times orthonormal random columns (a
    seeded QR) beyond: H^T H = n I then.  Hz: the same polynomial in the frame of X; random rows for the random basis,
    which has no meaning off the inputs -- the formulas hold for any Hz."""
    X, Z = np.asarray(X, float), np.asarray(Z, float)
    n, D = X.shape
    if p <= 5:
        if p == 1:
            deg, axes = 0, [0]
        elif p == 3:
            deg, axes = 2, [0]
        elif p == 4:
            deg, axes = (1, [0, 1, 2]) if D >= 3 else (3, [0])
        elif p == 5:
            deg, axes = (2, [0, 1]) if D >= 2 else (4, [0])
        else:
            raise ValueError("no polynomial case with %d columns" % p)
        c, s = basis.polynomial_frame(X, axes)
        H, Hz = basis.polynomial(X, deg, axes, c, s), basis.polynomial(Z, deg, axes, c, s)
        assert H.shape[1] == p
        return H, Hz
    rng = np.random.default_rng(seed + p)
    M = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, p - 1))], axis=1)
    Q, Rr = np.linalg.qr(M)
    Q = Q * np.sign(np.diag(Rr))[None, :] * np.sqrt(n)  # column 0: exactly the constant up to rounding
    Q[:, 0] = 1.0
    Hz = np.concatenate([np.ones((len(Z), 1)), rng.normal(size=(len(Z), p - 1))], axis=1)
    return np.ascontiguousarray(Q), np.ascontiguousarray(Hz)


def dense(K, y, H, dK=None):
    """dict(beta, cov, alpha (alpha~), lml, lml0, grad or None, W, A, condA) from the dense K."""
    y, H = np.asarray(y, float), np.asarray(H, float)
    n, p = H.shape
    L = np.linalg.cholesky(K)
    solve = lambda B: np.linalg.solve(L.T, np.linalg.solve(L, B))  # noqa: E731
    alpha, W = solve(y), solve(H)
    A = H.T @ W
    A = 0.5 * (A + A.T)
    g = H.T @ alpha
    LA = np.linalg.cholesky(A)
    beta = np.linalg.solve(LA.T, np.linalg.solve(LA, g))
    cov = np.linalg.inv(A)
    cov = 0.5 * (cov + cov.T)
    at = alpha - W @ beta
    lml0 = -0.5 * y @ alpha - np.log(np.diag(L)).sum() - 0.5 * n * LOG_2PI
    lml = lml0 + 0.5 * g @ beta - np.log(np.diag(LA)).sum() + 0.5 * p * LOG_2PI
    grad = None
    if dK is not None:
        Kinv = np.linalg.inv(K)
        Kinv = 0.5 * (Kinv + Kinv.T)
        Wm = np.outer(at, at) + W @ cov @ W.T - Kinv
        grad = np.array([0.5 * (Wm * d).sum() for d in dK])
    return dict(beta=beta, cov=cov, alpha=at, lml=lml, lml0=lml0, grad=grad, W=W, A=A, condA=np.linalg.cond(A))


def cross(D, simil, lt, X, Z, events=None, axis=0):
    """(Ks n x m, prior m) at the test points."""
    desc = kernel.build_desc(D, simil, NOISE)
    ths = np.exp(np.asarray(lt, float))[:-1]
    X, Z = np.asarray(X, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    prior = np.diag(gram_np(desc, ths, Z, Z)).copy()
    Ks = gram_np(desc, ths, X, Z)
    if events:
        Ks = Ks * R.discount_matrix(events, Z[:, axis], X[:, axis]).T
    return Ks, prior


def produce_dense(K, Ks, prior, d, Hz):
    """(mu_b, sigma_b, mu_0, sigma_0) from K, the cross-covariances, the prior variances, dense()'s dict and Hz."""
    V = np.linalg.solve(np.linalg.cholesky(K), Ks)
    alpha = d["alpha"] + d["W"] @ d["beta"]
    Rm = Hz - Ks.T @ d["W"]
    var0 = prior - (V * V).sum(0)
    mu0 = Ks.T @ alpha
    return mu0 + Rm @ d["beta"], np.sqrt(var0 + ((Rm @ d["cov"]) * Rm).sum(1)), mu0, np.sqrt(var0)


def reference(D, simil, lt, X, y, H, events=None, axis=0, want_grad=True):
    if want_grad:
        K, dK = LR.gram(D, simil, lt, X, events, axis, want_grad=True)
    else:
        K, dK = LR.gram(D, simil, lt, X, events, axis), None
    return K, dense(K, y, H, dK)


_CASES = {}


def case(fam, n, p, events=False, want_grad=True):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, n, p, bool(events), want_grad)
    if key not in _CASES:
        D, simil, _ = FAMILIES[fam]
        ev = EVENTS if events else None
        X, y, _ = inputs(n, 1, D)
        Z = inputs(1, max(MS), D)[2]
        H, Hz = case_basis(X, Z, p)
        y = y + 25.0 + H @ np.linspace(1.0, -1.0, p)  # a mean worth estimating
        lt = log_theta(fam)
        K, d = reference(D, simil, lt, X, y, H, ev, want_grad=want_grad)
        Ks, prior = cross(D, simil, lt, X, Z, ev)
        mu, sigma, mu0, sigma0 = produce_dense(K, Ks, prior, d, Hz)
        _CASES[key] = dict(d, X=X, y=y, Z=Z, H=H, Hz=Hz, K=K, mu=mu, sigma=sigma, mu0=mu0, sigma0=sigma0, lt=lt)
    return _CASES[key]
