"""The Hessian of the LML in the log hyperparameters (gogp_lml_hessian): the numpy reference its tests share, in
np.longdouble and without any second derivative of the kernel.

The analytic gradient 1/2 tr(W K_p), W = alpha alpha^T - K^-1, from the descriptor evaluation the other references
have (gram_ref.pair_values for K, grad_reduce_ref.slot_sums / assemble for the sums over W) on a long-double Cholesky
inverse, is differentiated by central differences in log theta at the steps h = 1e-3 and h / 2 and Richardson-
extrapolated.  The tolerance of a comparison comes from the reference alone: entrywise 10 |H(h) - H(extrapolated)|, the
truncation the extrapolation removed, plus 1e-9 max|H| for the fp64 arithmetic of the device.
"""
import numpy as np

import gram_ref as GR
import grad_reduce_ref as G
from gogp_amd import kernel
from handle_state_ref import inputs

LD = np.longdouble
H_STEP = 1e-3

#: name -> (NDim, similarity, noise, theta): the three descriptors of the tests
CASES = {
    "ard": (3, kernel.Scaled(kernel.ARD(kernel.Normal, 3)), kernel.UniformNoise, [1.0, 0.7, 0.9, 1.3, 0.1]),
    "sum": (1, kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))]),
            kernel.ConstantNoiseParam(0.1), [1.0, 0.6, 0.5, 0.8, 0.07, 0.3]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), kernel.UniformNoise, [1.2, 0.6, 0.15]),
}


def data(name, n):
    """(D, simil, noise, X, y, x = log theta) of one case at n rows: the leading coordinates of handle_state_ref.inputs."""
    D, simil, noise, theta = CASES[name]
    c = inputs(n)
    return D, simil, noise, np.ascontiguousarray(c.X[:, :D]), c.y, np.log(np.array(theta))


def inverse(K):
    """K^-1 of a symmetric positive definite long-double matrix, by its Cholesky factor."""
    n = len(K)
    L, Li = np.zeros_like(K), np.zeros_like(K)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    for i in range(n):
        Li[i, i] = 1 / L[i, i]
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
    return Li.T @ Li


def parts(desc, x, X, y):
    """(kp, K^-1, alpha) at x = log theta, long doubles."""
    th = np.exp(np.asarray(x, float))
    kp = G.kp_from_desc(desc, th[:desc.ntheta_simil], th[desc.ntheta_simil:])
    Kinv = inverse(GR.pair_values(kp, X, X, "ld", diag_noise=True)[0])
    return kp, Kinv, Kinv @ y.astype(LD)


def gradient(desc, x, X, y):
    kp, Kinv, alpha = parts(desc, x, X, y)
    slots = G.slot_sums(kp, X, len(X), alpha, [Kinv])[0][0]
    return G.assemble(desc, slots, kp.dnoise)


_CACHE = {}


def hessian(name, n):
    """(H, tol) of one case, both (P, P) float64, computed once."""
    if (name, n) not in _CACHE:
        D, simil, noise, X, y, x = data(name, n)
        desc = kernel.build_desc(D, simil, noise)

        def diff(h):
            rows = []
            for p in range(len(x)):
                e = np.zeros(len(x))
                e[p] = h
                rows.append((gradient(desc, x + e, X, y) - gradient(desc, x - e, X, y)) / (2 * LD(h)))
            return np.array(rows)

        d1, d2 = diff(H_STEP), diff(H_STEP / 2)
        H = (4 * d2 - d1) / 3
        tol = 10 * np.abs(d1 - H) + 1e-9 * np.abs(H).max()
        _CACHE[name, n] = (H.astype(np.float64), tol.astype(np.float64))
    return _CACHE[name, n]
