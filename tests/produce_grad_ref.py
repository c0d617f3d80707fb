"""GP.ProduceGradient (gogp_produce_gradient): the inputs its tests share and the dense numpy reference, on top of the
oracle's gram_np / xgrad_np.

    K  = k(X, X) + noise_var I = L L^T,  alpha = K^-1 y,  Ks = k(X, Z),  W^T = (K^-1 Ks)^T          (m x n)
    mu = Ks^T alpha,  sigma^2 = k(z, z) - diag(Ks^T K^-1 Ks)
    dmu    = sum_i alpha_i dk(z_j, x_i)/dz_j                = xgrad_np(Z, X, tile(alpha))
    dsigma = -2 sum_i W_ij dk(z_j, x_i)/dz_j / (2 sigma_j)  = -2 xgrad_np(Z, X, W^T) / (2 sigma)

k(z, z) of every family is the sum of the output scales: it does not depend on z.  With event discounts Ks and both
weight matrices carry the pairs' discounts (piecewise constant in z).
"""
import numpy as np

import events_ref as R
from gogp_amd import kernel
from oracle.oracle import gram_np, xgrad_np

D64 = 64
EVENTS = kernel.parse_events(R.SELFCHECK)
NOISE = kernel.UniformNoise
TN = [0.3]  # noise variance 0.09

#: name -> (NDim, Simil, theta_simil); the noise is UniformNoise with std 0.3 throughout
FAMILIES = {
    "matern52": (1, kernel.Scaled(kernel.Matern52), [1.0, 0.7]),
    "ard_rbf3": (3, kernel.Scaled(kernel.ARD(kernel.Normal, 3)), [1.2, 0.9, 1.0, 1.1]),
    "hyperpriors": (1, kernel.Sum([kernel.Scaled(kernel.Matern52),
                                   kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))], order=[0, 2, 1, 3, 4]),
                    [1.0, 0.5, 0.6, 1.3, 0.05]),
    "matern32_2d": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8]),
    "ard_rbf64": (D64, kernel.Scaled(kernel.ARD(kernel.Normal, D64)),
                  [1.1] + list(np.sqrt(D64 / 6.0) * (1 + np.arange(D64) / (2.0 * D64)))),
}
FOUR = ["matern52", "ard_rbf3", "hyperpriors", "matern32_2d"]


def inputs(n, m, D, seed=7):
    """X uniform in [-2, 2]^D, Z uniform in [-2.5, 2.5]^D, y = sin(sum x) + 0.1 noise."""
    rng = np.random.default_rng(seed + 1000 * D)
    X = rng.uniform(-2.0, 2.0, (n, D))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=n)
    Z = rng.uniform(-2.5, 2.5, (m, D))
    return X, y, Z


def event_inputs(n, m, seed=7, margin=1e-3):
    """The same for the events kernel: no test point within `margin` of an event boundary."""
    X, y, Z = inputs(n, m, 1, seed)
    bounds = np.array([b for e in EVENTS for b in e[:2]])
    for j in range(m):
        while np.abs(Z[j, 0] - bounds).min() < margin:
            Z[j, 0] += 2 * margin
    return X, y, Z, bounds


def reference(D, simil, ts, X, y, Z, noise_var=TN[0] ** 2, events=None, axis=0):
    """(mu, sigma, dmu, dsigma) of the dense GP; `simil` without its events, which are given apart."""
    desc = kernel.build_desc(D, simil, NOISE)
    ths = np.asarray(ts, dtype=float)
    X, Z = np.asarray(X, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    n, m = len(X), len(Z)
    prior = np.diag(gram_np(desc, ths, Z, Z)).copy()
    if n == 0:
        return np.zeros(m), np.sqrt(prior), np.zeros((m, D)), np.zeros((m, D))
    K = gram_np(desc, ths, X, X)
    Ks = gram_np(desc, ths, X, Z)
    Dm = np.ones((m, n))
    if events:
        K = K * R.discount_matrix(events, X[:, axis], X[:, axis])
        Dm = R.discount_matrix(events, Z[:, axis], X[:, axis])
        Ks = Ks * Dm.T
    K = K + noise_var * np.eye(n)
    L = np.linalg.cholesky(K)
    al = np.linalg.solve(L.T, np.linalg.solve(L, y))
    V = np.linalg.solve(L, Ks)
    Wt = np.linalg.solve(L.T, V).T
    mu = Ks.T @ al
    sigma = np.sqrt(prior - (V * V).sum(0))
    dmu = xgrad_np(desc, ths, Z, X, np.tile(al, (m, 1)) * Dm)
    dsigma = -2.0 * xgrad_np(desc, ths, Z, X, Wt * Dm) / (2.0 * sigma)[:, None]
    return mu, sigma, dmu, dsigma


def assert_derivative(got, want, tag=""):
    """A derivative array lies within 1e-6 of its largest absolute component (the suite's rule for gradients)."""
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got) - want).max()
    print("%s: max |err| = %.3e of largest component %.3e (%.2e relative)" % (tag, err, scale, err / scale))
    assert err <= 1e-6 * scale, (tag, err, scale)
