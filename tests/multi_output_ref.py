"""Multi-output (gogp_multi_*): T output columns at shared inputs, kernel and hyperparameters.  The numpy reference its
tests share, built on loo_ref.gram (K with the noise on its diagonal, and the list dK / d log theta_p).  Families,
events, noise and inputs: those of tests/produce_grad_ref.py.

    L = cholesky(K),  A = K^-1 Y,
    lml_t = -1/2 y_t^T a_t - sum_i log L_ii - n/2 log 2 pi,          total = sum_t lml_t,
    grad_p = 1/2 sum_ab (A A^T - T K^-1)_ab (dK_p)_ab,
    mu = Ks^T A (m x T),  sigma^2 = k(z, z) - diag(Ks^T K^-1 Ks)  (shared by the outputs, no noise).
"""
import numpy as np

import events_ref as R
import loo_ref as LR
from gogp_amd import kernel
from oracle.oracle import gram_np
from produce_grad_ref import EVENTS, FAMILIES, NOISE, TN, inputs  # noqa: F401  (shared with the tests)

LOG_2PI = float(np.log(2.0 * np.pi))


def outputs(X, T, y0=None, seed=3):
    """n x T: column t = a_t sin(sum x + phi_t) + 0.1 noise from a fixed seed; column 0 = y0 (the handle's own y)."""
    rng = np.random.default_rng(seed)
    n = len(X)
    a, phi = rng.uniform(0.5, 1.5, T), rng.uniform(0.0, 2.0 * np.pi, T)
    Y = a[None, :] * np.sin(X.sum(1)[:, None] + phi[None, :]) + 0.1 * rng.normal(size=(n, T))
    if y0 is not None:
        Y[:, 0] = y0
    return np.ascontiguousarray(Y)


def dense(K, Y, dK=None):
    """(A, lml (T), grad or None) from the dense K."""
    Y = np.asarray(Y, float)
    n, T = Y.shape
    L = np.linalg.cholesky(K)
    A = np.linalg.solve(L.T, np.linalg.solve(L, Y))
    lml = -0.5 * (Y * A).sum(0) - np.log(np.diag(L)).sum() - 0.5 * n * LOG_2PI
    grad = None
    if dK is not None:
        Kinv = np.linalg.inv(K)
        Kinv = 0.5 * (Kinv + Kinv.T)
        W = A @ A.T - T * Kinv
        grad = np.array([0.5 * (W * d).sum() for d in dK])
    return A, lml, grad


def produce(D, simil, log_theta, X, A, Z, events=None, axis=0):
    """(mu m x T, sigma m) at the test points Z for the solutions A."""
    desc = kernel.build_desc(D, simil, NOISE)
    ths = np.exp(np.asarray(log_theta, float))[:-1]
    X, Z = np.asarray(X, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    prior = np.diag(gram_np(desc, ths, Z, Z)).copy()
    if len(X) == 0:
        return np.zeros((len(Z), A.shape[1])), np.sqrt(prior)
    Ks = gram_np(desc, ths, X, Z)
    if events:
        Ks = Ks * R.discount_matrix(events, Z[:, axis], X[:, axis]).T
    K = LR.gram(D, simil, log_theta, X, events, axis)
    V = np.linalg.solve(np.linalg.cholesky(K), Ks)
    return Ks.T @ A, np.sqrt(prior - (V * V).sum(0))


def reference(D, simil, log_theta, X, Y, events=None, axis=0):
    """(A, lml, grad) of the dense process at exp(log_theta)."""
    K, dK = LR.gram(D, simil, log_theta, X, events, axis, want_grad=True)
    return dense(K, Y, dK)
