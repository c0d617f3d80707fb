"""Leave-one-out cross-validation (gogp_loo, gogp_loo_gradient): the numpy references its tests share.  Families,
events, noise and inputs: those of tests/produce_grad_ref.py.

Two independent things (Rasmussen & Williams section 5.4.2):

  * brute_force: the definition.  For every i the process is refitted to the other n - 1 rows with numpy.linalg and
    predicts y_i; none of the closed forms below is used:
        mu_i = k_i^T K_-i^-1 y_-i,  sigma_i^2 = K_ii - k_i^T K_-i^-1 k_i,
        log p_i = -1/2 log(2 pi sigma_i^2) - (y_i - mu_i)^2 / (2 sigma_i^2)
    (K carries the noise on its diagonal: K_ii is the prior variance of the noisy observation);
  * closed_form: with kappa_i = [K^-1]_ii from np.linalg.inv and alpha = K^-1 y,
        mu_i = y_i - alpha_i / kappa_i,  sigma_i^2 = 1 / kappa_i,
        log p_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi,
        d sum_i log p_i / d log theta_p = sum_ab W_ab dK_ab / d log theta_p,
        W = 1/2 (u alpha^T + alpha u^T) - K^-1 diag(w) K^-1,  v = alpha / kappa,  u = K^-1 v,
        w = 1/2 (1 + alpha^2 / kappa) / kappa,
    the noise parameter (UniformNoise: variance theta_n^2) with dK / d log theta_n = 2 theta_n^2 I.
"""
import numpy as np

import events_ref as R
from gogp_amd import kernel
from oracle.oracle import gram_np
from produce_grad_ref import EVENTS, FAMILIES, FOUR, NOISE, TN, inputs  # noqa: F401  (shared with the tests)

LOG_2PI = float(np.log(2.0 * np.pi))


def gram(D, simil, log_theta, X, events=None, axis=0, want_grad=False):
    """K = k(X, X) + theta_n^2 I at theta = exp(log_theta) = [theta_simil | theta_n] and, want_grad, the list of
    dK / d log theta_p, the noise parameter last; event discounts applied to the similarity."""
    desc = kernel.build_desc(D, simil, NOISE)
    th = np.exp(np.asarray(log_theta, dtype=float))
    ths, tn = th[:-1], th[-1]
    X = np.asarray(X, float).reshape(-1, D)
    n = len(X)
    out = gram_np(desc, ths, X, X, want_grad=want_grad)
    K, dK = out if want_grad else (out, None)
    if events:
        Dm = R.discount_matrix(events, X[:, axis], X[:, axis])
        K = K * Dm
        dK = [d * Dm for d in dK] if want_grad else None
    K = K + tn * tn * np.eye(n)
    if want_grad:
        return K, list(dK) + [2.0 * tn * tn * np.eye(n)]
    return K


def brute_force(K, y):
    """(mu, sigma, logp) by n refits on n - 1 rows each."""
    y = np.asarray(y, float)
    n = len(y)
    mu, sigma, logp = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        L = np.linalg.cholesky(K[np.ix_(keep, keep)])
        k = K[keep, i]
        a = np.linalg.solve(L.T, np.linalg.solve(L, y[keep]))
        q = np.linalg.solve(L, k)
        mu[i] = k @ a
        var = K[i, i] - q @ q
        sigma[i] = np.sqrt(var)
        logp[i] = -0.5 * np.log(2.0 * np.pi * var) - 0.5 * (y[i] - mu[i]) ** 2 / var
    return mu, sigma, logp


def closed_form(K, y, dK=None):
    """(mu, sigma, logp) and, with the list dK of derivative matrices, the gradient of sum(logp) (else None)."""
    y = np.asarray(y, float)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(K, y)
    kap = np.diag(Kinv).copy()
    mu = y - alpha / kap
    sigma = np.sqrt(1.0 / kap)
    logp = 0.5 * np.log(kap) - 0.5 * alpha * alpha / kap - 0.5 * LOG_2PI
    grad = None
    if dK is not None:
        u = Kinv @ (alpha / kap)
        w = 0.5 * (1.0 + alpha * alpha / kap) / kap
        W = 0.5 * (np.outer(u, alpha) + np.outer(alpha, u)) - (Kinv * w[None, :]) @ Kinv
        grad = np.array([(W * d).sum() for d in dK])
    return mu, sigma, logp, grad


def reference(D, simil, log_theta, X, y, events=None, axis=0):
    """The dense closed form at exp(log_theta): (mu, sigma, logp, grad)."""
    K, dK = gram(D, simil, log_theta, X, events, axis, want_grad=True)
    return closed_form(K, y, dK)
