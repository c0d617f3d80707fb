"""The inducing-point approximation (gogp_sparse_*): the numpy reference its tests share.  Families, noise and inputs:
those of tests/produce_grad_ref.py (UniformNoise with one parameter, the last of x = log theta).

Collapsed variational bound of Titsias (2009), whitened, with s2 the noise variance and eps the jitter:

    Kuu = k(U, U) + eps I = L L^T,  V = L^-1 k(U, X) (M x N),  B = I + V V^T / s2,  r = V y,  g = B^-1 r,
    t0 = sum_f k(x_f, x_f),
    F = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - y^T y / (2 s2) + r^T g / (2 s2^2) - (t0 - s2 (tr B - M)) / (2 s2).

Gradient, with Y = L^-T:  T = I - B^-1 - g g^T / s2^2,  P = Y T Y^T / (2 s2),  m = Y g,
    W = 2 P k(U, X) + m y^T / s2^2  (M x N),   G = 1/2 Y (2 I - B - B^-1 - g g^T / s2^2) Y^T  (M x M),
    dF/dlog theta_p = sum W dKuf_p + sum G dKuu_p - sum_f dk(x_f, x_f)_p / (2 s2),
    dF/ds2 = (M - tr B^-1) / (2 s2) - N / (2 s2) + y^T y / (2 s2^2) - r^T g / s2^3 + g^T (B - I) g / (2 s2^3)
             + (t0 - s2 (tr B - M)) / (2 s2^2),        noise component = 2 s2 dF/ds2  (s2 = theta_n^2).
Produce at z:  v = L^-1 k(U, z),  mu = v^T g / s2,  sigma^2 = k(z, z) - |v|^2 + v^T B^-1 v.

`reference` is chunk-free and built on loo_ref.gram of the stacked points [U; X]; `reference_chunked` walks X in chunks
(the cross-covariance of a chunk from gram_np) and never holds anything of size N^2.
"""
import numpy as np

import loo_ref as LR
from gogp_amd import kernel
from oracle.oracle import gram_np
from produce_grad_ref import FAMILIES, FOUR, NOISE, TN, inputs  # noqa: F401  (shared with the tests)

LOG_2PI = float(np.log(2.0 * np.pi))


def blocks(D, simil, log_theta, U, X, want_grad=False):
    """Kuu (no jitter, no noise), Kuf, diag Kff and -- want_grad -- the lists of their derivatives in log theta_simil."""
    U, X = np.asarray(U, float).reshape(-1, D), np.asarray(X, float).reshape(-1, D)
    M = len(U)
    S = np.vstack([U, X])
    tn2 = float(np.exp(2.0 * np.asarray(log_theta, float)[-1]))
    out = LR.gram(D, simil, log_theta, S, want_grad=want_grad)
    K, dK = out if want_grad else (out, None)
    K = K - tn2 * np.eye(len(S))  # the noise off the diagonal again
    Kuu, Kuf, kff = K[:M, :M], K[:M, M:], np.diag(K)[M:].copy()
    if not want_grad:
        return Kuu, Kuf, kff, None
    dK = dK[:-1]  # the last one is the noise parameter's
    return Kuu, Kuf, kff, [(d[:M, :M], d[:M, M:], np.diag(d)[M:].copy()) for d in dK]


class State:
    """What the bound leaves behind for the gradient and Produce."""


def _finish(st, N, M, s2, yty, t0, A, r, L):
    B = np.eye(M) + A / s2
    LB = np.linalg.cholesky(B)
    Binv = np.linalg.inv(B)
    Binv = 0.5 * (Binv + Binv.T)
    g = np.linalg.solve(LB.T, np.linalg.solve(LB, r))
    trBmM = np.trace(A) / s2
    F = (-0.5 * N * LOG_2PI - np.log(np.diag(LB)).sum() - 0.5 * N * np.log(s2) - yty / (2 * s2) + r @ g / (2 * s2 * s2)
         - (t0 - s2 * trBmM) / (2 * s2))
    st.N, st.M, st.s2, st.L, st.B, st.Binv, st.g, st.r, st.yty, st.t0, st.trBmM = N, M, s2, L, B, Binv, g, r, yty, t0, trBmM
    st.bound = F
    Y = np.linalg.inv(L).T
    T = np.eye(M) - Binv - np.outer(g, g) / (s2 * s2)
    st.Y = Y
    st.P = Y @ T @ Y.T / (2 * s2)
    st.mvec = Y @ g
    st.G = 0.5 * Y @ (2 * np.eye(M) - B - Binv - np.outer(g, g) / (s2 * s2)) @ Y.T
    st.dF_ds2 = ((M - np.trace(Binv)) / (2 * s2) - N / (2 * s2) + yty / (2 * s2 * s2) - r @ g / s2 ** 3
                 + g @ (B - np.eye(M)) @ g / (2 * s2 ** 3) + (t0 - s2 * trBmM) / (2 * s2 * s2))
    return st


def reference(D, simil, log_theta, X, y, U, eps, want_grad=True):
    """(bound, grad or None, state): chunk-free."""
    x = np.asarray(log_theta, float)
    y = np.asarray(y, float).reshape(-1)
    Kuu, Kuf, kff, dK = blocks(D, simil, x, U, X, want_grad)
    M, N = Kuf.shape
    s2 = float(np.exp(2.0 * x[-1]))
    L = np.linalg.cholesky(Kuu + eps * np.eye(M))
    V = np.linalg.solve(L, Kuf)
    st = _finish(State(), N, M, s2, y @ y, kff.sum(), V @ V.T, V @ y, L)
    st.Kuu = Kuu
    grad = None
    if want_grad:
        W = 2.0 * st.P @ Kuf + np.outer(st.mvec, y) / (s2 * s2)
        grad = np.array([(W * duf).sum() + (st.G * duu).sum() - dff.sum() / (2 * s2) for duu, duf, dff in dK]
                        + [2.0 * s2 * st.dF_ds2])
    return st.bound, grad, st


def _desc_ths(D, simil, x):
    return kernel.build_desc(D, simil, NOISE), np.exp(np.asarray(x, float)[:-1])


def reference_chunked(D, simil, log_theta, X, y, U, eps, chunk, want_grad=True):
    """The same in chunks of `chunk` rows of X: two passes, nothing of size N^2 (or N x M) is kept."""
    x = np.asarray(log_theta, float)
    X, U = np.asarray(X, float).reshape(-1, D), np.asarray(U, float).reshape(-1, D)
    y = np.asarray(y, float).reshape(-1)
    N, M = len(X), len(U)
    desc, ths = _desc_ths(D, simil, x)
    s2 = float(np.exp(2.0 * x[-1]))
    out = gram_np(desc, ths, U, U, want_grad=want_grad)
    Kuu, dKuu = out if want_grad else (out, None)
    L = np.linalg.cholesky(Kuu + eps * np.eye(M))
    # k(x, x) is the sum of the output scales for every family: from one point
    A, r, t0 = np.zeros((M, M)), np.zeros(M), N * gram_np(desc, ths, X[:1], X[:1])[0, 0]
    for f0 in range(0, N, chunk):
        Xc = X[f0:f0 + chunk]
        V = np.linalg.solve(L, gram_np(desc, ths, U, Xc))
        A += V @ V.T
        r += V @ y[f0:f0 + chunk]
    st = _finish(State(), N, M, s2, y @ y, t0, A, r, L)
    st.Kuu = Kuu
    grad = None
    if want_grad:
        grad = np.array([(st.G * d).sum() for d in dKuu] + [2.0 * s2 * st.dF_ds2])
        _, d1 = gram_np(desc, ths, X[:1], X[:1], want_grad=True)
        for p in range(len(ths)):
            grad[p] -= N * d1[p][0, 0] / (2 * s2)
        for f0 in range(0, N, chunk):
            Xc, yc = X[f0:f0 + chunk], y[f0:f0 + chunk]
            Kuf, dKuf = gram_np(desc, ths, U, Xc, want_grad=True)
            W = 2.0 * st.P @ Kuf + np.outer(st.mvec, yc) / (s2 * s2)
            for p in range(len(ths)):
                grad[p] += (W * dKuf[p]).sum()
    return st.bound, grad, st


def produce(D, simil, log_theta, st, U, Z):
    """(mu, sigma) at the test points from the state of `reference`; latent, unclamped."""
    x = np.asarray(log_theta, float)
    desc, ths = _desc_ths(D, simil, x)
    U, Z = np.asarray(U, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    prior = np.array([gram_np(desc, ths, Z[j:j + 1], Z[j:j + 1])[0, 0] for j in range(len(Z))])
    if st is None or st.N == 0:
        return np.zeros(len(Z)), np.sqrt(prior)
    v = np.linalg.solve(st.L, gram_np(desc, ths, U, Z))
    mu = v.T @ st.g / st.s2
    var = prior - (v * v).sum(0) + (v * (st.Binv @ v)).sum(0)
    return mu, np.sqrt(var)


def direct_bound(D, simil, log_theta, X, y, U, eps):
    """The unwhitened form: log N(y | 0, Q + s2 I) - tr(Kff - Q) / (2 s2), Q = Kfu (Kuu + eps I)^-1 Kuf."""
    x = np.asarray(log_theta, float)
    Kuu, Kuf, kff, _ = blocks(D, simil, x, U, X)
    M, N = Kuf.shape
    s2 = float(np.exp(2.0 * x[-1]))
    Q = Kuf.T @ np.linalg.solve(Kuu + eps * np.eye(M), Kuf)
    C = Q + s2 * np.eye(N)
    sign, logdet = np.linalg.slogdet(C)
    y = np.asarray(y, float)
    return -0.5 * N * LOG_2PI - 0.5 * logdet - 0.5 * y @ np.linalg.solve(C, y) - (kff.sum() - np.trace(Q)) / (2 * s2)
