"""Sparse multi-output (gogp_sparse_multi_*): the matrix form in numpy that its tests share, on the quantities of
tests/sparse_ref.py (blocks, the chunked walk) and the oracle's xgrad_np.

Y is N x T with columns y_t; kernel, theta, noise s2, jitter eps and U are shared.  L, V, B, Yu = L^-T, t0 as in sparse_ref:

    R = V Y (M x T),  Gamma = B^-1 R,  c0 = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - (t0 - s2 (tr B - M)) / (2 s2),
    bound_t = c0 - y_t^T y_t / (2 s2) + r_t^T gamma_t / (2 s2^2),      total = sum_t bound_t (column order),
    Tm = T (I - B^-1) - Gamma Gamma^T / s2^2,  P = Yu Tm Yu^T / (2 s2),  Mm = Yu Gamma,  W = 2 P k(U, X) + Mm Y^T / s2^2,
    G = 1/2 Yu (T (2 I - B - B^-1) - Gamma Gamma^T / s2^2) Yu^T,
    d total / d log theta_p = sum W dKuf_p + sum G dKuu_p - T / (2 s2) sum_f dk(x_f, x_f)_p,
    d total / d s2 = T [(M - tr B^-1) / (2 s2) - N / (2 s2) + (t0 - s2 (tr B - M)) / (2 s2^2)] + tr(Y^T Y) / (2 s2^2)
                     - tr(R^T Gamma) / s2^3 + (tr(R^T Gamma) - tr(Gamma^T Gamma)) / (2 s2^3),
    d total / d u_ad = sum_f W_af dk(u_a, x_f)/du_ad + 2 sum_b G_ab dk(u_a, u_b)/du_ad,
    mu(z)[t] = v^T gamma_t / s2,   sigma(z) as sparse_ref.produce.

`reference` is chunk-free, `reference_chunked` walks X in chunks and never holds anything of size N x M.
"""
import numpy as np

import sparse_ref as SR
from oracle.oracle import gram_np, xgrad_np


class State:
    """What the multi observe leaves behind for the gradient and Produce."""


def _finish(st, N, M, T, s2, yty, t0, A, R, L):
    """yty: the T sums y_t^T y_t; A = V V^T; R = V Y."""
    B = np.eye(M) + A / s2
    LB = np.linalg.cholesky(B)
    Binv = np.linalg.inv(B)
    Binv = 0.5 * (Binv + Binv.T)
    Gam = np.linalg.solve(LB.T, np.linalg.solve(LB, R))
    trBmM = np.trace(A) / s2
    c0 = -0.5 * N * SR.LOG_2PI - np.log(np.diag(LB)).sum() - 0.5 * N * np.log(s2) - (t0 - s2 * trBmM) / (2 * s2)
    rtg, gtg = (R * Gam).sum(0), (Gam * Gam).sum(0)
    st.bounds = c0 - yty / (2 * s2) + rtg / (2 * s2 * s2)
    st.total = 0.0
    for b in st.bounds:  # column order
        st.total += b
    st.N, st.M, st.T, st.s2, st.L, st.B, st.Binv, st.Gam, st.R = N, M, T, s2, L, B, Binv, Gam, R
    Yu = np.linalg.inv(L).T
    GG = Gam @ Gam.T / (s2 * s2)
    st.Yu = Yu
    st.P = Yu @ (T * (np.eye(M) - Binv) - GG) @ Yu.T / (2 * s2)
    st.Mm = Yu @ Gam
    st.G = 0.5 * Yu @ (T * (2 * np.eye(M) - B - Binv) - GG) @ Yu.T
    st.dF_ds2 = (T * ((M - np.trace(Binv)) / (2 * s2) - N / (2 * s2) + (t0 - s2 * trBmM) / (2 * s2 * s2))
                 + yty.sum() / (2 * s2 * s2) - rtg.sum() / s2 ** 3 + (rtg.sum() - gtg.sum()) / (2 * s2 ** 3))
    return st


def reference(D, simil, log_theta, X, Y, U, eps, want_grad=True):
    """(total, bounds (T), grad or None, dU (M x D) or None, state): chunk-free."""
    x = np.asarray(log_theta, float)
    X, U = np.asarray(X, float).reshape(-1, D), np.asarray(U, float).reshape(-1, D)
    Y = np.asarray(Y, float).reshape(len(X), -1)
    T = Y.shape[1]
    Kuu, Kuf, kff, dK = SR.blocks(D, simil, x, U, X, want_grad)
    M, N = Kuf.shape
    s2 = float(np.exp(2.0 * x[-1]))
    L = np.linalg.cholesky(Kuu + eps * np.eye(M))
    V = np.linalg.solve(L, Kuf)
    st = _finish(State(), N, M, T, s2, (Y * Y).sum(0), kff.sum(), V @ V.T, V @ Y, L)
    st.Kuu = Kuu
    grad = dU = None
    if want_grad:
        W = 2.0 * st.P @ Kuf + st.Mm @ Y.T / (s2 * s2)
        grad = np.array([(W * duf).sum() + (st.G * duu).sum() - T * dff.sum() / (2 * s2) for duu, duf, dff in dK]
                        + [2.0 * s2 * st.dF_ds2])
        desc, ths = SR._desc_ths(D, simil, x)
        dU = xgrad_np(desc, ths, U, X, W) + 2.0 * xgrad_np(desc, ths, U, U, st.G)
    return st.total, st.bounds, grad, dU, st


def reference_chunked(D, simil, log_theta, X, Y, U, eps, chunk, want_grad=True):
    """The same in chunks of `chunk` rows of X: two passes, nothing of size N^2 (or N x M) is kept."""
    x = np.asarray(log_theta, float)
    X, U = np.asarray(X, float).reshape(-1, D), np.asarray(U, float).reshape(-1, D)
    Y = np.asarray(Y, float).reshape(len(X), -1)
    N, M, T = len(X), len(U), Y.shape[1]
    desc, ths = SR._desc_ths(D, simil, x)
    s2 = float(np.exp(2.0 * x[-1]))
    out = gram_np(desc, ths, U, U, want_grad=want_grad)
    Kuu, dKuu = out if want_grad else (out, None)
    L = np.linalg.cholesky(Kuu + eps * np.eye(M))
    A, R, t0 = np.zeros((M, M)), np.zeros((M, T)), N * gram_np(desc, ths, X[:1], X[:1])[0, 0]
    for f0 in range(0, N, chunk):
        V = np.linalg.solve(L, gram_np(desc, ths, U, X[f0:f0 + chunk]))
        A += V @ V.T
        R += V @ Y[f0:f0 + chunk]
    st = _finish(State(), N, M, T, s2, (Y * Y).sum(0), t0, A, R, L)
    st.Kuu = Kuu
    grad = dU = None
    if want_grad:
        grad = np.array([(st.G * d).sum() for d in dKuu] + [2.0 * s2 * st.dF_ds2])
        _, d1 = gram_np(desc, ths, X[:1], X[:1], want_grad=True)
        for p in range(len(ths)):
            grad[p] -= T * N * d1[p][0, 0] / (2 * s2)
        dU = 2.0 * xgrad_np(desc, ths, U, U, st.G)
        for f0 in range(0, N, chunk):
            Xc, Yc = X[f0:f0 + chunk], Y[f0:f0 + chunk]
            Kuf, dKuf = gram_np(desc, ths, U, Xc, want_grad=True)
            W = 2.0 * st.P @ Kuf + st.Mm @ Yc.T / (s2 * s2)
            for p in range(len(ths)):
                grad[p] += (W * dKuf[p]).sum()
            dU += xgrad_np(desc, ths, U, Xc, W)
    return st.total, st.bounds, grad, dU, st


def produce(D, simil, log_theta, st, U, Z, T=None):
    """(mu m x T, sigma m) at the test points from the state of `reference`; latent, unclamped."""
    x = np.asarray(log_theta, float)
    desc, ths = SR._desc_ths(D, simil, x)
    U, Z = np.asarray(U, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    prior = np.array([gram_np(desc, ths, Z[j:j + 1], Z[j:j + 1])[0, 0] for j in range(len(Z))])
    if st is None or st.N == 0:
        return np.zeros((len(Z), T if T is not None else st.T)), np.sqrt(prior)
    v = np.linalg.solve(st.L, gram_np(desc, ths, U, Z))
    mu = v.T @ st.Gam / st.s2
    var = prior - (v * v).sum(0) + (v * (st.Binv @ v)).sum(0)
    return mu, np.sqrt(var)


def outputs(X, T, seed=11):
    """T output columns at the inputs X: smooth functions of different frequencies and offsets plus noise."""
    rng = np.random.default_rng(seed)
    X = np.asarray(X, float)
    w = rng.normal(size=(X.shape[1], T)) * 2.0
    ph = rng.uniform(0, 2 * np.pi, T)
    return np.sin(X @ w + ph) * rng.uniform(0.5, 1.5, T) + 0.1 * rng.normal(size=(len(X), T))
