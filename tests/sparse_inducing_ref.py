"""The derivative of the collapsed bound in the inducing points (gogp_sparse_gradient_inducing): the numpy reference its
tests share, on top of tests/sparse_ref.py and the oracle's xgrad_np.

With W (M x N), G (M x M, symmetric), P and m of sparse_ref (W = 2 P k(U, X) + m y^T / s2^2):

    dF/du_ad = sum_f W_af dk(u_a, x_f)/du_ad  +  2 sum_b G_ab dk(u_a, u_b)/du_ad

The factor 2: u_a enters Kuu through row a and column a.  The jitter eps I and t0 = sum_f k(x_f, x_f) do not depend on
U.  A pair with u_a == u_b or u_a == x_f contributes exact zeros (xgrad_np: every closed form carries the factor
a_d - b_d or sign(a_d - b_d)).

`du_reference` is chunk-free; `du_reference_chunked` walks X in chunks as sparse_ref.reference_chunked does.
"""
import numpy as np

import sparse_ref as SR
from oracle.oracle import gram_np, xgrad_np


def displaced_subset(X, M, seed=5, scale=0.05):
    """M inducing points: a random subset of X displaced by scale * normal (no inducing point on an observation)."""
    rng = np.random.default_rng(seed)
    X = np.asarray(X, float)
    return X[rng.choice(len(X), M, replace=False)] + scale * rng.normal(size=(M, X.shape[1]))


def du_reference(D, simil, log_theta, X, y, U, eps):
    """(bound, grad, dU (M x D), state): chunk-free."""
    x = np.asarray(log_theta, float)
    X, U = np.asarray(X, float).reshape(-1, D), np.asarray(U, float).reshape(-1, D)
    y = np.asarray(y, float).reshape(-1)
    F, grad, st = SR.reference(D, simil, x, X, y, U, eps)
    desc, ths = SR._desc_ths(D, simil, x)
    W = 2.0 * st.P @ gram_np(desc, ths, U, X) + np.outer(st.mvec, y) / (st.s2 * st.s2)
    dU = xgrad_np(desc, ths, U, X, W) + 2.0 * xgrad_np(desc, ths, U, U, st.G)
    return F, grad, dU, st


def du_reference_chunked(D, simil, log_theta, X, y, U, eps, chunk):
    """The same in chunks of `chunk` rows of X: nothing of size N x M is kept."""
    x = np.asarray(log_theta, float)
    X, U = np.asarray(X, float).reshape(-1, D), np.asarray(U, float).reshape(-1, D)
    y = np.asarray(y, float).reshape(-1)
    F, grad, st = SR.reference_chunked(D, simil, x, X, y, U, eps, chunk)
    desc, ths = SR._desc_ths(D, simil, x)
    dU = 2.0 * xgrad_np(desc, ths, U, U, st.G)
    for f0 in range(0, len(X), chunk):
        Xc, yc = X[f0:f0 + chunk], y[f0:f0 + chunk]
        W = 2.0 * st.P @ gram_np(desc, ths, U, Xc) + np.outer(st.mvec, yc) / (st.s2 * st.s2)
        dU += xgrad_np(desc, ths, U, Xc, W)
    return F, grad, dU, st
