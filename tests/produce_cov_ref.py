"""GP.ProduceCovariance / GP.Sample (gogp_produce_covariance, gogp_produce_samples): the dense numpy reference their
tests share.  Inputs, families, events, noise: those of tests/produce_grad_ref.py.

    K = k(X, X) + noise_var I = L L^T,  alpha = K^-1 y,  Ks = k(X, Z),  V = L^-1 Ks
    mu = Ks^T alpha,  cov = k(Z, Z) - V^T V                                     (m x m, no noise term)

With event discounts k(Z, Z), Ks and K carry the pairs' discounts.
"""
import numpy as np

import events_ref as R
from gogp_amd import kernel
from oracle.oracle import gram_np
from produce_grad_ref import EVENTS, FAMILIES, FOUR, NOISE, TN, event_inputs, inputs  # noqa: F401  (shared with the tests)


def grams(D, simil, ts, X, Z, noise_var=TN[0] ** 2, events=None, axis=0):
    """(K with the noise, Ks, Kzz) of the dense GP, event discounts applied."""
    desc = kernel.build_desc(D, simil, NOISE)
    ths = np.asarray(ts, dtype=float)
    X, Z = np.asarray(X, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    K, Ks, Kzz = gram_np(desc, ths, X, X), gram_np(desc, ths, X, Z), gram_np(desc, ths, Z, Z)
    if events:
        K = K * R.discount_matrix(events, X[:, axis], X[:, axis])
        Ks = Ks * R.discount_matrix(events, X[:, axis], Z[:, axis])
        Kzz = Kzz * R.discount_matrix(events, Z[:, axis], Z[:, axis])
    return K + noise_var * np.eye(len(X)), Ks, Kzz


def reference(D, simil, ts, X, y, Z, events=None, noise_var=TN[0] ** 2, axis=0):
    """(mu, cov) of the dense GP; `simil` without its events, which are given apart."""
    X, Z = np.asarray(X, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    K, Ks, Kzz = grams(D, simil, ts, X, Z, noise_var, events, axis)
    if len(X) == 0:
        return np.zeros(len(Z)), Kzz
    L = np.linalg.cholesky(K)
    al = np.linalg.solve(L.T, np.linalg.solve(L, y))
    V = np.linalg.solve(L, Ks)
    return Ks.T @ al, Kzz - V.T @ V
