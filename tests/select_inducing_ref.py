"""Greedy conditional-variance selection of inducing points (gogp_sparse_select_inducing): the numpy reference its
tests share.  Families, noise and inputs: those of tests/produce_grad_ref.py.

A partial Cholesky factorisation of K = k(X, X) (no noise) with diagonal pivoting:

    d_i = K_ii
    for j = 0 .. M-1:
        p = the lowest index among the maximisers of d;  stop (m = j) unless d_p > tol
        piv[j] = p,  pv[j] = d_p
        l_i = (K_ip - sum_{t<j} L[i][t] L[p][t]) / sqrt(d_p) for the rows not yet selected,  l_p = sqrt(d_p),
        l_i = 0 for the rows selected earlier;  L[:, j] = l;  d_i -= l_i^2;  d_p = 0 (selected rows keep 0)
    trace = sum_i d_i

`greedy` runs it on a dense K; `replay` follows a GIVEN pivot sequence, in fp64 or np.longdouble, and returns the
residual diagonal before every step and after the last -- what the GPU tests hold the device's picks against.  Both take
K as a dense array or as a `Columns` (columns of k(X, X) on demand: N = 70001 has no dense K).
"""
import numpy as np

from gogp_amd import kernel
from oracle.oracle import gram_np
from produce_grad_ref import FAMILIES, FOUR, NOISE, TN, inputs  # noqa: F401  (shared with the tests)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


class Columns:
    """Columns of k(X, X) at the natural parameters ths, one at a time (gram_np)."""

    def __init__(self, D, simil, ths, X):
        self.desc = kernel.build_desc(D, simil, NOISE)
        self.ths = np.asarray(ths, float)
        self.X = np.ascontiguousarray(np.asarray(X, float).reshape(-1, D))
        self._diag = None
        self._cols = {}

    def __len__(self):
        return len(self.X)

    def col(self, p):
        p = int(p)
        if p not in self._cols:  # (both replays of a test ask for the same columns)
            self._cols[p] = gram_np(self.desc, self.ths, self.X, self.X[p:p + 1])[:, 0]
        return self._cols[p]

    def diag(self):
        if self._diag is None:
            # k(x, x) does not depend on x for any family here: the sum of the output scales, as one row gives it
            k00 = gram_np(self.desc, self.ths, self.X[:1], self.X[:1])[0, 0]
            self._diag = np.full(len(self.X), k00)
        return self._diag


def dense(D, simil, ths, X):
    """K = k(X, X), dense, and the descriptor."""
    desc = kernel.build_desc(D, simil, NOISE)
    X = np.ascontiguousarray(np.asarray(X, float).reshape(-1, D))
    return gram_np(desc, np.asarray(ths, float), X, X)


def _col(K, p):
    return K.col(p) if isinstance(K, Columns) else K[:, p]


def _diag(K):
    return K.diag() if isinstance(K, Columns) else np.diag(K)


def greedy(K, M, tol):
    """(piv, pv, L, d, trace) of the recurrence in fp64: piv, pv of length m <= min(M, N), L (N x m), d the final residual
    diagonal."""
    N = len(K)
    d = np.array(_diag(K), dtype=np.float64)
    L = np.zeros((N, min(M, N)))
    piv, pv = [], []
    for j in range(min(M, N)):
        p = int(np.argmax(d)) if N else 0  # argmax returns the first maximiser
        if not d[p] > tol:
            break
        dp = d[p]
        l = (_col(K, p) - L[:, :j] @ L[p, :j]) / np.sqrt(dp)
        l[piv] = 0.0
        l[p] = np.sqrt(dp)
        L[:, j] = l
        d = d - l * l
        piv.append(p)
        pv.append(dp)
        d[piv] = 0.0
    m = len(piv)
    return np.array(piv, dtype=np.int64), np.array(pv), L[:, :m].copy(), d, float(d.sum())


def replay(K, piv, dtype=np.float64):
    """The residual diagonals of the recurrence along the GIVEN pivots, in `dtype` (np.float64 or np.longdouble) on the
    fp64 kernel values: an array (len(piv) + 1, N) -- row j is d before step j, the last row d after the last step -- and
    the factor L (N x len(piv))."""
    N, m = len(K), len(piv)
    d = np.array(_diag(K), dtype=dtype)
    L = np.zeros((N, m), dtype=dtype)
    out = np.zeros((m + 1, N), dtype=dtype)
    out[0] = d
    for j, p in enumerate(piv):
        p = int(p)
        sq = np.sqrt(d[p])
        l = (np.asarray(_col(K, p), dtype=dtype) - L[:, :j] @ L[p, :j]) / sq
        l[np.asarray(piv[:j], dtype=np.int64)] = 0
        l[p] = sq
        L[:, j] = l
        d = d - l * l
        d[np.asarray(piv[:j + 1], dtype=np.int64)] = 0
        out[j + 1] = d
    return out, L
