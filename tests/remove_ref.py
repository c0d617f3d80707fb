"""gogp_remove (GP.Remove): the inputs its tests share and a numpy restatement of compaction + orthogonal rank-m update.

With S the removed indices and kept the rest, Lt = L[kept, kept] is lower triangular with a positive diagonal and
    K[kept, kept] = Lt Lt^T + W W^T,  W = L[kept, S]:
a gather and a rank-m update, here by one Householder reflector per column acting on (l_kk, w_k1 .. w_km) from the
right of [Lt | W], in passes of at most PASS columns of W (a sum of updates), as gogp_amd/csrc/remove.hip runs it.
Families, inputs and tolerances are those of tests/append_ref.py.
"""
import math

import numpy as np

import append_ref as A

PASS = 32


def _scattered(n, fixed, extra, seed):
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(n), np.asarray(fixed, dtype=np.int64))
    return tuple(sorted(set(fixed) | set(int(i) for i in rng.choice(rest, extra, replace=False))))


IDX_520 = _scattered(520, (0, 127, 128, 255, 256, 383, 519), 33, 3)
IDX_700 = _scattered(700, (), 330, 4)

#: (n, removed, family): the smallest shapes at which each mechanism of the removal can go wrong
SHAPES = [
    (5, tuple(range(5)), "scaled_rbf3"),        # the empty process
    (1, (0,), "matern32"),                      # the empty process
    (2, (0,), "hyperpriors"),                   # single row left
    (100, (0,), "ard_rbf3"),                    # inside the one-launch range before and after
    (130, (0, 1, 2), "scaled_rbf3"),            # drops from the general range to n' <= 128
    (140, (3, 50, 77, 139), "ard_rbf3"),        # the widest update of the narrow kernel instance (m = 4)
    (140, (3, 50, 77, 100, 139), "matern32"),   # the narrowest of the wide one
    (257, (256,), "matern32"),                  # last row only: npad 512 -> 256, no update, factor = old leading block
    (257, (0,), "hyperpriors"),                 # restride down and a full-length update
    (300, tuple(range(64)), "ard_rbf3"),        # whole passes of W
    (300, tuple(range(65)), "scaled_rbf3"),     # one more pass for a single column
    (520, IDX_520, "matern32"),                 # both sides of every 128 / 256 boundary, zero-topped W columns
    (700, IDX_700, "hyperpriors"),              # more removed than a block, npad 768 -> 512, many passes
]
#: the 520 shape with its first index replaced by 200, and the same without what is still below 200: the rows above the
#: first removed index keep their bits (the first: rows < its smallest index; the second: rows < 200)
REPLACED = (520, tuple(sorted((set(IDX_520) - {min(IDX_520)}) | {200})), "matern32")
UNTOUCHED = (520, tuple(i for i in REPLACED[1] if i >= 200), "matern32")
AFTER_OBSERVE = (300, tuple(range(5, 300, 9)), "ard_rbf3")
RESTORED = (600, tuple(range(3, 600, 31)), "scaled_rbf3")  # after restore(L, Alpha): no z on the handle
APPENDED = (300, 40, tuple(range(7, 340, 17)), "scaled_rbf3")  # Absorb 300, Append 40, Remove 20 scattered
SLIDING = (200, 130, "hyperpriors")  # window, steps
M_TEST = A.M_TEST


def inputs(n, D):
    """append_ref.inputs; a single row is the first of two (the outputs are standardised: one row alone has no spread)."""
    X, y, Z = A.inputs(max(n, 2), D)
    return X[:n], y[:n], Z


def shape_id(s):
    n, idx, fam = s
    return "%d-%d@%d-%s" % (n, len(idx), idx[0], fam)


def kept_of(n, idx):
    keep = np.ones(n, dtype=bool)
    keep[list(idx)] = False
    return np.flatnonzero(keep)


def remove_update(L, idx, width=PASS):
    """The factor of K[kept, kept] from the factor L of K: gather, then Householder passes of <= width columns."""
    n = len(L)
    idx = np.asarray(sorted(idx), dtype=np.int64)
    kept = kept_of(n, idx)
    n1 = len(kept)
    Lt = np.tril(L[np.ix_(kept, kept)]).copy()
    for off in range(0, len(idx), width):
        cols = idx[off:off + width]
        W = L[np.ix_(kept, cols)].copy()
        W[kept[:, None] < cols[None, :]] = 0.0  # above the diagonal of L
        for k in range(n1):
            b = W[k].copy()
            ss = float(b @ b)
            if ss == 0.0:  # exact identity: beta is undefined
                continue
            a = Lt[k, k]
            r = math.sqrt(a * a + ss)
            v0 = -ss / (a + r)  # Parlett: a - r without cancellation
            u = b / v0
            tau = -v0 / r
            Lt[k, k] = r
            W[k] = 0.0
            if k + 1 < n1:
                t = tau * (Lt[k + 1:, k] + W[k + 1:] @ u)
                Lt[k + 1:, k] -= t
                W[k + 1:] -= np.outer(t, u)
    return Lt


def state_after_remove(L, y, idx):
    """(L', alpha', lml') of the kept rows from the factor of all rows, as gogp_remove leaves them."""
    kept = kept_of(len(L), idx)
    L1 = remove_update(L, idx)
    n1 = len(kept)
    if n1 == 0:
        return L1, np.zeros(0), 0.0
    z = np.linalg.solve(L1, y[kept])
    alpha = np.linalg.solve(L1.T, z)
    lml = -0.5 * n1 * math.log(2 * math.pi) - np.log(np.diag(L1)).sum() - 0.5 * y[kept] @ alpha
    return L1, alpha, lml
