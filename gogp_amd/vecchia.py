"""Neighbour tables of Vecchia's approximation (GP.SetVecchia, GP.VecchiaProduce): host helpers, numpy only.

A table has one row per target and m <= 63 columns of int32: distinct row indices of the data, then -1 padding.  The
tables of SetVecchia are causal -- row i holds indices below i, row 0 is empty.  The order within a row is kept by the
library; these helpers list neighbours from the nearest (or latest) outwards.
"""
from __future__ import annotations

import numpy as np

MAX_M = 63


def _m_ok(m: int) -> int:
    m = int(m)
    if not 0 <= m <= MAX_M:
        raise ValueError("m: 0 .. %d conditioning rows" % MAX_M)
    return m


def previous(n: int, m: int) -> np.ndarray:
    """The time-series table: row i conditions on the rows i - 1, i - 2, ... i - m (those that exist).  With it term i of
    VecchiaTerms is the one-step-ahead forecast of y_i from a window of m observations."""
    n, m = int(n), _m_ok(m)
    t = np.arange(n, dtype=np.int64)[:, None] - 1 - np.arange(m, dtype=np.int64)[None, :]
    t[t < 0] = -1
    return np.ascontiguousarray(t, dtype=np.int32).reshape(n, m)


def _scaled(x, lengths, ndim=None) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1 if ndim is None else ndim)
    if lengths is not None:
        x = x / np.broadcast_to(np.asarray(lengths, dtype=np.float64), (x.shape[1],))
    return np.ascontiguousarray(x)


def _d2(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Squared distances, summed over the dimensions in index order from the differences themselves: equidistant
    points tie exactly, which the expansion |a|^2 - 2 a.b + |b|^2 would leave to rounding."""
    d2 = np.zeros((len(a), len(b)))
    for d in range(a.shape[1]):
        diff = a[:, d, None] - b[None, :, d]
        d2 += diff * diff
    return d2


def _smallest(d2: np.ndarray, k: int) -> np.ndarray:
    """Per row the indices of the k smallest entries, by value and then by index (a stable sort keeps ties at the lower
    index); +inf marks entries that may not be taken."""
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    taken = np.take_along_axis(d2, order, axis=1)
    return np.where(np.isfinite(taken), order, -1)


def nearest(x, m: int, lengths=None, chunk: int = 1024) -> np.ndarray:
    """For every row its m nearest EARLIER rows under the Euclidean distance of x / lengths (``lengths``: one scale per
    dimension or one for all; None: unscaled), nearest first, ties to the lower index.  Brute force in chunks of rows:
    O(N^2 D) time and O(chunk N) memory, meant for N up to about 1e5 -- beyond that bring a table from a spatial index.
    GP.VecchiaNeighbours and GP.SetVecchiaNearest run the same search on the device and return this table integer for
    integer."""
    m = _m_ok(m)
    xs = _scaled(x, lengths)
    n = len(xs)
    out = np.full((n, m), -1, dtype=np.int32)
    if m == 0 or n == 0:
        return out
    for r0 in range(0, n, max(int(chunk), 1)):
        r1 = min(n, r0 + max(int(chunk), 1))
        d2 = _d2(xs[r0:r1], xs[:r1])
        d2[np.arange(r1)[None, :] >= np.arange(r0, r1)[:, None]] = np.inf
        k = min(m, r1)
        out[r0:r1, :k] = _smallest(d2, k)
    return out


def nearest_to(x, z, m: int, lengths=None, chunk: int = 1024) -> np.ndarray:
    """For every test point (row of z) its m nearest rows of x, as ``nearest`` measures them: the table of
    GP.VecchiaProduce."""
    m = _m_ok(m)
    xs = _scaled(x, lengths)
    zs = _scaled(z, lengths, xs.shape[1])
    if zs.shape[1] != xs.shape[1]:
        raise ValueError("nearest_to: x and z differ in dimension")
    n, mz = len(xs), len(zs)
    out = np.full((mz, m), -1, dtype=np.int32)
    if m == 0 or n == 0 or mz == 0:
        return out
    k = min(m, n)
    for r0 in range(0, mz, max(int(chunk), 1)):
        r1 = min(mz, r0 + max(int(chunk), 1))
        out[r0:r1, :k] = _smallest(_d2(zs[r0:r1], xs), k)
    return out
