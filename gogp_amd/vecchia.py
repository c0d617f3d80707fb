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


# ---- blocks of targets on a shared conditioning set (GP.SetVecchiaBlocks, GP.VecchiaBlockProduce) ---------------------------
MAX_BLOCK = 128


def _block_ok(t: int, c: int):
    t, c = int(t), int(c)
    if t < 1 or c < 0 or t + c > MAX_BLOCK:
        raise ValueError("blocks: t >= 1 targets, c >= 0 conditioning rows, t + c <= %d" % MAX_BLOCK)
    return t, c


def _pack(cond, targ, w):
    tbl = np.full((len(cond), w), -1, dtype=np.int32)
    for k, (a, b) in enumerate(zip(cond, targ)):
        tbl[k, :len(a)] = a
        tbl[k, len(a):len(a) + len(b)] = b
    return (tbl, np.array([len(a) for a in cond], dtype=np.int32), np.array([len(b) for b in targ], dtype=np.int32))


def block_previous(n: int, t: int, c: int):
    """(tbl, nc, nt) of consecutive blocks of t targets (the last one shorter), each conditioned on the c rows before its
    first target, the latest first.  block_previous(n, 1, m) names the rows of previous(n, m)."""
    t, c = _block_ok(t, c)
    n = int(n)
    starts = range(0, n, t)
    cond = [np.arange(s - 1, max(s - c, 0) - 1, -1) for s in starts]
    targ = [np.arange(s, min(s + t, n)) for s in starts]
    return _pack(cond, targ, t + c)


def _centroid(xs: np.ndarray, t: int) -> np.ndarray:
    """The centroids of the consecutive blocks of t rows of xs (the last one shorter), one row per block, in a stated
    order of operations: the rows are summed in index order, one IEEE add per row, and the sum is divided once by the row
    count; a block of one row is the row itself, undivided.  The device (GP.VecchiaBlockTables) does the same, so both
    name the same rows.  For two or more dimensions this is ndarray.mean(axis=0) bit for bit; for one dimension and eight
    or more rows numpy's mean adds eight interleaved partial sums, so this centroid may differ from it in the last bit,
    which changes a table only where two keys lie within that bit."""
    n = len(xs)
    starts = np.arange(0, n, t)
    cnt = np.minimum(t, n - starts)
    acc = xs[starts].copy()
    for p in range(1, min(t, n)):  # vectorised over the blocks: a loop over the positions within a block
        live = cnt > p
        acc[live] += xs[starts[live] + p]
    many = cnt > 1
    acc[many] /= cnt[many, None].astype(np.float64)
    return acc


def block_nearest(x, t: int, c: int, lengths=None):
    """(tbl, nc, nt) of consecutive blocks of t targets in the given order, each conditioned on the c EARLIER rows (rows
    before its first target) nearest to the block's centroid (_centroid) under the Euclidean distance of x / lengths,
    nearest first, ties to the lower index.  O(N^2 D / t) on the host; GP.VecchiaBlockTables and GP.SetVecchiaBlocksNearest
    run the same search on the device and return this table integer for integer.  block_nearest(x, 1, m) names the rows
    of nearest(x, m)."""
    t, c = _block_ok(t, c)
    xs = _scaled(x, lengths)
    n = len(xs)
    cens = _centroid(xs, t)
    cond, targ = [], []
    for s in range(0, n, t):
        e = min(s + t, n)
        k = min(c, s)
        if k:
            cen = cens[s // t:s // t + 1]
            cond.append(_smallest(_d2(cen, xs[:s]), k)[0])
        else:
            cond.append(np.zeros(0, dtype=np.int64))
        targ.append(np.arange(s, e))
    return _pack(cond, targ, t + c)


def group_nearest_to(x, z, g: int, c: int, lengths=None):
    """For GP.VecchiaBlockProduce: consecutive groups of g test points (rows of z), each conditioned on the c rows of x
    nearest to the group's centroid (_centroid).  Returns (offsets, (tbl, nc)): ng + 1 offsets into z, the ng x c table and
    counts.  GP.VecchiaBlockTables(x, g, c, lengths, z) and GP.VecchiaBlockProduceNearest find the same table on the
    device."""
    g, c = int(g), int(c)
    if g < 1 or not 0 <= c <= MAX_BLOCK:
        raise ValueError("group_nearest_to: g >= 1 test points, 0 <= c <= %d conditioning rows" % MAX_BLOCK)
    xs = _scaled(x, lengths)
    zs = _scaled(z, lengths, xs.shape[1])
    if zs.shape[1] != xs.shape[1]:
        raise ValueError("group_nearest_to: x and z differ in dimension")
    mz, k = len(zs), min(c, len(xs))
    offsets = np.append(np.arange(0, mz, g, dtype=np.int64), mz) if mz else np.zeros(1, dtype=np.int64)
    cens = _centroid(zs, g) if mz else zs
    cond = []
    for i in range(len(offsets) - 1):
        cen = cens[i:i + 1]
        cond.append(_smallest(_d2(cen, xs), k)[0] if k else np.zeros(0, dtype=np.int64))
    tbl, nc, _ = _pack(cond, [()] * len(cond), c)
    return offsets, (tbl, nc)
