"""A plain restatement of the definition of the block tables (include/gogp_hip.h, "Block tables built on the device"),
for tests/test_vecchia_bknn_kernel.py and tests/test_vecchia_block_tables_*.py.  Elementwise IEEE operations in a stated
order only -- no reductions, whose order numpy chooses -- and a lexicographic sort of the keys."""
import numpy as np


def scaled(x, lengths):
    x = np.asarray(x, dtype=np.float64)
    return x if lengths is None else x / np.asarray(lengths, dtype=np.float64)[None, :]


def centroids(xs, t):
    """Row k: the rows k t .. of xs added in index order, one add per row, divided once by their count (not for one row)."""
    out = []
    for s in range(0, len(xs), t):
        rows = xs[s:s + t]
        acc = rows[0].copy()
        for r in rows[1:]:
            acc = acc + r
        out.append(acc / np.float64(len(rows)) if len(rows) > 1 else acc)
    return np.array(out).reshape(-1, xs.shape[1])


def lists(xs, cen, limits, c):
    """(idx, d2, cnt): per centroid the min(c, .) smallest keys (d2, j) over j < limits[k] with d2 finite; -1 / 0.0 padded."""
    nq = len(cen)
    idx, d2o, cnt = np.full((nq, c), -1, np.int32), np.zeros((nq, c)), np.zeros(nq, np.int32)
    for k in range(nq):
        cand = xs[:limits[k]]
        d2 = np.zeros(len(cand))
        for d in range(xs.shape[1]):
            diff = cen[k, d] - cand[:, d]
            d2 = d2 + diff * diff
        j = np.arange(len(cand))
        keep = np.isfinite(d2)
        order = np.lexsort((j[keep], d2[keep]))[:c]
        cnt[k] = len(order)
        idx[k, :len(order)] = j[keep][order]
        d2o[k, :len(order)] = d2[keep][order]
    return idx, d2o, cnt


def causal(x, t, c, lengths=None):
    """(idx, d2, cnt, cen) of the blocks of t rows of x over the rows before each block."""
    xs = scaled(x, lengths)
    cen = centroids(xs, t)
    return lists(xs, cen, [min(k * t, len(xs)) for k in range(len(cen))], c) + (cen,)


def query(x, z, g, c, lengths=None):
    """(idx, d2, cnt, cen) of the groups of g rows of z over all rows of x."""
    xs, zs = scaled(x, lengths), scaled(z, lengths)
    cen = centroids(zs, g)
    return lists(xs, cen, [len(xs)] * len(cen), c) + (cen,)


def pack(idx, cnt, n, t):
    """The block table (tbl, nc, nt) of causal()'s lists."""
    nb, c = idx.shape
    tbl = np.full((nb, t + c), -1, np.int32)
    nt = np.zeros(nb, np.int32)
    for k in range(nb):
        targ = np.arange(k * t, min(k * t + t, n))
        tbl[k, :cnt[k]] = idx[k, :cnt[k]]
        tbl[k, cnt[k]:cnt[k] + len(targ)] = targ
        nt[k] = len(targ)
    return tbl, cnt.copy(), nt


def rows(n, D, kind, seed=0):
    """Inputs: 'grid' -- small integer coordinates, so that many rows coincide and many distances tie exactly -- or
    'random'."""
    rng = np.random.default_rng([n, D, seed])
    if kind == "grid":
        return rng.integers(0, 4, size=(n, D)).astype(np.float64)
    return rng.normal(size=(n, D))
