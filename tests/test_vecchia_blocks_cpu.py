"""Vecchia on blocks of targets (gogp_vecchia_blocks_*), the part that needs no GPU: gogp_vecchia_blocks_check on the
helpers' tables and on four broken ones, and the helpers against the single-target tables of gogp_amd/vecchia.py."""
import ctypes

import numpy as np
import pytest

from gogp_amd import _lib
from gogp_amd import vecchia as VT

EARG, OK = _lib.GOGP_EARG, _lib.GOGP_OK


def check(blocks, n):
    tbl, nc, nt = (np.ascontiguousarray(a, dtype=np.int32) for a in blocks)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return _lib.lib().gogp_vecchia_blocks_check(p(tbl), p(nc), p(nt), len(nc), tbl.shape[1], n)


X = np.random.default_rng(251).uniform(-2.0, 2.0, (150, 3))


@pytest.mark.parametrize("t,c", [(1, 0), (1, 63), (1, 127), (7, 20), (64, 64), (128, 0), (32, 96)])
def test_check_accepts_the_helpers_tables(t, c):
    assert check(VT.block_previous(150, t, c), 150) == OK
    assert check(VT.block_nearest(X, t, c, lengths=[1.0, 2.0, 0.5]), 150) == OK
    assert check(VT.block_previous(150, t, c), 151) == EARG  # row 150 is never a target
    off, (tbl, nc) = VT.group_nearest_to(X, X[:11] + 0.1, 5, c)
    assert list(off) == [0, 5, 10, 11] and tbl.shape == (3, c) and (nc == min(c, 150)).all()
    assert all(len(set(r[:k])) == k and (r[:k] >= 0).all() and (r[:k] < 150).all() for r, k in zip(tbl, nc))


def test_check_refuses():
    tbl, nc, nt = VT.block_previous(12, 4, 3)  # blocks [.. | 0-3], [3 2 1 | 4-7], [7 6 5 | 8-11]
    assert check((tbl, nc, nt), 12) == OK
    for why, edit in (("a row targeted twice", lambda t: t.__setitem__((2, 3), 4)),
                      ("a row never targeted", lambda t: t.__setitem__((2, 6), -1)),
                      ("a duplicate inside a block", lambda t: t.__setitem__((1, 1), 3)),
                      ("a conditioning row from a later block", lambda t: t.__setitem__((1, 0), 9))):
        bad, cnt = tbl.copy(), nt.copy()
        edit(bad)
        if why == "a row never targeted":
            cnt[2] = 3
        assert check((bad, nc, cnt), 12) == EARG, why


@pytest.mark.parametrize("m", [0, 1, 7, 63])
def test_single_targets_name_the_rows_of_the_neighbour_tables(m):
    for blocks, table in ((VT.block_previous(150, 1, m), VT.previous(150, m)), (VT.block_nearest(X, 1, m), VT.nearest(X, m))):
        tbl, nc, nt = blocks
        assert (nt == 1).all() and np.array_equal(nc, (table >= 0).sum(1))
        for i in range(150):
            assert np.array_equal(tbl[i, :nc[i]], table[i, :nc[i]]) and tbl[i, nc[i]] == i
