"""The selection of gogp_amd/csrc/vecchia_bknn.hip in isolation (test hook gogp_test_vecchia_bknn) against the plain
restatement of tests/vecchia_bknn_ref.py: lists integer for integer, squared distances and centroids bit for bit.

Shapes: N across the tile of 256 candidates and a slab's boundaries; (t, c) with c beyond the earlier rows (short lists,
-1 padded), block 0 without a conditioning row, a shorter last block, both capacity instances (c <= 64, c <= 128) and both
kinds of dimension instance (D = 1, 3 in registers, D = 9 generic); one slab and three; a tile of 8 queries and one of 3,
whose last tile is partly filled.  Integer-grid rows with t a power of two make centroids and distances exact and ties
plentiful, so the lower-index rule decides; random rows beside them.

Reference counterpart: none."""
import functools

import numpy as np
import pytest

import vecchia_bknn_ref as R

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 64, 65, 129, 257, 1000]
TC = [(1, 5), (1, 127), (3, 7), (5, 123), (16, 100), (64, 64), (128, 0)]
LENGTHS = {1: [0.7], 3: [0.5, 2.0, 1.25], 9: [0.5, 2.0, 1.25, 3.0, 0.75, 1.0, 4.0, 0.3, 1.5]}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def expected(n, D, t, c, scaled, kind):
    x = R.rows(n, D, kind)
    return x, R.causal(x, t, c, np.array(LENGTHS[D]) if scaled else None)


def same(got, want, what):
    (nbr, d2, cnt, cen), (widx, wd2, wcnt, wcen) = got, want
    assert np.array_equal(bits(cen), bits(wcen)), what + ": centroids"
    if widx.shape[1]:
        assert np.array_equal(cnt, wcnt), what + ": counts"
        assert np.array_equal(nbr, widx), what + ": lists"
        assert np.array_equal(bits(d2), bits(wd2)), what + ": distances"


@pytest.mark.parametrize("D", [1, 3, 9])
@pytest.mark.parametrize("t,c", TC)
def test_causal_lists(t, c, D):
    from gogp_amd import gp
    for n in NS:
        for scaled in (False, True):
            kind = "grid" if (n + scaled) % 2 else "random"
            x, want = expected(n, D, t, c, scaled, kind)
            la = np.array(LENGTHS[D]) if scaled else None
            for qt, slabs in ((0, 1), (3, 3)):
                got = gp.vecchia_bknn_check(x, n, D, t, c, lengths=la, qt=qt, slabs=slabs)
                same(got, want, "n %d t %d c %d D %d scaled %d qt %d slabs %d" % (n, t, c, D, scaled, qt, slabs))
    # the plan's own split of the largest shape, whatever it is
    x, want = expected(1000, D, t, c, False, "grid")
    same(gp.vecchia_bknn_check(x, 1000, D, t, c), want, "planned")


@pytest.mark.parametrize("D", [1, 3, 9])
@pytest.mark.parametrize("g,c", [(1, 5), (4, 128), (7, 64), (16, 100)])
def test_query_lists(g, c, D):
    """Groups of test points over all rows: few queries over many candidates, which the plan cuts into slabs."""
    from gogp_amd import gp
    for n, mz in ((1, 3), (65, 1), (1000, 30), (1000, 9)):
        x, z = R.rows(n, D, "grid"), R.rows(mz, D, "grid", seed=1) + (0.0 if mz % 2 else 0.5)
        la = np.array(LENGTHS[D])
        want = R.query(x, z, g, c, la)
        for qt, slabs in ((0, 0), (0, 1), (3, 3)):
            got = gp.vecchia_bknn_check(x, n, D, g, c, Z=z, mz=mz, lengths=la, qt=qt, slabs=slabs)
            same(got, want, "n %d mz %d g %d c %d D %d qt %d slabs %d" % (n, mz, g, c, D, qt, slabs))
