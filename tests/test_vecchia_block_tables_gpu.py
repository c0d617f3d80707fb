"""Block tables built on the device through the public calls (GP.VecchiaBlockTables, SetVecchiaBlocksNearest,
VecchiaBlockReneighbour, VecchiaBlockTable, VecchiaBlockProduceNearest): integer for integer the tables of
gogp_amd.vecchia.block_nearest / group_nearest_to, and bit for bit the results of the block calls on those tables.

Reference counterpart: none."""
import numpy as np
import pytest

import vecchia_bknn_ref as R

pytestmark = pytest.mark.gpu

D = 3
LENGTHS = np.array([0.5, 2.0, 1.25])
NOISE_STD = 0.05 ** 0.5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def new_gp():
    from gogp_amd import kernel as GK
    from gogp_amd.gp import GP
    return GP(D, GK.Matern52, GK.UniformNoise, ThetaSimil=[1.5], ThetaNoise=[NOISE_STD], device=0)


X0 = np.log(np.array([1.5, NOISE_STD]))


def data(n, kind="random"):
    x = R.rows(n, D, kind)
    return x, np.sin(x.sum(axis=1)) + 0.1 * np.cos(3.0 * x[:, 0])


def same_tables(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("n,t,c", [(1, 3, 7), (65, 1, 5), (257, 3, 7), (1000, 5, 123), (1000, 16, 100), (257, 64, 64),
                                   (129, 128, 0)])
def test_tables_equal_the_host_helpers(n, t, c):
    from gogp_amd import vecchia as VT
    g = new_gp()
    for kind, la in (("grid", None), ("random", LENGTHS)):
        x, _ = data(n, kind)
        same_tables(g.VecchiaBlockTables(x, t, c, la), VT.block_nearest(x, t, c, la))
        z = R.rows(11, D, kind, seed=2)
        same_tables(g.VecchiaBlockTables(x, t, c, la, z=z), VT.group_nearest_to(x, z, t, c, la)[1])
    if t == 1:
        tbl, nc, nt = g.VecchiaBlockTables(x, 1, c, LENGTHS)
        nbr = g.VecchiaNeighbours(x, c, LENGTHS)
        assert np.array_equal(nc, (nbr >= 0).sum(axis=1)) and (nt == 1).all()
        for k in range(n):
            assert np.array_equal(tbl[k, :nc[k]], nbr[k, :nc[k]]) and tbl[k, nc[k]] == k
    g.close()


@pytest.mark.parametrize("n,t,c", [(300, 16, 48), (257, 5, 123)])
def test_resident_table_observe_gradient_reneighbour_produce(n, t, c):
    from gogp_amd import _lib
    from gogp_amd import vecchia as VT
    from gogp_amd.gp import GogpError
    x, y = data(n)
    z = R.rows(13, D, "random", seed=3)
    g, ref = new_gp(), new_gp()
    g.Absorb(x[:40], y[:40])
    dense = g.Observe(X0), g.Gradient()

    def check(la):
        """g holds the device's table under la: equal to the host's, and every result bit-equal to the host-table path"""
        host = VT.block_nearest(x, t, c, la)
        same_tables(g.VecchiaBlockTable(), host)
        ref.SetVecchiaBlocks(x, y, host)
        assert bits(g.VecchiaBlockObserve(X0)) == bits(ref.VecchiaBlockObserve(X0))
        assert np.array_equal(bits(g.VecchiaBlockGradient()), bits(ref.VecchiaBlockGradient()))
        for gsz, cz in ((4, None), (1, 20)):
            off, groups = VT.group_nearest_to(x, z, gsz, c if cz is None else cz, la)
            mu, sg, tab = g.VecchiaBlockProduceNearest(z, gsz, cz, table=True)
            same_tables(tab, groups)
            wmu, wsg = ref.VecchiaBlockProduce(z, off, groups)
            assert np.array_equal(bits(mu), bits(wmu)) and np.array_equal(bits(sg), bits(wsg))

    g.SetVecchiaBlocksNearest(x, y, t, c, LENGTHS)
    check(LENGTHS)
    g.VecchiaBlockReneighbour(2.0 * LENGTHS[::-1])
    for call in (g.VecchiaBlockGradient, lambda: g.VecchiaBlockProduceNearest(z, 4)):
        with pytest.raises(GogpError) as e:
            call()
        assert e.value.code == _lib.GOGP_ESTATE
    check(2.0 * LENGTHS[::-1])
    # a caller's table of consecutive blocks can be rebuilt; one of another shape cannot
    g.SetVecchiaBlocks(x, y, VT.block_previous(n, t, c))
    g.VecchiaBlockReneighbour(None)
    same_tables(g.VecchiaBlockTable(), VT.block_nearest(x, t, c))
    odd = (np.array([[1, 0, -1], [0, 2, -1]], np.int32), np.array([0, 1], np.int32), np.array([2, 1], np.int32))
    g.SetVecchiaBlocks(x[:3], y[:3], odd)
    with pytest.raises(GogpError) as e:
        g.VecchiaBlockReneighbour(None)
    assert e.value.code == _lib.GOGP_ESTATE
    # the dense state of the handle is untouched
    assert g.Observe(X0) == dense[0] and np.array_equal(bits(g.Gradient()), bits(dense[1]))
    g.close()
    ref.close()
