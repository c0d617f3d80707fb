"""Neighbour tables built on the device, through the C ABI and Python (GP.VecchiaNeighbours, SetVecchiaNearest,
VecchiaReneighbour, VecchiaNeighbourTable, VecchiaProduceNearest, VecchiaModel.reneighbour).

The yardstick is the naive per-row loop below (a stable sort on unfused float64 distances), with
gogp_amd.vecchia.nearest / nearest_to as a second witness; the tables are equal integer for integer, and everything
computed on a device-built table has the bits of the same calls on the host's table.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

from gogp_amd import _lib, kernel
from gogp_amd import vecchia as VT

pytestmark = pytest.mark.gpu

ES, EA = _lib.GOGP_ESTATE, _lib.GOGP_EARG


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def naive(x, z, m, lengths):
    xs = x / lengths if lengths is not None else x
    zs = xs if z is None else (z / lengths if lengths is not None else z)
    out = np.full((len(zs), m), -1, np.int32)
    for i in range(len(zs)):
        lim = i if z is None else len(xs)
        d2 = np.zeros(lim)
        for d in range(xs.shape[1]):
            diff = zs[i, d] - xs[:lim, d]
            d2 = d2 + diff * diff
        order = np.argsort(d2, kind="stable")[:m]
        out[i, :len(order)] = order
    return out


def data(N, D, seed=0):
    rng = np.random.default_rng([431, N, D, seed])
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=N)
    v = rng.uniform(0.0, 0.02, N)
    return X, y, v


FAMILIES = {
    "radial": (lambda D: kernel.Scaled(kernel.Matern52), lambda D: np.log([1.0, 0.4, 0.1])),
    "ard": (lambda D: kernel.ARD(kernel.Normal, D), lambda D: np.log(np.r_[np.linspace(0.3, 0.9, D), 0.1])),
}


def make_gp(D, family="radial"):
    from gogp_amd.gp import GP
    return GP(D, FAMILIES[family][0](D), kernel.UniformNoise, device=0)


def check_table(t, n, causal):
    p = t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return _lib.lib().gogp_vecchia_check(p, t.shape[0], t.shape[1], n, int(causal)) == _lib.GOGP_OK


@pytest.mark.parametrize("N,D,m", [(1000, 8, 63), (2500, 3, 31)])
def test_neighbours_equal_the_host(N, D, m):
    X, _, _ = data(N, D)
    Z = np.random.default_rng(433).uniform(0, 1, (70, D))
    ln = np.linspace(0.5, 2.0, D)
    g = make_gp(D)
    for lengths in (None, ln):
        t = g.VecchiaNeighbours(X, m, lengths)
        assert t.dtype == np.int32 and t.shape == (N, m)
        assert np.array_equal(t, naive(X, None, m, lengths))
        assert np.array_equal(t, VT.nearest(X, m, lengths))
        assert check_table(t, N, True)
        tz = g.VecchiaNeighbours(X, m, lengths, z=Z)
        assert np.array_equal(tz, naive(X, Z, m, lengths))
        assert np.array_equal(tz, VT.nearest_to(X, Z, m, lengths))
        assert check_table(tz, N, False)
    assert np.array_equal(g.VecchiaNeighbours(X, m, 0.7), VT.nearest(X, m, 0.7)), "a scalar length"
    assert g.VecchiaNeighbours(X, 0).shape == (N, 0)
    with pytest.raises(_lib_error()) as e:
        g.VecchiaNeighbourTable()
    assert e.value.code == ES, "the one-shot call left no Vecchia state"
    g.close()


def _lib_error():
    from gogp_amd.gp import GogpError
    return GogpError


def evaluate(g, x):
    value = g.VecchiaObserve(x)
    return [np.array([value])] + list(g.VecchiaTerms()) + [g.VecchiaGradient()]


def same_bits(a, b, what):
    for k, (u, w) in enumerate(zip(a, b)):
        assert np.array_equal(bits(u), bits(w)), (what, k)


@pytest.mark.parametrize("family", ["radial", "ard"])
def test_set_nearest_gives_the_bits_of_the_hosts_table(family):
    N, D, m = 700, 3, 15
    X, y, v = data(N, D)
    x = FAMILIES[family][1](D)
    ln = np.array([0.4, 1.0, 2.5])
    t = VT.nearest(X, m, ln)
    assert np.array_equal(t, naive(X, None, m, ln))
    a, b = make_gp(D, family), make_gp(D, family)
    a.SetVecchiaNearest(X, y, m, ln, v)
    b.SetVecchia(X, y, t, v)
    assert np.array_equal(a.VecchiaNeighbourTable(), t)
    assert np.array_equal(b.VecchiaNeighbourTable(), t)
    same_bits(evaluate(a, x), evaluate(b, x), family)
    # without lengths and without variances
    a.SetVecchiaNearest(X, y, m)
    b.SetVecchia(X, y, VT.nearest(X, m))
    same_bits(evaluate(a, x), evaluate(b, x), family + ", unscaled")
    a.close()
    b.close()


def test_reneighbour():
    N, D, m = 600, 3, 31
    X, y, v = data(N, D, 1)
    x = FAMILIES["radial"][1](D)
    l1, l2 = np.array([1.0, 1.0, 1.0]), np.array([0.2, 1.0, 3.0])
    t2 = VT.nearest(X, m, l2)
    assert not np.array_equal(t2, VT.nearest(X, m, l1)), "the lengths matter"
    fresh = make_gp(D)
    fresh.SetVecchia(X, y, t2, v)
    want = evaluate(fresh, x)
    a = make_gp(D)
    a.SetVecchiaNearest(X, y, m, l1, v)
    a.VecchiaObserve(x)
    a.VecchiaGradient()
    a.VecchiaReneighbour(l2)
    with pytest.raises(_lib_error()) as e:
        a.VecchiaGradient()
    assert e.value.code == ES, "the observe before the reneighbour is dropped"
    with pytest.raises(_lib_error()) as e:
        a.VecchiaProduceNearest(X[:3])
    assert e.value.code == ES
    assert np.array_equal(a.VecchiaNeighbourTable(), t2)
    same_bits(evaluate(a, x), want, "after reneighbour")
    # on data that came with a caller's table
    b = make_gp(D)
    b.SetVecchia(X, y, VT.previous(N, m), v)
    b.VecchiaObserve(x)
    with pytest.raises(_lib_error()) as e:
        b.VecchiaProduceNearest(X[:3])
    assert e.value.code == ES, "a caller's table has no lengths to fall back on"
    b.VecchiaReneighbour(l2)
    assert np.array_equal(b.VecchiaNeighbourTable(), t2)
    same_bits(evaluate(b, x), want, "reneighbour on a caller's table")
    # without data
    c = make_gp(D)
    for call in (lambda: c.VecchiaReneighbour(l2), c.VecchiaNeighbourTable, lambda: c.VecchiaProduceNearest(X[:3])):
        with pytest.raises(_lib_error()) as e:
            call()
        assert e.value.code == ES
    for g in (fresh, a, b, c):
        g.close()


@pytest.mark.parametrize("mz", [1, 5, 300])
def test_produce_nearest(mz):
    N, D, m = 900, 3, 31
    X, y, v = data(N, D, 2)
    Z = np.random.default_rng([439, mz]).uniform(0, 1, (mz, D))
    x = FAMILIES["radial"][1](D)
    ln, other = np.array([0.5, 1.0, 2.0]), np.array([2.0, 1.0, 0.5])
    g = make_gp(D)
    g.SetVecchiaNearest(X, y, m, ln, v)
    g.VecchiaObserve(x)
    tz = VT.nearest_to(X, Z, m, ln)
    assert np.array_equal(tz, naive(X, Z, m, ln))
    want = g.VecchiaProduce(Z, tz)
    mu, sigma, t = g.VecchiaProduceNearest(Z, table=True)  # the resident lengths
    assert np.array_equal(t, tz)
    same_bits((mu, sigma), want, "resident lengths")
    mu, sigma = g.VecchiaProduceNearest(Z, lengths=ln)
    same_bits((mu, sigma), want, "the same lengths, given")
    to = VT.nearest_to(X, Z, m, other)
    mu, none, t = g.VecchiaProduceNearest(Z, lengths=other, sigma=False, table=True)
    assert none is None and np.array_equal(t, to)
    same_bits((mu,), g.VecchiaProduce(Z, to)[:1], "other lengths")
    g.close()


def test_the_dense_state_is_untouched():
    N, D, m = 300, 3, 7
    X, y, v = data(N, D, 3)
    x = FAMILIES["radial"][1](D)
    from gogp_amd.gp import GP
    g = GP(D, FAMILIES["radial"][0](D), kernel.UniformNoise, X=X, Y=y, device=0)
    before = (np.array([g.Observe(x)]), g.Gradient())
    g.VecchiaNeighbours(X, m, 0.5, z=X[:9])
    g.SetVecchiaNearest(X, y, m, 0.5, v)
    g.VecchiaObserve(x)
    g.VecchiaReneighbour([0.3, 1.0, 2.0])
    g.VecchiaObserve(x)
    g.VecchiaNeighbourTable()
    g.VecchiaProduceNearest(X[:40] + 0.01)
    same_bits((g.Gradient(),), before[1:], "the dense gradient straight after the new calls")
    after = (np.array([g.Observe(x)]), g.Gradient())
    same_bits(after, before, "a dense evaluation after the new calls")
    g.close()


def test_model_reneighbours_between_two_runs():
    from gogp_amd import optimize
    from gogp_amd.gp import VecchiaModel
    N, D, m = 500, 3, 15
    X, y, _ = data(N, D, 4)
    x0 = FAMILIES["radial"][1](D) + 0.3
    lengths_of = lambda x: float(np.exp(x[1]))  # noqa: E731 -- Scaled(Matern52): theta = [c, length | noise]
    g = make_gp(D)
    g.SetVecchiaNearest(X, y, m, lengths_of(x0))
    model = VecchiaModel(g, lengths_of=lengths_of)
    r1 = optimize.lbfgs(model, x0, major_iterations=3)
    x1 = np.asarray(r1.x, dtype=float)
    model.reneighbour(x1)
    assert np.array_equal(g.VecchiaNeighbourTable(), VT.nearest(X, m, lengths_of(x1)))
    v1 = model.Observe(x1)
    fresh = make_gp(D)
    fresh.SetVecchia(X, y, VT.nearest(X, m, lengths_of(x1)))
    assert bits(np.array([v1]))[0] == bits(np.array([fresh.VecchiaObserve(x1)]))[0]
    r2 = optimize.lbfgs(model, x1, major_iterations=3)
    v2 = model.Observe(np.asarray(r2.x, dtype=float))
    print("VecchiaModel: %.6f after the reneighbour, %.6f after the second run" % (v1, v2))
    assert np.isfinite(v2) and v2 >= v1
    with pytest.raises(ValueError):
        VecchiaModel(g).reneighbour(x1)
    fresh.close()
    g.close()
