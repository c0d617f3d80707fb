"""The nearest-neighbour search of gogp_amd/csrc/vecchia_knn.hip in isolation, through the hook gogp_test_vecchia_knn on
caller-supplied rows, against a naive per-row loop written here: a stable sort on float64 distances that numpy sums from
the differences without fusing.  gogp_amd.vecchia.nearest / nearest_to are a second witness.

No tolerance anywhere: the key (d2, j) is a strict total order and the device forms d2 with the host's roundings, so the
table equals the loop's integer for integer and the distances of the entries taken are equal in bits.

Reference counterpart: none."""
import functools

import numpy as np
import pytest

from cases import NAN64
from gogp_amd import vecchia as VT

pytestmark = pytest.mark.gpu

F64 = np.float64
NS = [1, 2, 63, 64, 65, 129, 257, 1000]  # tiles of 64 targets: one and two tile edges, last tiles of one target
MS = [0, 1, 7, 31, 32, 63]               # the instances of 32 and of 64 entries per lane
DS = [1, 3, 8, 17]                       # rows in registers (1, 3, 8) and in LDS (17)


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def naive(x, z, m, lengths):
    """(table, d2 of the entries) row by row; z None: the causal table of x."""
    xs = x / lengths if lengths is not None else x
    zs = xs if z is None else (z / lengths if lengths is not None else z)
    T, D = len(zs), xs.shape[1]
    nbr, d2o = np.full((T, m), -1, np.int32), np.zeros((T, m))
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(T):
            lim = i if z is None else len(xs)
            if lim == 0 or m == 0:
                continue
            d2 = np.zeros(lim)
            for d in range(D):
                diff = zs[i, d] - xs[:lim, d]
                d2 = d2 + diff * diff
            order = np.argsort(d2, kind="stable")[:m]
            order = order[np.isfinite(d2[order])]
            nbr[i, :len(order)] = order
            d2o[i, :len(order)] = d2[order]
    return nbr, d2o


def lengths_of(D, seed=0):
    return 10.0 ** np.random.default_rng([401, D, seed]).uniform(-3, 3, D)


@functools.lru_cache(maxsize=None)
def problem(N, D, query, scaled):
    """Rows, test points (query form: as many as rows), lengths and the naive table at m = 63; a smaller m is its prefix."""
    rng = np.random.default_rng([389, N, D])
    x = rng.uniform(-2, 2, (N, D))
    z = rng.uniform(-2, 2, (N, D)) if query else None
    ln = lengths_of(D) if scaled else None
    if ln is not None:
        x, z = x * ln, (None if z is None else z * ln)  # a few length scales across in every dimension
    t, d2 = naive(x, z, 63, ln)
    for a in (x, z, ln, t, d2):
        if a is not None:
            a.setflags(write=False)
    return x, z, ln, t, d2


def search(gpm, X, m, Z=None, lengths=None, slabs=0, tile_cap=0):
    """One launch with sentinels behind every array: NaN rows behind X and Z, the index n (which names them) behind the
    table.  Returns (table, d2, scaled copy)."""
    n, D = X.shape
    T = n if Z is None else len(Z)
    Xp = np.concatenate([X.reshape(-1), np.full(2 * D, NAN64)])
    Zp = None if Z is None else np.concatenate([Z.reshape(-1), np.full(2 * D, NAN64)])
    nbr0 = None if m == 0 else np.concatenate([np.full(T * m, -7, np.int32), np.full(3, n, np.int32)])
    d20 = None if m == 0 else np.full(T * m + 3, NAN64)
    xs0 = np.full(n * D + 5, NAN64)
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=F64)
    nb, dd, xs = gpm.vecchia_knn_check(Xp, n, D, m, nbr0, d20, xs0, Z=Zp, targets=T, lengths=ln, slabs=slabs,
                                       tile_cap=tile_cap)
    assert np.array_equal(bits(xs[n * D:]), bits(xs0[n * D:])), "behind the scaled copy"
    if m == 0:
        assert nb is None and dd is None
        return np.zeros((T, 0), np.int32), np.zeros((T, 0)), xs[:n * D].reshape(n, D)
    assert np.array_equal(nb[T * m:], nbr0[T * m:]), "behind the table"
    assert np.array_equal(bits(dd[T * m:]), bits(d20[T * m:])), "behind the distances"
    return nb[:T * m].reshape(T, m), dd[:T * m].reshape(T, m), xs[:n * D].reshape(n, D)


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), ("table", what)
    assert np.array_equal(bits(got[1]), bits(want[1])), ("d2", what)


@pytest.mark.parametrize("D", DS)
def test_scaled_copy_is_the_hosts_division(gpm, D):
    """x / lengths in bits, lengths from 1e-3 to 1e3, values of every magnitude in between; lengths None: a copy."""
    rng = np.random.default_rng([397, D])
    x = rng.normal(size=(257, D)) * 10.0 ** rng.uniform(-6, 6, (257, D))
    for seed in range(3):
        ln = lengths_of(D, seed)
        assert ln.min() >= 1e-3 and ln.max() <= 1e3
        xs = search(gpm, x, 1, lengths=ln)[2]
        assert np.array_equal(bits(xs), bits(x / ln)), seed
    assert np.array_equal(bits(search(gpm, x, 1)[2]), bits(x))


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "lengths"])
@pytest.mark.parametrize("query", [False, True], ids=["causal", "query"])
@pytest.mark.parametrize("D", DS)
def test_shapes(gpm, D, query, scaled):
    """Every N x m of the lists above: rows with fewer than m candidates show the -1 padding (the first m rows of a causal
    table, every row of a query over N < m rows)."""
    for N in NS:
        x, z, ln, t, d2 = problem(N, D, query, scaled)
        for m in MS:
            got = search(gpm, x, m, Z=z, lengths=ln)
            same(got, (t[:, :m], d2[:, :m]), (N, m))
            if m:
                short = np.arange(N) < m if not query else np.full(N, N < m)  # rows with fewer than m candidates
                assert (got[0][short, -1] == -1).all() and (got[0][~short] >= 0).all()
        if N in (65, 257):  # the second witness
            want = VT.nearest(x, 31, ln) if z is None else VT.nearest_to(x, z, 31, ln)
            assert np.array_equal(t[:, :31], want)


def lattice():
    g = np.arange(6, dtype=F64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


@pytest.mark.parametrize("case", ["lattice", "shuffled", "repeated", "scaled"])
def test_exact_ties_go_to_the_lower_index(gpm, case):
    """Integer lattices: every distance is exact and most tie; repeated rows: distance 0."""
    rng = np.random.default_rng(409)
    x, ln = lattice(), None
    if case == "shuffled":
        x = np.ascontiguousarray(x[rng.permutation(len(x))])
    elif case == "repeated":
        x = np.ascontiguousarray(rng.uniform(-1, 1, (40, 3))[rng.integers(0, 40, 216)])
    elif case == "scaled":
        ln = np.array([0.5, 2.0, 1.0])
    z = np.ascontiguousarray(x[rng.integers(0, len(x), 70)] + (0.0 if case == "repeated" else 0.5))
    for m in (7, 63):
        want = naive(x, None, m, ln)
        same(search(gpm, x, m, lengths=ln), want, (case, m))
        assert np.array_equal(want[0], VT.nearest(x, m, ln))
        wz = naive(x, z, m, ln)
        same(search(gpm, x, m, Z=z, lengths=ln), wz, (case, m, "query"))
        assert np.array_equal(wz[0], VT.nearest_to(x, z, m, ln))
    t = naive(x, None, 63, ln)
    tied = sum(len(np.unique(r[:int((t[0][i] >= 0).sum())])) < int((t[0][i] >= 0).sum()) for i, r in enumerate(t[1]))
    assert tied > 100, "the case has ties among the entries taken"


@pytest.mark.parametrize("m", [7, 63])
@pytest.mark.parametrize("query", [False, True], ids=["causal", "query"])
def test_the_plan_does_not_show(gpm, m, query):
    """N = 300, D = 3 (five tiles, the last of 44 targets): 2, 7 and 64 slabs cut the candidates at 150, at multiples of 43
    and of 5 -- inside every tile's causal range, and most of 64 slabs hold no earlier row of the early targets -- and a
    grid of 1 or 3 workgroups walks the work units.  Every launch gives the bits of the naive loop, two identical launches
    the same bits."""
    rng = np.random.default_rng([419, m])
    x = np.round(rng.uniform(-2, 2, (300, 3)), 1)  # a tenth's grid: ties across the slab edges
    z = np.round(rng.uniform(-2, 2, (70, 3)), 1) if query else None
    ln = np.array([0.7, 1.9, 1.0])
    want = naive(x, z, m, ln)
    for slabs in (0, 1, 2, 7, 64):
        for cap in (0, 1, 3):
            same(search(gpm, x, m, Z=z, lengths=ln, slabs=slabs, tile_cap=cap), want, (slabs, cap))
    same(search(gpm, x, m, Z=z, lengths=ln, slabs=7, tile_cap=3), want, "again")
    # a target alone: the same row as inside the full launch
    for i in (0, 1, 64, 150, 299):
        if query:
            if i < len(z):
                got = search(gpm, x, m, Z=z[i:i + 1], lengths=ln)
                same(got, (want[0][i:i + 1], want[1][i:i + 1]), i)
        elif i > 0:
            got = search(gpm, np.ascontiguousarray(x[:i]), m, Z=x[i:i + 1], lengths=ln)
            same(got, (want[0][i:i + 1], want[1][i:i + 1]), i)


def test_a_row_that_overflows_is_never_taken(gpm):
    """Row 5 holds 1e200: every distance to it is +inf.  It is in no row of the table, its own row is empty, and the other
    rows hold what they hold without it."""
    rng = np.random.default_rng(421)
    x = rng.uniform(-2, 2, (129, 3))
    z = rng.uniform(-2, 2, (66, 3))
    big = x.copy()
    big[5, 1] = 1e200
    for m in (7, 63):
        for slabs in (0, 3):
            t, d2, _ = search(gpm, big, m, slabs=slabs)
            same((t, d2), naive(big, None, m, None), (m, slabs))
            assert not (t == 5).any() and (t[5] == -1).all()
            rest = np.delete(np.arange(129), 5)
            t0, d0 = naive(np.ascontiguousarray(x[rest]), None, m, None)
            back = np.where(t0 >= 0, rest[np.maximum(t0, 0)], -1)
            same((t[rest], d2[rest]), (back, d0), "the other rows")
            tz, dz, _ = search(gpm, big, m, Z=z, slabs=slabs)
            same((tz, dz), naive(big, z, m, None), (m, slabs, "query"))
            assert not (tz == 5).any()
