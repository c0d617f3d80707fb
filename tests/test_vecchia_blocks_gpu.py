"""Vecchia on blocks of targets on the GPU through the public calls (GP.SetVecchiaBlocks / VecchiaBlockObserve /
VecchiaBlockTerms / VecchiaBlockGradient / VecchiaBlockProduce), against the long-double restatement of
tests/vecchia_blocks_ref.py, which does not use the kernel's rank-t identity.

Tolerance: the scheme of tests/test_vecchia_kernel.py.  Every term is held to FACTOR = 8 x the restatement's own
float64-minus-long-double difference, relative to the quantity's largest magnitude (mu in units of y), times that
magnitude; the value and each component of the gradient, sums over the blocks, to that file's allowance for a launch's
sum (`judge`); the restatement's difference must itself stay
below 1e-10 (unit scale, noise variance 0.05, inputs on a few length scales: a condition on the inputs).  Every figure is
printed before it is asserted (-s).  Worst ratio recorded on an MI355X: DESIGN.md section 4, "Vecchia: blocks of targets"."""
import functools

import numpy as np
import pytest

import grad_reduce_ref as G
import gram_ref as R
import vecchia_blocks_ref as B
import vecchia_ref as V

pytestmark = pytest.mark.gpu

LD = np.longdouble
FACTOR = 8.0
NOISE_STD = 0.05 ** 0.5
#: (c, t) of one launch, in an order in which every conditioning set exists: the sizes at which the 16-blocking, the 4-wide
#: k step of the SYRK over [c, n), the padding and the full tile can each go wrong
SHAPES = [(0, 128), (0, 17), (0, 1), (15, 1), (16, 16), (63, 1), (127, 1), (64, 64), (100, 3)]
FAMILIES = list(R.RADIAL) + ["periodic", "max_terms", "hyperpriors", "ard"]
CASES = [(k, D) for k in FAMILIES for D in (1, 3)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def problem(kind, D, shapes=tuple(SHAPES), with_v=None):
    from gogp_amd import kernel as GK
    simil, ts = B.kernel_of(kind, D)
    desc = GK.build_desc(D, simil, GK.UniformNoise)
    kp = G.kp_from_desc(desc, ts, [NOISE_STD])
    blocks, N = B.random_blocks(np.random.default_rng([257, D, len(shapes)]), shapes)
    X, y, v = V.inputs(D + len(kind), N, D)
    if with_v is None:
        with_v = (len(kind) + D) % 2 == 0  # variances in half the cases
    return dict(D=D, N=N, simil=simil, ts=ts, desc=desc, kp=kp, X=X, y=y, v=v if with_v else None, blocks=blocks,
                x=np.log(np.array(list(ts) + [NOISE_STD])))


def gp_of(p, **kw):
    from gogp_amd import kernel as GK
    from gogp_amd.gp import GP
    return GP(p["D"], p["simil"], GK.UniformNoise, ThetaSimil=list(p["ts"]), ThetaNoise=[NOISE_STD], device=0, **kw)


def run(p, blocks=None, X=None, y=None, v=None, grid=0, grad=True):
    g = gp_of(p)
    if grid:
        g.set_option("vecchia_blocks_grid", grid)
    sel = X is not None
    g.SetVecchiaBlocks(X if sel else p["X"], y if sel else p["y"], blocks or p["blocks"], v if sel else p["v"])
    value = g.VecchiaBlockObserve(p["x"])
    out = dict(value=value, terms=np.stack(g.VecchiaBlockTerms(), axis=1), grad=g.VecchiaBlockGradient() if grad else None)
    g.close()
    return out


SUMS = ("value", "grad")


def quantities(p, r):
    """name -> array.  Of a reference result the value and the gradient's components are the BLOCKS' contributions (nb
    each); of a device result they are the launch's sums."""
    t = np.asarray(r["terms"])
    q = dict(mu=t[:, 0], s=t[:, 1], logp=t[:, 2])
    if "sblk" in r:
        grads = np.stack([G.assemble(p["desc"], row, p["kp"].dnoise) for row in r["sblk"]])
        q.update(value=r["vblk"], **{"grad%d" % i: grads[:, i] for i in range(grads.shape[1])})
    else:
        q.update(value=np.atleast_1d(r["value"]), **{"grad%d" % i: np.atleast_1d(g) for i, g in enumerate(r["grad"])})
    return q


def judge(p, got, ld, f64, what, terms=True):
    """Every quantity element by element (terms False: the value and the gradient only); returns the worst |err| / allowed.
    The terms: FACTOR x share x magnitude.  The value and each gradient component are sums over the blocks, which the
    public calls return whole: the share is taken over the blocks' contributions and the sum is allowed what
    tests/test_vecchia_kernel.py allows a launch's value -- (FACTOR x share x nb + gamma(nb + 1)) x sum of the magnitudes.
    A quantity that vanishes identically (the length scale's derivative of a single row) must vanish on the device too."""
    worst = 0.0
    want_all, f64_all, got_all = quantities(p, ld), quantities(p, f64), quantities(p, got)
    for q, want in want_all.items():
        summed = q.startswith(SUMS)
        if not terms and not summed:
            continue
        mag = max(float(np.abs(want).max()), float(np.abs(p["y"]).max()) if q == "mu" else 0.0)
        if mag == 0:
            assert not np.asarray(got_all[q]).any(), "%s %s" % (what, q)
            continue
        share = float(np.abs(f64_all[q].astype(LD) - want).max()) / mag
        assert share < 1e-10 and (summed or share > 0), "%s %s: the restatement's own difference %.3g" % (what, q, share)
        if summed:
            nb = len(want)
            err = abs(float(LD(got_all[q][0]) - want.sum()))
            allowed = (FACTOR * share * nb + G.gamma(nb + 1)) * float(np.abs(want).sum())
        else:
            err = float(np.abs(np.asarray(got_all[q], LD) - want).max())
            allowed = FACTOR * share * mag
        print("%s %-6s |err| %.3g, allowed %.3g" % (what, q, err, allowed))
        assert err <= allowed, "%s %s: |err| %.3g, allowed %.3g" % (what, q, err, allowed)
        worst = max(worst, err / allowed)
    return worst


@functools.lru_cache(maxsize=None)
def reference(kind, D, shapes=tuple(SHAPES), with_v=None):
    p = problem(kind, D, shapes, with_v)
    return tuple(B.observe(p["kp"], p["X"], p["y"], p["v"], p["blocks"], m) for m in ("ld", "f64"))


@pytest.mark.parametrize("case", CASES, ids=["%s-D%d" % c for c in CASES])
def test_long_double(case):
    """One launch of nine blocks of unequal shape: terms, value and every gradient component."""
    p = problem(*case)
    ld, f64 = reference(*case)
    assert not ld["failed"]
    print("vecchia blocks: worst |err| / allowed, %s-D%d: %.3f" % (case + (judge(p, run(p), ld, f64, "%s-D%d" % case),)))


@pytest.mark.parametrize("N", [1, 97, 128])
def test_one_block_is_the_dense_lml(N):
    """One block (0, N) equals Observe + Gradient of the same build, to the allowance of the restatement at that shape."""
    p = problem("matern52", 3, ((0, N),), True)
    ld, f64 = reference("matern52", 3, ((0, N),), True)
    got = run(p)
    judge(p, got, ld, f64, "one block N %d" % N, terms=False)
    d = gp_of(p)
    d.Absorb(p["X"], p["y"], p["v"])
    dense = dict(value=d.Observe(p["x"]), terms=got["terms"], grad=d.Gradient())
    d.close()
    judge(p, dense, ld, f64, "dense N %d" % N, terms=False)


def test_single_targets_are_the_vecchia_calls():
    """nt = 1 everywhere, c = 31: VecchiaObserve / VecchiaGradient on the corresponding table, to the allowance."""
    from gogp_amd import vecchia as VT
    N = 150
    p = dict(problem("hyperpriors", 3, ((0, 128), (0, 22)), True))
    X = p["X"]
    t = VT.nearest(X, 31)
    blocks = VT.block_nearest(X, 1, 31)
    p.update(blocks=blocks)
    ld, f64 = (B.observe(p["kp"], X, p["y"], p["v"], blocks, m) for m in ("ld", "f64"))
    got = run(p)
    judge(p, got, ld, f64, "nt = 1")
    g = gp_of(p)
    g.SetVecchia(X, p["y"], t, p["v"])
    one = dict(value=g.VecchiaObserve(p["x"]), terms=np.stack(g.VecchiaTerms(), axis=1), grad=g.VecchiaGradient())
    g.close()
    assert N == p["N"]
    judge(p, one, ld, f64, "the vecchia calls", terms=False)


def test_a_capped_grid_and_a_block_alone():
    """5 workgroups walk 40 blocks: two launches give identical bits, the terms are those of the free grid, and a block
    alone (its rows renumbered in the table's order) has the bits it has in the launch."""
    shapes = tuple([(0, 30)] + [(c, t) for c, t in [(7, 3), (30, 5), (16, 16), (1, 2), (25, 7), (12, 1), (20, 9)] * 6][:39])
    p = problem("max_terms", 3, shapes, True)
    a, b, free = run(p, grid=5), run(p, grid=5), run(p)
    assert a["value"] == b["value"] and np.array_equal(bits(a["terms"]), bits(b["terms"])) and np.array_equal(bits(a["grad"]), bits(b["grad"]))
    assert np.array_equal(bits(a["terms"]), bits(free["terms"])), "a block's terms depend on the grid"
    ld, f64 = reference("max_terms", 3, shapes, True)
    judge(p, a, ld, f64, "5 workgroups")
    tbl, nc, nt = p["blocks"]
    for k in (3, 17, 39):
        rows = tbl[k, :nc[k] + nt[k]]
        n = len(rows)
        # the conditioning rows first become single-row blocks without conditioning (each a target once), then the block
        one = np.full((nc[k] + 1, n), -1, np.int32)
        one[:nc[k], 0] = np.arange(nc[k])
        one[nc[k], :n] = np.arange(n)
        alone = run(p, (one, np.array([0] * nc[k] + [nc[k]], np.int32), np.array([1] * nc[k] + [nt[k]], np.int32)),
                    X=p["X"][rows], y=p["y"][rows], v=p["v"][rows], grad=False)
        assert np.array_equal(bits(alone["terms"][nc[k]:]), bits(a["terms"][rows[nc[k]:]])), "block %d" % k


def test_an_indefinite_block():
    """Rows 100 apart under the Normal kernel without noise: K is the identity but for a duplicated row, whose pivot is
    exactly 0 (the construction of tests/test_batch_windows_gpu.py).  Blocks 2 and 4 hold the duplicate."""
    from gogp_amd import kernel as GK
    from gogp_amd import _lib
    from gogp_amd.gp import GP, FactorizeError
    X = 100.0 * np.arange(24, dtype=float)[:, None]
    X[9] = X[5]
    X[17] = X[5]
    y = np.cos(np.arange(24.0))
    tbl = np.full((6, 8), -1, np.int32)
    nc, nt = np.array([0, 2, 1, 3, 2, 4], np.int32), np.array([4, 4, 4, 4, 4, 4], np.int32)
    for k in range(6):
        tbl[k, nc[k]:nc[k] + 4] = np.arange(4 * k, 4 * k + 4)
    tbl[1, :2], tbl[2, :1], tbl[3, :3], tbl[4, :2], tbl[5, :4] = (0, 3), (5,), (1, 2, 6), (5, 9), (0, 4, 8, 12)
    ok = tbl.copy()
    ok[2, 0], ok[4, :2] = 4, (4, 8)  # the same blocks on other rows: no duplicate inside a block

    def go(table):
        g = GP(1, GK.Normal, GK.ConstantNoise(0.0), ThetaSimil=[2.0], device=0)
        g.SetVecchiaBlocks(X, y, (table, nc, nt))
        try:
            value, failed = g.VecchiaBlockObserve(np.log([2.0])), None
        except FactorizeError:
            value, failed = np.nan, _lib.lib().gogp_notpd_index(g._h)
        terms = np.stack(g.VecchiaBlockTerms(), axis=1)
        g.close()
        return value, failed, terms

    value, failed, terms = go(tbl)
    base = go(ok)
    assert failed == 2 and np.isnan(value) and base[1] is None and np.isfinite(base[2]).all()
    bad = np.r_[8:12, 16:20]
    assert np.isnan(terms[bad]).all()
    keep = np.setdiff1d(np.arange(24), bad)
    assert np.array_equal(bits(terms[keep]), bits(base[2][keep])), "another block's terms moved"


@pytest.mark.parametrize("kind", ["matern52", "max_terms", "ard"])
def test_produce(kind):
    """Groups of 1 and 5 test points on 0, 1 and 128 conditioning rows; mu in units of y."""
    p = problem(kind, 3, tuple(SHAPES), True)
    rng = np.random.default_rng(263)
    Z = rng.uniform(-3.0, 3.0, (18, 3))
    off = np.array([0, 1, 6, 7, 12, 13, 18], np.int64)
    ncz = np.array([0, 0, 1, 1, 128, 128], np.int32)
    tblz = np.full((6, 128), -1, np.int32)
    for g in range(6):
        tblz[g, :ncz[g]] = rng.choice(p["N"], size=ncz[g], replace=False)
    ld, f64 = (B.produce(p["kp"], p["X"], p["y"], p["v"], Z, off, (tblz, ncz), m) for m in ("ld", "f64"))
    g = gp_of(p)
    g.SetVecchiaBlocks(p["X"], p["y"], p["blocks"], p["v"])
    g.VecchiaBlockObserve(p["x"])
    mu, sigma = g.VecchiaBlockProduce(Z, off, (tblz, ncz))
    mu2, none = g.VecchiaBlockProduce(Z, off, (tblz, ncz), sigma=False)
    g.close()
    assert none is None and np.array_equal(bits(mu), bits(mu2))
    for q, got, want, w64, mag in (("mu", mu, ld[0], f64[0], max(float(np.abs(ld[0]).max()), float(np.abs(p["y"]).max()))),
                                   ("sigma", sigma, ld[1], f64[1], float(np.abs(ld[1]).max()))):
        share = float(np.abs(w64.astype(LD) - want).max()) / mag
        err = float(np.abs(got.astype(LD) - want).max())
        print("produce %s %-5s |err| %.3g, allowed %.3g" % (kind, q, err, FACTOR * share * mag))
        assert 0 < share < 1e-10 and err <= FACTOR * share * mag


def test_stored_results_never_go_stale():
    """New data drop what an observe stored (gradient and produce then want a new observe), and the dense state of the same
    handle returns the bits it returned before the block calls."""
    from gogp_amd import _lib
    from gogp_amd.gp import GogpError
    p = problem("matern52", 3, ((0, 30), (7, 3), (30, 5)), True)
    g = gp_of(p)
    g.Absorb(p["X"], p["y"])
    lml, grad = g.Observe(p["x"]), g.Gradient()
    off, groups = np.array([0, 2], np.int64), (np.array([[3, 1, 4]], np.int32), np.array([3], np.int32))

    def stale():
        for call in (g.VecchiaBlockGradient, lambda: g.VecchiaBlockProduce(p["X"][:2] + 0.1, off, groups)):
            with pytest.raises(GogpError) as e:
                call()
            assert e.value.code == _lib.GOGP_ESTATE

    g.SetVecchiaBlocks(p["X"], p["y"], p["blocks"], p["v"])
    stale()
    g.VecchiaBlockObserve(p["x"])
    first = g.VecchiaBlockGradient(), g.VecchiaBlockProduce(p["X"][:2] + 0.1, off, groups)[0]
    g.SetVecchiaBlocks(p["X"], p["y"], p["blocks"], p["v"])
    stale()
    g.VecchiaBlockObserve(p["x"])
    assert np.array_equal(bits(g.VecchiaBlockGradient()), bits(first[0]))
    assert np.array_equal(bits(g.VecchiaBlockProduce(p["X"][:2] + 0.1, off, groups)[0]), bits(first[1]))
    assert g.Observe(p["x"]) == lml and np.array_equal(bits(g.Gradient()), bits(grad))
    g.close()
