"""GP.SetInducing / SparseGradientInducing (gogp_sparse_set_inducing, gogp_sparse_gradient_inducing) on the GPU against
the numpy reference of tests/sparse_inducing_ref.py (tests/test_sparse_inducing_cpu.py pins it to central differences),
and sparse_ugrad_kernel in isolation through its test hook.

sparse_ugrad_kernel alone: against xgrad_np(desc, ths, U, X, Wt[:, :M].T + outer(mvec, y) s4), every component within
1e-6 of the largest (produce_grad_ref.assert_derivative, the suite's gradient rule).  Wt has mixed signs, ldw = M + 5 and
NaN in its padding columns: a read past M shows.  Shapes: rows = 130, M = 70 is three row tiles (the last with 2 rows)
and two column tiles (the second with 6 inducing points); D = 64 takes four dimension passes and the raised LDS limit;
rows = 1100 is the first multiple of 100 at which the slab rule gives more than one slab with a short last one (18 row
tiles in slabs of 4: five slabs, the last of two tiles, its second tile of 12 rows) -- asserted from the launch's own
slab function.

Through the C ABI: the options of tests/test_sparse_gpu.py (eps = 1e-2, "sparse_chunk" = 256), N = 700 (three chunks, a
ragged last one), M = 48 and 300 (one and two 256-panels).  dU by the 1e-6 rule; grad bit for bit gogp_sparse_gradient's.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

import grad_reduce_ref as GR
import sparse_inducing_ref as IR
import sparse_ref as SR
from gogp_amd import _lib, kernel, optimize, synth
from oracle.oracle import xgrad_np
from produce_grad_ref import assert_derivative

pytestmark = pytest.mark.gpu

JIT = -2
EPS = 10.0 ** JIT
N0 = 700
_REF = {}


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- sparse_ugrad_kernel in isolation -----------------------------------------------------------------------------------
def _hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4, accumulate=False, du0=None, extra=0):
    X, U, Wt = (np.ascontiguousarray(a, float).reshape(-1) for a in (X, U, Wt))
    y, mvec = np.ascontiguousarray(y, float), np.ascontiguousarray(mvec, float)
    D = U.size // len(mvec)
    dU = np.zeros(len(mvec) * D + extra) if du0 is None else np.array(du0, float).reshape(-1)
    rc = _lib.hooks().gogp_test_sparse_ugrad(0, kp.hook(gpm), _dp(X), X.size, len(y), _dp(U), U.size, len(mvec), _dp(Wt),
                                             Wt.size, ldw, _dp(y), y.size, _dp(mvec), mvec.size, s4, int(accumulate),
                                             _dp(dU), dU.size)
    assert rc == _lib.GOGP_OK
    return dU


def _kernel_case(gpm, fam, rows, M, seed=3):
    D, simil, ts = SR.FAMILIES[fam]
    desc = kernel.build_desc(D, simil, SR.NOISE)
    ths = np.asarray(ts, float)
    kp = GR.kp_from_desc(desc, ths, SR.TN)
    rng = np.random.default_rng(seed + rows + M)
    X = SR.inputs(rows, 1, D)[0]
    U = SR.inputs(M, 1, D, seed=11)[0]
    ldw = M + 5
    Wt = np.full((rows, ldw), np.nan)
    Wt[:, :M] = rng.normal(size=(rows, M))  # mixed sign
    y, mvec, s4 = rng.normal(size=rows), rng.normal(size=M), 1.0 / 0.09 ** 2
    got = _hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4).reshape(M, D)
    want = xgrad_np(desc, ths, U, X, Wt[:, :M].T + np.outer(mvec, y) * s4)
    assert_derivative(got, want, "%s rows %d M %d" % (fam, rows, M))
    return kp, X, U, Wt, ldw, y, mvec, s4, got


@pytest.mark.parametrize("fam", SR.FOUR + ["ard_rbf64"])
def test_ugrad_kernel_against_the_pair_sum(gpm, fam):
    _kernel_case(gpm, fam, 130, 70)


@pytest.mark.parametrize("rows,M", [(1, 70), (130, 1), (1, 1), (64, 64), (65, 129)])
def test_ugrad_kernel_edge_shapes(gpm, rows, M):
    _kernel_case(gpm, "ard_rbf3", rows, M)
    _kernel_case(gpm, "hyperpriors", rows, M)


def test_ugrad_kernel_several_slabs_with_a_ragged_last_one(gpm):
    rows, M = 1100, 70
    tps = ctypes.c_int(0)
    nslab = _lib.hooks().gogp_test_sparse_ugrad_slabs(rows, M, ctypes.byref(tps))
    ntr = (rows + 63) // 64
    print("rows %d, M %d: %d slabs of %d row tiles for %d tiles" % (rows, M, nslab, tps.value, ntr))
    assert rows <= 2000 and nslab >= 2
    assert 0 < ntr - (nslab - 1) * tps.value < tps.value  # the last slab holds fewer tiles
    assert rows % 64  # and its last tile fewer rows
    _kernel_case(gpm, "ard_rbf3", rows, M)
    _kernel_case(gpm, "hyperpriors", rows, M)


def test_ugrad_kernel_accumulates_repeats_and_keeps_to_its_rows(gpm):
    kp, X, U, Wt, ldw, y, mvec, s4, got = _kernel_case(gpm, "ard_rbf64", 130, 70)
    M, D = got.shape
    again = _hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4)
    np.testing.assert_array_equal(again.reshape(M, D), got)  # fixed order: the same bits
    base = np.arange(1.0, (M + 3) * D + 1.0)  # three rows beyond M
    acc = _hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4, accumulate=True, du0=base)
    np.testing.assert_array_equal(acc[:M * D], base[:M * D] + got.reshape(-1))
    np.testing.assert_array_equal(acc[M * D:], base[M * D:])
    over = _hook(gpm, kp, X, U, Wt, ldw, y, mvec, s4, accumulate=False, du0=base)
    np.testing.assert_array_equal(over[:M * D], got.reshape(-1))
    np.testing.assert_array_equal(over[M * D:], base[M * D:])


# ---- through the C ABI --------------------------------------------------------------------------------------------------
def _x(fam):
    return np.log(np.array(list(SR.FAMILIES[fam][2]) + SR.TN))


def _ref(fam, N, M, eps=EPS):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, N, M, eps)
    if key not in _REF:
        D, simil, _ = SR.FAMILIES[fam]
        X, y, Z = SR.inputs(N, 7, D)
        if M <= N:
            U = IR.displaced_subset(X, M)
        else:
            U = np.vstack([X, np.random.default_rng(5).uniform(-2.0, 2.0, (M - N, D))])
        F, grad, dU, st = IR.du_reference(D, simil, _x(fam), X, y, U, eps)
        _REF[key] = dict(X=X, y=y, Z=Z, U=U, F=F, grad=grad, dU=dU)
    return _REF[key]


def _gp(fam, jit=JIT, chunk=256, **kw):
    from gogp_amd.gp import GP
    D, s, ts = SR.FAMILIES[fam]
    g = GP(D, s, SR.NOISE, ThetaSimil=ts, ThetaNoise=SR.TN, device=0, **kw)
    if kw.get("precision", 64) == 64:
        g.set_option("sparse_jitter_log10", jit)
        g.set_option("sparse_chunk", chunk)
    return g


@pytest.mark.parametrize("M", [48, 300])
@pytest.mark.parametrize("fam", SR.FOUR)
def test_values_and_bits(fam, M):
    r = _ref(fam, N0, M)
    x = _x(fam)
    g = _gp(fam)
    g.SetSparse(r["X"], r["y"], r["U"])
    g.SparseObserve(x)
    plain = g.SparseGradient()
    grad, dU = g.SparseGradientInducing()
    assert dU.shape == r["dU"].shape
    assert_derivative(dU, r["dU"], "dU %s M %d" % (fam, M))
    assert_derivative(grad, r["grad"], "grad %s M %d" % (fam, M))
    np.testing.assert_array_equal(grad, plain)  # the bits of gogp_sparse_gradient
    grad2, dU2 = g.SparseGradientInducing()
    np.testing.assert_array_equal(grad2, grad)
    np.testing.assert_array_equal(dU2, dU)
    np.testing.assert_array_equal(g.SparseGradient(), plain)  # and gogp_sparse_gradient afterwards still its own
    g.close()


@pytest.mark.parametrize("M", [48, 300])
def test_chunk_sizes_agree(M):
    fam = "ard_rbf3"
    r = _ref(fam, N0, M)
    outs = []
    for chunk in (256, 1024):
        g = _gp(fam, chunk=chunk)
        g.SetSparse(r["X"], r["y"], r["U"])
        g.SparseObserve(_x(fam))
        outs.append(g.SparseGradientInducing()[1])
        g.close()
    d = np.abs(outs[0] - outs[1]).max() / np.abs(outs[1]).max()
    print("M = %d dU: chunk 256 against 1024: %.3e of the largest" % (M, d))
    assert d <= 1e-11, d


def test_larger_case_against_the_chunked_reference():
    """N = 2500 at "sparse_chunk" = 1024: two full chunks and a ragged one (452 rows), M = 300."""
    fam, N, M = "matern32_2d", 2500, 300
    D, simil, _ = SR.FAMILIES[fam]
    X, y, _ = SR.inputs(N, 7, D)
    U = IR.displaced_subset(X, M)
    x = _x(fam)
    F, grad, dU, _ = IR.du_reference_chunked(D, simil, x, X, y, U, EPS, 1024)
    g = _gp(fam, chunk=1024)
    g.SetSparse(X, y, U)
    g.SparseObserve(x)
    got_grad, got = g.SparseGradientInducing()
    assert_derivative(got, dU, "dU N = 2500, M = 300")
    assert_derivative(got_grad, grad, "grad N = 2500, M = 300")
    g.close()


def test_ragged_last_chunk_that_takes_more_slabs_than_a_full_one():
    """M = 2048, "sparse_chunk" = 16640, N = 33024: the full chunk goes in 52 slabs (five row tiles each), the 16384-row
    tail in 64 (four each) -- the buffer of partials has to hold the larger count.  Against the same handle's result at
    "sparse_chunk" = 16384 (64 slabs in every chunk), by the suite's rule for gradients: a tail that wrote past its
    partials would land in the two M x D parts behind them."""
    fam, N, M = "matern32_2d", 33024, 2048
    D, simil, _ = SR.FAMILIES[fam]
    tps = ctypes.c_int(0)
    f = _lib.hooks().gogp_test_sparse_ugrad_slabs
    assert f(16640, M, ctypes.byref(tps)) < f(N - 16640, M, ctypes.byref(tps))
    X, y, _ = SR.inputs(N, 7, D)
    U = IR.displaced_subset(X, M)
    outs = []
    for chunk in (16384, 16640):
        g = _gp(fam, chunk=chunk)
        g.SetSparse(X, y, U)
        g.SparseObserve(_x(fam))
        outs.append(g.SparseGradientInducing())
        np.testing.assert_array_equal(g.SparseGradientInducing()[1], outs[-1][1])  # and the same bits again
        g.close()
    assert_derivative(outs[1][1], outs[0][1], "dU, chunk 16640 against 16384")
    assert_derivative(outs[1][0], outs[0][0], "grad, chunk 16640 against 16384")


def test_set_inducing_equals_a_fresh_set_data():
    fam, M = "ard_rbf3", 48
    r = _ref(fam, N0, M)
    x = _x(fam)
    U1 = r["U"]
    U2 = IR.displaced_subset(r["X"], M, seed=17)
    outs = []
    for moved in (False, True):
        g = _gp(fam)
        if moved:
            g.SetSparse(r["X"], r["y"], U1)
            g.SparseObserve(x)
            g.SparseGradientInducing()
            g.SetInducing(U2)
        else:
            g.SetSparse(r["X"], r["y"], U2)
        outs.append((np.array([g.SparseObserve(x)]), *g.SparseGradientInducing(), *g.SparseProduce(r["Z"])))
        g.close()
    for what, a, b in zip(("bound", "grad", "dU", "mu", "sigma"), *outs):
        np.testing.assert_array_equal(a, b, err_msg=what)


def test_lifecycle_and_refusals():
    from gogp_amd.gp import GP
    fam = "matern52"
    D, simil, ts = SR.FAMILIES[fam]
    r = _ref(fam, N0, 48)
    X, y, U, Z = r["X"], r["y"], np.ascontiguousarray(r["U"]), np.ascontiguousarray(r["Z"][:3])
    x = _x(fam)
    P = x.size
    L = _lib.lib()
    v, grad, dU, mu, sg = ctypes.c_double(0.0), np.zeros(P), np.zeros(U.shape), np.zeros(3), np.zeros(3)
    g = _gp(fam)
    assert L.gogp_sparse_set_inducing(g._h, _dp(U), 48) == _lib.GOGP_ESTATE  # before gogp_sparse_set_data
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_ESTATE
    g.SetSparse(X, y, U)
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_ESTATE  # before observe
    g.SparseObserve(x)
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_OK
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, None) == _lib.GOGP_EARG
    assert L.gogp_sparse_gradient_inducing(g._h, None, P, _dp(dU)) == _lib.GOGP_EARG
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P - 1, _dp(dU)) == _lib.GOGP_EARG
    # refused set_inducing calls leave the observed state alone
    Ub = U.copy()
    Ub[5, 0] = np.nan
    for args in ((_dp(U), 47), (_dp(U), 49), (_dp(U), 0), (None, 48), (_dp(Ub), 48)):
        assert L.gogp_sparse_set_inducing(g._h, *args) == _lib.GOGP_EARG, args[1]
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_OK
    # an accepted one asks for a new observe
    assert L.gogp_sparse_set_inducing(g._h, _dp(U), 48) == _lib.GOGP_OK
    assert L.gogp_sparse_gradient(g._h, _dp(grad), P) == _lib.GOGP_ESTATE
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_ESTATE
    assert L.gogp_sparse_produce(g._h, _dp(Z), 3, _dp(mu), _dp(sg)) == _lib.GOGP_ESTATE
    assert L.gogp_sparse_observe(g._h, _dp(x), P, ctypes.byref(v)) == _lib.GOGP_OK
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_OK
    assert_derivative(dU, r["dU"], "after set_inducing with the same points")
    # event discounts are out of scope: refused, by name
    ev = np.array([0.0, 1.0, 0.5])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == _lib.GOGP_OK
    assert L.gogp_sparse_set_inducing(g._h, _dp(U), 48) == _lib.GOGP_EARG
    assert b"event" in L.gogp_last_error(g._h)
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_EARG
    assert L.gogp_set_events(g._h, None, 0, 0) == _lib.GOGP_OK
    assert L.gogp_sparse_observe(g._h, _dp(x), P, ctypes.byref(v)) == _lib.GOGP_OK
    assert L.gogp_sparse_gradient_inducing(g._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_OK
    assert_derivative(dU, r["dU"], "events cleared again")
    g.close()
    g32 = GP(D, simil, SR.NOISE, ThetaSimil=ts, ThetaNoise=SR.TN, device=0, precision=32)
    assert L.gogp_sparse_set_inducing(g32._h, _dp(U), 48) == _lib.GOGP_EARG
    assert b"precision = 32" in L.gogp_last_error(g32._h)
    assert L.gogp_sparse_gradient_inducing(g32._h, _dp(grad), P, _dp(dU)) == _lib.GOGP_EARG
    g32.close()


def test_sharded_handles_are_refused():
    import loopback
    from gogp_amd.sharded import ShardedGP
    fam = "matern52"
    D, simil, _ = SR.FAMILIES[fam]
    U = np.ascontiguousarray(_ref(fam, N0, 48)["U"])
    P = _x(fam).size

    def rank_fn(r, lb):
        sh = ShardedGP(D, simil, SR.NOISE, device=0, grid=(1, 2), rank=r, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        L = _lib.lib()
        grad, dU = np.zeros(P), np.zeros(U.shape)
        rcs = (L.gogp_sparse_set_inducing(sh._h, _dp(U), 48), L.gogp_sparse_gradient_inducing(sh._h, _dp(grad), P, _dp(dU)))
        msg = L.gogp_last_error(sh._h)
        sh.close()
        return rcs, msg

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rcs, msg in outs:
        assert rcs == (_lib.GOGP_EARG, _lib.GOGP_EARG) and b"sharded" in msg


def test_no_observations():
    fam = "ard_rbf3"
    D, simil, ts = SR.FAMILIES[fam]
    X = SR.inputs(30, 7, D)[0]
    g = _gp(fam)
    g.SetSparse(np.zeros((0, D)), np.zeros(0), X)
    assert g.SparseObserve(_x(fam)) == 0.0
    grad, dU = g.SparseGradientInducing()
    assert grad.shape == (len(ts) + 1,) and not grad.any()
    assert dU.shape == (30, D) and not dU.any()
    g.SetInducing(X[::-1].copy())
    assert g.SparseObserve(_x(fam)) == 0.0
    g.close()


def test_more_inducing_points_than_observations():
    fam = "matern32_2d"
    r = _ref(fam, 20, 48)
    g = _gp(fam)
    g.SetSparse(r["X"], r["y"], r["U"])
    g.SparseObserve(_x(fam))
    grad, dU = g.SparseGradientInducing()
    assert_derivative(dU, r["dU"], "M = 48 > N = 20")
    g.close()


def test_duplicated_inducing_points():
    """The jitter carries them; the coincident pairs add exact zeros."""
    fam = "matern32_2d"
    D, simil, _ = SR.FAMILIES[fam]
    X, y, _ = SR.inputs(200, 7, D)
    U = np.vstack([X[:24], X[:24]])
    dU = IR.du_reference(D, simil, _x(fam), X, y, U, EPS)[2]
    g = _gp(fam)
    g.SetSparse(X, y, U)
    g.SparseObserve(_x(fam))
    got = g.SparseGradientInducing()[1]
    assert np.isfinite(got).all()
    assert_derivative(got, dU, "duplicated inducing points")
    g.close()


def test_dense_state_is_untouched_and_the_sparse_state_survives():
    """One of two twins interleaves the new calls with the dense ones: Produce, Gradient, LOO and MultiLML return the
    same bits.  (The pattern of tests/test_sparse_gpu.py.)"""
    fam = "ard_rbf3"
    D, simil, _ = SR.FAMILIES[fam]
    r = _ref(fam, N0, 48)
    U2 = IR.displaced_subset(r["X"], 48, seed=17)
    Xd, yd, Zd = SR.inputs(300, 33, D, seed=21)
    Yd = np.stack([yd, yd ** 2, np.cos(yd)], axis=1)

    def run(sparse):
        g = _gp(fam)
        sp = []
        if sparse:
            g.SetSparse(r["X"], r["y"], r["U"])
            sp.append(g.SparseObserve(_x(fam)))
        g.X, g.Y = Xd, yd
        out = [np.array([g.Observe(_x(fam))])]
        if sparse:
            sp.append(g.SparseObserve(_x(fam)))  # survives the dense set_data
            g.SparseGradientInducing()
        out += [g.Gradient(), *g.Produce(Zd)]
        if sparse:
            g.SetInducing(U2)
            sp.append(g.SparseObserve(_x(fam)))
            g.SparseGradientInducing()
        out += [*g.LOO(), g.LOOGradient()]
        g.SetOutputs(Yd)
        if sparse:
            g.SetInducing(r["U"])
            sp.append(g.SparseObserve(_x(fam)))
            g.SparseGradientInducing()
        out += [np.array([g.MultiLML()[0]]), g.MultiGradient(), *g.Produce(Zd), g.L, g.Alpha]
        if sparse:
            assert sp[0] == sp[1] == sp[3] and sp[2] != sp[0]
        g.close()
        return out

    for u, v in zip(run(False), run(True)):
        np.testing.assert_array_equal(u, v)


# ---- SparseModel(inducing=True) -------------------------------------------------------------------------------------------
def test_optimiser_moves_the_inducing_points_and_raises_the_bound():
    """optimize.lbfgs over x = [log theta | U] for ten iterations, then bound and gradient at the point it ends at against
    the reference.  Ten, not to convergence: at a stationary point every component of the gradient is the rounding residue
    of sums whose terms are of the size of the starting gradient (8e2 here) and cancel, so a rule relative to the largest
    component measures nothing there -- run to |grad|_inf <= 1e-3 (612 iterations) the two gradients differ by 2.0e-7
    absolute, 2.5e-10 of those terms, beside a largest component of 9.9e-4.  An ascent that has just begun still has
    components of the size of its terms."""
    from gogp_amd.gp import GP, SparseModel
    n, D, M = 600, 2, 40
    X, y = synth.make_inputs(n, D, 5)
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, SR.NOISE, device=0)
    g.set_option("sparse_jitter_log10", -6)
    U0 = X[np.random.default_rng(5).choice(n, M, replace=False)].copy()
    g.SetSparse(X, y, U0)
    m = SparseModel(g, inducing=True)
    th0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    x0 = np.concatenate([th0, U0.reshape(-1)])
    start = m.Observe(x0)
    g0 = m.Gradient()
    assert g0.shape == x0.shape
    res = optimize.lbfgs(m, x0, major_iterations=10, gradient_threshold=1e-3)
    end = m.Observe(res.x)
    g1 = m.Gradient()
    P = th0.size
    print("sparse objective with inducing points: start %.9f, end %.9f after %d iterations, %d evaluations; |grad| %.3e -> "
          "%.3e; inducing points moved by at most %.3e" % (start, end, res.iterations, res.evaluations, np.linalg.norm(g0),
                                                           np.linalg.norm(g1), np.abs(res.x[P:] - x0[P:]).max()))
    assert end > start
    assert np.abs(res.x[P:] - x0[P:]).max() > 0.0
    # bound and gradient at the final x against the reference
    Uf = res.x[P:].reshape(M, D)
    F, grad, dU, _ = IR.du_reference(D, simil, res.x[:P], X, y, Uf, 1e-6)
    print("final x: bound %.12e (reference %.12e)" % (end, F))
    assert abs(end - F) <= 1e-6 * abs(F)
    assert_derivative(g1, np.concatenate([grad, dU.reshape(-1)]), "gradient at the final x")
    # the default model takes the hyperparameters only
    with pytest.raises(ValueError, match="hyperparameters only"):
        SparseModel(g).Observe(res.x)
    with pytest.raises(ValueError):
        m.Observe(res.x[:-1])
    g.close()
