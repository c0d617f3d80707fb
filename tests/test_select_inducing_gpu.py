"""GP.SelectInducing / SetSparseGreedy / SparseModel.reselect (gogp_sparse_select_inducing*) on the GPU, through the C ABI.

Pivot sequences are NOT compared with an independent reference run: far from the pivot many rows are nearly tied
(relative gaps down to 8e-13 on these inputs) and a legitimate rounding difference reorders them.  Instead the DEVICE's
sequence is replayed on the CPU (tests/select_inducing_ref.py: replay) in fp64 and in long double, and
    delta_j = the running maximum over the steps <= j of |d64 - dld|_inf, floored at 2.2e-16 * max k(x, x)
measures the rounding level of the recurrence itself (5e-16 .. 3e-15 absolute on every case here, at every step).  Then
  pick         the long-double residual at the device's pick >= the long-double maximum - 64 delta_j;
  pivot value  pivots[j] within 64 delta_j of the long-double residual at the pick;
  trace        within N delta_m of the long-double sum (N residuals, each off by at most delta);
  U and m      U == X[idx] bit for bit, no index twice, m <= min(M, N);
  stop rule    m == M, or the long-double residual maximum after step m <= tol + 64 delta_m;
  first pick   idx[0] == 0: all of k(x, x) are the same bits.
The factor 64 covers the device's elementary functions and its different summation order: a simulated device (kernel
values perturbed by +-2 ulp, a four-way split of the dot product) always picked the exact maximiser and was off by at
most 4.1 delta in the pivot values.  What keeps the rule from hiding a wrong pick is asserted on the reference:
64 delta_j <= 1e-6 * (long-double residual at the pick) at every step.

Cases: FOUR x (N, M, tol) in {(1, 1, 1e-8), (63, 63, 1e-8), (257, 37, 1e-8), (257, 257, 1e-6), (700, 130, 1e-8),
(1000, 300, 1e-8)} (the fourth stops early for matern52 and hyperpriors), ard_rbf64 at (300, 40, 1e-8) for D = 64, and one
multi-workgroup ragged case, N = 70001, D = 2, M = 64.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

import select_inducing_ref as SI
import sparse_ref as SR
from gogp_amd import _lib

pytestmark = pytest.mark.gpu

EPSM = 2.2e-16
SHAPES = [(1, 1, 1e-8), (63, 63, 1e-8), (257, 37, 1e-8), (257, 257, 1e-6), (700, 130, 1e-8), (1000, 300, 1e-8)]
CASES = [(f,) + s for f in SI.FOUR for s in SHAPES] + [("ard_rbf64", 300, 40, 1e-8), ("matern32_2d", 70001, 64, 1e-8)]
_RUN = {}


def _x(fam):
    return np.log(np.array(list(SI.FAMILIES[fam][2]) + SI.TN))


def _gp(fam, jit=-2, **kw):
    from gogp_amd.gp import GP
    D, s, ts = SI.FAMILIES[fam]
    g = GP(D, s, SI.NOISE, ThetaSimil=ts, ThetaNoise=SI.TN, device=0, **kw)
    if kw.get("precision", 64) == 64:
        g.set_option("sparse_jitter_log10", jit)
        g.set_option("sparse_chunk", 256)
    return g


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _run(fam, N, M, tol):
    """One selection on the device: computed once, shared, read only."""
    key = (fam, N, M, tol)
    if key not in _RUN:
        D = SI.FAMILIES[fam][0]
        X = SI.inputs(N, 1, D)[0]
        g = _gp(fam)
        out = g.SelectInducing(_x(fam), M, X=X, tol=tol)
        g.close()
        _RUN[key] = (X,) + out
    return _RUN[key]


def _same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


@pytest.mark.parametrize("fam,N,M,tol", CASES, ids=["%s-%d-%d-%g" % c for c in CASES])
def test_selection_against_the_replay_of_its_own_pivots(fam, N, M, tol):
    X, idx, U, pivots, trace = _run(fam, N, M, tol)
    D, simil, _ = SI.FAMILIES[fam]
    ths = np.exp(_x(fam)[:-1])  # the natural parameters as the library forms them
    K = SI.Columns(D, simil, ths, X)
    m = len(idx)
    assert 1 <= m <= min(M, N) and len(pivots) == m and U.shape == (m, D)
    assert idx[0] == 0
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < N
    np.testing.assert_array_equal(U, X[idx])
    R64, _ = SI.replay(K, idx, np.float64)
    Rld, _ = SI.replay(K, idx, SI.LD)
    kmax = float(K.diag().max())
    delta = np.maximum(np.maximum.accumulate(np.abs(R64 - Rld).max(axis=1).astype(np.float64)), EPSM * kmax)
    steps = np.arange(m)
    at_pick = Rld[steps, idx].astype(np.float64)
    top = Rld[:m].max(axis=1).astype(np.float64)
    print("%s N %d M %d tol %g: m %d, delta %.3g .. %.3g, 64 delta / residual at the pick at most %.3g, pick short of the "
          "maximum by at most %.3g delta, pivot values off by at most %.3g delta, trace off by %.3g of N delta"
          % (fam, N, M, tol, m, delta.min(), delta.max(), (64 * delta[:m] / at_pick).max(),
             ((top - at_pick) / delta[:m]).max(), (np.abs(pivots - at_pick) / delta[:m]).max(),
             abs(trace - float(Rld[m].sum())) / (N * delta[m])))
    assert np.all(64 * delta[:m] <= 1e-6 * at_pick)  # on the reference: the rule below cannot hide a wrong pick
    assert np.all(at_pick >= top - 64 * delta[:m])
    assert np.all(np.abs(pivots - at_pick) <= 64 * delta[:m])
    assert abs(trace - float(Rld[m].sum())) <= N * delta[m]
    assert m == M or float(Rld[m].max()) <= tol + 64 * delta[m]


def test_the_early_stop_case_stops_early():
    for fam in ("matern52", "hyperpriors"):
        assert len(_run(fam, 257, 257, 1e-6)[1]) < 257


def test_identical_calls_and_the_resident_form_return_identical_bits():
    fam, N, M, tol = "ard_rbf3", 700, 130, 1e-8
    first = _run(fam, N, M, tol)
    X = first[0]
    g = _gp(fam)
    again = g.SelectInducing(_x(fam), M, X=X, tol=tol)
    _same(first[1:], again)
    y = np.sin(X.sum(1))
    g.SetSparse(X, y, X[5:9])  # any inducing points
    _same(first[1:], g.SelectInducing(_x(fam), M, tol=tol))
    g.SparseObserve(_x(fam))
    _same(first[1:], g.SelectInducing(_x(fam), M, tol=tol))
    g.close()


def test_negative_tol_is_the_jitter():
    fam, N, M = "matern52", 257, 257
    X = SI.inputs(N, 1, 1)[0]
    g = _gp(fam, jit=-6)
    _same(g.SelectInducing(_x(fam), M, X=X, tol=None), _run(fam, N, M, 1e-6)[1:])
    _same(g.SelectInducing(_x(fam), M, X=X, tol=-3.0), _run(fam, N, M, 1e-6)[1:])
    g.close()


def test_handle_state_is_untouched():
    """Twins: one runs selections between its calls, the other does not.  Dense Produce and Gradient, and the sparse
    observe, gradient and produce, return identical bits; the selection runs before the sparse data's first observe and
    after one."""
    fam = "ard_rbf3"
    D = SI.FAMILIES[fam][0]
    x = _x(fam)
    Xd, yd, Zd = SI.inputs(300, 33, D, seed=21)
    Xs, ys, Zs = SI.inputs(700, 7, D)
    U = Xs[::15][:40].copy()
    outs = []
    for select in (False, True):
        g = _gp(fam)
        sel = (lambda **kw: g.SelectInducing(x + 0.1, 50, **kw)) if select else (lambda **kw: None)
        g.X, g.Y = Xd, yd
        lml = g.Observe(x)
        sel(X=Xs)
        mu, sg = g.Produce(Zd)
        sel(X=Xd)
        grad = g.Gradient()
        g.SetSparse(Xs, ys, U)
        sel()  # resident, before the first observe
        F = g.SparseObserve(x)
        sel()  # ... and after one
        sgrad = g.SparseGradient()
        sel(X=Xd)
        smu, ssg = g.SparseProduce(Zs)
        mu2, sg2 = g.Produce(Zd)  # the dense state is still there
        outs.append((np.array([lml, F]), mu, sg, grad, sgrad, smu, ssg, mu2, sg2))
        g.close()
    _same(*outs)


def test_more_points_than_rows_no_rows_and_refusals():
    from gogp_amd.gp import GP, GogpError
    fam = "matern32_2d"
    D, simil, ts = SI.FAMILIES[fam]
    x = _x(fam)
    X = SI.inputs(20, 1, D)[0]
    g = _gp(fam)
    # M > N: every row at most, and the same picks as M = N
    idx, U, pv, tr = g.SelectInducing(x, 48, X=X, tol=0.0)
    assert len(idx) <= 20 and len(set(idx.tolist())) == len(idx)
    _same((idx, U, pv, tr), g.SelectInducing(x, 20, X=X, tol=0.0))
    # N == 0
    idx0, U0, pv0, tr0 = g.SelectInducing(x, 5, X=np.zeros((0, D)))
    assert len(idx0) == 0 and U0.shape == (0, D) and tr0 == 0.0
    # pivots, U and trace may be NULL; the entries from m on are left alone
    L = _lib.lib()
    idxb, m = np.full(30, -7, dtype=np.int64), ctypes.c_int64(-1)
    Xc = np.ascontiguousarray(X)
    assert L.gogp_sparse_select_inducing(g._h, _dp(x), x.size, _dp(Xc), 20, 30, 0.0, _ip(idxb), None, None, ctypes.byref(m),
                                         None) == _lib.GOGP_OK
    assert m.value == len(idx) and np.array_equal(idxb[:m.value], idx) and np.all(idxb[m.value:] == -7)
    # refusals
    pvb, Ub, tr = np.zeros(30), np.zeros(30 * D), ctypes.c_double(0.0)

    def call(xx=x, ln=None, Xp=Xc, N=20, M=5, tol=1e-8, ip=idxb, mp=m):
        return L.gogp_sparse_select_inducing(g._h, None if xx is None else _dp(xx), x.size if ln is None else ln,
                                             None if Xp is None else _dp(Xp), N, M, tol, None if ip is None else _ip(ip),
                                             _dp(pvb), _dp(Ub), None if mp is None else ctypes.byref(mp), ctypes.byref(tr))

    assert call() == _lib.GOGP_OK
    bad_x, bad_X = x.copy(), Xc.copy()
    bad_x[0], bad_X[3, 1] = np.nan, np.inf
    for kw in (dict(xx=None), dict(ln=x.size - 1), dict(xx=bad_x), dict(Xp=bad_X), dict(Xp=None), dict(N=-1), dict(M=0),
               dict(M=_lib.GOGP_SPARSE_MAX_M + 1), dict(tol=float("inf")), dict(tol=float("nan")), dict(ip=None),
               dict(mp=None)):
        assert call(**kw) == _lib.GOGP_EARG, kw
    assert call(tol=-1.0) == _lib.GOGP_OK and call(M=_lib.GOGP_SPARSE_MAX_M) == _lib.GOGP_OK
    # the resident form needs the sparse data
    res = lambda: L.gogp_sparse_select_inducing_resident(g._h, _dp(x), x.size, 5, 1e-8, _ip(idxb), _dp(pvb), _dp(Ub),  # noqa: E731
                                                         ctypes.byref(m), ctypes.byref(tr))
    assert res() == _lib.GOGP_ESTATE and b"sparse_set_data" in L.gogp_last_error(g._h)
    g.SetSparse(X, np.zeros(20), X[:3])
    assert res() == _lib.GOGP_OK
    # event discounts and fp32 handles: refused as everywhere on the sparse path
    ev = np.array([0.0, 1.0, 0.5])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == _lib.GOGP_OK
    assert call() == _lib.GOGP_EARG and b"event" in L.gogp_last_error(g._h)
    assert res() == _lib.GOGP_EARG
    assert L.gogp_set_events(g._h, None, 0, 0) == _lib.GOGP_OK
    assert call() == _lib.GOGP_OK
    g.close()
    g32 = GP(D, simil, SI.NOISE, ThetaSimil=ts, ThetaNoise=SI.TN, device=0, precision=32)
    with pytest.raises(GogpError) as e:
        g32.SelectInducing(x, 5, X=X)
    assert e.value.code == _lib.GOGP_EARG
    g32.close()


def test_set_sparse_greedy_and_reselect_end_to_end():
    """The bound at the greedily chosen points equals the reference's at U = X[idx] under the sparse tests' rule
    (rel = 300 cond(Kuu + eps I) 2.2e-16 with eps = 1e-2, asserted below 1e-8 on the reference); reselect moves the points
    to the selection at another theta, and where the selection stops short of M it raises and leaves them."""
    from gogp_amd.gp import GogpError, SparseModel
    fam, N, M = "ard_rbf3", 700, 48
    D, simil, _ = SI.FAMILIES[fam]
    X, y, _ = SI.inputs(N, 1, D)
    x = _x(fam)
    g = _gp(fam, jit=-2)

    def check(idx, xx, tag):
        F = g.SparseObserve(xx)
        Fr, _, st = SR.reference(D, simil, xx, X, y, X[idx], 1e-2, want_grad=False)
        cond = np.linalg.cond(st.Kuu + 1e-2 * np.eye(len(idx)))
        rel = 300.0 * cond * EPSM
        print("%s: bound %.12e (reference %.12e), rel err %.3e, allowed %.3e" % (tag, F, Fr, abs(F - Fr) / abs(Fr), rel))
        assert rel < 1e-8 and np.isfinite(F)
        assert abs(F - Fr) <= rel * abs(Fr)
        return F

    idx = g.SetSparseGreedy(X, y, M, x, tol=1e-8)
    assert len(idx) == M and len(set(idx.tolist())) == M
    idx_again, _, pv, _ = g.SelectInducing(x, M, X=X, tol=1e-8)
    _same((idx,), (idx_again,))
    F0 = check(idx, x, "SetSparseGreedy")
    model = SparseModel(g)
    assert model.Observe(x) == F0
    with pytest.raises(GogpError):
        model.reselect(x, tol=float(pv[10]))  # the residual at the eleventh pick is not above it: 10 points of 48
    assert g.SparseObserve(x) == F0  # the inducing points are where they were
    x2 = x + np.array([0.0, 0.4, -0.3, 0.2, 0.0])
    idx2 = model.reselect(x2)
    assert len(idx2) == M and not np.array_equal(idx2, idx)
    check(idx2, x2, "reselect")
    g.close()
