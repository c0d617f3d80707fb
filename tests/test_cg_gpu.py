"""The iterative exact GP (GP.SetCG / CGSolve / CGAlpha / CGSolveColumns / CGProduce; gogp_cg_*) on the GPU, through the C
ABI, against dense numpy linear algebra (tests/cg_ref.py: alpha* = numpy.linalg.solve, cond = numpy.linalg.cond).

Shared settings: output scale 1.5, noise variance 1e-2, v uniform in [0, 0.05], y drawn from the prior, inputs uniform in
a box.  Cases (cg_ref.CASES): Normal 1-D, Matern-3/2 1-D, Matern-5/2 2-D (N = 600), Normal 3-D (N = 1000), a periodic +
Matern sum (1-D, N = 500), an ARD Normal kernel at D = 8 (N = 600), and N = 4097 at D = 8, the last also against a dense
handle (SetNoiseVariances + Absorb).  Conditions:
  1  tol = 1e-8: no error, converged, rel_residual <= 2 tol;
  2  the reported rel_residual equals the residual recomputed in long double from the returned alpha within the
     product's bound divided by |y|;
  3  |alpha - alpha*| <= (cond rel_residual + cond n u) |alpha*|;
  4  the four tabulated cases: iterations at rank 64 at most HALF the reference's at rank 0; rank 128 on the first case
     with piv_tol = 0: rank_used < 128;
  5  the same bits from two identical calls; the same bits and counts for cg_check = 1 and the default;
  6  CGSolveColumns, T in {1, 17, 64, 65, 130}: condition 3 per column, a zero column gives zeros after 0 iterations, a
     column has the same bits alone as inside its block;
  7  CGProduce, m in {1, 64, 65, 130}: |mu_j - mu*_j| <= |k*_j| |alpha - alpha*| + the product's bound; |q_j - q*_j| <=
     |k*_j| cond rel_residual_j |s*_j| for q = k*^T K^^-1 k* (sigma compared through q); sigma=False solves nothing;
  8  max_iter = 2 on the Matern cases: ConvergenceError, outputs written, converged = False, rel_residual > tol;
  9  refusals and state; dense and sparse results keep their bits across a CG sequence, and the reverse.
Every device result is computed once per case and shared, read only."""
import ctypes

import numpy as np
import pytest

import cg_ref as C
import gram_ref as R
from gogp_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-8
KEPT = "matern52_2d"  # the case whose solved handle the column, forecast and state tests go on using
_RUN = {}


def _gp(name, **kw):
    from gogp_amd.gp import GP
    p = C.problem(name)
    return GP(p["D"], p["simil"], C.NOISE, ThetaSimil=list(p["theta"]), device=0, **kw)


def _solved(name, rank=64):
    """(gp handle, info dict, alpha) of CGSolve at tol 1e-8: one per case, shared, read only."""
    key = (name, rank)
    if key not in _RUN:
        p = C.problem(name)
        g = _gp(name)
        g.SetCG(p["X"], p["y"], p["v"])
        info = g.CGSolve(p["x"], rank=rank, tol=TOL, max_iter=1000)
        a = g.CGAlpha()
        a.setflags(write=False)
        if name != KEPT:  # one handle stays for the column and forecast tests; the others are done
            g.close()
            g = None
        _RUN[key] = (g, info, a)
    return _RUN[key]


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_handles():
    """The handles of _solved go back to the library's pool of stream sets when the module is done."""
    yield
    for g, _, _ in _RUN.values():
        if g is not None:
            g.close()
    _RUN.clear()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", list(C.CASES))
def test_solve(name):
    p = C.problem(name)
    g, info, a = _solved(name)
    rel = info["rel_residual"]
    err = float(np.linalg.norm(a - p["alpha"]))
    ld, bnd = C.true_residual_ld(p, a)
    print("%s: cond %.3g, rank %d, %d iterations, %d products, rel_residual %.3g (recurrence %.3g; long double %.3g +- %.3g), "
          "|alpha - alpha*| / bound %.3g" % (name, p["cond"], info["rank_used"], info["iterations"], info["products"], rel,
                                             info["rel_residual_recurrence"], ld, bnd, err / C.alpha_bound(p, rel)))
    assert info["converged"] and rel <= 2 * TOL and 0 < info["rank_used"] <= 64 and info["blocks"] == 1  # 1
    # products LAUNCHED: the iterations up to the next look at the status word (cg_check = 8) and the true residual's one
    assert info["iterations"] + 1 <= info["products"] <= info["iterations"] + 8
    assert abs(rel - ld) <= bnd                                                                           # 2
    assert err <= C.alpha_bound(p, rel)                                                                   # 3
    assert abs(info["yt_alpha"] - float(p["y"] @ a)) <= 1e-12 * float(np.abs(p["y"]) @ np.abs(a))
    if name in C.TABULATED:                                                                               # 4
        ref0, _ = C.reference_solve(name, 0, TOL)
        assert 2 * info["iterations"] <= ref0["iterations"][0]


def test_against_the_dense_handle():
    """N = 4097: alpha of the dense factorisation on the same data (SetNoiseVariances + Absorb) -- both within their own
    bound of alpha*, so within the sum of the two of each other."""
    name = "normal_8d_4097"
    p = C.problem(name)
    _, info, a = _solved(name)
    d = _gp(name)
    d.Absorb(p["X"], p["y"], v=p["v"])
    ad = np.array(d.Alpha)
    d.close()
    dense_own = p["cond"] * p["N"] * C.U * float(np.linalg.norm(p["alpha"]))
    assert np.linalg.norm(ad - p["alpha"]) <= dense_own
    assert np.linalg.norm(a - ad) <= C.alpha_bound(p, info["rel_residual"]) + dense_own


def test_rank_stops_early():
    name = C.TABULATED[0]
    p = C.problem(name)
    g = _gp(name)
    g.SetCG(p["X"], p["y"], p["v"])
    info = g.CGSolve(p["x"], rank=128, tol=TOL, piv_tol=0.0)
    assert 0 < info["rank_used"] < 128 and info["converged"]
    j = g.CGSolve(p["x"], rank=0, tol=TOL)  # plain Jacobi
    assert j["rank_used"] == 0 and j["converged"] and j["iterations"] > 2 * info["iterations"]
    assert np.linalg.norm(g.CGAlpha() - p["alpha"]) <= C.alpha_bound(p, j["rel_residual"])
    g.close()


@pytest.mark.parametrize("name", ["matern32_1d", "ard_8d"])
def test_same_bits(name):
    p = C.problem(name)
    _, info, a = _solved(name)
    g = _gp(name)
    g.SetCG(p["X"], p["y"], p["v"])
    for check in (8, 1, 3):                                                                               # 5
        g.set_option("cg_check", check)
        i2 = g.CGSolve(p["x"], rank=64, tol=TOL, max_iter=1000)
        assert np.array_equal(bits(g.CGAlpha()), bits(a)), check
        assert i2["iterations"] == info["iterations"] and i2["converged"]
        assert i2["rel_residual"] == info["rel_residual"] and i2["yt_alpha"] == info["yt_alpha"]
        assert i2["rel_residual_recurrence"] == info["rel_residual_recurrence"]
    g.close()


COLS_CASE = KEPT


def _rhs(T):
    p = C.problem(COLS_CASE)
    rng = np.random.default_rng([96, T])
    B = rng.standard_normal((T, p["N"])) * 10.0 ** rng.integers(-3, 3, T)[:, None]
    if T > 1:
        B[T // 2] = 0.0
    return B


@pytest.mark.parametrize("T", [1, 17, 64, 65, 130])
def test_solve_columns(T):
    p = C.problem(COLS_CASE)
    g, _, _ = _solved(COLS_CASE)
    B = _rhs(T)
    S, cols = g.CGSolveColumns(B, tol=TOL, max_iter=1000)
    info = dict(g.cg_info)
    want = np.linalg.solve(p["Kh"], B.T).T
    assert cols["converged"].all() and info["blocks"] == -(-T // 64)
    for t in range(T):                                                                                    # 6
        if not B[t].any():
            assert cols["iterations"][t] == 0 and not S[t].any() and cols["rel_residual"][t] == 0
            continue
        bound = (p["cond"] * cols["rel_residual"][t] + p["cond"] * p["N"] * C.U) * np.linalg.norm(want[t])
        assert cols["rel_residual"][t] <= 2 * TOL and np.linalg.norm(S[t] - want[t]) <= bound, t
    assert len(set(cols["iterations"].tolist())) > 1 or T == 1
    for t in sorted({0, T // 2, T - 1, min(T - 1, 69)}):  # alone: the same bits and the same count
        s1, c1 = g.CGSolveColumns(B[t:t + 1], tol=TOL, max_iter=1000)
        assert np.array_equal(bits(s1[0]), bits(S[t])), t
        assert c1["iterations"][0] == cols["iterations"][t] and c1["rel_residual"][0] == cols["rel_residual"][t]
    S0, c0 = g.CGSolveColumns(np.zeros((0, p["N"])), tol=TOL)
    assert S0.shape == (0, p["N"])


@pytest.mark.parametrize("m", [1, 64, 65, 130])
def test_produce(m):
    name = KEPT
    p = C.problem(name)
    g, info, a = _solved(name)
    rng = np.random.default_rng([97, m])
    Z = rng.uniform(0.0, 4.0, (m, p["D"]))
    mu, sg = g.CGProduce(Z, tol=TOL)
    cols, pinfo = g.cg_cols, dict(g.cg_info)
    Ks = R._f64(R.pair_values(p["kp"], Z, p["X"], "f64")[0])  # m x N
    Sstar = np.linalg.solve(p["Kh"], Ks.T).T
    mu_ld, mu_bnd = C.kmm(p["kp"], Z, p["X"], np.asarray(a)[None, :])          # the product at the device's own alpha
    mustar, _ = C.kmm(p["kp"], Z, p["X"], np.asarray(p["alpha"])[None, :])     # mu* = k*^T alpha* in long double
    kn = np.linalg.norm(Ks, axis=1)
    da = float(np.linalg.norm(a - p["alpha"]))
    assert (np.abs(mu.astype(np.longdouble) - mustar[0]).astype(float) <= kn * da + mu_bnd[0]).all()                  # 7
    assert (np.abs(mu.astype(np.longdouble) - mu_ld[0]).astype(float) <= mu_bnd[0]).all()
    prior = R.prior_values(p["kp"])
    q, qstar = prior - sg * sg, np.einsum("ij,ij->i", Ks, Sstar)
    assert cols["converged"].all() and np.isfinite(sg).all()
    qb = kn * p["cond"] * cols["rel_residual"] * np.linalg.norm(Sstar, axis=1)
    print("m %d: worst |q - q*| / bound %.3g, products %d, blocks %d" % (m, (np.abs(q - qstar) / qb).max(), pinfo["products"],
                                                                         pinfo["blocks"]))
    assert (np.abs(q - qstar) <= qb).all()
    assert pinfo["blocks"] == -(-m // 64)
    mu2, none = g.CGProduce(Z, sigma=False)
    assert none is None and np.array_equal(bits(mu2), bits(mu))
    assert g.cg_info["blocks"] == 0 and g.cg_info["products"] == -(-m // 64)  # the mean's products alone: no solve


@pytest.mark.parametrize("name", C.MATERN)
def test_max_iter(name):
    from gogp_amd.gp import ConvergenceError
    p = C.problem(name)
    g = _gp(name)
    g.SetCG(p["X"], p["y"], p["v"])
    with pytest.raises(ConvergenceError) as e:                                                            # 8
        g.CGSolve(p["x"], rank=64, tol=TOL, max_iter=2)
    r = e.value.result
    assert e.value.code == _lib.GOGP_ENOCONV and not r["converged"] and r["iterations"] == 2 and r["rel_residual"] > TOL
    assert r["products"] == 3 and np.isfinite(r["yt_alpha"])
    a = g.CGAlpha()
    assert np.isfinite(a).all() and a.any()
    with pytest.raises(ConvergenceError) as e:
        g.CGSolveColumns(np.stack([p["y"], np.zeros(p["N"])]), tol=TOL, max_iter=2)
    S, cols = e.value.result
    assert list(cols["converged"]) == [False, True] and np.array_equal(bits(S[0]), bits(a)) and not S[1].any()
    with pytest.raises(ConvergenceError) as e:
        g.CGProduce(p["X"][:3], tol=TOL, max_iter=2)
    mu, sg = e.value.result
    assert np.isfinite(mu).all() and np.isfinite(sg).all() and not g.cg_cols["converged"].any()
    g.close()


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_refusals_and_state():
    from gogp_amd.gp import GogpError
    name = "matern32_1d"
    p = C.problem(name)
    L = _lib.lib()
    X, y, v, x, N = p["X"].copy(), p["y"].copy(), p["v"].copy(), p["x"].copy(), p["N"]
    g = _gp(name)
    info, col = _lib.CCgInfo(), (_lib.CCgCol * 4)()
    out, Z = np.zeros(4 * N), np.zeros((3, p["D"]))

    def solve(h, xx=x, ln=None, rank=8, piv=-1.0, tol=TOL, it=500, inf=info):
        return L.gogp_cg_solve(h, _dp(xx), x.size if ln is None else ln, rank, piv, tol, it, ctypes.byref(inf) if inf else None, col)

    def later(h):
        return (L.gogp_cg_get_alpha(h, _dp(out), N), L.gogp_cg_solve_columns(h, _dp(y), 1, TOL, 500, _dp(out), col),
                L.gogp_cg_produce(h, _dp(Z), 3, _dp(out), _dp(out[3:]), TOL, 500, col))

    ES, EA, OK = _lib.GOGP_ESTATE, _lib.GOGP_EARG, _lib.GOGP_OK
    assert solve(g._h) == ES and later(g._h) == (ES,) * 3                      # before SetCG
    for args in ((None, _dp(y), None, N), (_dp(X), None, None, N), (_dp(X), _dp(y), None, 0), (_dp(X), _dp(y), None, -1)):
        assert L.gogp_cg_set_data(g._h, *args) == EA
    for i in range(3):  # a non-finite value in X, y, v
        b = [X.copy(), y.copy(), v.copy()]
        b[i].reshape(-1)[5] = np.nan
        assert L.gogp_cg_set_data(g._h, _dp(b[0]), _dp(b[1]), _dp(b[2]), N) == EA
    vb = v.copy()
    vb[7] = -1e-300
    assert L.gogp_cg_set_data(g._h, _dp(X), _dp(y), _dp(vb), N) == EA
    assert solve(g._h) == ES                                                    # a refused set_data sets nothing
    g.SetCG(X, y, v)
    assert later(g._h) == (ES,) * 3                                             # before a solve
    xb = x.copy()
    xb[0] = np.inf
    for kw in (dict(xx=None), dict(ln=x.size + 1), dict(xx=xb), dict(rank=-1), dict(rank=1025), dict(tol=0.0),
               dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(it=0), dict(piv=float("nan")),
               dict(inf=None)):
        assert solve(g._h, **kw) == EA, kw
    assert later(g._h) == (ES,) * 3
    assert solve(g._h) == OK and info.rank_used == 8
    assert later(g._h) == (OK,) * 3
    Bb = y.copy()
    Bb[3] = np.nan
    assert L.gogp_cg_solve_columns(g._h, _dp(Bb), 1, TOL, 50, _dp(out), col) == EA
    assert L.gogp_cg_solve_columns(g._h, None, 1, TOL, 50, _dp(out), col) == EA
    assert L.gogp_cg_solve_columns(g._h, _dp(y), -1, TOL, 50, _dp(out), col) == EA
    assert L.gogp_cg_solve_columns(g._h, _dp(y), 1, 0.0, 50, _dp(out), col) == EA
    assert L.gogp_cg_solve_columns(g._h, _dp(y), 1, TOL, 0, _dp(out), col) == EA
    assert L.gogp_cg_solve_columns(g._h, None, 0, TOL, 50, None, None) == OK
    Zb = Z.copy()
    Zb[1, 0] = np.inf
    assert L.gogp_cg_produce(g._h, _dp(Zb), 3, _dp(out), None, TOL, 50, None) == EA
    assert L.gogp_cg_produce(g._h, _dp(Z), 3, None, None, TOL, 50, None) == EA
    assert L.gogp_cg_produce(g._h, _dp(Z), 3, _dp(out), _dp(out[3:]), -1.0, 50, None) == EA
    assert L.gogp_cg_produce(g._h, _dp(Z), 3, _dp(out), None, -1.0, 0, None) == OK  # no solve: tol and max_iter are not used
    assert L.gogp_cg_produce(g._h, None, 0, None, None, TOL, 50, None) == OK
    assert L.gogp_cg_get_alpha(g._h, _dp(out), N - 1) == EA and L.gogp_cg_get_alpha(g._h, None, N) == EA
    for val in (0, 1025):
        assert L.gogp_set_option(g._h, b"cg_check", val) == EA
    # event discounts and fp32 handles: refused, by name (sharded ones: test_sharded_handles_are_refused)
    ev = np.array([0.0, 1.0, 0.5])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == OK
    assert solve(g._h) == EA and later(g._h) == (EA,) * 3 and L.gogp_cg_set_data(g._h, _dp(X), _dp(y), None, N) == EA
    assert b"event" in L.gogp_last_error(g._h)
    assert L.gogp_set_events(g._h, None, 0, 0) == OK
    assert later(g._h) == (OK,) * 3
    g.SetCG(None, None)
    assert solve(g._h) == ES and later(g._h) == (ES,) * 3
    g.close()
    g32 = _gp(name, precision=32)
    assert L.gogp_cg_set_data(g32._h, _dp(X), _dp(y), None, N) == EA and solve(g32._h) == EA
    with pytest.raises(GogpError) as e:
        g32.SetCG(X, y)
    assert e.value.code == EA and "precision = 32" in str(e.value)
    g32.close()
    # D = diag(noise_var + v_i) must be positive: no noise and a zero among the variances is refused, all positive is not
    from gogp_amd import kernel
    from gogp_amd.gp import GP
    g0 = GP(p["D"], p["simil"], kernel.ConstantNoise(0.0), ThetaSimil=list(p["theta"]), device=0)
    v0 = v + 0.01
    v0[11] = 0.0
    g0.SetCG(X, y, v0)
    assert solve(g0._h) == EA and b"positive" in L.gogp_last_error(g0._h)
    g0.SetCG(X, y)
    assert solve(g0._h) == EA
    g0.SetCG(X, y, v + 0.01)
    assert solve(g0._h) == OK
    g0.close()
    # the Python layer
    g = _gp(name)
    with pytest.raises(ValueError):
        g.SetCG(X, y[:-1])
    with pytest.raises(ValueError):
        g.SetCG(X, y, v[:-1])
    with pytest.raises(GogpError) as e:
        g.CGAlpha()
    assert e.value.code == ES
    g.close()


def test_sharded_handles_are_refused():
    import loopback
    from gogp_amd.sharded import ShardedGP
    name = "matern32_1d"
    p = C.problem(name)
    X, y, x, N = p["X"].copy(), p["y"].copy(), p["x"].copy(), p["N"]

    def rank_fn(r, lb):
        sh = ShardedGP(p["D"], p["simil"], C.NOISE, device=0, grid=(1, 2), rank=r, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        L = _lib.lib()
        info, col = _lib.CCgInfo(), (_lib.CCgCol * 4)()
        out, Z = np.zeros(N + 8), np.zeros((3, p["D"]))
        rcs, msgs = [], []
        for call in (lambda: L.gogp_cg_set_data(sh._h, _dp(X), _dp(y), None, N),
                     lambda: L.gogp_cg_solve(sh._h, _dp(x), x.size, 8, -1.0, TOL, 50, ctypes.byref(info), col),
                     lambda: L.gogp_cg_get_alpha(sh._h, _dp(out), N),
                     lambda: L.gogp_cg_solve_columns(sh._h, _dp(y), 1, TOL, 50, _dp(out), col),
                     lambda: L.gogp_cg_produce(sh._h, _dp(Z), 3, _dp(out), _dp(out[3:]), TOL, 50, col)):
            rcs.append(call())
            msgs.append(L.gogp_last_error(sh._h))
        sh.close()
        return rcs, msgs

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rcs, msgs in outs:
        assert rcs == [_lib.GOGP_EARG] * 5 and all(b"sharded" in m for m in msgs), (rcs, msgs)


def test_other_state_keeps_its_bits():
    """A dense Observe + Gradient and a SparseObserve return the same bits before and after a CG sequence, and a CG
    sequence the same bits before and after them."""
    name = KEPT
    p = C.problem(name)
    _, info, a = _solved(name)
    g = _gp(name)
    n0 = 300
    g.X, g.Y = p["X"][:n0], p["y"][:n0]
    g.SetSparse(p["X"], p["y"], p["X"][:40])

    def dense_sparse():
        lml = g.Observe(p["x"])
        return lml, g.Gradient().copy(), g.SparseObserve(p["x"]), g.SparseGradient().copy()

    def same(u, w):
        return all(np.array_equal(bits(np.atleast_1d(np.asarray(q, float))), bits(np.atleast_1d(np.asarray(r, float))))
                   for q, r in zip(u, w))

    before = dense_sparse()
    g.SetCG(p["X"], p["y"], p["v"])
    i1 = g.CGSolve(p["x"], rank=64, tol=TOL)
    a1 = g.CGAlpha()
    mu1, sg1 = g.CGProduce(p["X"][:5] + 0.01)
    assert np.array_equal(bits(a1), bits(a)) and i1["iterations"] == info["iterations"]
    after = dense_sparse()
    assert same(before, after)
    mu2, sg2 = g.CGProduce(p["X"][:5] + 0.01)  # the CG state survived the dense and sparse calls
    assert np.array_equal(bits(g.CGAlpha()), bits(a)) and same((mu1, sg1), (mu2, sg2))
    mu_d, sg_d = g.Produce(p["X"][:5] + 0.01)   # ... and the dense forecast is still the dense data's
    assert same(dense_sparse(), before) and np.isfinite(mu_d).all() and np.isfinite(sg_d).all()
    g.close()
