"""Greedy selection of inducing points (gogp_sparse_select_inducing), the part that needs no GPU: the numpy reference
of tests/select_inducing_ref.py pinned to dense linear algebra, the binding tables, and the argument refusals of the C
calls and of the two hooks, which validate before they touch a device.

The reference, on FOUR x (N, M) in {(63, 63), (257, 37), (700, 130)} at tol = 1e-8:
  (L L^T)[piv] == K[piv] and trace == tr K - |L|_F^2 to 1e-12 of max k(x, x);
  L[piv] against np.linalg.cholesky(K[piv][:, piv]) within 300 * cond * 2.2e-16 of its largest element, the sparse tests'
  rule (a dense fp64 factorisation carries about cond * eps relative over a few hundred operations);
  pv non-increasing (up to 1e-12 of max k(x, x): rounding), no index twice, and duplicated rows of X never both chosen.

Reference counterpart: none."""
import ctypes
import os
import re

import numpy as np
import pytest

import grad_reduce_ref as GR
import select_inducing_ref as SI
from gogp_amd import _lib, kernel

EARG, EHIP, OK = _lib.GOGP_EARG, _lib.GOGP_EHIP, _lib.GOGP_OK
OKS = (OK, EHIP)  # no GPU here: GOGP_EHIP, on a GPU: GOGP_OK
CASES = [(63, 63), (257, 37), (700, 130)]
TOL = 1e-8


def _case(name, N):
    D, simil, ts = SI.FAMILIES[name]
    X = SI.inputs(N, 1, D)[0]
    return D, X, SI.dense(D, simil, ts, X)


@pytest.mark.parametrize("N,M", CASES)
@pytest.mark.parametrize("name", SI.FOUR)
def test_reference_is_a_pivoted_cholesky(name, N, M):
    D, X, K = _case(name, N)
    piv, pv, L, d, trace = SI.greedy(K, M, TOL)
    m = len(piv)
    kmax = np.diag(K).max()
    assert 1 <= m <= min(M, N) and L.shape == (N, m)
    assert piv[0] == 0  # every k(x, x) is the same: the lowest index wins
    assert len(set(piv.tolist())) == m
    assert np.all(np.diff(pv) <= 1e-12 * kmax), np.diff(pv).max()
    assert m == M or d.max() <= TOL
    assert np.abs((L @ L.T)[piv] - K[piv]).max() <= 1e-12 * kmax
    assert abs(trace - (np.trace(K) - (L * L).sum())) <= 1e-12 * kmax
    assert np.all(d[piv] == 0.0)
    Lp = L[piv]
    assert np.all(np.triu(Lp, 1) == 0.0)
    np.testing.assert_array_equal(np.diag(Lp), np.sqrt(pv))
    Kuu = K[np.ix_(piv, piv)]
    C = np.linalg.cholesky(Kuu)
    rel = 300 * np.linalg.cond(Kuu) * SI.EPS
    print("%s N %d M %d: m %d, cond %.3g, |L[piv] - chol| %.3g (allowed %.3g)"
          % (name, N, M, m, np.linalg.cond(Kuu), np.abs(Lp - C).max(), rel * np.abs(C).max()))
    assert np.abs(Lp - C).max() <= rel * np.abs(C).max()
    # replay of the reference's own sequence returns its residuals, in both precisions' code path
    R64, L64 = SI.replay(K, piv, np.float64)
    np.testing.assert_array_equal(R64[-1], d)
    np.testing.assert_array_equal(L64, L)
    np.testing.assert_array_equal(R64[np.arange(m), piv], pv)
    Rld, _ = SI.replay(K, piv, SI.LD)
    assert np.abs(Rld[-1].astype(float) - d).max() <= 1e-12 * kmax
    # ... and the lazily evaluated columns are the dense matrix's
    Dn, simil, ts = SI.FAMILIES[name]
    cols = SI.Columns(Dn, simil, ts, X)
    np.testing.assert_array_equal(cols.col(int(piv[-1])), K[:, piv[-1]])
    np.testing.assert_array_equal(cols.diag(), np.diag(K))


@pytest.mark.parametrize("name", SI.FOUR)
def test_reference_never_picks_a_duplicated_row_twice(name):
    D, simil, ts = SI.FAMILIES[name]
    X = SI.inputs(120, 1, D)[0]
    dup = np.array([3, 3, 17, 40, 40, 40, 119])
    Xd = np.vstack([X, X[dup]])  # rows 120 .. 126 repeat rows of X
    twin = {120 + k: int(s) for k, s in enumerate(dup)}
    piv = SI.greedy(SI.dense(D, simil, ts, Xd), 127, TOL)[0]
    seen = set()
    for p in piv.tolist():
        src = twin.get(p, p)
        assert src not in seen, (p, src)
        seen.add(src)


def test_symbols_bound_and_declared():
    """Fails on the parent commit: the two gogp_sparse_select_inducing* symbols and the two hooks are in the binding's
    tables with the headers' argument counts, the headers declare them and the libraries export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_sparse_select_inducing": 12, "gogp_sparse_select_inducing_resident": 10}
    want_hooks = {"gogp_test_select_step": 23, "gogp_test_select_run": 20}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def header(name):
        with open(os.path.join(root, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    h, hh = header("gogp_hip.h"), header("gogp_testhooks.h")
    for tab, text, names in ((table, h, want), (hooks, hh, want_hooks)):
        for name, nargs in names.items():
            assert name in tab and len(tab[name][1]) == nargs, name
            m = re.search(r"int %s\(([^)]*)\);" % name, text)
            assert m and len(m.group(1).split(",")) == nargs, name
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    for name in want:
        assert getattr(lib, name) is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None
    from gogp_amd import gp
    for name in ("SelectInducing", "SetSparseGreedy"):
        assert callable(getattr(gp.GP, name))
    assert callable(gp.SparseModel.reselect) and callable(gp.select_step_check) and callable(gp.select_run_check)
    # the C++ and Go mirrors call both forms
    src = open(os.path.join(root, "gogp_amd", "host", "gogp.hpp")).read()
    go = open(os.path.join(root, "go", "gogp", "gp.go")).read()
    for name in want:
        assert name + "(" in src and "C." + name + "(" in go, name
    assert "double SelectInducing(" in src and "double SelectInducingResident(" in src
    assert "func (gp *GP) SelectInducing(logtheta, x []float64, m int, tol float64)" in go


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def test_c_abi_refusals_that_need_no_device():
    """A NULL handle is refused by both calls before anything is touched."""
    _lib.build()
    L = _lib.lib()
    one = np.zeros(1)
    dp = one.ctypes.data_as(_lib._dp)
    idx = np.zeros(1, dtype=np.int64)
    ip = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    m, tr = ctypes.c_int64(0), ctypes.c_double(0.0)
    assert L.gogp_sparse_select_inducing(None, dp, 1, dp, 1, 1, 1e-8, ip, dp, dp, ctypes.byref(m), ctypes.byref(tr)) == EARG
    assert L.gogp_sparse_select_inducing_resident(None, dp, 1, 1, 1e-8, ip, dp, dp, ctypes.byref(m), ctypes.byref(tr)) == EARG


# ---- the hooks refuse bad shapes before they touch a device -----------------------------------------------------------
def _step(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    D, N, ldn, j = 2, g("N", 300), g("ldn", 512), g("j", 3)
    kp = gp.kparams(D, [dict(kind=g("kind", 0), c=1.5, inv_len=0.7)], events=g("events", ()))
    X = np.zeros(max(g("x_len", 300 * D), 1))
    Lt = np.zeros(max(g("lt_len", 4 * 512), 1))
    d = np.zeros(max(g("d_len", 300), 1))
    sel = np.zeros(max(g("sel_len", 300), 1), dtype=np.uint8)
    nb = g("part_len", 2)
    pv, pi = np.zeros(max(nb, 1)), np.full(max(nb, 1), g("part_i", 0), dtype=np.int64)
    ov, oi = np.zeros(max(g("out_len", 2), 1)), np.zeros(max(g("out_len", 2), 1), dtype=np.int64)
    p, dpv = ctypes.c_int64(0), ctypes.c_double(0.0)
    dp, ip = gp._dp, gp._ip
    return _lib.hooks().gogp_test_select_step(
        -1, None if g("kp_null", False) else kp, dp(X), X.size, N, None if g("lt_null", False) else dp(Lt), Lt.size, ldn, j,
        g("tol", 1e-8), dp(d), d.size, sel.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), sel.size, dp(pv), ip(pi), nb,
        g("max_blocks", 0), dp(ov), ip(oi), g("out_len", 2), None if g("p_null", False) else ctypes.byref(p), ctypes.byref(dpv))


STEP_REFUSED = [dict(N=0), dict(N=(1 << 22) + 1), dict(ldn=256), dict(ldn=520), dict(j=-1), dict(j=4096), dict(j=4),
                dict(lt_len=4 * 512 - 1), dict(x_len=599), dict(d_len=299), dict(sel_len=299), dict(part_len=1),
                dict(part_len=3), dict(out_len=1), dict(part_i=-1), dict(part_i=300), dict(tol=-1.0),
                dict(tol=float("nan")), dict(tol=float("inf")), dict(max_blocks=-1), dict(max_blocks=1), dict(kind=7),
                dict(events=((0.0, 1.0, 0.5),)), dict(kp_null=True), dict(lt_null=True), dict(p_null=True)]


@pytest.mark.parametrize("bad", STEP_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in STEP_REFUSED])
def test_step_hook_refuses(gpm, bad):
    assert _step(gpm, **bad) == EARG


def _run(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    D, N, M = 2, g("N", 300), g("M", 40)
    kp = gp.kparams(D, [dict(kind=g("kind", 0), c=1.5, inv_len=0.7)], events=g("events", ()))
    X = np.zeros(max(g("x_len", 300 * D), 1))
    d0 = np.zeros(max(g("d0_len", 300), 1))
    cap = max(M, 1) if M <= 4096 else 1
    idx, piv = np.zeros(cap, dtype=np.int64), np.zeros(cap)
    U = np.zeros(max(g("u_len", 40 * D), 1))
    Lt = np.zeros(max(g("lt_len", 40 * 512), 1))
    d = np.zeros(max(g("d_len", 300), 1))
    m, tr = ctypes.c_int64(0), ctypes.c_double(0.0)
    dp, ip = gp._dp, gp._ip
    return _lib.hooks().gogp_test_select_run(
        -1, None if g("kp_null", False) else kp, dp(X), X.size, N, M, g("tol", 1e-8), g("max_blocks", 0),
        dp(d0) if g("with_d0", True) else None, d0.size, None if g("idx_null", False) else ip(idx), dp(piv),
        dp(U) if g("with_u", True) else None, g("u_len", 40 * D), dp(Lt) if g("with_lt", True) else None, Lt.size,
        dp(d) if g("with_d", True) else None, d.size, ctypes.byref(m), None if g("tr_null", False) else ctypes.byref(tr))


RUN_REFUSED = [dict(N=0), dict(N=(1 << 22) + 1), dict(M=0), dict(M=4097), dict(x_len=599), dict(d0_len=299),
               dict(u_len=79), dict(lt_len=40 * 512 - 1), dict(d_len=299), dict(tol=-1.0), dict(tol=float("nan")),
               dict(max_blocks=-1), dict(kind=7), dict(events=((0.0, 1.0, 0.5),)), dict(kp_null=True), dict(idx_null=True),
               dict(tr_null=True)]


@pytest.mark.parametrize("bad", RUN_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in RUN_REFUSED])
def test_run_hook_refuses(gpm, bad):
    assert _run(gpm, **bad) == EARG


def test_hooks_accept_the_valid_neighbours(gpm):
    for ok in [{}, dict(j=0, lt_len=512), dict(N=1, ldn=256, part_len=1, lt_len=4 * 256), dict(max_blocks=2),
               dict(max_blocks=1, part_len=1), dict(tol=0.0), dict(part_i=299)]:
        assert _step(gpm, **ok) in OKS, ok
    for ok in [{}, dict(with_d0=False, d0_len=0), dict(with_u=False, u_len=0), dict(with_lt=False, lt_len=0),
               dict(with_d=False, d_len=0), dict(M=4096, u_len=4096 * 2, lt_len=300 * 512), dict(M=1), dict(max_blocks=1),
               dict(tol=0.0)]:
        assert _run(gpm, **ok) in OKS, ok


def test_select_blocks_rule(gpm):
    assert [gpm.select_blocks(n) for n in (1, 256, 257, 1000, 70001, 1 << 20)] == [1, 1, 2, 4, 274, 1024]
    assert gpm.select_blocks(1000, 3) == 3 and gpm.select_blocks(1000, 9) == 4 and gpm.select_blocks(255, 1) == 1


def test_kp_of_a_family_is_accepted_by_the_hooks(gpm):
    """The families' parameter blocks (grad_reduce_ref.kp_from_desc) pass the hooks' validation, ARD in 64 dimensions
    included."""
    for name in SI.FOUR + ["ard_rbf64"]:
        D, simil, ts = SI.FAMILIES[name]
        kp = GR.kp_from_desc(kernel.build_desc(D, simil, SI.NOISE), np.asarray(ts, float), SI.TN).hook(gpm)
        X = np.zeros(5 * D)
        idx, piv = np.zeros(2, dtype=np.int64), np.zeros(2)
        m, tr = ctypes.c_int64(0), ctypes.c_double(0.0)
        rc = _lib.hooks().gogp_test_select_run(-1, kp, gpm._dp(X), X.size, 5, 2, 1e-8, 0, None, 0, gpm._ip(idx), gpm._dp(piv),
                                               None, 0, None, 0, None, 0, ctypes.byref(m), ctypes.byref(tr))
        assert rc in OKS, name
