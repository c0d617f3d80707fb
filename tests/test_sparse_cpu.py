"""The inducing-point approximation without a GPU: the numpy reference of tests/sparse_ref.py (what gogp_sparse_observe,
gogp_sparse_gradient and gogp_sparse_produce evaluate) against the oracle's LML for U = X, the inequalities of a
variational bound, central differences, its own chunked form; the binding of the four symbols and the two hooks, and
the refusals that need no device.

U = X: with Kuu + eps I for Kuu the bound is the LML of Q + s2 I, Q = K (K + eps I)^-1 K = K - eps I + O(eps^2), minus
tr(K - Q) / (2 s2).  The allowed difference is the eps-perturbation of the LML, 1/2 eps |tr(Kn^-1) - alpha^T alpha| with
Kn = K + s2 I the dense noisy matrix and alpha = Kn^-1 y, computed in the test, plus the rounding bound of
tests/test_multi_output_cpu.py (rtol = 1e-9, atol = 1e-11: dense fp64 Cholesky solves of matrices with cond <~ 1e3).

Gradient against central differences: the step and the tolerance rule of tests/test_loo_cpu.py -- |D(2 h) - D(h)| plus
four times eps_machine cond |F| / h, with cond the larger of cond(Kuu + eps I) and cond(B) of the reference."""
import os
import re

import numpy as np
import pytest

import sparse_ref as SR
from gogp_amd import _lib, kernel
from oracle.oracle import FastOracle

H = 1e-3
EPSM = np.finfo(float).eps
MAX_M = _lib.GOGP_SPARSE_MAX_M  # the feature's binding: without it this module does not import
EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)

#: name -> (NDim, Simil, theta_simil)
CASES = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8]),
    "ard_rbf3": SR.FAMILIES["ard_rbf3"],
    "hyperpriors": SR.FAMILIES["hyperpriors"],
}


def _case(name, n=60):
    D, simil, ts = CASES[name]
    X, y, Z = SR.inputs(n, 7, D)
    return D, simil, np.log(np.array(list(ts) + SR.TN)), X, y, Z


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_with_u_equal_x_is_the_oracle_lml(name):
    D, simil, x, X, y, _ = _case(name)
    eps = 1e-10
    F = SR.reference(D, simil, x, X, y, X, eps, want_grad=False)[0]
    o = FastOracle(D, simil, SR.NOISE)
    o.set_data(X, y)
    lml = o.Observe(x)
    Kn = SR.LR.gram(D, simil, x, X)
    alpha = np.linalg.solve(Kn, y)
    first = 0.5 * eps * abs(np.trace(np.linalg.inv(Kn)) - alpha @ alpha)
    bound = first + 1e-9 * abs(lml) + 1e-11
    print("%s: bound %.12e, oracle LML %.12e, |diff| = %.3e, allowed %.3e (eps term %.3e)"
          % (name, F, lml, abs(F - lml), bound, first))
    assert abs(F - lml) <= bound


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_inequalities(name):
    D, simil, x, X, y, _ = _case(name)
    o = FastOracle(D, simil, SR.NOISE)
    o.set_data(X, y)
    lml = o.Observe(x)
    prev = -np.inf
    for M in (8, 16, 32):
        F = SR.reference(D, simil, x, X, y, X[:M], 1e-10, want_grad=False)[0]
        Fd = SR.direct_bound(D, simil, x, X, y, X[:M], 1e-10)
        print("%s M = %d: bound %.9e (unwhitened form %.9e), LML %.9e" % (name, M, F, Fd, lml))
        np.testing.assert_allclose(F, Fd, rtol=1e-9, atol=1e-9)
        slack = 1e-9 * abs(lml)
        assert F <= lml + slack
        assert F >= prev - slack  # nested subsets: more inducing points never lower the bound
        prev = F


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_against_central_differences(name):
    D, simil, x, X, y, _ = _case(name)
    U, eps = X[:48], 1e-8  # (48 of 60: with fewer the bound is too rough in the period for a step of 1e-3)
    F0, grad, st = SR.reference(D, simil, x, X, y, U, eps)
    assert grad.shape == x.shape

    def F(xx):
        return SR.reference(D, simil, xx, X, y, U, eps, want_grad=False)[0]

    cond = max(np.linalg.cond(st.Kuu + eps * np.eye(len(U))), np.linalg.cond(st.B))
    for p in range(len(x)):
        e = np.zeros(len(x))
        e[p] = 1.0
        d1 = (F(x + H * e) - F(x - H * e)) / (2 * H)
        d2 = (F(x + 2 * H * e) - F(x - 2 * H * e)) / (4 * H)
        tol = abs(d2 - d1) + 4.0 * EPSM * cond * abs(F0) / H
        print("%s grad[%d] = %.9e, central difference %.9e, |diff| = %.3e, tolerance %.3e (truncation %.3e)"
              % (name, p, grad[p], d1, abs(grad[p] - d1), tol, abs(d2 - d1)))
        assert abs(grad[p] - d1) <= tol, (name, p, grad[p], d1, tol)
        assert tol < 1e-3 * max(1.0, np.abs(grad).max())  # the check has teeth


@pytest.mark.parametrize("name", sorted(CASES))
def test_chunked_reference_equals_the_chunk_free_one(name):
    D, simil, x, X, y, Z = _case(name, 130)
    # 13 inducing points and eps = 1e-6: the two differ by the order of N = 130 additions, ~130 * 1.1e-16 relative, times
    # what cond(Kuu + eps I) and cond(B) amplify; few, well separated inducing points keep that below 1e-12
    U = X[::10]
    F, g, st = SR.reference(D, simil, x, X, y, U, 1e-6)
    for chunk in (1, 37, 64, 200):
        Fc, gc, stc = SR.reference_chunked(D, simil, x, X, y, U, 1e-6, chunk)
        print("%s chunk %d: |dF| = %.3e, max |dgrad| = %.3e" % (name, chunk, abs(Fc - F), np.abs(gc - g).max()))
        assert abs(Fc - F) <= 1e-12 * abs(F)
        assert np.abs(gc - g).max() <= 1e-12 * np.abs(g).max()
        mu, sg = SR.produce(D, simil, x, st, U, Z)
        muc, sgc = SR.produce(D, simil, x, stc, U, Z)
        np.testing.assert_allclose(muc, mu, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(sgc, sg, rtol=1e-10, atol=1e-12)


def test_symbols_bound_and_declared():
    """Fails on the parent commit: the four gogp_sparse_* symbols and the two hooks are in the binding's tables with the
    headers' argument counts, include/gogp_hip.h declares them and GOGP_SPARSE_MAX_M, and the libraries export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_sparse_set_data": 6, "gogp_sparse_observe": 4, "gogp_sparse_gradient": 3, "gogp_sparse_produce": 5}
    want_hooks = {"gogp_test_sparse_syrk": 14, "gogp_test_sparse_grad": 18}
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
    assert re.search(r"#define GOGP_SPARSE_MAX_M 4096\b", h) and _lib.GOGP_SPARSE_MAX_M == 4096
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    for name in want:
        assert getattr(lib, name) is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None


# ---- the hooks refuse bad shapes before they touch a device ---------------------------------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _syrk(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    rows, M, Mp, ld, ldb = g("rows", 37), g("M", 200), g("Mp", 256), g("ld", 264), g("ldb", 256)
    Vt = np.zeros(max(g("vt_len", 36 * 264 + 256), 1))
    y = np.zeros(max(g("y_len", 37), 1))
    B = np.zeros(max(g("b_len", 256 * 256), 1))
    r = np.zeros(max(g("r_len", 256), 1))
    dp = gp._dp
    return _lib.hooks().gogp_test_sparse_syrk(-1, None if g("vt_null", False) else dp(Vt), Vt.size, ld, rows, M, Mp,
                                              None if g("y_null", False) else dp(y), y.size,
                                              None if g("b_null", False) else dp(B), B.size, ldb,
                                              None if g("r_null", False) else dp(r), r.size)


SYRK_REFUSED = [dict(rows=0), dict(rows=(1 << 16) + 1), dict(M=0), dict(M=257), dict(Mp=0), dict(Mp=200), dict(Mp=4160),
                dict(ld=255), dict(ldb=255), dict(vt_len=36 * 264 + 255), dict(b_len=256 * 256 - 1), dict(y_len=36),
                dict(r_len=255), dict(vt_null=True), dict(y_null=True), dict(b_null=True), dict(r_null=True)]


@pytest.mark.parametrize("bad", SYRK_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in SYRK_REFUSED])
def test_syrk_hook_refuses(gpm, bad):
    assert _syrk(gpm, **bad) == EARG


def _grad(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    D = 2
    rows, M, ldw = g("rows", 130), g("M", 70), g("ldw", 72)
    kp = gp.kparams(D, [dict(kind=g("kind", 0), c=1.5, inv_len=0.7)], events=g("events", ()))
    X = np.zeros(max(g("x_len", 130 * D), 1))
    U = np.zeros(max(g("u_len", 70 * D), 1))
    Wt = np.zeros(max(g("wt_len", 129 * 72 + 70), 1))
    y = np.zeros(max(g("y_len", 130), 1))
    mv = np.zeros(max(g("m_len", 70), 1))
    out = np.zeros(_lib.GOGP_TEST_NACC)
    dp = gp._dp
    return _lib.hooks().gogp_test_sparse_grad(-1, None if g("kp_null", False) else kp, dp(X), X.size, rows, dp(U), U.size, M,
                                              None if g("wt_null", False) else dp(Wt), Wt.size, ldw, dp(y), y.size, dp(mv),
                                              mv.size, g("s4", 1.0), 0, None if g("out_null", False) else dp(out))


GRAD_REFUSED = [dict(rows=0), dict(rows=(1 << 16) + 1), dict(M=0), dict(M=4097), dict(ldw=69), dict(x_len=259),
                dict(u_len=139), dict(wt_len=129 * 72 + 69), dict(y_len=129), dict(m_len=69), dict(s4=float("nan")),
                dict(kind=7), dict(events=((0.0, 1.0, 0.5),)), dict(kp_null=True), dict(wt_null=True), dict(out_null=True)]


@pytest.mark.parametrize("bad", GRAD_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in GRAD_REFUSED])
def test_grad_hook_refuses(gpm, bad):
    assert _grad(gpm, **bad) == EARG


def test_hooks_accept_the_valid_neighbours(gpm):
    # (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for ok in [{}, dict(rows=1, vt_len=256, y_len=1), dict(M=256), dict(M=1), dict(ld=256, vt_len=37 * 256)]:
        assert _syrk(gpm, **ok) in OKS, ok
    for ok in [{}, dict(rows=1, x_len=2, y_len=1, wt_len=70), dict(M=1, u_len=2, m_len=1), dict(ldw=70, wt_len=130 * 70)]:
        assert _grad(gpm, **ok) in OKS, ok


def test_c_abi_refusals_that_need_no_device():
    """NULL handles are refused by every call before anything is touched."""
    _lib.build()
    L = _lib.lib()
    one = np.zeros(1)
    dp = one.ctypes.data_as(_lib._dp)
    import ctypes
    v = ctypes.c_double(0.0)
    assert L.gogp_sparse_set_data(None, dp, dp, 1, dp, 1) == EARG
    assert L.gogp_sparse_observe(None, dp, 1, ctypes.byref(v)) == EARG
    assert L.gogp_sparse_gradient(None, dp, 1) == EARG
    assert L.gogp_sparse_produce(None, dp, 1, dp, dp) == EARG
