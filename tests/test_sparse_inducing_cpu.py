"""Learning the inducing points without a GPU: the numpy reference of tests/sparse_inducing_ref.py (what
gogp_sparse_gradient_inducing returns in dU) against central differences of the bound and against its own chunked form,
its behaviour on coincident points; the binding of the two new symbols and the hooks, and the refusals that need no
device.

Central differences: N = 150, M = 12, eps = 1e-2, h = 1e-5, U a random subset of X displaced by 0.05 * normal, on the
bound of sparse_ref.reference_chunked.  Every component within 1e-5 of the largest: the disagreement measured when the
formula was derived was at most 1.9e-7 of the largest component (`hyperpriors`; 2e-10 .. 9e-8 for the others), and the
margin of 50 covers the differences' own error (truncation h^2 and rounding eps_machine |F| / h), not the formula's."""
import ctypes
import os
import re

import numpy as np
import pytest

import sparse_inducing_ref as IR
import sparse_ref as SR
from gogp_amd import _lib

EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)
N, M, EPS, H = 150, 12, 1e-2, 1e-5


def _x(fam):
    return np.log(np.array(list(SR.FAMILIES[fam][2]) + SR.TN))


def _case(fam, n=N, m=M):
    D, simil, _ = SR.FAMILIES[fam]
    X, y, _ = SR.inputs(n, 1, D)
    return D, simil, _x(fam), X, y, IR.displaced_subset(X, m)


@pytest.mark.parametrize("fam", sorted(SR.FAMILIES))
def test_reference_against_central_differences(fam):
    D, simil, x, X, y, U = _case(fam)
    dU = IR.du_reference(D, simil, x, X, y, U, EPS)[2]
    assert dU.shape == (M, D)

    def F(V):
        return SR.reference_chunked(D, simil, x, X, y, V, EPS, 64, want_grad=False)[0]

    num = np.zeros_like(dU)
    for a in range(M):
        for d in range(D):
            e = np.zeros_like(U)
            e[a, d] = H
            num[a, d] = (F(U + e) - F(U - e)) / (2 * H)
    scale = np.abs(dU).max()
    err = np.abs(dU - num).max()
    print("%s: dU against central differences: max |err| = %.3e of largest component %.3e (%.2e relative)"
          % (fam, err, scale, err / scale))
    assert scale > 0.0
    assert err <= 1e-5 * scale, (fam, err, scale)


@pytest.mark.parametrize("fam", sorted(SR.FAMILIES))
def test_chunked_reference_equals_the_chunk_free_one(fam):
    D, simil, x, X, y, U = _case(fam)
    F, g, dU, _ = IR.du_reference(D, simil, x, X, y, U, EPS)
    for chunk in (1, 37, 64, 200):
        Fc, gc, dUc, _ = IR.du_reference_chunked(D, simil, x, X, y, U, EPS, chunk)
        d = np.abs(dUc - dU).max() / np.abs(dU).max()
        print("%s chunk %d: max |ddU| = %.3e of the largest" % (fam, chunk, d))
        assert d <= 1e-12, (fam, chunk, d)


@pytest.mark.parametrize("fam", ["matern32_2d", "hyperpriors", "ard_rbf3"])
def test_coincident_points_give_finite_rows(fam):
    D, simil, x, X, y, U = _case(fam)
    U2 = np.vstack([U, U[:3]])  # three duplicated inducing points
    dU = IR.du_reference(D, simil, x, X, y, U2, EPS)[2]
    assert dU.shape == (M + 3, D) and np.isfinite(dU).all()
    Xs = X[:40]
    dUx = IR.du_reference(D, simil, x, Xs, y[:40], Xs, EPS)[2]  # U = X, M = N
    assert dUx.shape == (40, D) and np.isfinite(dUx).all()


def test_symbols_bound_and_declared():
    """Fails on the parent commit: gogp_sparse_set_inducing, gogp_sparse_gradient_inducing and the hooks are in the
    binding's tables with the headers' argument counts, the headers declare them and the libraries export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_sparse_set_inducing": 3, "gogp_sparse_gradient_inducing": 4}
    want_hooks = {"gogp_test_sparse_ugrad": 19, "gogp_test_sparse_ugrad_slabs": 3, "gogp_test_sparse_ugrad_slabs_bound": 2}
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


# ---- the hook refuses bad shapes before it touches a device ----------------------------------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _ugrad(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    D = 2
    rows, M_, ldw = g("rows", 130), g("M", 70), g("ldw", 72)
    kp = gp.kparams(D, [dict(kind=g("kind", 0), c=1.5, inv_len=0.7)], events=g("events", ()))
    X = np.zeros(max(g("x_len", 130 * D), 1))
    U = np.zeros(max(g("u_len", 70 * D), 1))
    Wt = np.zeros(max(g("wt_len", 129 * 72 + 70), 1))
    y = np.zeros(max(g("y_len", 130), 1))
    mv = np.zeros(max(g("m_len", 70), 1))
    dU = np.zeros(max(g("du_len", 70 * D), 1))
    dp = gp._dp
    nul = lambda k, p: None if g(k, False) else p  # noqa: E731
    return _lib.hooks().gogp_test_sparse_ugrad(-1, nul("kp_null", kp), nul("x_null", dp(X)), X.size, rows,
                                               nul("u_null", dp(U)), U.size, M_, nul("wt_null", dp(Wt)), Wt.size, ldw,
                                               nul("y_null", dp(y)), y.size, nul("m_null", dp(mv)), mv.size, g("s4", 1.0), 0,
                                               nul("du_null", dp(dU)), dU.size)


UGRAD_REFUSED = [dict(rows=0), dict(rows=(1 << 16) + 1), dict(M=0), dict(M=4097), dict(ldw=69), dict(x_len=259),
                 dict(u_len=139), dict(wt_len=129 * 72 + 69), dict(y_len=129), dict(m_len=69), dict(du_len=139),
                 dict(s4=float("nan")), dict(kind=7), dict(events=((0.0, 1.0, 0.5),)), dict(kp_null=True), dict(x_null=True),
                 dict(u_null=True), dict(wt_null=True), dict(y_null=True), dict(m_null=True), dict(du_null=True)]


@pytest.mark.parametrize("bad", UGRAD_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in UGRAD_REFUSED])
def test_ugrad_hook_refuses(gpm, bad):
    assert _ugrad(gpm, **bad) == EARG


def test_ugrad_hook_accepts_the_valid_neighbours(gpm):
    # (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for ok in [{}, dict(rows=1, x_len=2, y_len=1, wt_len=70), dict(M=1, u_len=2, m_len=1, du_len=2),
               dict(ldw=70, wt_len=130 * 70), dict(du_len=141)]:
        assert _ugrad(gpm, **ok) in OKS, ok


def test_slab_rule_is_a_function_of_the_shape(gpm):
    """Slabs of whole 64-row tiles that cover every row, at most 2048 workgroups, no device."""
    tps = ctypes.c_int(0)
    f = _lib.hooks().gogp_test_sparse_ugrad_slabs
    for rows, M_ in [(1, 1), (64, 64), (130, 70), (1100, 70), (8192, 48), (8192, 4096), (65536, 4096), (65536, 1)]:
        ns = f(rows, M_, ctypes.byref(tps))
        ntr = (rows + 63) // 64
        assert ns >= 1 and tps.value >= 1
        assert (ns - 1) * tps.value < ntr <= ns * tps.value, (rows, M_, ns, tps.value)
        assert ns * ((M_ + 63) // 64) <= 2048
    for rows, M_ in [(0, 1), (1, 0), (65537, 1), (1, 4097)]:
        assert f(rows, M_, ctypes.byref(tps)) == 0


@pytest.mark.parametrize("M_", [1, 512, 2048, 3000, 4096])
def test_slab_bound_covers_every_shorter_chunk(gpm, M_):
    """gogp_sparse_gradient_inducing sizes one buffer of partials for all its chunks, the ragged last one included, and
    the slab count is not monotone in the rows: the bound at `chunk` covers the count at every r <= chunk, for every
    "sparse_chunk" the option accepts.  (The count depends on r through ceil(r / 64) alone.)"""
    f, fb = _lib.hooks().gogp_test_sparse_ugrad_slabs, _lib.hooks().gogp_test_sparse_ugrad_slabs_bound
    tps = ctypes.c_int(0)
    worst = np.maximum.accumulate([f(64 * k, M_, ctypes.byref(tps)) for k in range(1, 1025)])  # max over r <= 64 k
    for chunk in range(256, 65536 + 1, 256):
        b = fb(chunk, M_)
        assert b >= worst[chunk // 64 - 1], (M_, chunk, b, worst[chunk // 64 - 1])
        assert b * ((M_ + 63) // 64) <= 2048 or b == 1
    assert fb(0, M_) == 0 and fb(65537, M_) == 0 and fb(256, 0) == 0 and fb(256, 4097) == 0


def test_slab_count_is_not_monotone_where_the_bound_matters(gpm):
    """M = 2048, "sparse_chunk" = 16640, N = 33024: the 16384-row tail takes 64 slabs, the full chunk 52."""
    f, fb = _lib.hooks().gogp_test_sparse_ugrad_slabs, _lib.hooks().gogp_test_sparse_ugrad_slabs_bound
    tps = ctypes.c_int(0)
    assert f(16640, 2048, ctypes.byref(tps)) == 52 and f(16384, 2048, ctypes.byref(tps)) == 64
    assert fb(16640, 2048) >= 64
    assert f(8448, 4096, ctypes.byref(tps)) == 27 and f(8192, 4096, ctypes.byref(tps)) == 32
    assert fb(8448, 4096) >= 32


def test_c_abi_refusals_that_need_no_device():
    """NULL handles are refused before anything is touched."""
    _lib.build()
    L = _lib.lib()
    one = np.zeros(1)
    dp = one.ctypes.data_as(_lib._dp)
    assert L.gogp_sparse_set_inducing(None, dp, 1) == EARG
    assert L.gogp_sparse_gradient_inducing(None, dp, 1, dp) == EARG
