"""Sparse multi-output without a GPU: the matrix form of tests/sparse_multi_ref.py (what gogp_sparse_multi_* evaluate)
against the column-wise sum of the single-output reference of tests/sparse_ref.py, its Produce, the oracle's LML for
U = X and its own chunked form; the slab functions of launch_sparse_xty; the binding of the five symbols and the three
hooks, and the refusals that need no device.

Matrix form against the columns: the two evaluate the same expressions from the same factors, the matrix form with
Gamma and the sums over t inside products -- a few hundred additions of terms of one sign and size apart, at
N = 150, M = 20 and eps = 1e-6 (few, displaced inducing points: cond(Kuu + eps I) and cond(B) stay small): 1e-12 relative
for the total and the bounds, 1e-10 of the largest component for the gradient and dU."""
import ctypes
import os
import re

import numpy as np
import pytest

import sparse_inducing_ref as SI
import sparse_multi_ref as SM
import sparse_ref as SR
from gogp_amd import _lib
from oracle.oracle import FastOracle

MAX_T = _lib.GOGP_SPARSE_MULTI_MAX_T  # the feature's binding: without it this module does not import
EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)
N, M, EPS = 150, 20, 1e-6
_COLS = {}


def _x(fam):
    return np.log(np.array(list(SR.FAMILIES[fam][2]) + SR.TN))


def _case(fam, T):
    D, simil, _ = SR.FAMILIES[fam]
    X, _, Z = SR.inputs(N, 7, D)
    U = SI.displaced_subset(X, M)
    Y = SM.outputs(X, 5)[:, :T]  # (the columns of the smaller T are those of the larger: one reference per column)
    return D, simil, X, Y, Z, U


def _column(fam, t):
    """The single-output reference of column t: computed once, shared, read only."""
    if (fam, t) not in _COLS:
        D, simil, X, Y, Z, U = _case(fam, 5)
        F, grad, dU, st = SI.du_reference(D, simil, _x(fam), X, Y[:, t], U, EPS)
        _COLS[(fam, t)] = (F, grad, dU, SR.produce(D, simil, _x(fam), st, U, Z))
    return _COLS[(fam, t)]


@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("fam", SR.FOUR)
def test_matrix_form_is_the_sum_over_the_columns(fam, T):
    D, simil, X, Y, Z, U = _case(fam, T)
    total, bounds, grad, dU, st = SM.reference(D, simil, _x(fam), X, Y, U, EPS)
    cols = [_column(fam, t) for t in range(T)]
    want_b = np.array([c[0] for c in cols])
    want_total = 0.0
    for b in want_b:
        want_total += b
    want_g, want_du = sum(c[1] for c in cols), sum(c[2] for c in cols)
    print("%s T = %d: total %.12e, rel err %.3e; bounds max rel err %.3e; gradient %.3e and dU %.3e of the largest component"
          % (fam, T, total, abs(total - want_total) / abs(want_total), (np.abs(bounds - want_b) / np.abs(want_b)).max(),
             np.abs(grad - want_g).max() / np.abs(want_g).max(), np.abs(dU - want_du).max() / np.abs(want_du).max()))
    assert bounds.shape == (T,) and grad.shape == _x(fam).shape and dU.shape == U.shape
    assert abs(total - want_total) <= 1e-12 * abs(want_total)
    assert (np.abs(bounds - want_b) <= 1e-12 * np.abs(want_b)).all()
    assert np.abs(grad - want_g).max() <= 1e-10 * np.abs(want_g).max()
    assert np.abs(dU - want_du).max() <= 1e-10 * np.abs(want_du).max()
    # mu column t is the single-output Produce of column t, sigma is shared
    mu, sigma = SM.produce(D, simil, _x(fam), st, U, Z)
    assert mu.shape == (len(Z), T)
    for t in range(T):
        np.testing.assert_allclose(mu[:, t], cols[t][3][0], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(sigma, cols[t][3][1], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("fam", SR.FOUR)
def test_chunked_form_equals_the_chunk_free_one(fam):
    D, simil, X, Y, Z, U = _case(fam, 3)
    total, bounds, grad, dU, st = SM.reference(D, simil, _x(fam), X, Y, U, EPS)
    for chunk in (1, 37, 64, 200):
        tc, bc, gc, duc, stc = SM.reference_chunked(D, simil, _x(fam), X, Y, U, EPS, chunk)
        print("%s chunk %d: |d total| = %.3e, max |d grad| = %.3e, max |d dU| = %.3e"
              % (fam, chunk, abs(tc - total), np.abs(gc - grad).max(), np.abs(duc - dU).max()))
        assert abs(tc - total) <= 1e-12 * abs(total)
        assert (np.abs(bc - bounds) <= 1e-12 * np.abs(bounds)).all()
        assert np.abs(gc - grad).max() <= 1e-10 * np.abs(grad).max()
        assert np.abs(duc - dU).max() <= 1e-10 * np.abs(dU).max()
        mu, sg = SM.produce(D, simil, _x(fam), st, U, Z)
        muc, sgc = SM.produce(D, simil, _x(fam), stc, U, Z)
        np.testing.assert_allclose(muc, mu, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(sgc, sg, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("fam", SR.FOUR)
def test_u_equal_x_is_the_sum_of_the_oracle_lmls(fam):
    """The rule of tests/test_sparse_cpu.py per column (the eps-perturbation of the LML plus the dense solves' rounding),
    summed over the columns."""
    D, simil, _ = SR.FAMILIES[fam]
    X, _, _ = SR.inputs(60, 7, D)
    Y = SM.outputs(X, 3)
    eps = 1e-10
    total, bounds, _, _, _ = SM.reference(D, simil, _x(fam), X, Y, X, eps, want_grad=False)
    Kn = SR.LR.gram(D, simil, _x(fam), X)
    trinv = np.trace(np.linalg.inv(Kn))
    o = FastOracle(D, simil, SR.NOISE)
    want, allowed = 0.0, 0.0
    for t in range(Y.shape[1]):
        o.set_data(X, Y[:, t])
        lml = o.Observe(_x(fam))
        alpha = np.linalg.solve(Kn, Y[:, t])
        bt = 0.5 * eps * abs(trinv - alpha @ alpha) + 1e-9 * abs(lml) + 1e-11
        assert abs(bounds[t] - lml) <= bt, (fam, t, bounds[t], lml, bt)
        want += lml
        allowed += bt
    print("%s U = X: total %.12e, sum of the oracle's LMLs %.12e, |diff| = %.3e, allowed %.3e" % (fam, total, want, abs(total - want), allowed))
    assert abs(total - want) <= allowed


# ---- the slab functions of launch_sparse_xty ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


@pytest.mark.parametrize("T", [1, 64, 65, 128])
@pytest.mark.parametrize("Mi", [1, 64, 2048, 4096])
def test_slab_bound_covers_every_chunk_length(gpm, Mi, T):
    """The partials are sized by sparse_xty_slabs_bound(chunk): for every accepted "sparse_chunk" (a multiple of 256 in
    256 .. 65536) and every chunk length r <= it, the launch's own slab count must not exceed it.  Shown as: the count of
    every r in 1 .. 65536 is within the bound at r, and the bound never falls as r grows."""
    hk = _lib.hooks()
    rps = ctypes.c_int64(0)
    top = 65536
    slabs, bound, per = np.zeros(top + 1, np.int64), np.zeros(top + 1, np.int64), np.zeros(top + 1, np.int64)
    for r in range(1, top + 1):
        slabs[r] = hk.gogp_test_sparse_xty_slabs(r, Mi, T, ctypes.byref(rps))
        per[r] = rps.value
        bound[r] = hk.gogp_test_sparse_xty_slabs_bound(r, Mi, T)
    r = np.arange(top + 1)
    assert (slabs[1:] >= 1).all() and (slabs[1:] <= bound[1:]).all()
    assert (np.diff(bound[1:]) >= 0).all()
    for chunk in range(256, top + 1, 256):  # every accepted option value, spelled out
        assert slabs[1:chunk + 1].max() <= bound[chunk], chunk
    # the slabs cover the rows, none is empty, a slab is whole 32-row passes, the grid fits
    assert (per[1:] % 32 == 0).all() and (per[1:] >= 256).all()
    assert (slabs[1:] * per[1:] >= r[1:]).all() and ((slabs[1:] - 1) * per[1:] < r[1:]).all()
    tiles = ((Mi + 63) // 64) * ((T + 63) // 64)
    assert (slabs[1:] * tiles <= max(1024, tiles)).all() and slabs.max() <= 65535
    print("M = %d, T = %d: up to %d slabs, bound at 8192 / 65536 rows: %d / %d" % (Mi, T, slabs.max(), bound[8192], bound[top]))


def test_slab_functions_refuse_out_of_range(gpm):
    hk = _lib.hooks()
    for rows, Mi, T in ((0, 64, 1), (65537, 64, 1), (256, 0, 1), (256, 4097, 1), (256, 64, 0), (256, 64, 129)):
        assert hk.gogp_test_sparse_xty_slabs(rows, Mi, T, None) == 0
        assert hk.gogp_test_sparse_xty_slabs_bound(rows, Mi, T) == 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_bound_and_declared():
    """Fails on the parent commit: the five gogp_sparse_multi_* symbols and the three hooks are in the binding's tables
    with the headers' argument counts, include/gogp_hip.h declares them and GOGP_SPARSE_MULTI_MAX_T, and the libraries
    export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_sparse_multi_set_outputs": 4, "gogp_sparse_multi_observe": 5, "gogp_sparse_multi_gradient": 3,
            "gogp_sparse_multi_gradient_inducing": 4, "gogp_sparse_multi_produce": 5}
    want_hooks = {"gogp_test_sparse_xty": 14, "gogp_test_sparse_xty_slabs": 4, "gogp_test_sparse_xty_slabs_bound": 3}
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
    assert re.search(r"#define GOGP_SPARSE_MULTI_MAX_T 128\b", h) and MAX_T == 128
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    for name in want:
        assert getattr(lib, name) is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None


def test_c_abi_refusals_that_need_no_device():
    """NULL handles are refused by every call before anything is touched."""
    _lib.build()
    L = _lib.lib()
    one = np.zeros(1)
    dp = one.ctypes.data_as(_lib._dp)
    v = ctypes.c_double(0.0)
    assert L.gogp_sparse_multi_set_outputs(None, dp, 1, 1) == EARG
    assert L.gogp_sparse_multi_set_outputs(None, None, 0, 0) == EARG
    assert L.gogp_sparse_multi_observe(None, dp, 1, ctypes.byref(v), dp) == EARG
    assert L.gogp_sparse_multi_gradient(None, dp, 1) == EARG
    assert L.gogp_sparse_multi_gradient_inducing(None, dp, 1, dp) == EARG
    assert L.gogp_sparse_multi_produce(None, dp, 1, dp, dp) == EARG


def _xty(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    rows, Mi, Mp, ld, ldy, T, ldr = g("rows", 37), g("M", 200), g("Mp", 256), g("ld", 264), g("ldy", 6), g("T", 3), g("ldr", 256)
    Vt = np.zeros(max(g("vt_len", 36 * 264 + 200), 1))
    Y = np.zeros(max(g("y_len", 36 * 6 + 3), 1))
    R = np.zeros(max(g("r_len", 63 * 256 + 256), 1))
    dp = gp._dp
    return _lib.hooks().gogp_test_sparse_xty(-1, None if g("vt_null", False) else dp(Vt), Vt.size, ld, rows, Mi, Mp,
                                             None if g("y_null", False) else dp(Y), Y.size, ldy, T,
                                             None if g("r_null", False) else dp(R), R.size, ldr)


XTY_REFUSED = [dict(rows=0), dict(rows=(1 << 16) + 1), dict(M=0), dict(M=257), dict(Mp=0), dict(Mp=200), dict(Mp=4160),
               dict(T=0), dict(T=129), dict(ld=199), dict(ldy=2), dict(ldr=255), dict(vt_len=36 * 264 + 199),
               dict(y_len=36 * 6 + 2), dict(r_len=63 * 256 + 255), dict(T=65, ldy=65, y_len=37 * 65), dict(vt_null=True),
               dict(y_null=True), dict(r_null=True)]


@pytest.mark.parametrize("bad", XTY_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in XTY_REFUSED])
def test_xty_hook_refuses(gpm, bad):
    assert _xty(gpm, **bad) == EARG


def test_xty_hook_accepts_the_valid_neighbours(gpm):
    # (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for ok in [{}, dict(rows=1, vt_len=200, y_len=3), dict(M=256, vt_len=36 * 264 + 256), dict(M=1), dict(ldy=3, y_len=37 * 3),
               dict(T=65, ldy=65, y_len=37 * 65, r_len=128 * 256)]:
        assert _xty(gpm, **ok) in OKS, ok
