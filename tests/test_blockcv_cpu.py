"""Leave-block-out cross-validation without a GPU: the closed forms of tests/blockcv_ref.py (what gogp_blockcv and
gogp_blockcv_gradient evaluate) against the definition -- one refit per block on the rows outside it --, the two host
functions gogp_blockcv_check and gogp_blockcv_groups, and the binding of the symbols.

Values: closed form against brute force at rtol = 1e-9, atol = 1e-11, the bound of tests/test_loo_cpu.py and its
argument: both sides are O(1) and differ by rounding that cond(K) amplifies; n <= 140, prior variance <= 2.3 and noise
variance 0.09 give cond(K) <= (140 * 2.3 + 0.09) / 0.09 ~ 4e3, the blocks of K^-1 are no worse conditioned than K, so
~4e3 * 2.2e-16 * (a few hundred operations) ~ 1e-10 relative at the worst -- the issue's own numpy check saw 2e-13 --
and a wrong formula is off in the first digit.

Gradient: closed form against the central difference D(h) of the brute-force total in x = log theta, h = 1e-3, with the
tolerance of tests/test_loo_cpu.py, taken from the reference itself: the measured truncation |D(2 h) - D(h)| (three times
the truncation error of D(h)) plus four times the rounding eps cond(K) |L| / h."""
import ctypes
import os
import re

import numpy as np
import pytest

import blockcv_ref as BR
import loo_ref as LR
from gogp_amd import _lib, kernel

H = 1e-3
EPS = np.finfo(float).eps
I64P = ctypes.POINTER(ctypes.c_int64)

#: name -> (family, n, block lengths)
CASES = {
    "mixed37": ("normal", 37, (1, 5, 13, 11, 1, 6)),
    "one128": ("normal", 140, (128, 12)),
}
FAMILIES = {"normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8])}


def _case(name):
    fam, n, lengths = CASES[name]
    D, simil, ts = FAMILIES[fam]
    X, y, _ = LR.inputs(n, 1, D)
    x = np.log(np.array(list(ts) + LR.TN))
    start = BR.starts(lengths)
    assert start[-1] == n
    return D, simil, x, X, y, start


def _ip(a):
    return a.ctypes.data_as(I64P)


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_values_against_refits(name):
    D, simil, x, X, y, start = _case(name)
    K = LR.gram(D, simil, x, X)
    bf = BR.brute_force(K, y, start)
    cf = BR.closed_form(K, y, start)
    for what, a, b in zip(("mu", "sigma", "logp"), cf, bf):
        print("%s %s: max |closed - refit| = %.3e" % (name, what, np.abs(a - b).max()))
    for a, b in zip(cf, bf):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11)


def test_blocks_of_one_row_are_loo():
    D, simil, x, X, y, _ = _case("mixed37")
    K, dK = LR.gram(D, simil, x, X, want_grad=True)
    loo = LR.closed_form(K, y, dK)
    bcv = BR.closed_form(K, y, np.arange(len(y) + 1), dK)
    for what, a, b in zip(("mu", "sigma", "logp", "grad"), bcv, loo):
        print("%s: max |block - LOO| = %.3e" % (what, np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_gradient_against_central_differences(name):
    D, simil, x, X, y, start = _case(name)
    K, dK = LR.gram(D, simil, x, X, want_grad=True)
    grad = BR.closed_form(K, y, start, dK)[3]
    assert grad.shape == x.shape

    def score(xx):
        return BR.brute_force(LR.gram(D, simil, xx, X), y, start)[2].sum()

    L0, cond = score(x), np.linalg.cond(K)
    for p in range(len(x)):
        e = np.zeros(len(x))
        e[p] = 1.0
        d1 = (score(x + H * e) - score(x - H * e)) / (2 * H)
        d2 = (score(x + 2 * H * e) - score(x - 2 * H * e)) / (4 * H)
        tol = abs(d2 - d1) + 4.0 * EPS * cond * abs(L0) / H
        print("%s grad[%d] = %.9e, central difference %.9e, |diff| = %.3e, tolerance %.3e (truncation %.3e)"
              % (name, p, grad[p], d1, abs(grad[p] - d1), tol, abs(d2 - d1)))
        assert abs(grad[p] - d1) <= tol, (name, p, grad[p], d1, tol)
        assert tol < 1e-3 * max(1.0, np.abs(grad).max())  # the check has teeth


def test_square_root_of_the_block_weight():
    """S_B S_B^T = Sigma_B + v v^T, also at w = 0 (gamma = 1/2 there).  Both sides are products of O(1) matrices of at most
    13 columns: a few dozen roundings, 1e-13 relative to the largest entry leaves two orders of margin."""
    D, simil, x, X, y, start = _case("mixed37")
    K = LR.gram(D, simil, x, X)
    Q = np.linalg.inv(K)
    for alpha in (np.linalg.solve(K, y), np.zeros(len(y))):
        for f in range(len(start) - 1):
            a, b = int(start[f]), int(start[f + 1])
            _, Xb, w, v = BR.block_terms(Q, alpha, a, b)
            S = BR.sqrt_factor(Xb, w, v)
            M = Xb.T @ Xb + np.outer(v, v)
            err = np.abs(S @ S.T - M).max() / np.abs(M).max()
            print("block %d (|w|^2 = %.3e): max |S S^T - M| / max |M| = %.3e" % (f, w @ w, err))
            assert err <= 1e-13
    # the two forms of gamma agree, and the one the device uses is exact at 0
    for w2 in (0.0, 1e-30, 1e-9, 0.3, 7.0, 1e6):
        g = 1.0 / (np.sqrt(1.0 + w2) + 1.0)
        assert abs(2 * g + g * g * w2 - 1.0) <= 4 * EPS
    assert 1.0 / (np.sqrt(1.0 + 0.0) + 1.0) == 0.5


def test_check_refusals():
    L = _lib.lib()

    def check(start, n, F=None):
        st = np.asarray(start, dtype=np.int64)
        return L.gogp_blockcv_check(_ip(st), len(st) - 1 if F is None else F, n)

    assert check([0, 3, 10], 10) == _lib.GOGP_OK
    assert check([0], 0) == _lib.GOGP_OK  # the empty process
    assert check(np.arange(0, 129 * 128, 128), 128 * 128) == _lib.GOGP_OK
    assert check([0, 128], 128) == _lib.GOGP_OK
    assert check([1, 3, 10], 10) == _lib.GOGP_EARG  # start[0] != 0
    assert check([0, 3, 3, 10], 10) == _lib.GOGP_EARG  # an empty block
    assert check([0, 5, 3, 10], 10) == _lib.GOGP_EARG  # not increasing
    assert check([0, 3, 10], 11) == _lib.GOGP_EARG  # start[F] != n
    assert check([0, 3, 10], 9) == _lib.GOGP_EARG
    assert check([0, 129], 129) == _lib.GOGP_EARG  # a block longer than GOGP_BLOCKCV_MAX
    assert check([0, 1, 130, 131], 131) == _lib.GOGP_EARG
    assert check([0], 5) == _lib.GOGP_EARG  # no blocks, but rows
    assert check([0, 3], 3, F=-1) == _lib.GOGP_EARG
    assert L.gogp_blockcv_check(None, 1, 3) == _lib.GOGP_EARG
    assert _lib.GOGP_BLOCKCV_MAX == BR.MAX_BLOCK == 128


def _groups(start):
    L = _lib.lib()
    st = np.asarray(start, dtype=np.int64)
    F = len(st) - 1
    first = np.full(F + 1, -7, dtype=np.int64)
    ng = ctypes.c_int64(-1)
    assert L.gogp_blockcv_groups(_ip(st), F, _ip(first), ctypes.byref(ng)) == _lib.GOGP_OK
    return first[:ng.value + 1], ng.value


@pytest.mark.parametrize("name", ["ones", "full", "65s", "random"])
def test_groups_against_the_mirror(name):
    rng = np.random.default_rng(20240611)
    # "65s": 65 + 1 + 65 > 128, a group closes after every pair
    lengths = {"ones": np.ones(300, dtype=int), "full": np.full(7, 128), "65s": np.array([65, 1] * 5 + [65]),
               "random": rng.integers(1, 129, size=200)}[name]
    start = BR.starts(lengths)
    first, ng = _groups(start)
    np.testing.assert_array_equal(first, BR.groups(start))
    assert first[0] == 0 and first[-1] == len(lengths) and (np.diff(first) >= 1).all()  # every block once, in order
    cols = np.array([start[first[g + 1]] - start[first[g]] for g in range(ng)])
    assert (cols >= 1).all() and (cols <= 128).all()
    for g in range(ng - 1):  # greedy: the next block did not fit
        assert cols[g] + lengths[first[g + 1]] > 128
    assert ng <= 2 * start[-1] // 129 + 1
    if name == "ones":
        assert ng == 3 and list(cols) == [128, 128, 44]
    if name == "full":
        assert ng == 7
    if name == "65s":
        assert list(cols) == [66] * 5 + [65]


def test_groups_refusals_and_empty():
    L = _lib.lib()
    ng = ctypes.c_int64(-1)
    first = np.zeros(4, dtype=np.int64)
    st = np.zeros(1, dtype=np.int64)
    assert L.gogp_blockcv_groups(_ip(st), 0, _ip(first), ctypes.byref(ng)) == _lib.GOGP_OK and ng.value == 0
    bad = np.array([0, 200], dtype=np.int64)
    assert L.gogp_blockcv_groups(_ip(bad), 1, _ip(first), ctypes.byref(ng)) == _lib.GOGP_EARG
    assert L.gogp_blockcv_groups(None, 1, _ip(first), ctypes.byref(ng)) == _lib.GOGP_EARG


def test_symbols_bound_and_declared():
    """Fails on the parent commit: the four calls are in the binding's table with the header's argument counts, and
    include/gogp_hip.h declares them."""
    want = {"gogp_blockcv_check": 3, "gogp_blockcv_groups": 4, "gogp_blockcv": 7, "gogp_blockcv_gradient": 5}
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gogp_hip.h")) as f:
        header = f.read()
    for name, nargs in want.items():
        assert name in table and len(table[name][1]) == nargs, name
        m = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert re.search(r"#define GOGP_BLOCKCV_MAX 128\b", header)
    hooks = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    assert {"gogp_test_blockcv_groups", "gogp_test_blockcv_apply"} <= hooks
    from gogp_amd import gp
    for attr in ("BlockCV", "BlockCVScore", "BlockCVGradient"):
        assert hasattr(gp.GP, attr)
    assert list(gp.blocks(10, 4)) == [0, 4, 8, 10] and list(gp.blocks(8, 4)) == [0, 4, 8] and list(gp.blocks(0, 4)) == [0]
    assert gp.BlockCVModel is not None
