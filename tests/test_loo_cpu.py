"""Leave-one-out cross-validation without a GPU: the closed forms of tests/loo_ref.py (what gogp_loo and
gogp_loo_gradient evaluate) against the definition -- n refits on n - 1 rows -- and the binding of the two symbols.

Values: closed form against brute force at rtol = 1e-9, atol = 1e-11.  Both are O(1) and differ only by rounding that
cond(K) amplifies: n = 40, prior variance <= 2.3, noise variance 0.09 give cond(K) <= (40 * 2.3 + 0.09) / 0.09 ~ 1e3,
so ~1e3 * 2.2e-16 * (a few hundred operations) ~ 1e-11 relative; the bound leaves two orders of margin and a wrong
formula is off in the first digit.

Gradient: closed form against the central difference D(h) = (L(x + h e_p) - L(x - h e_p)) / (2 h) of the brute-force
L_LOO in x = log theta, h = 1e-3.  Its error has two parts, and the tolerance is their sum, both taken from the
reference itself and not from the code under test:
  * truncation  c h^2 + O(h^4), c = L''' / 6.  D(2 h) - D(h) = 3 c h^2 + O(h^4): that difference is measured and
    bounds the truncation error of D(h) three times over;
  * rounding    each L carries a relative error of about eps cond(K) (eps = 2.2e-16, cond(K) from np.linalg.cond at
    x), two of them are subtracted and divided by 2 h: eps cond(K) |L| / h; taken four times.
At h = 1e-3 these are ~1e-5 .. 1e-4 and ~4e-8 against components of size 0.1 .. 50."""
import os
import re

import numpy as np
import pytest

import loo_ref as LR
from gogp_amd import _lib, kernel

N = 40
H = 1e-3
EPS = np.finfo(float).eps

#: name -> (NDim, Simil, theta_simil, events); UniformNoise with std 0.3 throughout (one noise parameter)
CASES = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8], None),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8], None),
    "matern52": (2, kernel.Scaled(kernel.Matern52), [1.2, 0.9], None),
    "matern52textbook": (2, kernel.Scaled(kernel.Matern52Textbook), [0.9, 1.1], None),
    "sum_periodic": LR.FAMILIES["hyperpriors"] + (None,),
    "events": LR.FAMILIES["matern52"] + (LR.EVENTS,),
}


def _case(name):
    D, simil, ts, events = CASES[name]
    X, y, _ = LR.inputs(N, 1, D)
    x = np.log(np.array(list(ts) + LR.TN))
    return D, simil, x, X, y, events


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_values_against_refits(name):
    D, simil, x, X, y, events = _case(name)
    K = LR.gram(D, simil, x, X, events)
    if events:  # the discounts change this matrix
        assert np.abs(K - LR.gram(D, simil, x, X)).max() > 1e-2
    bf = LR.brute_force(K, y)
    cf = LR.closed_form(K, y)
    for what, a, b in zip(("mu", "sigma", "logp"), cf, bf):
        print("%s %s: max |closed - refit| = %.3e" % (name, what, np.abs(a - b).max()))
    for a, b in zip(cf, bf):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_gradient_against_central_differences(name):
    D, simil, x, X, y, events = _case(name)
    K, dK = LR.gram(D, simil, x, X, events, want_grad=True)
    grad = LR.closed_form(K, y, dK)[3]
    assert grad.shape == x.shape

    def score(xx):
        return LR.brute_force(LR.gram(D, simil, xx, X, events), y)[2].sum()

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


def test_symbols_bound_and_declared():
    """Fails on the parent commit: gogp_loo (handle, mu, sigma, logp, total) and gogp_loo_gradient (handle, grad, len)
    are in the binding's table with those argument counts, and include/gogp_hip.h declares them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "gogp_loo" in table and "gogp_loo_gradient" in table
    assert len(table["gogp_loo"][1]) == 5 and len(table["gogp_loo_gradient"][1]) == 3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gogp_hip.h")) as f:
        header = f.read()
    m = re.search(r"int gogp_loo\(([^)]*)\);", header)
    assert m and len(m.group(1).split(",")) == 5
    m = re.search(r"int gogp_loo_gradient\(([^)]*)\);", header)
    assert m and len(m.group(1).split(",")) == 3
