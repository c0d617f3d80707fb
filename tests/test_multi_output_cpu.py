"""Multi-output without a GPU: the dense reference of tests/multi_output_ref.py (what gogp_multi_lml, gogp_multi_gradient
and gogp_multi_produce evaluate) against the oracle's single-output LML and gradient column by column and against
central differences, the refusals of the kernel's test hook, and the binding of the five symbols.

Values against the oracle: n = 40, prior variance <= 2.3, noise variance 0.09 give cond(K) <= (40 * 2.3 + 0.09) / 0.09 ~
1e3; both sides are dense fp64 Cholesky solves of the same matrix, ~1e3 * 2.2e-16 * (a few hundred operations) ~ 1e-11
relative.  rtol = 1e-9, atol = 1e-11 leaves two orders of margin (the bound of tests/test_loo_cpu.py for its values).

Gradient against the central difference D(h) of the reference's total in x = log theta, h = 1e-3, with the step and the
bound of tests/test_loo_cpu.py: |D(2 h) - D(h)| (three times the truncation error of D(h)) plus four times the rounding
eps cond(K) |total| / h."""
import os
import re

import numpy as np
import pytest

import loo_ref as LR
import multi_output_ref as MR
from gogp_amd import _lib, kernel
from oracle.oracle import FastOracle

N = 40
H = 1e-3
EPS = np.finfo(float).eps
EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)

#: name -> (NDim, Simil, theta_simil, events)
CASES = {
    "normal": (2, kernel.Scaled(kernel.Normal), [1.1, 0.8], None),
    "matern32": (2, kernel.Scaled(kernel.Matern32), [1.0, 0.8], None),
    "ard_rbf3": MR.FAMILIES["ard_rbf3"] + (None,),
    "sum_periodic": MR.FAMILIES["hyperpriors"] + (None,),
    "events": MR.FAMILIES["matern52"] + (MR.EVENTS,),
}


def _case(name, T):
    D, simil, ts, events = CASES[name]
    X, y, Z = MR.inputs(N, 7, D)
    x = np.log(np.array(list(ts) + MR.TN))
    return D, simil, x, X, MR.outputs(X, T, y), Z, events


@pytest.mark.parametrize("name", ["normal", "matern32", "ard_rbf3", "sum_periodic"])
def test_reference_is_the_sum_of_the_oracle_over_the_columns(name):
    T = 3
    D, simil, x, X, Y, Z, _ = _case(name, T)
    A, lml, grad = MR.reference(D, simil, x, X, Y)
    want_g = np.zeros_like(grad)
    for t in range(T):
        o = FastOracle(D, simil, MR.NOISE)
        o.set_data(X, Y[:, t].copy())
        l = o.Observe(x)
        want_g += np.asarray(o.Gradient())
        print("%s column %d: lml %.12e, oracle %.12e" % (name, t, lml[t], l))
        np.testing.assert_allclose(lml[t], l, rtol=1e-9, atol=1e-11)
    print("%s: gradient %s, sum of the oracle's %s" % (name, grad, want_g))
    np.testing.assert_allclose(grad, want_g, rtol=1e-9, atol=1e-11 * max(1.0, np.abs(want_g).max()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_against_central_differences(name):
    D, simil, x, X, Y, Z, events = _case(name, 3)
    K, dK = LR.gram(D, simil, x, X, events, want_grad=True)
    grad = MR.dense(K, Y, dK)[2]
    assert grad.shape == x.shape

    def total(xx):
        return MR.dense(LR.gram(D, simil, xx, X, events), Y)[1].sum()

    L0, cond = total(x), np.linalg.cond(K)
    for p in range(len(x)):
        e = np.zeros(len(x))
        e[p] = 1.0
        d1 = (total(x + H * e) - total(x - H * e)) / (2 * H)
        d2 = (total(x + 2 * H * e) - total(x - 2 * H * e)) / (4 * H)
        tol = abs(d2 - d1) + 4.0 * EPS * cond * abs(L0) / H
        print("%s grad[%d] = %.9e, central difference %.9e, |diff| = %.3e, tolerance %.3e (truncation %.3e)"
              % (name, p, grad[p], d1, abs(grad[p] - d1), tol, abs(d2 - d1)))
        assert abs(grad[p] - d1) <= tol, (name, p, grad[p], d1, tol)
        assert tol < 1e-3 * max(1.0, np.abs(grad).max())  # the check has teeth


def test_one_output_reduces_to_the_single_output_quantities():
    D, simil, x, X, Y, Z, _ = _case("ard_rbf3", 1)
    y = Y[:, 0]
    K, dK = LR.gram(D, simil, x, X, want_grad=True)
    A, lml, grad = MR.dense(K, Y, dK)
    alpha = np.linalg.solve(K, y)
    np.testing.assert_allclose(A[:, 0], alpha, rtol=1e-9, atol=1e-11)
    sign, logdet = np.linalg.slogdet(K)
    np.testing.assert_allclose(lml[0], -0.5 * y @ alpha - 0.5 * logdet - 0.5 * N * np.log(2 * np.pi), rtol=1e-9, atol=1e-11)
    Kinv = np.linalg.inv(K)
    want = np.array([0.5 * ((np.outer(alpha, alpha) - Kinv) * d).sum() for d in dK])
    np.testing.assert_allclose(grad, want, rtol=1e-9, atol=1e-11)
    mu, sigma = MR.produce(D, simil, x, X, A, Z)
    import produce_grad_ref as PR
    mu1, sigma1, _, _ = PR.reference(D, simil, np.exp(x[:-1]), X, y, Z)
    np.testing.assert_allclose(mu[:, 0], mu1, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(sigma, sigma1, rtol=1e-9, atol=1e-11)


# ---- the test hook of multi_weight_kernel refuses bad arguments before it touches a device ------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _hook(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    T, n, npad, ld, ldk = g("T", 5), g("n", 300), g("npad", 512), g("ld", 520), g("ldk", 512)
    At = np.zeros(max(g("at_len", 4 * 520 + 512), 1))
    Kinv = np.zeros(max(g("kinv_len", 512 * 512), 1))
    G = np.zeros(max(g("g_len", 512 * 512), 1))
    dp = gp._dp
    return _lib.hooks().gogp_test_multi_weight(-1, None if g("at_null", False) else dp(At), At.size, ld, T,
                                               None if g("kinv_null", False) else dp(Kinv), Kinv.size, ldk, n, npad,
                                               None if g("g_null", False) else dp(G), G.size)


REFUSED = [dict(T=0), dict(T=129), dict(n=0), dict(n=513), dict(npad=0), dict(npad=500), dict(npad=1 << 16), dict(ld=511),
           dict(ldk=511), dict(at_len=4 * 520 + 511), dict(kinv_len=512 * 512 - 1), dict(g_len=512 * 512 - 1),
           dict(at_null=True), dict(kinv_null=True), dict(g_null=True)]


@pytest.mark.parametrize("bad", REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in REFUSED])
def test_hook_refuses(gpm, bad):
    assert _hook(gpm, **bad) == EARG


def test_hook_accepts_the_valid_neighbours(gpm):
    # (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for ok in [{}, dict(T=1, at_len=512), dict(T=128, at_len=127 * 520 + 512), dict(n=512), dict(n=1), dict(ld=512)]:
        assert _hook(gpm, **ok) in OKS, ok
    with pytest.raises(TypeError):
        gpm.multi_weight_check(np.zeros(512, np.float32), 512, 1, np.zeros(512 * 512), 512, 1, 512, np.zeros(512 * 512))


def test_symbols_bound_and_declared():
    """Fails on the parent commit: the five gogp_multi_* symbols are in the binding's table with the header's argument
    counts, include/gogp_hip.h declares them and GOGP_MULTI_MAX_T, and the library exports them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    want = {"gogp_multi_set_outputs": 4, "gogp_multi_lml": 3, "gogp_multi_gradient": 3, "gogp_multi_get_alpha": 2,
            "gogp_multi_produce": 5}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gogp_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, nargs in want.items():
        assert name in table and len(table[name][1]) == nargs, name
        m = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert re.search(r"#define GOGP_MULTI_MAX_T 128\b", header) and _lib.GOGP_MULTI_MAX_T == 128
    _lib.build()
    lib = _lib.lib()
    for name in want:
        assert getattr(lib, name) is not None
