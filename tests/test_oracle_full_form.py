"""The full Observe form of the CPU reference (oracle.FastOracle): x = [log theta | X.ravel() | y]
(gp/gp.go:366-369), whose Gradient() also returns dLML/dX (gp/gp.go:118-129) and dLML/dy = -alpha
(gp/gp.go:488-493).  FastOracle is what the GPU tests of tests/test_full_form_gradient.py compare the
library with at sizes the faithful Oracle (a dense dK per input coordinate: P + n D matrices of n x n)
cannot reach, so it is pinned here, without a GPU, against
  * the faithful Oracle on every kernel family at n in {37, 70} and on ARD kernels up to D = 40,
  * central differences of its own LML at n = 500,
  * the edges: duplicate input rows, rows that differ in one coordinate, inputs offset by ~1e6 length
    scales.
Both of FastOracle's pair loops are checked: the C/OpenMP one (use_c=True, the default the GPU tests use)
and the numpy one (use_c=False), which shares no derivative code with the C oracle."""
import numpy as np
import pytest

from gogp_amd import kernel
from cases import ANYNOISE, CASES

FAMILIES = CASES + [ANYNOISE]
#: a periodic kernel over several dimensions with one length scale each (the CASES periodic one is 1-D)
PERIODIC_ARD = ("periodic_ard3", 3, kernel.Scaled(kernel.ARD(kernel.Periodic, 3)), kernel.UniformNoise,
                [1.0, 0.7, 0.8, 0.9, 0.45], [0.2])


def _data(rng, n, D):
    X = rng.uniform(0, 1, (n, D))
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=n)
    return X, (y - y.mean()) / y.std()


def _full_x(ts, tn, X, y):
    return np.concatenate([np.log(np.array(list(ts) + list(tn), dtype=float)), X.reshape(-1), y])


def _parts(g, P, n, D):
    return g[:P], g[P:P + n * D], g[P + n * D:]


def _rel(a, b):
    """max |a - b| relative to max(1, |b|_inf)"""
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else 0.0


def _fd(f, x, j, h):
    """dLML/dx_j by the five-point central difference (truncation O(h^4)): at h = 1e-4 it neither needs the
    small steps at which the LML's rounding (~1e-11 here) dominates, nor lets the third derivative -- large for
    the periodic kernels -- through, as the three-point one does (5e-6 at any h for the 1-D periodic case)"""
    def at(t):
        xt = x.copy()
        xt[j] += t
        return f.Observe(xt)
    return (8.0 * (at(h) - at(-h)) - (at(2 * h) - at(-2 * h))) / (12.0 * h)


def _tol(name):
    # anynoise: a constant noise variance of 1e-5 under Matern-5/2 (cond(K) ~ 1e7 at these sizes); the two
    # restatements factor K in a different order (unblocked loop vs LAPACK), measured 3e-11 apart
    return 1e-9 if name == "anynoise" else 1e-10


def _against_faithful(name, D, simil, noise, ts, tn, X, y, tol):
    from oracle.oracle import FastOracle, Oracle
    n = len(y)
    P = len(ts) + len(tn)
    x = _full_x(ts, tn, X, y)
    o = Oracle(D, simil, noise)
    lml_o, grad_o = o.Observe(x), o.Gradient()
    assert grad_o.shape == x.shape
    for use_c in (True, False):
        f = FastOracle(D, simil, noise, use_c=use_c)
        lml = f.Observe(x)
        grad = f.Gradient()
        assert grad.shape == x.shape
        tag = (name, n, use_c)
        assert abs(lml - lml_o) <= tol * abs(lml_o), (tag, lml, lml_o)
        np.testing.assert_array_equal(f.X, X)  # X and y taken from x (gp/gp.go:391-396)
        np.testing.assert_array_equal(f.Y, y)
        for part, got, want in zip(("theta", "X", "y"), _parts(grad, P, n, D), _parts(grad_o, P, n, D)):
            assert np.all(np.isfinite(got)), (tag, part)
            assert _rel(got, want) <= tol, (tag, part, _rel(got, want))
        np.testing.assert_array_equal(grad[P + n * D:], -f.Alpha)
    return grad_o


@pytest.mark.parametrize("n", [37, 70])
@pytest.mark.parametrize("name,D,simil,noise,ts,tn", FAMILIES + [PERIODIC_ARD],
                         ids=[c[0] for c in FAMILIES + [PERIODIC_ARD]])
def test_full_form_matches_faithful_oracle(name, D, simil, noise, ts, tn, n):
    X, y = _data(np.random.default_rng(1000 + n + D), n, D)
    _against_faithful(name, D, simil, noise, ts, tn, X, y, _tol(name))


@pytest.mark.parametrize("kind", ["normal", "matern52"])
@pytest.mark.parametrize("D", [9, 17, 40])
def test_full_form_ard_matches_faithful_oracle(D, kind):
    """ARD length scales at the dimensions where the GPU kernel changes instance (9: 16 accumulators, 17 and
    40: passes of 32)."""
    base = kernel.Normal if kind == "normal" else kernel.Matern52
    simil = kernel.Scaled(kernel.ARD(base, D))
    ts = [1.1] + list(np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D)))
    X, y = _data(np.random.default_rng(D), 70, D)
    _against_faithful("ard_" + kind, D, simil, kernel.UniformNoise, ts, [0.2], X, y, 1e-10)


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", [c for c in FAMILIES + [PERIODIC_ARD] if c[0] in (
    "ard_rbf", "matern32", "matern52_ref", "matern52_textbook", "periodic", "hyperpriors", "periodic_ard3")],
    ids=lambda v: v if isinstance(v, str) else None)
def test_full_form_against_central_differences(name, D, simil, noise, ts, tn):
    """Every hyperparameter, 16 input coordinates spread over the rows (first, last, random) and dimensions,
    and 4 outputs, against five-point central differences of FastOracle's own LML at n = 500."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(500 + D)
    n = 500
    X, y = _data(rng, n, D)
    P = len(ts) + len(tn)
    x = _full_x(ts, tn, X, y)
    f = FastOracle(D, simil, noise)
    f.Observe(x)
    grad = f.Gradient()
    xin = [P, P + D - 1, P + n * D - 1] + list(P + rng.choice(n * D, 13, replace=False))
    xout = [P + n * D, x.size - 1] + list(P + n * D + rng.choice(n, 2, replace=False))
    for j in list(range(P)) + xin + xout:
        fd = _fd(f, x, j, 1e-4)
        assert abs(fd - grad[j]) <= 1e-6 * max(1.0, abs(fd)), (name, j, fd, grad[j])


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", FAMILIES + [PERIODIC_ARD],
                         ids=[c[0] for c in FAMILIES + [PERIODIC_ARD]])
def test_full_form_duplicate_and_one_coordinate_rows(name, D, simil, noise, ts, tn):
    """Exact duplicates (i != j with r = 0: Matern's sqrt(r^2) at 0, the periodic sign(x_i - x_j) = 0) and rows
    that differ in one coordinate only.  FastOracle gives the faithful oracle's answer: both take df/d(r^2),
    finite at r = 0, times x_i - x_j (or sign(x_i - x_j) sin(0)), so a duplicate pair adds an exact zero.  The
    LML is differentiable there (k is at least C^1 in x for every family): a central difference at a duplicate
    row's coordinates agrees with the gradient as well."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(77 + D)
    n = 40
    X, y = _data(rng, n, D)
    X[7] = X[3]
    X[21] = X[3]   # three copies of one point
    X[30] = X[12]
    X[25] = X[9]
    X[25, D - 1] += 0.125   # one coordinate apart (for D = 1: a pair at distance 1/8)
    X[33] = X[9]
    X[33, 0] -= 1e-7        # ... and a near-duplicate
    P = len(ts) + len(tn)
    x = _full_x(ts, tn, X, y)
    f = FastOracle(D, simil, noise)
    f.Observe(x)
    # default_noise and anynoise add a noise variance of 1e-10 / 1e-5: with exact duplicates K is then
    # nearly singular (cond(K) ~ 1e11 / 1e7 here).  anynoise: the two restatements agree to cond(K) * 1e-16,
    # the bound stated for it.  default_noise: K is singular to working precision; K^-1, hence W and every
    # gradient component, carries errors of order cond(K)^2 eps (the two restatements differ by 1.5e-3), so
    # only the LML (to cond(K) * 1e-16) and finiteness are asserted.  Where cond(K) > 1e6 the LML's rounding
    # would dominate the difference quotients below, which therefore run on the other families only.
    kappa = np.linalg.cond(f.Lc @ f.Lc.T)
    if kappa > 1e9:
        from oracle.oracle import Oracle
        assert name == "default_noise", (name, kappa)
        o = Oracle(D, simil, noise)
        lml_o = o.Observe(x)
        assert abs(f.LML() - lml_o) <= 1e-16 * kappa * abs(lml_o)
        assert np.all(np.isfinite(o.Gradient())) and np.all(np.isfinite(f.Gradient()))
        return
    grad_o = _against_faithful(name, D, simil, noise, ts, tn, X, y, max(_tol(name), 1e-16 * kappa))
    if kappa > 1e6:
        assert name == "anynoise", (name, kappa)
        return
    for i in (3, 7, 21, 12, 30, 25, 33):
        for d in range(D):
            j = P + i * D + d
            fd = _fd(f, x, j, 1e-4)
            assert abs(fd - grad_o[j]) <= 1e-6 * max(1.0, abs(fd)), (name, i, d, fd, grad_o[j])


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", [c for c in FAMILIES + [PERIODIC_ARD] if c[0] in (
    "scaled_rbf", "ard_rbf", "matern32", "periodic", "hyperpriors", "periodic_ard3")],
    ids=lambda v: v if isinstance(v, str) else None)
def test_full_form_offset_inputs(name, D, simil, noise, ts, tn):
    """Inputs offset by 2^21 (over 1e6 length scales), built as in test_ard_gradient_offset_inputs: the
    power-of-two offset keeps every per-dimension difference x_i - x_j of the shifted points equal, bit for
    bit, to that of X0 = (X + off) - off.  Every kernel here depends on the inputs through those differences
    only, so FastOracle on the shifted problem returns exactly what it returns on X0 -- and the faithful oracle
    agrees on the shifted problem itself."""
    from oracle.oracle import FastOracle, Oracle
    rng = np.random.default_rng(4242 + D)
    n = 60
    X, y = _data(rng, n, D)
    off = 2.0 ** 21
    Xo = X + off
    X0 = Xo - off
    assert off / max(ts) > 1e6
    a, b = FastOracle(D, simil, noise), FastOracle(D, simil, noise)
    assert a.Observe(_full_x(ts, tn, Xo, y)) == b.Observe(_full_x(ts, tn, X0, y))
    ga, gb = a.Gradient(), b.Gradient()
    P = len(ts) + len(tn)
    np.testing.assert_array_equal(ga[P:], gb[P:])  # rows summed in a fixed order
    # (the hyperparameter part's OpenMP reduction adds the threads' partial sums in whatever order they finish)
    assert _rel(ga[:P], gb[:P]) <= 1e-13
    o = Oracle(D, simil, noise)
    lml_o = o.Observe(_full_x(ts, tn, Xo, y))
    grad_o = o.Gradient()
    tol = _tol(name)
    assert abs(a.LML() - lml_o) <= tol * abs(lml_o)
    assert _rel(ga, grad_o) <= tol
    # the same through the numpy pair loop
    c = FastOracle(D, simil, noise, use_c=False)
    c.Observe(_full_x(ts, tn, Xo, y))
    assert _rel(c.Gradient(), grad_o) <= tol


def test_full_form_state_follows_the_last_observe():
    """Full form, then hyperparameters-only form (gradient length back to P), Absorb (no full form), full form
    at another n: the gradient's length and contents follow the last call, as in gp.GP."""
    from oracle.oracle import FastOracle
    name, D, simil, noise, ts, tn = CASES[1]
    P = len(ts) + len(tn)
    rng = np.random.default_rng(5)
    f = FastOracle(D, simil, noise)
    X1, y1 = _data(rng, 90, D)
    g1 = f.Observe(_full_x(ts, tn, X1, y1)), f.Gradient()
    assert g1[1].size == P + 90 * (D + 1)
    assert f.Observe(np.log(ts + tn)) == g1[0]  # the data stay those of the full-form call
    assert _rel(f.Gradient(), g1[1][:P]) <= 1e-13  # (OpenMP partial sums: order of completion)
    f.Absorb(X1, y1, ts, tn)
    assert f.Gradient().size == P
    X2, y2 = _data(rng, 33, D)
    f.Observe(_full_x(ts, tn, X2, y2))
    g2 = f.Gradient()
    fresh = FastOracle(D, simil, noise)
    fresh.Observe(_full_x(ts, tn, X2, y2))
    g3 = fresh.Gradient()
    np.testing.assert_array_equal(g2[P:], g3[P:])
    assert _rel(g2[:P], g3[:P]) <= 1e-13
    with pytest.raises(ValueError):
        f.Observe(np.concatenate([np.log(ts + tn), [0.5]]))  # gp/gp.go:398-400 panic("len(x)")


def test_full_form_at_the_largest_ndim_in_seconds():
    """n = 4200, D = 64 (the GPU test's largest shape): both the reduction and the OpenMP input gradient finish
    in seconds, and a sample of rows agrees with the numpy pair loop."""
    import time

    from oracle.oracle import FastOracle, xgrad_np
    D, n = 64, 4200
    X, y = _data(np.random.default_rng(64), n, D)
    simil = kernel.Scaled(kernel.ARD(kernel.Normal, D))
    ts = [1.1] + list(np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D)))
    f = FastOracle(D, simil, kernel.UniformNoise)
    t0 = time.perf_counter()
    f.Observe(_full_x(ts, [0.2], X, y))
    grad = f.Gradient()
    assert time.perf_counter() - t0 < 60.0
    P = D + 2
    gx = grad[P:P + n * D].reshape(n, D)
    import scipy.linalg as sla
    rows = np.array([0, 1, 63, 64, 2047, n - 1])
    E = np.zeros((n, rows.size))
    E[rows, np.arange(rows.size)] = 1.0
    Kinv_rows = sla.cho_solve((f.Lc, True), E).T
    W = np.outer(f.Alpha[rows], f.Alpha) - Kinv_rows
    want = xgrad_np(f.desc, f.ts, X[rows], X, W)
    assert _rel(gx[rows], want) <= 1e-10
